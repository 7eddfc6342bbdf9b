// hn_render_image.h -- render_image_kernel: whole images from poses
// (run_nerf_helpers.py:310-392 render() under render_path, :395-459), one
// launch for a list of views.  A persistent grid of the training forward's
// 4-wave workgroups: every wave loops over rays -- the pixel's ray made here
// from the pose and K (pixel_ray, the samplers' arithmetic; then ndc_ray where
// the launch asks for NDC rays), then the forward's own passes from the same
// device functions (render_fwd_kernel's results bit for bit, at 64 + 128 or
// 64 + 64 samples) -- and writes rgb, depth and acc only.  Nothing is saved for a
// backward: z, raw and the samples' coarse origins live in LDS, the two coarse
// feature tiles a fine pass takes its coarse twins from in a slot of the
// workspace that the wave owns for the whole launch.
//
// The passes are hn_render_fwd.h's shared body (coarse_z, pass_start,
// pass_tiles, importance_sort); this file holds the kernel's arguments, the
// pixel mapping, the persistent loop and ImageTiles, the policy for a tile's
// results: no masks, no stores but the coarse tiles into the slot, every dead
// tile's colours skipped.
#pragma once
#include "hn_render_fwd.h"
#include "hn_sampler.h"

namespace hn {

// 4 workgroups per CU (4 waves per SIMD, as the forward) on 256 CUs; a
// compile-time count, so the workspace's size needs no device
constexpr int kImgBlocks = 1024;
// its workgroup: 4 waves and the ring, whichever form the training forward runs
constexpr int kImgBlockWaves = kFwdWaves;
constexpr int kImgSlotFloats = 2 * 1024;   // a wave's two coarse feature tiles (store_feat's layout)
static_assert(kImgBlocks % 8 == 0, "one band of ray groups per XCD residue");
// 2 x 2 pixel blocks per side of a tile of the ray order (16 x 16 pixels)
constexpr int kImgTile = 8;

// hn_render_image_variant's bits
enum : int { kImgReencode = 1, kImgRowMajor = 2 };

struct ImageK {
  FieldK f;
  int variant;
  int n_views, H, W, pose_stride;
  uint32_t Hb, Wb;       // the image in 2 x 2 pixel blocks
  uint32_t groups;       // ray groups (4 rays) of the launch
  float fx, fy, cx, cy, near, far;
  int ndc;               // 1: the pixel's ray goes through ndc_ray (hn_view_args.ndc)
  float sx, sy;          // ... with these factors
  const float* poses;
  float* slots;          // [4 kImgBlocks][kImgSlotFloats], or NULL: every fine sample encoded
  float *rgb, *depth, *acc, *rays;
};

// What a wave needs only where a ray starts and ends -- the camera, the image's
// sizes, the pose and output pointers -- staged in LDS beside the grid sizes
// and read back per ray, so that none of it holds a scalar register through
// the tile loops (as kernel arguments they did: 108 scalar spills).
struct ImagePix {
  float fx, fy, cx, cy, near, far;
  int H, W, pose_stride, variant;
  uint32_t Hb, Wb;
  int ndc;
  float sx, sy;
  const float* poses;
  float *rgb, *depth, *acc, *rays;
};
constexpr int kImgPixLds = (sizeof(ImagePix) + 15) / 16 * 4;   // floats
static_assert(sizeof(ImagePix) % 4 == 0, "copied as words");
HN_DEV void image_pix_load(const float* lds, ImagePix& x) {
  uint32_t* w = reinterpret_cast<uint32_t*>(&x);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(ImagePix) / 4); ++i)
    w[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(lds[i]));
}

// Ray group -> view and 2 x 2 pixel block.  A view's blocks go tile by tile
// (kImgTile x kImgTile blocks, the tiles row by row), a whole tile in Morton
// order of its blocks, a tile the image's edge cuts row by row: every block
// of the view exactly once, at a closed-form position.
HN_DEV void image_group_block(uint32_t Hb, uint32_t Wb, uint32_t grp, uint32_t& view, uint32_t& bx, uint32_t& by) {
  const uint32_t per_view = Hb * Wb;
  view = grp / per_view;
  uint32_t i = grp - view * per_view;
  const uint32_t ty = i / (Wb * kImgTile);
  i -= ty * Wb * kImgTile;
  const uint32_t th = min((uint32_t)kImgTile, Hb - ty * kImgTile);
  const uint32_t tx = i / (kImgTile * th);
  i -= tx * kImgTile * th;
  const uint32_t tw = min((uint32_t)kImgTile, Wb - tx * kImgTile);
  uint32_t dx, dy;
  if (tw == kImgTile && th == kImgTile) {   // Morton: x in the even bits
    dx = (i & 1u) | ((i >> 1) & 2u) | ((i >> 2) & 4u);
    dy = ((i >> 1) & 1u) | ((i >> 2) & 2u) | ((i >> 3) & 4u);
  } else {
    dy = i / tw;
    dx = i - dy * tw;
  }
  bx = tx * kImgTile + dx;
  by = ty * kImgTile + dy;
}

// render_image_kernel's policy for the shared tile loops (hn_render_fwd.h)
struct ImageTiles {
  static constexpr bool kMasks = false;
  float* slot;           // the wave's two coarse tiles, or NULL: every fine sample encoded
  const uint8_t* srcl;   // the fine samples' coarse origins (LDS)
  HN_DEV const float* twins() const { return slot; }
  HN_DEV int origin(int q) const { return (int)srcl[q]; }
  HN_DEV bool skip_dead(int) const { return true; }
  HN_DEV void save_feat(int pass, int tau, int lane, const f32x16& feat) const {
    if (pass == 0 && slot) store_feat(slot, 0, tau, lane, feat, false);
  }
  HN_DEV void save_masks(int, int, int, const uint32_t (&)[3]) const {}
  HN_DEV void save_raw(int, int, const float4&) const {}
};

HN_DEV float wave_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// kNiT: the importance samples, kNi or kNi64 -- a compile-time shape, as
// render_fwd_kernel's (the merge network, the fine tile loop, the fine
// composite's samples per lane; u holds kNiT values).  kNdc: the launch's
// flag for NDC rays (ImageK::ndc), ndc_ray at the ray's start.
template <int kNiT, bool kNdc>
__global__ __launch_bounds__(64 * kImgBlockWaves)
__attribute__((amdgpu_waves_per_eu(kFwdWavesPerSimd, kFwdWavesPerSimd)))
void render_image_kernel(ImageK k) {
  constexpr int kSfT = kSc + kNiT;   // the ray's fine samples
  __shared__ __attribute__((aligned(16))) float smem[kImgBlockWaves * kFLds + kGsLds + kImgPixLds];
  __shared__ __attribute__((aligned(16))) float fring[kImgBlockWaves][768];
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane0 = threadIdx.x & 63;
  float* gsl = smem + kImgBlockWaves * kFLds;
  const float* pixl = gsl + kGsLds;
  stage_grid_sizes(k.f.g, gsl);
  if (threadIdx.x == 64) {
    ImagePix x;
    x.fx = k.fx; x.fy = k.fy; x.cx = k.cx; x.cy = k.cy; x.near = k.near; x.far = k.far;
    x.H = k.H; x.W = k.W; x.pose_stride = k.pose_stride; x.variant = k.variant;
    x.Hb = k.Hb; x.Wb = k.Wb;
    x.ndc = k.ndc; x.sx = k.sx; x.sy = k.sy;
    x.poses = k.poses;
    x.rgb = k.rgb; x.depth = k.depth; x.acc = k.acc; x.rays = k.rays;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&x);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(ImagePix) / 4); ++i) gsl[kGsLds + i] = __uint_as_float(w[i]);
  }
  __syncthreads();
  float* slot = k.slots ? k.slots + ((size_t)blockIdx.x * kImgBlockWaves + wave) * kImgSlotFloats : nullptr;

  // ---- coarse z_vals (:514-536) and their mid points: near, far and t_vals
  // are the launch's, so every ray of the wave shares them ----
  {
    const int lane = lane0;
    float* L = smem + wave * kFLds;
    const float z = coarse_z(k.f.tvals[lane], k.near, k.far, k.f.lindisp);
    L[kFZc + lane] = z;
    L[kFZsrc + lane] = z;
    lds_fence_wave();
    if (lane < kSc - 1) L[kFBins + lane] = .5f * (L[kFZc + lane + 1] + L[kFZc + lane]);
    lds_fence_wave();
  }

  // XCD-aware, as the forward's grp: workgroup b runs on XCD b % 8, and each
  // residue walks one contiguous band of the ray groups, its workgroups side
  // by side on consecutive groups.  (Measured on 8 views of 800 x 800, config
  // 2 after 1,000 steps: chunks of 128 groups dealt round-robin over the XCDs
  // instead, 283.8 against 276.5 ms; the waves that share a SIMD started a
  // quarter of a ray's time apart, 277.4-277.7 against 277.3 ms: neither kept.)
  const uint32_t nbx = gridDim.x / 8, xcd = blockIdx.x % 8;
  const uint32_t lo = (uint32_t)((uint64_t)k.groups * xcd / 8), hi = (uint32_t)((uint64_t)k.groups * (xcd + 1) / 8);
  for (uint32_t grp = lo + blockIdx.x / 8; grp < hi; grp += nbx) {
    // the lane index and the wave's LDS offset made opaque per ray: what
    // depends on them alone (the sort network's and the tiles' lane predicates,
    // dozens of 64-bit masks; the row sum's addresses) is then formed where it
    // is used, as in the forward, not hoisted out of this loop and held in
    // scalar registers through it (87 scalar spills)
    int lane = lane0, woff = wave * kFLds;
    asm volatile("" : "+v"(lane), "+s"(woff));
    float* L = smem + woff;
    // the fine samples' coarse origins: over the coarse weights, which
    // sample_pdf_wave has consumed by the time the merge writes them
    uint8_t* srcl = reinterpret_cast<uint8_t*>(L + kFW);
    // ---- the wave's pixel and its ray ----
    int64_t ray;
    Ray r;
    {
      ImagePix x;
      image_pix_load(pixl, x);
      int px, py;
      uint32_t view;
      if (x.variant & kImgRowMajor) {   // 4 consecutive pixels of the (view, row, column) order
        const uint32_t per_view = (uint32_t)x.H * (uint32_t)x.W;   // < 2^31: groups is
        ray = (int64_t)grp * kImgBlockWaves + wave;
        if (ray >= (int64_t)k.n_views * per_view) continue;
        view = (uint32_t)(ray / per_view);
        const uint32_t i = (uint32_t)(ray - (int64_t)view * per_view);
        py = (int)(i / (uint32_t)x.W);
        px = (int)(i - (uint32_t)py * (uint32_t)x.W);
      } else {                          // a 2 x 2 pixel block
        uint32_t bx, by;
        image_group_block(x.Hb, x.Wb, grp, view, bx, by);
        px = (int)(2 * bx) + (wave & 1);
        py = (int)(2 * by) + (wave >> 1);
        if (px >= x.W || py >= x.H) continue;
        ray = ((int64_t)view * x.H + py) * x.W + px;
      }
      float v[11];
      pixel_ray(x.fx, x.fy, x.cx, x.cy, x.near, x.far, x.poses + (size_t)view * x.pose_stride, px, py, v);
      if constexpr (kNdc) ndc_ray(x.sx, x.sy, v);   // (near, far and the view direction stay the world ray's)
      if (x.rays && lane == 0) {
#pragma unroll
        for (int a = 0; a < 11; ++a) x.rays[11 * ray + a] = v[a];
      }
      // the ray on the scalar unit, as the forward's loaded one
#pragma unroll
      for (int a = 0; a < 11; ++a) v[a] = wave_uniform(v[a]);
      make_ray(v, r);
      r.dnorm = wave_uniform(r.dnorm);
    }
    float sh8[8];
    ray_sh(r, lane >> 5, sh8);
    ImageTiles pol{slot, srcl};

    // ---- coarse network (:540); the last ray's final (unused) ring fill drained ----
    pass_start(k.f.Pc, sh8, L, fring[wave], lane, true);
    pass_tiles<0>(k.f, gsl, fring[wave], L, r, lane, pol);
    lds_fence_wave();
    CompOut co;
    composite_fwd<kSc / 64>(L + kFRaw, L + kFZc, nullptr, kSc, r.dnorm, k.f.white != 0, L + kFW, co, lane);

    // ---- importance sampling (:547-551), the det uniforms ----
    importance_sort<kNiT>(L, k.f.u, srcl, lane);

    // ---- fine network (:556); the drain: the slot's tiles are written ----
    pass_start(k.f.Pf, sh8, L, fring[wave], lane, true);
    pass_tiles<1, ImageTiles, kSfT>(k.f, gsl, fring[wave], L, r, lane, pol);
    lds_fence_wave();
    CompOut fo;
    composite_fwd<kSfT / 64>(L + kFRaw, L + kFZs, nullptr, kSfT, r.dnorm, k.f.white != 0, nullptr, fo, lane);
    if (lane == 0) {
      ImagePix x;
      image_pix_load(pixl, x);
#pragma unroll
      for (int c = 0; c < 3; ++c) x.rgb[3 * ray + c] = fo.rgb[c];
      x.depth[ray] = fo.depth;
      x.acc[ray] = fo.acc;
    }
  }
}

}  // namespace hn
