// hn_train.hip -- the training-step driver pieces around the fused renderer
// (run_nerf.py:576-636), so one step is a handful of launches:
//   * hn_sample_rays: N_rand distinct pixels of one image (without
//     replacement), their rays (ray_util.py:62-80) packed as the ray batch
//     render() builds (run_nerf_helpers.py:355-368), and their target colours;
//   * hn_loss_fwd / hn_loss_bwd: the loss of run_nerf.py:612-636 (with the
//     data-parallel scaling of train.dp_loss) and its input gradients in
//     torch autograd's op order, instead of ~25 tiny eager kernels.
#include "hn_common.h"
#include "hn_loss.h"
#include "hn_sampler.h"

namespace hn {

// ---------------------------------------------------------------------------
// Pixel sampling without replacement: a keyed 4-round Feistel permutation of
// [0, 2^k) (k even, 2^k >= window size M), restricted to [0, M) by cycle
// walking, is a bijection of [0, M); sample i is perm(i), so the n samples
// are distinct for any seed.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_rays_kernel(hn_ray_sampler s, const float* __restrict__ image,
                                                          const float* __restrict__ c2w, int64_t n,
                                                          int half, NdcK ndc, float* __restrict__ rays,
                                                          float* __restrict__ target) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t M = (uint32_t)s.crop_h * (uint32_t)s.crop_w;
  uint32_t x = (uint32_t)i;
  do {
    x = feistel(x, half, s.seed);
  } while (x >= M);
  const int py = s.crop_y0 + (int)(x / (uint32_t)s.crop_w);
  const int px = s.crop_x0 + (int)(x % (uint32_t)s.crop_w);
  float ray[11];
  pixel_ray(s.fx, s.fy, s.cx, s.cy, s.near, s.far, c2w, px, py, ray);
  if (ndc.on) ndc_ray(ndc.sx, ndc.sy, ray);
#pragma unroll
  for (int a = 0; a < 11; ++a) rays[11 * i + a] = ray[a];
  const float* px3 = image + 3 * ((size_t)py * s.W + px);
#pragma unroll
  for (int a = 0; a < 3; ++a) target[3 * i + a] = px3[a];
}

// ---------------------------------------------------------------------------
// The same draw in Morton order of its pixels, and torch.rand restated: the
// workgroup bodies live in hn_sampler.h (the binned render backward runs them
// too, for the next step's batch); these kernels give each workgroup its own
// index.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void uniform_kernel(UniK u) {
  uniform_block<1024>(u, blockIdx.x);
}

// the tiles' counts, and beside them the batch's uniform draws
__global__ __launch_bounds__(kMortonThreads) void morton_count_kernel(MortonK k, UniK u) {
  if (blockIdx.x >= k.blocks)
    uniform_block<kMortonThreads>(u, blockIdx.x - k.blocks);
  else
    morton_count_block<kMortonThreads>(k, blockIdx.x);
}

__global__ __launch_bounds__(kMortonThreads) void morton_emit_kernel(MortonK k, NdcK ndc) {
  morton_emit_block(k, ndc, blockIdx.x);
}

// ---------------------------------------------------------------------------
// use_batching ray pool (run_nerf.py:505-521, 544-555).  The reference
// materialises rays_rgb = [every training pixel][ro, rd, rgb] (rays from
// get_rays_np, ray_util.py:82-93: float64 arithmetic under numpy 2, then
// .astype(float32)), shuffles it once and again after every epoch, and takes
// consecutive N_rand slices.  Here the shuffle is a keyed bijection of the
// pool index (cycle-walked Feistel, as the per-image sampler), so nothing is
// materialised: pool position q -> pixel perm(q) = (image, row, column) ->
// its ray, computed in float64 and rounded once, and its target colour.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_pool_kernel(hn_ray_pool p, const float* __restrict__ images,
                                                          const float* __restrict__ poses,
                                                          const int32_t* __restrict__ ids, int64_t start, int64_t n,
                                                          int half, NdcK ndc, float* __restrict__ rays,
                                                          float* __restrict__ target) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float r[11], t[3];
  pool_ray_final(p, images, poses, ids, half, ndc, (uint32_t)(start + i), r, t);
  pool_ray_store(r, t, (size_t)i, rays, target);
}

// The batch in Morton order of its rays' mid-depth points (the body in
// hn_sampler.h): workgroup 0 sorts and emits, the others make the step's
// uniform draws, as morton_count_kernel places them behind its own.
__global__ __launch_bounds__(kMortonThreads) void sample_pool_ordered_kernel(PoolOrderK k, UniK u, NdcK ndc) {
  if (blockIdx.x >= 1)
    uniform_block<kMortonThreads>(u, blockIdx.x - 1);
  else
    pool_order_block(k, ndc);
}

// ---------------------------------------------------------------------------
// Blender image preparation: load/load_blender.py:63 (uint8 PNG / 255. in
// float64, .astype(float32)), :78-86 (half_res: cv2.resize INTER_AREA to H/2 x
// W/2, stored into a float64 array) and run_nerf.py:259-262 (white_bkgd:
// rgb * a + (1 - a), float32 arithmetic at full resolution, float64 after
// half_res; the trainer's torch.Tensor rounds to float32).  INTER_AREA at an
// exact factor 2 is the 2 x 2 box mean; OpenCV's float path sums
// ((top-left + top-right) + (bottom-left + bottom-right)) * 0.25 (cv2 is not in
// the image: that order is restated).  One thread per output pixel.
// ---------------------------------------------------------------------------
HN_DEV float u8_unit(uint8_t v) { return (float)((double)v / 255.0); }

__global__ __launch_bounds__(256) void blender_images_kernel(const uint8_t* __restrict__ rgba, int64_t n_px, int H,
                                                             int W, int half, int mode, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_px) return;
  const int Ho = half ? H / 2 : H, Wo = half ? W / 2 : W;
  const int64_t img = t / ((int64_t)Ho * Wo);
  const int r = (int)(t / Wo % Ho), col = (int)(t % Wo);
  float v[4];
  if (!half) {
    const uint8_t* s = rgba + 4 * ((img * H + r) * (int64_t)W + col);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = u8_unit(s[c]);
  } else {
    const uint8_t* s0 = rgba + 4 * ((img * H + 2 * r) * (int64_t)W + 2 * col);
    const uint8_t* s1 = s0 + 4 * (int64_t)W;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      v[c] = ((u8_unit(s0[c]) + u8_unit(s0[4 + c])) + (u8_unit(s1[c]) + u8_unit(s1[4 + c]))) * 0.25f;
  }
  if (mode == 0) {   // RGBA as load_blender_data returns it
#pragma unroll
    for (int c = 0; c < 4; ++c) out[4 * t + c] = v[c];
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float o = v[c];
    if (mode == 1) {
      o = half ? (float)((double)v[c] * (double)v[3] + (1.0 - (double)v[3])) : v[c] * v[3] + (1.f - v[3]);
    }
    out[3 * t + c] = o;
  }
}

// ---------------------------------------------------------------------------
// Loss.  Forward: one workgroup, fp64 accumulation of the reductions (the
// value is reported, its gradient does not depend on the summation order).
// ---------------------------------------------------------------------------
constexpr int kLossThreads = 1024;

__global__ __launch_bounds__(kLossThreads) void loss_fwd_kernel(
    const float* __restrict__ rgb, const float* __restrict__ rgb0, const float* __restrict__ target,
    const float* __restrict__ sp, const float* __restrict__ sp0, int64_t n, const float* __restrict__ tv,
    int n_tv, float world, float sparse_w, float tv_w, float* __restrict__ out) {
  loss_fwd_block<kLossThreads>(rgb, rgb0, target, sp, sp0, n, tv, n_tv, world, sparse_w, tv_w, out);
}

// Backward, op for op as autograd evaluates the eager expression:
//   (mse + mse0) / world   -> g / world (DivBackward)
//   mean over 3n            -> (.) / 3n  (MeanBackward: expand, divide by numel)
//   (x - t) ** 2            -> (.) * (2 * (x - t))  (PowBackward)
//   sparse_w * sum(sp)      -> g * sparse_w;   tv_w * sum(tv) -> g * tv_w
HN_DEV void loss_bwd_elem(
    int64_t j, const float* __restrict__ rgb, const float* __restrict__ rgb0, const float* __restrict__ target,
    int64_t n, int n_tv, float world, float sparse_w, float tv_w, const float* __restrict__ g_loss,
    float* __restrict__ g_rgb, float* __restrict__ g_rgb0, float* __restrict__ g_sp, float* __restrict__ g_sp0,
    float* __restrict__ g_tv) {
  const float g = *g_loss;
  const float gm = (g / world) / (float)(3 * n);
  if (j < 3 * n) {
    g_rgb[j] = gm * (2.f * (rgb[j] - target[j]));
    if (rgb0) g_rgb0[j] = gm * (2.f * (rgb0[j] - target[j]));
  }
  if (j < n) {
    if (g_sp) g_sp[j] = g * sparse_w;
    if (g_sp0) g_sp0[j] = g * sparse_w;
  }
  if (g_tv && j < n_tv) g_tv[j] = g * tv_w;
}
__global__ __launch_bounds__(256) void loss_bwd_kernel(
    const float* __restrict__ rgb, const float* __restrict__ rgb0, const float* __restrict__ target, int64_t n,
    int n_tv, float world, float sparse_w, float tv_w, const float* __restrict__ g_loss,
    float* __restrict__ g_rgb, float* __restrict__ g_rgb0, float* __restrict__ g_sp, float* __restrict__ g_sp0,
    float* __restrict__ g_tv) {
  loss_bwd_elem((int64_t)blockIdx.x * blockDim.x + threadIdx.x, rgb, rgb0, target, n, n_tv, world, sparse_w, tv_w,
                g_loss, g_rgb, g_rgb0, g_sp, g_sp0, g_tv);
}
// Both in one launch (the trainer's step): workgroup 0 reduces the loss, the
// others write the gradients -- the backward does not depend on the loss
// value, so the two run side by side; results bitwise those of the two kernels.
__global__ __launch_bounds__(kLossThreads) void loss_fwd_bwd_kernel(
    const float* __restrict__ rgb, const float* __restrict__ rgb0, const float* __restrict__ target,
    const float* __restrict__ sp, const float* __restrict__ sp0, int64_t n, const float* __restrict__ tv,
    int n_tv, float world, float sparse_w, float tv_w, float* __restrict__ out, const float* __restrict__ g_loss,
    float* __restrict__ g_rgb, float* __restrict__ g_rgb0, float* __restrict__ g_sp, float* __restrict__ g_sp0,
    float* __restrict__ g_tv) {
  if (blockIdx.x == 0)
    loss_fwd_block<kLossThreads>(rgb, rgb0, target, sp, sp0, n, tv, n_tv, world, sparse_w, tv_w, out);
  else
    loss_bwd_elem((int64_t)(blockIdx.x - 1) * kLossThreads + threadIdx.x, rgb, rgb0, target, n, n_tv, world,
                  sparse_w, tv_w, g_loss, g_rgb, g_rgb0, g_sp, g_sp0, g_tv);
}

}  // namespace hn

using namespace hn;

// Every sampler entry point is its _ndc sibling with no hn_ray_ndc.
extern "C" int32_t hn_sample_rays_ndc(const hn_ray_sampler* s, const float* image, const float* c2w,
                                      int64_t n_rays, float* rays, float* target, const hn_ray_ndc* ndc,
                                      void* stream) {
  if (!s) return HN_E_NULL;
  if (n_rays < 0) return HN_E_SHAPE;
  if (n_rays == 0) return HN_OK;
  if (!image || !c2w || !rays || !target) return HN_E_NULL;
  if (s->H <= 0 || s->W <= 0 || s->crop_h <= 0 || s->crop_w <= 0 || s->crop_y0 < 0 || s->crop_x0 < 0 ||
      s->crop_y0 + s->crop_h > s->H || s->crop_x0 + s->crop_w > s->W)
    return HN_E_SHAPE;
  const uint64_t M = (uint64_t)s->crop_h * (uint64_t)s->crop_w;
  if ((uint64_t)n_rays > M || M > (1ull << 30)) return HN_E_SHAPE;   // without replacement
  NdcK nk;
  const int32_t st = make_ndc(ndc, nk);
  if (st) return st;
  int bits = 2;
  while ((1ull << bits) < M) bits += 2;
  const unsigned blocks = (unsigned)((n_rays + 255) / 256);
  hipLaunchKernelGGL(sample_rays_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *s, image, c2w, n_rays,
                     bits / 2, nk, rays, target);
  return hip_status(hipGetLastError());
}

extern "C" int32_t hn_sample_rays(const hn_ray_sampler* s, const float* image, const float* c2w, int64_t n_rays,
                                  float* rays, float* target, void* stream) {
  return hn_sample_rays_ndc(s, image, c2w, n_rays, rays, target, nullptr, stream);
}

extern "C" size_t hn_sample_rays_morton_workspace_bytes(const hn_ray_sampler* s) {
  uint32_t n_idx;
  unsigned blocks;
  if (!s || !morton_geometry(s, n_idx, blocks)) return 0;
  return (size_t)blocks * sizeof(int);
}

extern "C" int32_t hn_uniform_philox(uint64_t seed, const hn_uniform_draw* draws, int32_t n_draws, void* stream) {
  UniK u;
  const int32_t st = make_uni(seed, draws, n_draws, u);
  if (st) return st;
  const int64_t total = u.start[u.n];
  if (total == 0) return HN_OK;
  hipLaunchKernelGGL(uniform_kernel, dim3((unsigned)((total + 1023) / 1024)), dim3(1024), 0, (hipStream_t)stream, u);
  return hip_status(hipGetLastError());
}

// The draw's checks, then the NDC step's (an empty draw launches nothing and
// checks no further, as before)
static int32_t sample_morton(const hn_ray_sampler* s, const float* image, const float* c2w, int64_t n_rays,
                             float* rays, float* target, void* workspace, size_t ws_bytes, const UniK& u,
                             const hn_ray_ndc* ndc, hipStream_t stream) {
  MortonK k;
  int32_t st = make_morton(s, image, c2w, n_rays, rays, target, workspace, ws_bytes, k);
  if (st || k.n == 0) return st;
  NdcK nk;
  if ((st = make_ndc(ndc, nk))) return st;
  hipLaunchKernelGGL(morton_count_kernel, dim3(k.blocks + uni_blocks(u)), dim3(kMortonThreads), 0, stream, k, u);
  hipLaunchKernelGGL(morton_emit_kernel, dim3(k.blocks), dim3(kMortonThreads), 0, stream, k, nk);
  return hip_status(hipGetLastError());
}

extern "C" int32_t hn_sample_rays_morton_ndc(const hn_ray_sampler* s, const float* image, const float* c2w,
                                             int64_t n_rays, float* rays, float* target, void* workspace,
                                             size_t ws_bytes, const hn_ray_ndc* ndc, void* stream) {
  UniK u;
  make_uni(0, nullptr, 0, u);
  return sample_morton(s, image, c2w, n_rays, rays, target, workspace, ws_bytes, u, ndc, (hipStream_t)stream);
}

extern "C" int32_t hn_sample_rays_morton(const hn_ray_sampler* s, const float* image, const float* c2w,
                                         int64_t n_rays, float* rays, float* target, void* workspace,
                                         size_t ws_bytes, void* stream) {
  return hn_sample_rays_morton_ndc(s, image, c2w, n_rays, rays, target, workspace, ws_bytes, nullptr, stream);
}

extern "C" int32_t hn_sample_batch_morton_ndc(const hn_ray_sampler* s, const float* image, const float* c2w,
                                              int64_t n_rays, float* rays, float* target, void* workspace,
                                              size_t ws_bytes, uint64_t seed, const hn_uniform_draw* draws,
                                              int32_t n_draws, const hn_ray_ndc* ndc, void* stream) {
  UniK u;
  const int32_t st = make_uni(seed, draws, n_draws, u);
  if (st) return st;
  return sample_morton(s, image, c2w, n_rays, rays, target, workspace, ws_bytes, u, ndc, (hipStream_t)stream);
}

extern "C" int32_t hn_sample_batch_morton(const hn_ray_sampler* s, const float* image, const float* c2w,
                                          int64_t n_rays, float* rays, float* target, void* workspace,
                                          size_t ws_bytes, uint64_t seed, const hn_uniform_draw* draws,
                                          int32_t n_draws, void* stream) {
  return hn_sample_batch_morton_ndc(s, image, c2w, n_rays, rays, target, workspace, ws_bytes, seed, draws, n_draws,
                                    nullptr, stream);
}

extern "C" int32_t hn_loss_fwd(const float* rgb, const float* rgb0, const float* target, const float* sp,
                               const float* sp0, int64_t n_rays, const float* tv, int32_t n_tv, float world,
                               float sparse_w, float tv_w, float* out, void* stream) {
  if (n_rays <= 0 || n_tv < 0) return HN_E_SHAPE;
  if (!rgb || !target || !sp || !out) return HN_E_NULL;
  if ((rgb0 == nullptr) != (sp0 == nullptr)) return HN_E_NULL;
  hipLaunchKernelGGL(loss_fwd_kernel, dim3(1), dim3(kLossThreads), 0, (hipStream_t)stream, rgb, rgb0, target, sp,
                     sp0, n_rays, tv, n_tv, world, sparse_w, tv_w, out);
  return hip_status(hipGetLastError());
}

extern "C" int32_t hn_loss_bwd(const float* rgb, const float* rgb0, const float* target, int64_t n_rays,
                               int32_t n_tv, float world, float sparse_w, float tv_w, const float* g_loss,
                               float* g_rgb, float* g_rgb0, float* g_sp, float* g_sp0, float* g_tv,
                               void* stream) {
  if (n_rays <= 0 || n_tv < 0) return HN_E_SHAPE;
  if (!rgb || !target || !g_loss || !g_rgb) return HN_E_NULL;
  if ((rgb0 == nullptr) != (g_rgb0 == nullptr)) return HN_E_NULL;
  const int64_t m = 3 * n_rays > n_tv ? 3 * n_rays : n_tv;
  const unsigned blocks = (unsigned)((m + 255) / 256);
  hipLaunchKernelGGL(loss_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rgb, rgb0, target, n_rays,
                     n_tv, world, sparse_w, tv_w, g_loss, g_rgb, g_rgb0, g_sp, g_sp0, g_tv);
  return hip_status(hipGetLastError());
}

extern "C" int32_t hn_loss_fwd_bwd(const float* rgb, const float* rgb0, const float* target, const float* sp,
                                   const float* sp0, int64_t n_rays, const float* tv, int32_t n_tv, float world,
                                   float sparse_w, float tv_w, float* out, const float* g_loss, float* g_rgb,
                                   float* g_rgb0, float* g_sp, float* g_sp0, float* g_tv, void* stream) {
  if (n_rays <= 0 || n_tv < 0) return HN_E_SHAPE;
  if (!rgb || !target || !sp || !out || !g_loss || !g_rgb) return HN_E_NULL;
  if ((rgb0 == nullptr) != (sp0 == nullptr) || (rgb0 == nullptr) != (g_rgb0 == nullptr)) return HN_E_NULL;
  const int64_t m = 3 * n_rays > n_tv ? 3 * n_rays : n_tv;
  const unsigned blocks = 1u + (unsigned)((m + kLossThreads - 1) / kLossThreads);
  hipLaunchKernelGGL(loss_fwd_bwd_kernel, dim3(blocks), dim3(kLossThreads), 0, (hipStream_t)stream, rgb, rgb0,
                     target, sp, sp0, n_rays, tv, n_tv, world, sparse_w, tv_w, out, g_loss, g_rgb, g_rgb0, g_sp,
                     g_sp0, g_tv);
  return hip_status(hipGetLastError());
}

extern "C" int32_t hn_sample_pool_ndc(const hn_ray_pool* p, const float* images, const float* poses,
                                      const int32_t* image_ids, int64_t start, int64_t n_rays, float* rays,
                                      float* target, const hn_ray_ndc* ndc, void* stream) {
  if (!p) return HN_E_NULL;
  if (n_rays < 0 || start < 0) return HN_E_SHAPE;
  if (n_rays == 0) return HN_OK;
  if (!images || !poses || !image_ids || !rays || !target) return HN_E_NULL;
  if (p->n_images <= 0 || p->H <= 0 || p->W <= 0 || p->pose_stride < 12) return HN_E_SHAPE;
  const uint64_t N = (uint64_t)p->n_images * (uint64_t)p->H * (uint64_t)p->W;
  if (N > (1ull << 30) || (uint64_t)start + (uint64_t)n_rays > N) return HN_E_SHAPE;   // one epoch's positions
  NdcK nk;
  const int32_t st = make_ndc(ndc, nk);
  if (st) return st;
  int bits = 2;
  while ((1ull << bits) < N) bits += 2;
  const unsigned blocks = (unsigned)((n_rays + 255) / 256);
  hipLaunchKernelGGL(sample_pool_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p, images, poses,
                     image_ids, start, n_rays, bits / 2, nk, rays, target);
  return hip_status(hipGetLastError());
}

extern "C" int32_t hn_sample_pool(const hn_ray_pool* p, const float* images, const float* poses,
                                  const int32_t* image_ids, int64_t start, int64_t n_rays, float* rays, float* target,
                                  void* stream) {
  return hn_sample_pool_ndc(p, images, poses, image_ids, start, n_rays, rays, target, nullptr, stream);
}

extern "C" int32_t hn_sample_pool_ordered_ndc(const hn_ray_pool* p, const float* images, const float* poses,
                                              const int32_t* image_ids, int64_t start, int64_t n_rays,
                                              const float* box_min, const float* box_max, float* rays,
                                              float* target, uint32_t* keys, uint64_t seed,
                                              const hn_uniform_draw* draws, int32_t n_draws,
                                              const hn_ray_ndc* ndc, void* stream) {
  // hn_sample_pool's checks, in its order
  if (!p) return HN_E_NULL;
  if (n_rays < 0 || start < 0) return HN_E_SHAPE;
  if (n_rays == 0) return HN_OK;
  if (!images || !poses || !image_ids || !rays || !target) return HN_E_NULL;
  if (p->n_images <= 0 || p->H <= 0 || p->W <= 0 || p->pose_stride < 12) return HN_E_SHAPE;
  const uint64_t N = (uint64_t)p->n_images * (uint64_t)p->H * (uint64_t)p->W;
  if (N > (1ull << 30) || (uint64_t)start + (uint64_t)n_rays > N) return HN_E_SHAPE;   // one epoch's positions
  if (n_rays > HN_POOL_ORDER_MAX) return HN_E_SHAPE;   // one workgroup's LDS holds the batch
  if (!box_min || !box_max) return HN_E_NULL;
  PoolOrderK k;
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(box_min[a]) || !std::isfinite(box_max[a]) || !(box_max[a] > box_min[a])) return HN_E_SHAPE;
    k.box_min[a] = box_min[a];
    k.box_max[a] = box_max[a];
  }
  UniK u;
  int32_t st = make_uni(seed, draws, n_draws, u);
  if (st) return st;
  NdcK nk;
  if ((st = make_ndc(ndc, nk))) return st;
  int bits = 2;
  while ((1ull << bits) < N) bits += 2;
  k.p = *p;
  k.images = images;
  k.poses = poses;
  k.ids = image_ids;
  k.start = start;
  k.n = (int)n_rays;
  k.padded = 1;
  while (k.padded < k.n) k.padded <<= 1;
  k.half = bits / 2;
  k.rays = rays;
  k.target = target;
  k.keys = keys;
  hipLaunchKernelGGL(sample_pool_ordered_kernel, dim3(1 + uni_blocks(u)), dim3(kMortonThreads), 0,
                     (hipStream_t)stream, k, u, nk);
  return hip_status(hipGetLastError());
}

extern "C" int32_t hn_sample_pool_ordered(const hn_ray_pool* p, const float* images, const float* poses,
                                          const int32_t* image_ids, int64_t start, int64_t n_rays,
                                          const float* box_min, const float* box_max, float* rays, float* target,
                                          uint32_t* keys, uint64_t seed, const hn_uniform_draw* draws,
                                          int32_t n_draws, void* stream) {
  return hn_sample_pool_ordered_ndc(p, images, poses, image_ids, start, n_rays, box_min, box_max, rays, target, keys,
                                    seed, draws, n_draws, nullptr, stream);
}

extern "C" int32_t hn_blender_images(const uint8_t* rgba, int64_t n_images, int32_t H, int32_t W, int32_t half_res,
                                     int32_t mode, float* out, void* stream) {
  if (n_images < 0 || H <= 0 || W <= 0 || mode < 0 || mode > 2) return HN_E_SHAPE;
  if (half_res && ((H | W) & 1)) return HN_E_SHAPE;   // INTER_AREA at exactly half
  if (n_images == 0) return HN_OK;
  if (!rgba || !out) return HN_E_NULL;
  const int64_t n_px = n_images * (int64_t)(half_res ? H / 2 : H) * (half_res ? W / 2 : W);
  hipLaunchKernelGGL(blender_images_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     rgba, n_px, H, W, half_res ? 1 : 0, mode, out);
  return hip_status(hipGetLastError());
}
