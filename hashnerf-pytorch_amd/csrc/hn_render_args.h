// hn_render_args.h -- what every kernel of hn_render.hip shares: the kernel-
// argument structs (FieldK, RenderK, B1K, ScK, BinR), the backward
// schedules' names, a ray and its points, the saved feature / ReLU-mask cache, encode_tile, and
// the few device helpers both backward schedules use (DPP row shifts,
// voxel_cw, the exact-zero test, the sticky device fault word).
#pragma once
#include "hn_mlp.h"
#include "hn_render.h"
#include "hn_loss.h"
#include "hn_tv.h"

#include <type_traits>

namespace hn {

// levels per scheduling group of the forward's encode (8 gathers each):
// 1 level 0.2674, 2 levels 0.2666, 4 levels 0.2696 ms (r04z)
constexpr int kEncGroup = 2;

constexpr int kSc = 64, kNi = 128, kSf = 192;
// The second fine-pass shape (hn_render_cfg.n_importance = 64, the LLFF
// configurations): 128 fine samples = 4 tiles = 8 groups of 16.  The caller's
// per-ray tensors take its strides; the workspace (d raw, marks, lists, fine
// feature grads) and the feature cache keep the 64 + 128 strides, their tails
// unused.
constexpr int kNi64 = 64, kSf64 = kSc + kNi64;
constexpr int kFwdWaves = 4;
constexpr int kBwdBlocks = 256;          // persistent backward: one block per CU

// The field and the sampling: the part RenderK and ImageK share (field_args,
// hn_render.hip), and what the shared ray passes of hn_render_fwd.h read
struct FieldK {
  GridArgs g;
  int white, lindisp;
  const float* tvals;
  const float* u;
  const float* table;
  const float* Pc;   // the two nets' packed weights
  const float* Pf;
};

struct RenderK {
  FieldK f;
  int perturb;
  int64_t B;
  const float *rays, *t_rand, *noise_c, *noise_f;
  float *rgb, *depth, *acc, *sparsity, *rgb0, *depth0, *acc0, *sparsity0, *z_std;
  float *z_coarse, *z_fine, *raw_c, *raw_f;
  uint8_t* fine_src;
  float* feat;    // [B][8 tiles][1024] saved features or NULL
  int feat_nt;    // saved features stored nontemporally (tables past the MALL)
  int skip_dead;  // hn_render_fwd_args.skip_dead_color
  // render_fwd_kernel<true> (hn_render_fwd_args.loss): the training loss's
  // composite backward done by the ray's own forward wave -- hn_loss_bwd's
  // factors (g = 1) and the workspace's d raw, marks and stamp (B1K's)
  const float* ltarget;
  float lgm, lsparse;
  float* draw;
  uint8_t* uflags;
  unsigned long long* stamp;
};


// Arguments of the backward MLP kernel (kept lean: every field lives in SGPRs).
struct B1K {
  int64_t B;
  int32_t scramble;     // Feistel half-width of the chunk-position -> ray permutation, 0: identity
  int white;
  const float* rays;
  const float *noise_c, *noise_f;
  const float *Pc, *Pf;
  const float *z_coarse, *z_fine, *raw_c, *raw_f;
  const float* feat;
  const float *g_rgb, *g_depth, *g_acc, *g_sparsity, *g_rgb0, *g_depth0, *g_acc0, *g_sparsity0;
  const float* g_raw_f;
  float* slab;
  float* dfeat;         // [B][64][32] coarse-pass feature grads ([f][level] per point)
  float* draw;          // [B][64 + 192][4] d raw of every sample (composite pre-pass)
  // fine kernel: trilinear backward + scatter into the table gradient
  GridArgs g;
  const uint8_t* fine_src;
  float* d_table;
  // binned scatter (bin_geom): record buffer base, records per (block, bin),
  // log2 entries per bin, bins
  float* bins;
  int32_t bin_cap, bin_shift, nbins;
  float* dfeat_f;       // split backward: [B][6 fine tiles][1024] fine-pass feature grads (tile order)
  // ABI 13 training loss formed by the composite pre-pass (hn_render_loss;
  // lout NULL = none): hn_loss_bwd's upstream factors (g = 1), the value's inputs
  const float *ltarget, *lrgb, *lrgb0, *lsp, *lsp0, *ltv;
  int32_t n_tv;
  float lgm, lsparse, lworld, lsparse_w, ltv_w;
  float* lout;
  int32_t skip_zero;    // exact-zero skipping (!hn_render_cfg.dense_bwd)
  int32_t sf;           // fine samples per ray (kSf or kSf64): the stride of z_fine, raw_f, noise_f,
                        // g_raw_f, fine_src (the pre-pass, the lists' dense word)
  uint8_t* uflags;      // [B][kMarkB] marks (composite pre-pass): [0] coarse, [1] fine MLP tiles with a
                        // nonzero d raw -- as bits: 0-3 coarse 16-sample groups, 8-19 fine
                        // groups (the MLP backward's), 20-31 fine groups with a nonzero sample or
                        // coarse twin (the scatter's); sf = kSf64: 8 fine groups, bits 8-15 and 20-27
  int32_t* lmeta;       // work lists (render_lists_kernel): [0] coarse tiles, [1] fine tiles, [2] scatter
                        // tiles, [3] gsplit: the MLP waves g < gsplit run coarse tiles (slab_reduce_block)
  int32_t* lists;       // group codes (ray << 4 | group): coarse [4B] | fine [12B] | the scatter's [12B]
};

// Backward schedules (render_bwd_kernel MODE; bwd_plan picks one per call):
//   kModeSplit   binned (hn_bwd_binned.h): the MLP backward over work lists stores the feature
//                grads, a scatter kernel turns them into records per bin, an owner pass sums each
//                bin exactly.  Every benchmark line.
//   kModeAtomic  float-atomic, fused (hn_bwd_atomic.h): MLP waves hand each fine tile through an
//                LDS ring to a scatter wave issuing float atomics.  The only schedule for T > 22
//                and for grids whose cell index does not fit a bin.
enum : int { kModeAtomic = 0, kModeSplit = 2 };
// render_bwd_kernel's CAP: the atomic wave-instructions the scatter wave of
// the atomic schedule may have in flight, and the cap for a table beyond the
// MALL (measured at scatter_level_x, hn_bwd_atomic.h).  The binned
// instantiation is <kSwVmcnt, kModeSplit> and issues no atomics.
constexpr int kSwVmcnt = 8, kSwVmcntBig = 4;

struct Ray {
  float o[3], d[3], vd[3], near, far, dnorm;
};

// A ray from its 11 floats [o | d | near far | viewdir]
HN_DEV void make_ray(const float* __restrict__ rb, Ray& r) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r.o[a] = rb[a];
    r.d[a] = rb[3 + a];
    r.vd[a] = rb[8 + a];
  }
  r.near = rb[6];
  r.far = rb[7];
  r.dnorm = sqrtf(r.d[0] * r.d[0] + r.d[1] * r.d[1] + r.d[2] * r.d[2]);   // torch.norm (:595)
}
HN_DEV void load_ray(const float* __restrict__ rays, int64_t ray, Ray& r) { make_ray(rays + 11 * ray, r); }

// pts = rays_o + rays_d * z (:538, :552)
HN_DEV void ray_point(const Ray& r, float z, float pt[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) pt[a] = r.o[a] + r.d[a] * z;
}

// Saved features: tile t of a ray (t = 0,1 coarse, 2..7 fine) is 1024 floats,
// stored as 4 chunks of [64 lanes][float4] so that both the forward's store
// and the backward's load are fully coalesced dwordx4 accesses.
// After the 8 feature tiles: the tiles' ReLU masks of the two networks (tile
// t: 3 words [h0 | c0 | c1] x 64 lanes, bit 16 ob + r = D register r of
// output block ob of the lane), written by the forward.
constexpr int kTilesPerRay = (kSc + kSf) / 32;
constexpr int kMaskWordsPerTile = 3 * 64;
static_assert(kTilesPerRay * (1024 + kMaskWordsPerTile) == HN_RENDER_FEAT_PER_RAY, "feature cache layout");

// The forward stores its ReLU masks and the backward's forward recompute
// uses them with 2-part products (kSplitR = 2): the recomputed
// activations then differ from the forward's by ~2^-17 relative (the dW
// operands' own precision), but every ReLU decision is the forward's.

HN_DEV void store_masks(float* __restrict__ base, int64_t ray, int tile, int lane, const uint32_t (&m)[3], bool nt) {
  uint32_t* t = reinterpret_cast<uint32_t*>(base + (size_t)ray * HN_RENDER_FEAT_PER_RAY + kTilesPerRay * 1024) +
                tile * kMaskWordsPerTile;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (nt) __builtin_nontemporal_store(m[j], t + 64 * j + lane);
    else t[64 * j + lane] = m[j];
  }
}
HN_DEV void load_masks(const float* __restrict__ base, int64_t ray, int tile, int lane, uint32_t (&m)[3]) {
  const uint32_t* t = reinterpret_cast<const uint32_t*>(base + (size_t)ray * HN_RENDER_FEAT_PER_RAY +
                                                        kTilesPerRay * 1024) + tile * kMaskWordsPerTile;
#pragma unroll
  for (int j = 0; j < 3; ++j) m[j] = __builtin_nontemporal_load(t + 64 * j + lane);
}
HN_DEV void store_feat(float* __restrict__ base, int64_t ray, int tile, int lane, const f32x16& feat, bool nt) {
  f32x4* t = reinterpret_cast<f32x4*>(base + (size_t)ray * HN_RENDER_FEAT_PER_RAY + (size_t)tile * 1024);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const f32x4 v = {feat[4 * c], feat[4 * c + 1], feat[4 * c + 2], feat[4 * c + 3]};
    if (nt) __builtin_nontemporal_store(v, t + 64 * c + lane);
    else t[64 * c + lane] = v;
  }
}

HN_DEV void load_feat(const float* __restrict__ base, int64_t ray, int tile, int lane, f32x16& feat) {
  const f32x4* t = reinterpret_cast<const f32x4*>(base + (size_t)ray * HN_RENDER_FEAT_PER_RAY + (size_t)tile * 1024);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const f32x4 v = __builtin_nontemporal_load(t + 64 * c + lane);
    feat[4 * c] = v.x; feat[4 * c + 1] = v.y; feat[4 * c + 2] = v.z; feat[4 * c + 3] = v.w;
  }
}

// grid sizes [16][3] staged in LDS (saves 48 SGPRs), then their reciprocals
constexpr int kGsRcp = 48, kGsLds = 96;

// Hash-encode one point into the 32-feature tile layout (lane half h owns
// levels tile_level(m, h), m = 0..7).  hash_encoding.py:84-110.
HN_DEV void encode_tile(const GridArgs& g, const float* gsl, const float* __restrict__ table, const float pt[3], int h,
                        f32x16& feat) {
  // (Software-pipelining the levels -- level m + 1 or m + 2's gathers issued
  // before level m's are consumed -- measured slower: render_fwd_kernel 0.310
  // -> 0.330 / 0.323 ms, r04b; the other three waves of the SIMD already hide
  // the gathers' latency.  Loading a level's x-pairs as 16-B buffer loads
  // where both corners share an aligned pair of rows (4 + 4 loads instead
  // of 8) measured 0.2777 vs 0.2823 ms before the coarse-twin reuse, and
  // 0.2789 vs 0.2731 ms after it (r04h, r04l): not kept.)
  float xc[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) xc[a] = clamp_t(pt[a], g.bmin[a], g.bmax[a]);
  const uint32_t mask = (1u << g.log2T) - 1u;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int l0 = tile_level(m, 0), l1 = tile_level(m, 1);
    const uint32_t l = h ? l1 : l0;
    const float gs[3] = {gsl[3 * l], gsl[3 * l + 1], gsl[3 * l + 2]};
    const float rg[3] = {gsl[kGsRcp + 3 * l], gsl[kGsRcp + 3 * l + 1], gsl[kGsRcp + 3 * l + 2]};
    Voxel v;
    voxel_level_rcp(pt, xc, gs, rg, g.bmin, mask, v);
    float f0, f1;
    encode_level_off(table, l << g.log2T, v, f0, f1);
    feat[2 * m] = f0;
    feat[2 * m + 1] = f1;
    if ((m & (kEncGroup - 1)) == kEncGroup - 1) __builtin_amdgcn_sched_barrier(0);   // <= 8 x kEncGroup gathers in flight
  }
}

// shx8 (the backward's dW_c0 staging) only where it is asked for
HN_DEV void ray_sh(const Ray& r, int h, float sh8[8], float* shx8 = nullptr) {
  float sh[16];
  sh16(r.vd[0], r.vd[1], r.vd[2], sh);
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    sh8[s] = h ? sh[2 * s + 1] : sh[2 * s];
    if (shx8) shx8[s] = h ? sh[8 + s] : sh[s];
  }
}


HN_DEV void stage_grid_sizes(const GridArgs& g, float* gsl) {
  if (threadIdx.x < 48) {
    const float gs = g.gs[threadIdx.x / 3][threadIdx.x % 3];
    gsl[threadIdx.x] = gs;
    gsl[kGsRcp + threadIdx.x] = 1.f / gs;
  }
}

// ---- helpers of both backward schedules -----------------------------------
// DPP row shifts; lanes whose source is outside the row read 0 (bound_ctrl),
// which lets the compiler fold the shift into the consuming VALU op.
template <int CTRL>
HN_DEV uint32_t dpp_u(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, true);
}
template <int CTRL>
HN_DEV float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xf, 0xf, true));
}
constexpr int kRowShr1 = 0x111;              // lane i <- lane i-1 within its row
template <int D> constexpr int kRowShl = 0x100 + D;   // lane i <- lane i+D within its row

// Voxel of one (point, level) for the scatter: cell corner index and
// trilinear weights in the op order of hash_encoding.py:62-72 / :130-140.
HN_DEV void voxel_cw(const GridArgs& g, const float* gsl, const float pt[3], const float xc[3], int l,
                     int32_t cell[3], float w[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float gs = gsl[3 * l + a];
    const float q = (xc[a] - g.bmin[a]) / gs;   // exact IEEE divisions
    const int32_t i = (int32_t)floorf(q);
    const float vmin = (float)i * gs + g.bmin[a];
    const float vmax = vmin + gs;
    w[a] = (pt[a] - vmin) / (vmax - vmin);
    cell[a] = i;
  }
}

// Sticky device fault word (hn_device_faults), shared by the atomic kernel,
// the scatter kernel and the owner pass: a bounded wait that runs out, a
// record that finds no room, a non-finite record input or a gradient on a
// dead row sets its bit, so the host sees an error, never a hung GPU or
// silently partial gradients.
// kFaultNonFinite: a record input (feature grad or sample point) was NaN / Inf.
// The fixed-point owner pass cannot carry such a value (the reference's
// autograd would propagate it into embeddings[l].grad, hash_encoding.py:106),
// so the gradient of that launch is flagged invalid instead of silently
// dropping the contribution.
__device__ int g_hn_fault;
enum : int { kFaultSlot = 1, kFaultDrain = 2, kFaultCoarse = 4, kFaultDwBuf = 8 };
enum : int { kFaultBins = 16, kFaultNonFinite = 32, kFaultDeadRow = 64 };
// kFaultPrepass: hn_render_bwd_args.prepass_done without a training forward
// of the same n_rays on this workspace since the last backward (no stamp).
enum : int { kFaultPrepass = 128 };
HN_DEV void raise_fault(int bit) {
  if (lane_id() == 0) __hip_atomic_fetch_or(&g_hn_fault, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr int kMarkB = 4;   // unit-mark bytes per ray (B1K::uflags)
// Samples with d raw = 0 (relu(sigma) = 0) have no gradient at all: the
// binned schedule skips their MLP tiles, their feature grads and their zero
// records (render_lists_kernel, scatter_bins_kernel), unless
// hn_render_cfg.dense_bwd asks for every sample to be computed (B1K / ScK
// skip_zero = 0).
HN_DEV bool draw_nonzero(const float4& d) {
  return ((__float_as_uint(d.x) | __float_as_uint(d.y) | __float_as_uint(d.z) | __float_as_uint(d.w)) << 1) != 0u;
}

// ---- the composite backward of one ray's pass, shared by the pre-pass
// (render_comp_bwd_kernel) and the training forward (render_fwd_kernel<true>)
// The training loss's upstream gradients of a pass with outputs rgb
// (hn_loss_bwd_elem's op forms, g_loss = 1): lgm 2 (rgb - target), lsparse.
HN_DEV void loss_comp_grad(CompGrad& g, float lgm, float lsparse, float r0, float r1, float r2,
                           const float* __restrict__ target) {
  g.has_rgb = g.has_entropy = true;
  g.has_acc = g.has_depth = false;
  g.rgb[0] = lgm * (2.f * (r0 - target[0]));
  g.rgb[1] = lgm * (2.f * (r1 - target[1]));
  g.rgb[2] = lgm * (2.f * (r2 - target[2]));
  g.acc = g.depth = 0.f;
  g.entropy = lsparse;
}
// Bits 4 i .. 4 i + 3: the 16-lane quarters of a wave ballot that have a set bit
// (the 16-sample groups of samples 64 i .. 64 i + 63).
HN_DEV uint32_t group_bits(uint64_t b, int i) {
  uint32_t v = 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q) v |= (((b >> (16 * q)) & 0xffffull) != 0ull ? 1u : 0u) << (4 * i + q);
  return v;
}
// A pass's d raw (S samples in LDS) stored to the workspace; returns its MLP
// marks: bit t = a sample of 16-sample group t has a nonzero d raw.
HN_DEV uint32_t draw_store_marks(const float* rawb, float* __restrict__ dst, int S, int lane) {
  uint32_t nzu = 0u;
  for (int j = lane; j < S; j += 64) {
    const float4 d = *reinterpret_cast<const float4*>(rawb + 4 * j);
    *reinterpret_cast<float4*>(dst + 4 * j) = d;
    nzu |= group_bits(__ballot(draw_nonzero(d)), j >> 6);
  }
  return nzu;
}
// The coarse pass's nonzero-sample mask (bit s: coarse sample s).
HN_DEV unsigned long long coarse_nonzero_mask(const float* rawb, int lane) {
  return __ballot(draw_nonzero(*reinterpret_cast<const float4*>(rawb + 4 * lane)));
}
// The scatter's marks of a ray: bit t = a sample of fine group t, or its
// coarse twin (the same point, fine_src < 64; cm = coarse_nonzero_mask), has a
// nonzero d raw -- the group has feature grads to scatter.  kS: the ray's fine samples.
template <int kS = kSf>
HN_DEV uint32_t scatter_marks(const float* rawb, const uint8_t* __restrict__ fine_src, unsigned long long cm,
                              int lane) {
  uint32_t su = 0u;
  for (int j = lane; j < kS; j += 64) {
    const int src = fine_src[j];
    const bool nz = draw_nonzero(*reinterpret_cast<const float4*>(rawb + 4 * j)) ||
                    (src < kSc && ((cm >> src) & 1ull) != 0ull);
    su |= group_bits(__ballot(nz), j >> 6);
  }
  return su;
}
// Mark bytes 1-3 of a ray (bits 8-19: the fine MLP groups nzf, 20-31: the
// scatter's groups su); byte 0 is the coarse pass's MLP groups.  A 128-sample
// fine pass has 8 groups: bits 8-15 and 20-27, the others stay 0.
HN_DEV void store_fine_marks(uint8_t* __restrict__ uflags, int64_t ray, uint32_t nzf, uint32_t su) {
  const uint32_t v = nzf | (su << 12);
  uflags[kMarkB * ray + 1] = (uint8_t)v;
  uflags[kMarkB * ray + 2] = (uint8_t)(v >> 8);
  uflags[kMarkB * ray + 3] = (uint8_t)(v >> 16);
}

// The training forward's stamp in the workspace: one 64-bit word in the spare
// words behind the lists' counts (B1K::lmeta[4..7]), n_rays << 32 |
// kStampToken; the token's low byte counts the workgroups of the backward's
// first kernel, which check it with one atomic add each -- the last one
// clears it (render_lists_kernel; hn_render_bwd_args.prepass_done).
constexpr int kStampAt = 4;
constexpr unsigned long long kStampToken = 0x70726500ull, kStampCount = 0xffull;
HN_DEV constexpr unsigned long long stamp_word(int64_t n_rays) {
  return ((unsigned long long)n_rays << 32) | kStampToken;
}

// Arguments of scatter_bins_kernel (binned schedule).
struct ScK {
  GridArgs g;
  int64_t B;
  const float* rays;
  const float* z_fine;
  const uint8_t* fine_src;
  const float* dfeat_f;   // [B][6][1024] tile order (split render_bwd_kernel)
  const float* dfeat_c;   // [B][2][1024] tile order (coarse units of the split render_bwd_kernel)
  const float* draw;      // [B][64 + 192][4] d raw (composite pre-pass): zero = no feature grads to read
  int32_t scramble;       // the MLP backward's ray permutation (B1K::scramble; 0: identity)
  int32_t skip_zero;      // exact-zero skipping (!hn_render_cfg.dense_bwd)
  const int32_t* lmeta;   // render_lists_kernel's counts ([2] scatter groups, [3] the MLP waves' split)
  const int32_t* slist;   // its scatter group codes (ray << 4 | 16-sample group), or null: every unit
  float* bins;
  int32_t bin_cap, bin_shift, nbins;
  // TV term (loss.py:11-43) as records of the same bins: tv_off[l] = first
  // x-pair of level l (tv_off[L] pairs in all; 0 = no TV term), split evenly
  // over the blocks after their units
  int32_t tv_off[17];
  const float* g_tv;
  TvK tv;
  // The blocks then reduce the MLP backward's dW slabs (the
  // slab_reduce_kernel launch folded into this one; same per-element sums)
  const float* slab;       // NULL: no slab reduction here
  hn_mlp_grad dc, df;
  int32_t overwrite_mlp;
  int32_t has_mstep;       // the NeRFSmall tensors' RAdam steps run in the slab reduction (mstep)
  hn_radam_tensor mstep[10];
};

// Arguments of the binned schedule's overflow placement and owner pass
// (ovf_place_kernel, bin_reduce_kernel).
struct BinR {
  const float* bins;
  int64_t n_rays;
  int32_t nbins, cap, shift, log2T;
  float* d_table;          // or NULL (fused step only)
  int32_t overwrite;
  int32_t fused;           // 1: apply `step` to the table (p, m, v) with the bin's gradient
  hn_radam_tensor step;
  const uint32_t* live;    // fused step: live row pairs of levels < live_levels (hn_render_bwd_args.table_live)
  int32_t live_levels;
  int32_t bin0;            // first bin of the launch (hn_render_bwd_owner ranges)
};

}  // namespace hn

