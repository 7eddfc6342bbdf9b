// hn_render_fwd.h -- render_fwd_kernel: the whole forward of one training ray
// batch (run_nerf_helpers.py:464-574), one wave64 per ray, 4 waves per SIMD.
// Coarse z (linspace + stratified jitter) -> 2 coarse tiles of 32 points
// (hash-encode 16 levels + NeRFSmall on MFMA, the weight fragments through a
// per-wave LDS ring) -> composite -> sample_pdf 128 -> merge of the sorted
// runs (192) -> 6 fine tiles (a coarse sample's features reused) ->
// composite.  Saves each tile's features and ReLU masks for the backward,
// except (skip_dead) those of fine tiles without density.
#pragma once
#include "hn_render_args.h"

// The forward's waves raise their issue priority (s_setprio) while they
// encode: a wave that is issuing gathers gets its requests out ahead of the
// SIMD's other waves, whose MLP phases then overlap the gathers' latency.
// Measured (r04x, config 2, two runs each): render_fwd_kernel 0.2743 ->
// 0.2673 ms at priority 1 (0.2671 at 2), step 1.005 / 1.000 -> 0.993 / 0.994
// ms; scheduling only, so every result is unchanged.
#define HN_FWD_PRIO_HI() __builtin_amdgcn_s_setprio(1)
#define HN_FWD_PRIO_LO() __builtin_amdgcn_s_setprio(0)

namespace hn {

// LDS per forward wave (floats).
constexpr int kFZc = 0, kFZsrc = 64, kFZs = 256, kFRaw = 448, kFW = 1216, kFBins = 1280,
              kFCdf = 1344, kFC0 = 1408, kFLds = 1472;

// 4 waves per SIMD (<= 128 registers; the few spills sit outside the tile
// loops): one ray per wave, so a 4096-ray batch is exactly one round on 256
// CUs (3 waves: 0.427 ms, a 1/3-occupied second round; 4: 0.418 ms)
constexpr int kFwdWavesPerSimd = 4;

// (Round 4 measured 16-wave workgroups with each net's forward weight
// fragments staged in LDS instead of streamed from L2 per tile: the MLP phase
// ran ~3x faster but the gathers of 16 waves in step ~2.3x slower,
// render_fwd_kernel 0.294 vs 0.281 ms, and staggering half of the waves made it
// 0.301-0.313 ms; profiles/r04/r04e, r04f.)
constexpr int kFwdBlockWaves = kFwdWaves;


// One pass's composite.  kLoss: then also the training loss's composite
// backward from the same samples and totals (composite_bwd's two halves, so
// the d raw are the pre-pass's bit for bit), written over raw in LDS.
template <bool kLoss, int N>
HN_DEV void composite_pass(const RenderK& k, int64_t ray, float* rawb, const float* z, const float* noise, int S,
                           float dnorm, float* wout, CompOut& o, int lane) {
  if constexpr (!kLoss) {
    composite_fwd<N>(rawb, z, noise, S, dnorm, k.white != 0, wout, o, lane);
  } else {
    // (the ray's target colour asked for ahead of the composite that hides its latency)
    const float target[3] = {k.ltarget[3 * ray], k.ltarget[3 * ray + 1], k.ltarget[3 * ray + 2]};
    CompSamples<N> cs;
    composite_samples<N>(rawb, z, noise, S, dnorm, cs, lane);
    CompTotals t;
    composite_totals<N>(cs, t);
    composite_fwd_out<N>(cs, t, k.white != 0, wout, o, lane);
    CompGrad g;
    loss_comp_grad(g, k.lgm, k.lsparse, o.rgb[0], o.rgb[1], o.rgb[2], target);
    composite_bwd_raw<N>(cs, t, k.white != 0, g, nullptr, nullptr, rawb, lane);
    lds_fence_wave();
  }
}

// kLoss (hn_render_fwd_args.loss, the trainer's step): the wave also runs the
// composite backward of its ray's two passes on the raw / z it holds in LDS
// -- what render_comp_bwd_kernel would read back from memory, and the samples
// and totals its composite forward has just formed -- and writes the ray's d
// raw and marks into the backward's workspace (the binned schedule then
// launches no pre-pass).  Both passes' composites sit outside the tile loops.
// kLoss = false compiles to the forward without any of it.
template <bool kLoss>
__global__ __launch_bounds__(64 * kFwdBlockWaves)
__attribute__((amdgpu_waves_per_eu(kFwdWavesPerSimd, kFwdWavesPerSimd)))
void render_fwd_kernel(RenderK k) {
  __shared__ __attribute__((aligned(16))) float smem[kFwdBlockWaves * kFLds + kGsLds];
  // each wave's split-GEMM fragments one chunk ahead (FragRing, hn_mlp.h):
  // render_fwd_kernel 0.271 -> 0.266 ms, r05 ring (bitwise-identical outputs)
  __shared__ __attribute__((aligned(16))) float fring[kFwdBlockWaves][768];
  // the wave index (and with it the ray, its 11 floats and every per-ray
  // address) on the scalar unit: VGPR spills 45 -> 22, render_fwd_kernel
  // 0.296 -> 0.281 ms (r04e)
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int p = lane & 31, h = lane >> 5;
  float* gsl = smem + kFwdBlockWaves * kFLds;
  stage_grid_sizes(k.g, gsl);
  __syncthreads();
  // XCD-aware: workgroup b runs on XCD b % 8, so consecutive ray groups of a
  // spatially ordered batch go to one XCD and share its L2
  const int64_t nb = gridDim.x;
  // (round 6, r06k: chunks of 4 or 16 ray groups dealt round-robin over the
  // XCDs, or no XCD mapping at all, were no faster: 234.9 / 228.8 / 240.4 us
  // against 229.4 us -- the forward's per-XCD work is balanced already)
  const int64_t grp = nb % 8 == 0 ? (blockIdx.x % 8) * (nb / 8) + blockIdx.x / 8 : blockIdx.x;
  const int64_t ray = grp * kFwdBlockWaves + wave;
  if constexpr (kLoss) {
    // the stamp render_lists_kernel checks: d raw and marks of these n_rays follow
    if (blockIdx.x == 0 && threadIdx.x == 0) *k.stamp = stamp_word(k.B);
  }
  if (ray >= k.B) return;
  float* L = smem + wave * kFLds;
  float* zc = L + kFZc;
  float* zsrc = L + kFZsrc;
  float* zs = L + kFZs;
  float* rawb = L + kFRaw;
  float* wts = L + kFW;
  float* bins = L + kFBins;
  float* cdf = L + kFCdf;
  Ray r;
  load_ray(k.rays, ray, r);
  float sh8[8], shx8[8];
  float* c0l = L + kFC0;

  // ---- coarse z_vals (:514-536) ----
  auto zlin = [&](int i) {
    const float t = k.tvals[i];
    return k.lindisp ? 1.f / (1.f / r.near * (1.f - t) + 1.f / r.far * t)
                     : r.near * (1.f - t) + r.far * t;
  };
  float z = zlin(lane);
  if (k.perturb) {
    const float zm = lane > 0 ? zlin(lane - 1) : z;
    const float zp = lane < kSc - 1 ? zlin(lane + 1) : z;
    const float lower = lane > 0 ? .5f * (z + zm) : z;
    const float upper = lane < kSc - 1 ? .5f * (zp + z) : z;
    z = lower + (upper - lower) * k.t_rand[ray * kSc + lane];
  }
  zc[lane] = z;
  zsrc[lane] = z;
  k.z_coarse[ray * kSc + lane] = z;
  ray_sh(r, h, sh8, shx8);
  lds_fence_wave();

  // ---- coarse network (:540) ----
  c0sh_lds_store(opaque_ptr(k.Pc), sh8, c0l, lane);
  lds_fence_wave();
  fwd_ring_start(k.Pc, fring[wave], lane);
  for (int tau = 0; tau < kSc / 32; ++tau) {
    const float* P = opaque_ptr(k.Pc);
    const int q = 32 * tau + p;
    float pt[3];
    ray_point(r, zc[q], pt);
    f32x16 feat;
    HN_FWD_PRIO_HI();
    encode_tile(k.g, gsl, k.table, pt, h, feat);
    HN_FWD_PRIO_LO();
    if (k.feat) store_feat(k.feat, ray, tau, lane, feat, k.feat_nt != 0);
    MlpAct a;
    f32x16 c2;
    mlp_fwd_tile_src<true>(FragRing{P, fring[wave]}, feat, [&](int ob) { return c0sh_lds_load(c0l, ob, lane); },
                           a, c2, lane, k.skip_dead && k.noise_c == nullptr);
    if (k.feat) store_masks(k.feat, ray, tau, lane, a.m, k.feat_nt != 0);
    if (h == 0) {
      const float4 o4 = make_float4(c2[0], c2[1], c2[2], a.s1[0]);
      *reinterpret_cast<float4*>(rawb + 4 * q) = o4;
      *reinterpret_cast<float4*>(k.raw_c + (ray * kSc + q) * 4) = o4;
    }
  }
  lds_fence_wave();
  CompOut co;
  composite_pass<kLoss, kSc / 64>(k, ray, rawb, zc, k.noise_c ? k.noise_c + ray * kSc : nullptr, kSc, r.dnorm, wts,
                                  co, lane);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) k.rgb0[3 * ray + c] = co.rgb[c];
    k.depth0[ray] = co.depth;
    k.acc0[ray] = co.acc;
    k.sparsity0[ray] = co.entropy;
  }
  // kLoss: rawb now holds the coarse pass's d raw (it is free until the fine
  // tiles; wts stays intact for sample_pdf_wave)
  unsigned long long cmask = 0ull;   // the coarse samples with a nonzero d raw
  if constexpr (kLoss) {
    const uint32_t nzu = draw_store_marks(rawb, k.draw + (size_t)ray * (kSc + kSf) * 4, kSc, lane);
    if (lane == 0) k.uflags[kMarkB * ray] = (uint8_t)nzu;   // byte 0: the coarse groups
    cmask = coarse_nonzero_mask(rawb, lane);
  }

  // ---- importance sampling (:547-551) ----
  if (lane < kSc - 1) bins[lane] = .5f * (zc[lane + 1] + zc[lane]);
  lds_fence_wave();
  sample_pdf_wave(bins, wts + 1, kSc - 2, cdf, k.u + ray * kNi, kNi, zsrc + kSc, lane);
  lds_fence_wave();
  {
    const float s0 = zsrc[kSc + lane], s1 = zsrc[kSc + 64 + lane];
    const double mean = wave_sum((double)s0 + (double)s1) / kNi;
    const double d0 = (double)s0 - mean, d1 = (double)s1 - mean;
    const double var = wave_sum(d0 * d0 + d1 * d1) / kNi;
    if (lane == 0) k.z_std[ray] = (float)sqrt(var);
  }
  // sort(cat(z_vals, z_samples)) (:551): a merge of the sorted coarse run with
  // the bitonic-sorted importance samples (rawb is free until the fine tiles),
  // the all-pairs rank sort if the coarse run is ever out of order
  // (render_fwd_kernel 0.2998 -> 0.2966 ms, r04c)
  uint8_t* org = k.fine_src + ray * kSf;
  if (!merge_sort_z(zsrc, zs, rawb, lane, org)) rank_sort_wave(zsrc, zs, kSf, lane, org, kSc);
  for (int i = lane; i < kSf; i += 64) k.z_fine[ray * kSf + i] = zs[i];

  // ---- fine network (:556) ----
  c0sh_lds_store(opaque_ptr(k.Pf), sh8, c0l, lane);   // the coarse tiles' reads are done (in-order LDS)
  lds_fence_wave();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the coarse ring's last (unused) fill has landed
  fwd_ring_start(k.Pf, fring[wave], lane);
  // kLoss: the samples' coarse origins kept in LDS for the marks (zsrc is free
  // after the merge), read beside the first fine tile's own look at them
  uint8_t* srcl = reinterpret_cast<uint8_t*>(zsrc);
  if constexpr (kLoss) {
    for (int i = lane; i < kSf; i += 64) srcl[i] = k.fine_src[ray * kSf + i];
    lds_fence_wave();
  }
  for (int tau = 0; tau < kSf / 32; ++tau) {
    const float* P = opaque_ptr(k.Pf);
    const int q = 32 * tau + p;
    float pt[3];
    ray_point(r, zs[q], pt);
    f32x16 feat;
    // a third of the fine samples are the coarse samples again (the merge
    // keeps their z bitwise): with the feature cache present, those lanes load
    // the coarse tile's features (4 dwordx4, written by this wave) instead of
    // gathering 16 levels x 8 corners again -- a quarter of the ray's gathers
    // (render_fwd_kernel 0.282 -> 0.275 ms, r04h).  Encoding only the 128
    // importance samples as 4 full tiles first and loading every fine tile's
    // features back from the cache (a third fewer encode instructions) measured
    // slower: 0.301 ms, the waves then run their MLP tiles in step (r04j).
    // (kLoss: from the LDS copy -- no global round trip ahead of each tile's gathers)
    const int src = !k.feat ? 255 : kLoss ? (int)srcl[q] : (int)k.fine_src[ray * kSf + q];
    if (src >= kSc) {
      HN_FWD_PRIO_HI();
      encode_tile(k.g, gsl, k.table, pt, h, feat);
      HN_FWD_PRIO_LO();
    } else {
      const f32x4* t = reinterpret_cast<const f32x4*>(k.feat + (size_t)ray * HN_RENDER_FEAT_PER_RAY +
                                                      (size_t)(src >> 5) * 1024) + (src & 31) + 32 * h;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x4 v = t[64 * c];
        feat[4 * c] = v.x; feat[4 * c + 1] = v.y; feat[4 * c + 2] = v.z; feat[4 * c + 3] = v.w;
      }
    }
    MlpAct a;
    f32x16 c2;
    // skip_dead: a fine tile without density has no nonzero d raw, so the
    // binned backward (dense_bwd = 0: its work lists) never reads its
    // features or masks -- they are not stored
    const bool dead_skip = k.skip_dead && k.noise_f == nullptr;
    bool stored = !dead_skip;
    if (k.feat && stored) store_feat(k.feat, ray, kSc / 32 + tau, lane, feat, k.feat_nt != 0);
    mlp_fwd_tile_src<true>(FragRing{P, fring[wave]}, feat, [&](int ob) { return c0sh_lds_load(c0l, ob, lane); },
                           a, c2, lane, dead_skip, [&]() {
                             if (k.feat && !stored) store_feat(k.feat, ray, kSc / 32 + tau, lane, feat, k.feat_nt != 0);
                             stored = true;
                           });
    if (k.feat && stored) store_masks(k.feat, ray, kSc / 32 + tau, lane, a.m, k.feat_nt != 0);
    if (h == 0) {
      const float4 o4 = make_float4(c2[0], c2[1], c2[2], a.s1[0]);
      *reinterpret_cast<float4*>(rawb + 4 * q) = o4;
      *reinterpret_cast<float4*>(k.raw_f + (ray * kSf + q) * 4) = o4;
    }
  }
  lds_fence_wave();
  CompOut fo;
  composite_pass<kLoss, kSf / 64>(k, ray, rawb, zs, k.noise_f ? k.noise_f + ray * kSf : nullptr, kSf, r.dnorm,
                                  nullptr, fo, lane);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) k.rgb[3 * ray + c] = fo.rgb[c];
    k.depth[ray] = fo.depth;
    k.acc[ray] = fo.acc;
    k.sparsity[ray] = fo.entropy;
  }
  if constexpr (kLoss) {   // the fine pass's d raw and the ray's marks
    const uint32_t nzf = draw_store_marks(rawb, k.draw + ((size_t)ray * (kSc + kSf) + kSc) * 4, kSf, lane);
    const uint32_t su = scatter_marks(rawb, srcl, cmask, lane);
    if (lane == 0) store_fine_marks(k.uflags, ray, nzf, su);
  }
}

}  // namespace hn

