// hn_render_fwd.h -- render_fwd_kernel: the whole forward of one training ray
// batch (run_nerf_helpers.py:464-574), one wave64 per ray, 4 waves per SIMD.
// Coarse z (linspace + stratified jitter) -> 2 coarse tiles of 32 points
// (hash-encode 16 levels + NeRFSmall on MFMA, the weight fragments through a
// per-wave LDS ring, or the sigma nets resident in LDS: the two forms below)
// -> composite -> sample_pdf 128 -> merge of the sorted
// runs (192) -> 6 fine tiles (a coarse sample's features reused) ->
// composite.  Saves each tile's features and ReLU masks for the backward,
// except (skip_dead) those of fine tiles without density.
//
// The ray passes -- coarse_z, pass_start, pass_tiles (one tile loop, coarse
// and fine), importance_sort -- are written once here, for this kernel and for
// render_image_kernel (hn_render_image.h), whose pixels are this forward's bit
// for bit.  What a kernel does with a tile's results is its compile-time
// policy (TrainTiles below, ImageTiles there).
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

// Two forms of render_fwd_kernel, bit for bit the same results (the MFMA
// products and their order are the same; only where a GEMM's A fragments come
// from differs):
//   ring (kRes = false): 4-wave workgroups, every split-GEMM chunk through the
//     wave's private 3-KiB LDS ring (FragRing), one buffer_load ... lds round
//     trip per chunk;
//   resident (kRes = true): 16-wave workgroups, one per CU.  The workgroup
//     gathers the resident image of both packed nets (the map at kResRegs,
//     hn_mlp.h: sigma_net.0, sigma_net.1, color_net.0's geo half and
//     color_net.2, the zero rows of sigma_net.1 and color_net.2 packed out;
//     2 x 25,728 B) into LDS once, ahead of the kernel's only barrier, and
//     those regions -- 14 of a tile's 22 chunks, and all of a tile without
//     density -- are read there (FragRes): no vmcnt wait, no refill, no
//     reload at the pass switch.  color_net.1's 8 chunks are loaded at use.
//     LDS: 16 x kFLds + kGsLds + kResImageFloats floats = 146,048 B (+ the
//     loss mode's 1,024 key bytes).
// (Round 4's whole-net-in-LDS form, one net at a time with a reload and a
// barrier at the pass switch, every tile 22 chunks, lost 0.294 to 0.281 ms:
// the 16 waves marched in step; profiles/r04/r04e, r04f.)
// hn_render_fwd picks the resident form where the batch fills the device with
// 16-ray workgroups (fwd_pick_form, hn_render.hip).
constexpr int kFwdBlockWaves = kFwdWaves;   // the ring form's workgroup
constexpr int kFwdResWaves = 16;            // the resident form's
constexpr int kFwdResRuns = 4;              // ... made of this many runs of consecutive rays (the note at `run`)
constexpr int fwd_block_waves(bool res) { return res ? kFwdResWaves : kFwdBlockWaves; }

// ---- which runs a resident workgroup takes (the note at `run`) -------------
// Workgroup b runs on XCD b % 8.  Where the deal applies (fwd_res_deal_on) the
// batch's runs are cut into segments of kFwdResSeg consecutive rays, XCD x
// owns the segments = x (mod 8), and the XCD's runs -- in batch order -- are
// stably sorted by descending key (0..kFwdResRunRays: the run's rays whose
// target is not the background, a stand-in for the colour net's work) and
// dealt in rounds over the XCD's nb / 8 workgroups, even rounds forward and
// odd rounds backward: workgroup b / 8 gets one run of each round, a heavy
// one where its previous was light.  Every other grid keeps the map of
// fwd_res_band_run.  The functions below are the whole rule, host and device:
// hn_render_fwd_deal (hn_render.hip) states it through them for the tests and
// the cost model, the kernel differs only in how it finds the run at a sorted
// position (fwd_res_select_wave: ballots instead of the scalar scan).
#ifndef HN_HOST_DEV
#define HN_HOST_DEV __host__ __device__ inline
#endif
constexpr int kFwdResRunRays = kFwdResWaves / kFwdResRuns;   // 4
constexpr int kFwdResSeg = 64;                                // rays per segment
constexpr int kFwdResSegRuns = kFwdResSeg / kFwdResRunRays;
constexpr int kFwdResXcds = 8;
// the keys of an XCD's runs sit in LDS, one byte each: grids up to 16 x this many rays
constexpr int kFwdResMaxRuns = 1024;
static_assert(kFwdResSeg % kFwdResRunRays == 0 && kFwdResMaxRuns % kFwdResSegRuns == 0, "whole runs per segment");

// the runs of an XCD's share (nb / 8 workgroups)
HN_HOST_DEV int fwd_res_xcd_runs(int64_t nb) { return (int)(nb / kFwdResXcds) * kFwdResRuns; }
// the deal applies: 8 equal shares, each a whole number of segments that fits the key array
HN_HOST_DEV bool fwd_res_deal_on(int64_t nb) {
  return nb > 0 && nb % kFwdResXcds == 0 && nb / kFwdResXcds <= kFwdResMaxRuns / kFwdResRuns &&
         fwd_res_xcd_runs(nb) % kFwdResSegRuns == 0;
}
// run j (batch order) of XCD x's share, as a run of the batch
HN_HOST_DEV int64_t fwd_res_xcd_run(int x, int j) {
  return ((int64_t)(j / kFwdResSegRuns) * kFwdResXcds + x) * kFwdResSegRuns + j % kFwdResSegRuns;
}
// the sorted position that slot s of the XCD's workgroup w (of nw) takes
HN_HOST_DEV int fwd_res_deal_pos(int nw, int w, int s) { return s * nw + (s & 1 ? nw - 1 - w : w); }
// the map without keys, and of every grid the deal does not apply to: the
// XCD's band of consecutive runs in quarters, one run from each (nb % 8 != 0:
// the batch in quarters)
HN_HOST_DEV int64_t fwd_res_band_run(int64_t nb, int64_t block, int s) {
  return nb % kFwdResXcds == 0
             ? (block % kFwdResXcds) * (nb / kFwdResXcds * kFwdResRuns) + s * (nb / kFwdResXcds) + block / kFwdResXcds
             : s * nb + block;
}
// the run (of nr, key_at(j) in 0..kFwdResRunRays) at position pos of the stable
// descending sort: the scalar statement
template <class KeyAt>
HN_HOST_DEV int fwd_res_select(int nr, int pos, KeyAt&& key_at) {
  int cnt[kFwdResRunRays + 1] = {};
  for (int j = 0; j < nr; ++j) ++cnt[key_at(j)];
  int b = kFwdResRunRays;
  for (; b > 0 && pos >= cnt[b]; --b) pos -= cnt[b];
  for (int j = 0; j < nr; ++j)
    if (key_at(j) == b && pos-- == 0) return j;
  return 0;   // (not reached: pos < nr)
}
// the run that slot s of workgroup `block` takes; select(nr, pos) = the XCD's
// run at a sorted position
template <class Select>
HN_HOST_DEV int64_t fwd_res_deal(int64_t nb, int64_t block, int s, Select&& select) {
  if (!fwd_res_deal_on(nb)) return fwd_res_band_run(nb, block, s);
  const int nw = (int)(nb / kFwdResXcds);
  return fwd_res_xcd_run((int)(block % kFwdResXcds),
                         select(fwd_res_xcd_runs(nb), fwd_res_deal_pos(nw, (int)(block / kFwdResXcds), s)));
}
// fwd_res_select by one wave, the keys in LDS: the five buckets counted with
// ballots, then the run whose bucket and rank within it are the position's.
// Two passes of ceil(nr / 64) steps, or the first alone where all keys are equal.
HN_DEV int fwd_res_select_wave(const uint8_t* keys, int nr, int pos, int lane) {
  int cnt[kFwdResRunRays + 1] = {};
  for (int base = 0; base < nr; base += 64) {
    const int key = base + lane < nr ? (int)keys[base + lane] : -1;
#pragma unroll
    for (int b = 0; b <= kFwdResRunRays; ++b) cnt[b] += __popcll(__ballot(key == b));
  }
  int b = kFwdResRunRays;
#pragma unroll
  for (int t = kFwdResRunRays; t > 0; --t)
    if (b == t && pos >= cnt[t]) {
      pos -= cnt[t];
      b = t - 1;
    }
  // (all runs alike -- no target equals the background, or all do: the sort keeps the batch's order)
  if (cnt[b] == nr) return __builtin_amdgcn_readfirstlane(pos);
  int found = 0, seen = 0;
  for (int base = 0; base < nr; base += 64) {
    const bool mine = base + lane < nr && (int)keys[base + lane] == b;
    const uint64_t m = __ballot(mine);
    const int before = seen + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const uint64_t hit = __ballot(mine && before == pos);
    if (hit) found = base + __builtin_ctzll(hit);
    seen += __popcll(m);
  }
  return __builtin_amdgcn_readfirstlane(found);
}

// ---- the ray passes, shared with render_image_kernel -----------------------
// L: the wave's kFLds floats (the map above), ring: its FragRing slot (kRes:
// the workgroup's resident image of the pass's net), gsl: the block's
// staged grid sizes.  A policy Pol, every hook inline (pass: 0 coarse,
// 1 fine, a constant at each call):
//   kMasks           the tiles' ReLU masks are formed
//   twins()          the ray's two stored coarse tiles (store_feat's layout), or null
//   origin(q)        fine sample q's coarse sample, or 255 (asked only with twins)
//   skip_dead(pass)  mlp_fwd_tile_src's skip_dead
//   save_feat(pass, tau, lane, feat), save_masks(pass, tau, lane, m), save_raw(pass, q, o4): the stores

// coarse z_vals (:514-536) before the jitter
HN_DEV float coarse_z(float t, float near, float far, int lindisp) {
  return lindisp ? 1.f / (1.f / near * (1.f - t) + 1.f / far * t) : near * (1.f - t) + far * t;
}

// A pass's prologue: color_net.0's SH half of the ray into LDS (the previous
// pass's tiles have read theirs: in-order LDS), the net's first chunk into the
// ring.  drain: the previous pass's last (unused) ring fill lands first.
// kRes: there is no ring to start; the one wait per pass stays (the ray's
// coarse tiles are stored before its fine pass loads the twins from them).
template <bool kRes = false>
HN_DEV void pass_start(const float* P, const float sh8[8], float* L, float* ring, int lane, bool drain) {
  c0sh_lds_store(opaque_ptr(P), sh8, L + kFC0, lane);
  lds_fence_wave();
  if (drain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (!kRes) fwd_ring_start(P, ring, lane);
}

// The coarse twin src of a fine sample: its features from the ray's stored
// coarse tiles (4 dwordx4, written by this wave)
HN_DEV void load_twin_feat(const float* tiles, int src, int h, f32x16& feat) {
  const f32x4* t = reinterpret_cast<const f32x4*>(tiles + (size_t)(src >> 5) * 1024) + (src & 31) + 32 * h;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const f32x4 v = t[64 * c];
    feat[4 * c] = v.x; feat[4 * c + 1] = v.y; feat[4 * c + 2] = v.z; feat[4 * c + 3] = v.w;
  }
}

// importance sampling (:547-551), then sort(cat(z_vals, z_samples)) (:551): a
// merge of the sorted coarse run with the bitonic-sorted importance samples
// (rawb is free until the fine tiles), the all-pairs rank sort if the coarse
// run is ever out of order (render_fwd_kernel 0.2998 -> 0.2966 ms, r04c).
// zsrc keeps the samples as drawn; org[i]: sorted sample i's coarse origin.
// kNiT: the importance samples, kNi or kNi64 (merge_sort_z's NI = 2 or 1 per lane).
template <int kNiT = kNi>
HN_DEV void importance_sort(float* L, const float* u, uint8_t* org, int lane) {
  static_assert(kNiT == kNi || kNiT == kNi64, "importance_sort: 128 or 64 importance samples");
  float* zsrc = L + kFZsrc;
  lds_fence_wave();
  sample_pdf_wave(L + kFBins, L + kFW + 1, kSc - 2, L + kFCdf, u, kNiT, zsrc + kSc, lane);
  lds_fence_wave();
  if (!merge_sort_z<kNiT / 64>(zsrc, L + kFZs, L + kFRaw, lane, org))
    rank_sort_wave(zsrc, L + kFZs, kSc + kNiT, lane, org, kSc);
}

// A pass's tiles: kPass 0 the coarse network (:540), 2 tiles at zc; 1 the fine
// network (:556), kFineT / 32 tiles at zs (6, or 4 with 64 importance samples)
template <int kPass, class Pol, int kFineT = kSf, bool kRes = false>
HN_DEV void pass_tiles(const FieldK& f, const float* gsl, float* ring, float* L, const Ray& r, int lane, Pol& pol) {
  const int p = lane & 31, h = lane >> 5;
  for (int tau = 0; tau < (kPass ? kFineT : kSc) / 32; ++tau) {
    const float* P = opaque_ptr(kPass ? f.Pf : f.Pc);
    // (the 4-tile fine pass only: the staged grid sizes' address laundered per
    // tile, so encode_tile's twelve per-lane LDS addresses are formed in the
    // tile, not held in VGPRs across the loop -- with them hoisted one value
    // was reloaded from scratch in every fine tile; now none is.  The 6-tile
    // instantiations of the ring form are untouched; the resident form's take
    // it too.)
    if constexpr (kPass && (kFineT != kSf || kRes)) {
      int zero = 0;
      asm volatile("" : "+s"(zero));
      gsl += zero;
    }
    // (the resident image's address likewise: the per-lane LDS addresses of
    // its regions are formed in the tile, against one base, instead of one
    // VGPR per 64-KiB window and lane pattern held across both tile loops;
    // and the lane of the feature, mask and raw stores and of the encode's
    // level offsets, whose per-lane addresses were otherwise held across the
    // loop and reloaded from scratch in every tile)
    int lane_s = lane;
    if constexpr (kRes) {
      int zero = 0;
      asm volatile("" : "+s"(zero));
      ring += zero;
      lane_s += zero;
    }
    const int q = 32 * tau + p;
    float pt[3];
    ray_point(r, L[(kPass ? kFZs : kFZc) + q], pt);
    f32x16 feat;
    // a third of the fine samples are the coarse samples again (the merge
    // keeps their z bitwise): with the coarse tiles stored, those lanes load
    // the coarse tile's features instead of gathering 16 levels x 8 corners
    // again -- a quarter of the ray's gathers (render_fwd_kernel 0.282 ->
    // 0.275 ms, r04h).  Encoding only the 128 importance samples as 4 full
    // tiles first and loading every fine tile's features back from the cache
    // (a third fewer encode instructions) measured slower: 0.301 ms, the
    // waves then run their MLP tiles in step (r04j).
    const float* twins = kPass ? pol.twins() : nullptr;
    const int src = twins ? pol.origin(q) : 255;
    if (src >= kSc) {
      HN_FWD_PRIO_HI();
      encode_tile(f.g, gsl, f.table, pt, lane_s >> 5, feat);
      HN_FWD_PRIO_LO();
    } else {
      load_twin_feat(twins, src, h, feat);
    }
    MlpAct a;
    f32x16 c2;
    // skip_dead: a fine tile without density has no nonzero d raw, so the
    // binned backward (dense_bwd = 0: its work lists) never reads its
    // features or masks -- they are not stored.  (The coarse tiles' are: the twins.)
    const bool dead_skip = pol.skip_dead(kPass);
    bool stored = kPass == 0 || !dead_skip;
    if (stored) pol.save_feat(kPass, tau, lane_s, feat);
    using Src = std::conditional_t<kRes, FragRes, FragRing>;
    mlp_fwd_tile_src<Pol::kMasks>(Src{P, ring}, feat, [&](int ob) { return c0sh_lds_load(L + kFC0, ob, lane); },
                                  a, c2, lane, dead_skip, [&]() {
                                    if (!stored) pol.save_feat(kPass, tau, lane_s, feat);
                                    stored = true;
                                  });
    const float4 o4 = make_float4(c2[0], c2[1], c2[2], a.s1[0]);
    if (stored) pol.save_masks(kPass, tau, lane_s, a.m);
    if (h == 0) {
      *reinterpret_cast<float4*>(L + kFRaw + 4 * q) = o4;
      pol.save_raw(kPass, 32 * tau + (lane_s & 31), o4);
    }
  }
}

// render_fwd_kernel's policy: features and masks into the feature cache (where
// there is one), whose coarse tiles are the twins; raw to global memory.
// kSfT: the ray's fine samples, the stride of the caller's fine_src and raw_f
// (the cache's tile index stays pass * 2 + tau)
template <bool kLoss, int kSfT>
struct TrainTiles {
  static constexpr bool kMasks = true;
  const RenderK& k;
  int64_t ray;
  const uint8_t* srcl;   // kLoss: the samples' origins in LDS
  HN_DEV const float* twins() const { return k.feat ? k.feat + (size_t)ray * HN_RENDER_FEAT_PER_RAY : nullptr; }
  // (kLoss: from the LDS copy -- no global round trip ahead of each tile's gathers)
  HN_DEV int origin(int q) const { return kLoss ? (int)srcl[q] : (int)k.fine_src[ray * kSfT + q]; }
  HN_DEV bool skip_dead(int pass) const { return k.skip_dead && (pass ? k.noise_f : k.noise_c) == nullptr; }
  HN_DEV void save_feat(int pass, int tau, int lane, const f32x16& feat) const {
    if (k.feat) store_feat(k.feat, ray, pass * (kSc / 32) + tau, lane, feat, k.feat_nt != 0);
  }
  HN_DEV void save_masks(int pass, int tau, int lane, const uint32_t (&m)[3]) const {
    if (k.feat) store_masks(k.feat, ray, pass * (kSc / 32) + tau, lane, m, k.feat_nt != 0);
  }
  HN_DEV void save_raw(int pass, int q, const float4& o4) const {
    *reinterpret_cast<float4*>(pass ? k.raw_f + (ray * kSfT + q) * 4 : k.raw_c + (ray * kSc + q) * 4) = o4;
  }
};

// One pass's composite.  kLoss: then also the training loss's composite
// backward from the same samples and totals (composite_bwd's two halves, so
// the d raw are the pre-pass's bit for bit), written over raw in LDS.
template <bool kLoss, int N>
HN_DEV void composite_pass(const RenderK& k, int64_t ray, float* rawb, const float* z, const float* noise, int S,
                           float dnorm, float* wout, CompOut& o, int lane) {
  if constexpr (!kLoss) {
    composite_fwd<N>(rawb, z, noise, S, dnorm, k.f.white != 0, wout, o, lane);
  } else {
    // (the ray's target colour asked for ahead of the composite that hides its latency)
    const float target[3] = {k.ltarget[3 * ray], k.ltarget[3 * ray + 1], k.ltarget[3 * ray + 2]};
    CompSamples<N> cs;
    composite_samples<N>(rawb, z, noise, S, dnorm, cs, lane);
    CompTotals t;
    composite_totals<N>(cs, t);
    composite_fwd_out<N>(cs, t, k.f.white != 0, wout, o, lane);
    CompGrad g;
    loss_comp_grad(g, k.lgm, k.lsparse, o.rgb[0], o.rgb[1], o.rgb[2], target);
    composite_bwd_raw<N>(cs, t, k.f.white != 0, g, nullptr, nullptr, rawb, lane);
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
// kNiT: the importance samples, kNi or kNi64 -- a compile-time shape (the fine
// composite's samples per lane, the fine tile loop, the merge network's
// depth), so the 64 + 128 instantiations are the code they were before the
// second shape.  The workspace's d raw keeps its 64 + 192 stride for both.
// kRes: the resident form (the note at kFwdResWaves).
template <bool kLoss, int kNiT, bool kRes = false>
__global__ __launch_bounds__(64 * fwd_block_waves(kRes))
__attribute__((amdgpu_waves_per_eu(kFwdWavesPerSimd, kFwdWavesPerSimd)))
void render_fwd_kernel(RenderK k) {
  constexpr int kSfT = kSc + kNiT;   // the ray's fine samples
  constexpr int kBW = fwd_block_waves(kRes);
  __shared__ __attribute__((aligned(16))) float smem[kBW * kFLds + kGsLds];
  // each wave's split-GEMM fragments one chunk ahead (FragRing, hn_mlp.h):
  // render_fwd_kernel 0.271 -> 0.266 ms, r05 ring (bitwise-identical outputs);
  // kRes: the array holds the workgroup's resident image instead, the coarse
  // net's, then the fine net's (804 floats per wave)
  static_assert(kResImageFloats % (4 * kFwdResWaves) == 0, "a whole dwordx4 share per wave");
  __shared__ __attribute__((aligned(16))) float fring[kBW][kRes ? kResImageFloats / kFwdResWaves : 768];
  // the wave index (and with it the ray, its 11 floats and every per-ray
  // address) on the scalar unit: VGPR spills 45 -> 22, render_fwd_kernel
  // 0.296 -> 0.281 ms (r04e)
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  float* gsl = smem + kBW * kFLds;
  stage_grid_sizes(k.f.g, gsl);
  const int64_t nb = gridDim.x;
  // kRes && kLoss: the keys of the XCD's runs (fwd_res_deal), one byte each.
  // Their own kFwdResMaxRuns bytes, not a region that a wave reuses later: the
  // waves read them after the kernel's only barrier, each at its own pace.
  __shared__ uint8_t dkeys[kRes && kLoss ? kFwdResMaxRuns : 4];
  // A thread per ray of the XCD's share (8 of the 16 waves at 4096 rays; 1.5 KB
  // of targets per wave, the same for the XCD's workgroups: from L2).  A ray
  // counts where its target is not the background colour; past the batch's end
  // none does.  The first 64 x 16 rays' targets are asked for here and looked
  // at after the sigma copy below, so both are one round trip to memory under
  // the same barrier.
  const bool deal = kRes && kLoss && fwd_res_deal_on(nb);
  const int share = fwd_res_xcd_runs(nb) * kFwdResRunRays;   // deal: a multiple of 64
  const float bg = k.f.white ? 1.f : 0.f;
  auto load_targets = [&](int base, float (&t)[3]) {
    const int lr = base + lane;
    const int64_t ry = fwd_res_xcd_run((int)(blockIdx.x % kFwdResXcds), lr / kFwdResRunRays) * kFwdResRunRays +
                       lr % kFwdResRunRays;
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = ry < k.B ? k.ltarget[3 * ry + c] : bg;
  };
  auto store_keys = [&](int base, const float (&t)[3]) {
    const bool live = fabsf(t[0] - bg) > 1.f / 512 || fabsf(t[1] - bg) > 1.f / 512 || fabsf(t[2] - bg) > 1.f / 512;
    const uint64_t m = __ballot(live);
    if (lane < 64 / kFwdResRunRays)
      dkeys[base / kFwdResRunRays + lane] =
          (uint8_t)__popcll((m >> (kFwdResRunRays * lane)) & ((1u << kFwdResRunRays) - 1));
  };
  float tg[3] = {bg, bg, bg};
  if constexpr (kRes && kLoss) {
    if (deal && 64 * wave < share) load_targets(64 * wave, tg);
  }
  if constexpr (kRes) {
    // every wave of the workgroup, those past the batch's end too: they return
    // only after the barrier
    // the workgroup's image (the map at kResRegs, hn_mlp.h): dwordx4 j of it
    // from the packed net's dwordx4 res_src / 4 -- the kept lanes of a group
    // are consecutive in both, a zero lane is not copied
    constexpr int kN4 = kResImageFloats / 4, kC4 = kResNetFloats / 4;   // dwordx4: the image's, one net's
    const f32x4* srcc = reinterpret_cast<const f32x4*>(k.f.Pc);
    const f32x4* srcf = reinterpret_cast<const f32x4*>(k.f.Pf);
    f32x4* dst = reinterpret_cast<f32x4*>(&fring[0][0]);
#pragma unroll
    for (int i = 0; i < (kN4 + 64 * kBW - 1) / (64 * kBW); ++i) {
      const int j = i * 64 * kBW + (int)threadIdx.x;
      if (j < kN4) dst[j] = (j < kC4 ? srcc : srcf)[res_src(4 * (j < kC4 ? j : j - kC4)) >> 2];
    }
  }
  if constexpr (kRes && kLoss) {
    if (deal)
      for (int base = 64 * wave; base < share; base += 64 * kBW) {
        if (base != 64 * wave) load_targets(base, tg);   // (batches past 8192 rays)
        store_keys(base, tg);
      }
  }
  __syncthreads();
  // XCD-aware: workgroup b runs on XCD b % 8, so consecutive ray groups of a
  // spatially ordered batch go to one XCD and share its L2
  // (round 6, r06k: chunks of 4 or 16 ray groups dealt round-robin over the
  // XCDs, or no XCD mapping at all, were no faster: 234.9 / 228.8 / 240.4 us
  // against 229.4 us -- the forward's per-XCD work is balanced already)
  const int64_t grp = nb % 8 == 0 ? (blockIdx.x % 8) * (nb / 8) + blockIdx.x / 8 : blockIdx.x;
  int64_t ray = grp * kBW + wave;
  if constexpr (kRes) {
    // A CU runs its 16 rays from start to end, and a batch in spatial order
    // gives consecutive rays alike amounts of work (tiles with density run
    // the colour net): with 16 consecutive rays per workgroup the kernel
    // waits for the CUs whose rays are all heavy.  So the workgroup takes
    // kFwdResRuns runs of 4 consecutive rays (the ring form's group: they
    // share table rows in the CU's cache), one from each quarter of its XCD's
    // band of the batch.  Config 2, 4096 rays: render_fwd_kernel 0.2327 ms as
    // 1 run of 16, 0.2216 as 4 runs of 4, 0.2242 as 16 single rays
    // (profiles/r12/); the mean wave is resident for only ~3/4 of the launch.
    // Which four runs: fwd_res_deal (above).  Where the grid is 8 whole shares
    // of segments, the runs of the XCD's segments sorted by their keys and
    // dealt in a snake, so that a workgroup's runs are heavy and light by
    // cost and not by position, and an XCD's share is spread over the image
    // instead of one band of it; the keys are the loss mode's, without targets
    // the runs count alike and the sort keeps the batch's order.  Config 2:
    // render_fwd_kernel 0.2182 -> 0.2110 ms, the waves resident for 0.78 of
    // the launch instead of 0.70 (profiles/r18/; a sum-of-costs model said
    // 0.19 ms: DESIGN 8).  Segments of 32 / 128 / 256 rays: 0.2143 / 0.2117 /
    // 0.2142 ms; the keys within the XCD's band, no segments: 0.2155; the
    // segments without keys: 0.2180.
    constexpr int kW = kFwdResRunRays;
    const int s = wave / kW;
    const int64_t run = fwd_res_deal(nb, blockIdx.x, s, [&](int nr, int pos) {
      if constexpr (kLoss) return fwd_res_select_wave(dkeys, nr, pos, lane);
      else return pos;
    });
    ray = run * kW + wave % kW;   // every ray below 16 nb once; those past the batch's end leave below
  }
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
  Ray r;
  load_ray(k.rays, ray, r);
  float sh8[8];

  // ---- coarse z_vals (:514-536) ----
  auto zlin = [&](int i) { return coarse_z(k.f.tvals[i], r.near, r.far, k.f.lindisp); };
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
  ray_sh(r, lane >> 5, sh8);
  lds_fence_wave();

  // ---- coarse network (:540) ----
  // kLoss: the samples' coarse origins kept in LDS for the marks (zsrc is free
  // after the merge), read beside the first fine tile's own look at them
  uint8_t* srcl = reinterpret_cast<uint8_t*>(zsrc);
  TrainTiles<kLoss, kSfT> pol{k, ray, srcl};
  // the passes' fragment source: the wave's ring slot, or the net's resident regions
  float* srcc = kRes ? &fring[0][0] : fring[wave];
  float* srcf = kRes ? &fring[0][0] + kResNetFloats : fring[wave];
  pass_start<kRes>(k.f.Pc, sh8, L, srcc, lane, false);
  pass_tiles<0, TrainTiles<kLoss, kSfT>, kSf, kRes>(k.f, gsl, srcc, L, r, lane, pol);
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
  if (lane < kSc - 1) L[kFBins + lane] = .5f * (zc[lane + 1] + zc[lane]);
  importance_sort<kNiT>(L, k.f.u + ray * kNiT, k.fine_src + ray * kSfT, lane);
  {   // z_std of the samples as drawn (the sort reads zsrc only)
    if constexpr (kNiT == kNi) {
      const float s0 = zsrc[kSc + lane], s1 = zsrc[kSc + 64 + lane];
      const double mean = wave_sum((double)s0 + (double)s1) / kNi;
      const double d0 = (double)s0 - mean, d1 = (double)s1 - mean;
      const double var = wave_sum(d0 * d0 + d1 * d1) / kNi;
      if (lane == 0) k.z_std[ray] = (float)sqrt(var);
    } else {   // one sample per lane
      const double s0 = (double)zsrc[kSc + lane];
      const double d0 = s0 - wave_sum(s0) / kNiT;
      const double var = wave_sum(d0 * d0) / kNiT;
      if (lane == 0) k.z_std[ray] = (float)sqrt(var);
    }
  }
  for (int i = lane; i < kSfT; i += 64) k.z_fine[ray * kSfT + i] = zs[i];

  // ---- fine network (:556) ----
  pass_start<kRes>(k.f.Pf, sh8, L, srcf, lane, true);
  if constexpr (kLoss) {
    for (int i = lane; i < kSfT; i += 64) srcl[i] = k.fine_src[ray * kSfT + i];
    lds_fence_wave();
  }
  pass_tiles<1, TrainTiles<kLoss, kSfT>, kSfT, kRes>(k.f, gsl, srcf, L, r, lane, pol);
  lds_fence_wave();
  CompOut fo;
  composite_pass<kLoss, kSfT / 64>(k, ray, rawb, zs, k.noise_f ? k.noise_f + ray * kSfT : nullptr, kSfT, r.dnorm,
                                   nullptr, fo, lane);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) k.rgb[3 * ray + c] = fo.rgb[c];
    k.depth[ray] = fo.depth;
    k.acc[ray] = fo.acc;
    k.sparsity[ray] = fo.entropy;
  }
  if constexpr (kLoss) {   // the fine pass's d raw and the ray's marks
    const uint32_t nzf = draw_store_marks(rawb, k.draw + ((size_t)ray * (kSc + kSf) + kSc) * 4, kSfT, lane);
    const uint32_t su = scatter_marks<kSfT>(rawb, srcl, cmask, lane);
    if (lane == 0) store_fine_marks(k.uflags, ray, nzf, su);
  }
}

}  // namespace hn

