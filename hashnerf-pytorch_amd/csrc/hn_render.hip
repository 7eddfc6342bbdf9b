// hn_render.hip -- fused render_rays (run_nerf_helpers.py:464-574) for one
// training ray batch: the C entry points hn_render_fwd / hn_render_bwd, the
// pre-pass kernel of both backward schedules (not launched by the binned one
// after a training forward that did its work, hn_render_fwd_args.loss), and
// the host side; and hn_render_views / hn_render_image, the evaluation renderer
// (whole images from poses, hn_render_image.h); and hn_density_points /
// hn_density_lattice, the density queries (hn_density.h).  One
// translation unit; the device code is in the headers (each says what it holds).
#include "hn_render_args.h"   // kernel arguments, rays, feature cache, shared helpers
#include "hn_render_fwd.h"    // render_fwd_kernel
#include "hn_render_image.h"  // render_image_kernel: whole images from poses, nothing saved
#include "hn_mlp_bwd.h"       // one tile's MLP backward, dW slabs, render_bwd_kernel's declaration
#include "hn_bwd_binned.h"    // binned schedule: render_bwd_kernel<kSwVmcnt, kModeSplit>, records, owner pass
#include "hn_bwd_atomic.h"    // float-atomic fused schedule: render_bwd_kernel<CAP, kModeAtomic>
#include "hn_bwd_rays.h"      // the ray gradient: render_bwd_rays_kernel and its reduction
#include "hn_density.h"       // density queries: density_kernel (sigma / occupancy at points or on a lattice)

#include <math.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

namespace hn {

// Composite backward pre-pass of both schedules (raw2outputs backward,
// run_nerf_helpers.py:577-628 via the :541 / :558 chain): one wave per (ray,
// pass) at full occupancy writes d raw of every sample, so the MLP backward
// only loads one float4 per point instead of redoing the ray's scans.  It
// also forms the training loss's gradients and value (B1K::lout), marks the
// 16-sample groups with a nonzero d raw (B1K::uflags, the binned schedule's
// lists) and empties the binned schedule's overflow book.
__global__ __launch_bounds__(256) void render_comp_bwd_kernel(B1K k) {
  __shared__ float lds[kFwdWaves][kSf * 5];
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k.bins && blockIdx.x == 0) zero_ovf_book(k);   // binned scatter: no overflow records yet
  // the loss value (hn_loss_fwd's reduction): an extra workgroup 0 of its own,
  // dispatched first, so its serial sums run beside the rays' workgroups
  if (k.lout && blockIdx.x == 0) {
    loss_fwd_block<64 * kFwdWaves>(k.lrgb, k.lrgb0, k.ltarget, k.lsp, k.lsp0, k.B, k.ltv, k.n_tv, k.lworld,
                                   k.lsparse_w, k.ltv_w, k.lout);
    return;
  }
  const int64_t w = (int64_t)(blockIdx.x - (k.lout ? 1 : 0)) * kFwdWaves + wave;
  // the two waves of a ray (coarse 2r, fine 2r + 1) share the workgroup: the
  // coarse wave's nonzero-sample mask reaches the fine wave through LDS
  __shared__ unsigned long long cmask[kFwdWaves / 2];
  const bool active = w < 2 * k.B;
  uint32_t nzf = 0u;   // the fine wave's MLP groups
  const int64_t ray = w >> 1;
  const bool fine = (w & 1) != 0;
  float* rawb = lds[wave] + kSf;
  if (active) {
    const int S = fine ? k.sf : kSc;   // (the d raw below keep the 64 + 192 stride)
    float* zb = lds[wave];
    const float* zsrc = (fine ? k.z_fine : k.z_coarse) + ray * S;
    const float* rsrc = (fine ? k.raw_f : k.raw_c) + ray * S * 4;
    for (int j = lane; j < S; j += 64) {
      zb[j] = zsrc[j];
      *reinterpret_cast<float4*>(rawb + 4 * j) = *reinterpret_cast<const float4*>(rsrc + 4 * j);
    }
    lds_fence_wave();
    Ray r;
    load_ray(k.rays, ray, r);
    CompGrad g;
    const float* grgb = fine ? k.g_rgb : k.g_rgb0;
    const float* gacc = fine ? k.g_acc : k.g_acc0;
    const float* gdep = fine ? k.g_depth : k.g_depth0;
    const float* gent = fine ? k.g_sparsity : k.g_sparsity0;
    if (k.lout) {   // the training loss's gradients (hn_loss_bwd_elem's op forms, g_loss = 1)
      const float* x = (fine ? k.lrgb : k.lrgb0) + 3 * ray;
      loss_comp_grad(g, k.lgm, k.lsparse, x[0], x[1], x[2], k.ltarget + 3 * ray);
    } else {
      g.has_rgb = grgb != nullptr;
      g.has_acc = gacc != nullptr;
      g.has_depth = gdep != nullptr;
      g.has_entropy = gent != nullptr;
#pragma unroll
      for (int c = 0; c < 3; ++c) g.rgb[c] = g.has_rgb ? grgb[3 * ray + c] : 0.f;
      g.acc = g.has_acc ? gacc[ray] : 0.f;
      g.depth = g.has_depth ? gdep[ray] : 0.f;
      g.entropy = g.has_entropy ? gent[ray] : 0.f;
    }
    const float* noise = fine ? (k.noise_f ? k.noise_f + ray * S : nullptr)
                              : (k.noise_c ? k.noise_c + ray * S : nullptr);
    const float* graw = (fine && k.g_raw_f) ? k.g_raw_f + ray * S * 4 : nullptr;
    float* dst = k.draw + ((size_t)ray * (kSc + kSf) + (fine ? kSc : 0)) * 4;
    if (fine && S == kSf)
      composite_bwd<kSf / 64>(rawb, zb, noise, S, r.dnorm, k.white != 0, g, nullptr, graw, rawb, lane);
    else if (fine)
      composite_bwd<kSf64 / 64>(rawb, zb, noise, S, r.dnorm, k.white != 0, g, nullptr, graw, rawb, lane);
    else
      composite_bwd<kSc / 64>(rawb, zb, noise, S, r.dnorm, k.white != 0, g, nullptr, graw, rawb, lane);
    lds_fence_wave();
    // bit t: a sample of 16-sample group t has a nonzero d raw (the MLP's)
    const uint32_t nzu = draw_store_marks(rawb, dst, S, lane);
    if (lane == 0 && !fine) k.uflags[kMarkB * ray] = (uint8_t)nzu;   // byte 0: the coarse groups
    nzf = nzu;
    if (!fine) cmask[wave >> 1] = coarse_nonzero_mask(rawb, lane);
  }
  __syncthreads();
  if (active && fine) {
    // the scatter's marks (bits 20-31), beside the fine MLP groups (8-19)
    const uint8_t* src = k.fine_src + ray * k.sf;
    const uint32_t su = k.sf == kSf ? scatter_marks<kSf>(rawb, src, cmask[wave >> 1], lane)
                                    : scatter_marks<kSf64>(rawb, src, cmask[wave >> 1], lane);
    if (lane == 0) store_fine_marks(k.uflags, ray, nzf, su);
  }
}

// ---- host side --------------------------------------------------------------

static int32_t check_cfg(const hn_render_cfg* c) {
  if (!c) return HN_E_NULL;
  const hn_grid& g = c->grid;
  if (g.n_levels != 16 || g.n_features != 2) return HN_E_SHAPE;
  if (g.log2_hashmap_size < 1 || g.log2_hashmap_size > 24) return HN_E_SHAPE;
  if (c->n_samples != kSc || (c->n_importance != kNi && c->n_importance != kNi64)) return HN_E_SHAPE;
  if (c->scatter < 0 || c->scatter > 2) return HN_E_SHAPE;
  if (c->bin_cap < 0 || (c->bin_cap & 63)) return HN_E_SHAPE;
  if (c->dense_bwd < 0 || c->dense_bwd > 1) return HN_E_SHAPE;
  return HN_OK;
}
// hn_render_image(_variant)'s own refusal: 64 + 128 samples only (hn_render_views takes both counts)
static int32_t check_image_cfg(const hn_render_cfg* c) {
  const int32_t st = check_cfg(c);
  return st ? st : (c->n_importance != kNi ? HN_E_SHAPE : HN_OK);
}

static bool mlp_ok(const hn_mlp& w) { return w.sigma0 && w.sigma1 && w.color0 && w.color1 && w.color2; }
static bool grad_ok(const hn_mlp_grad& w) {
  return w.sigma0 && w.sigma1 && w.color0 && w.color1 && w.color2;
}

// Binned scatter geometry.  A bin is 2^13 consecutive table entries (its
// 2 x 2^13 64-bit accumulators are the owner's 128 KiB of LDS), or the whole
// table when that is smaller.  Region capacity per (block, bin): the records
// a block's rays can write into one bin without any run merging on average
// (192 unique points x 4 corner rows per level and ray, spread over the
// level's 2^T / 2^shift bins) + 128; sized so, a region overflows only on
// strongly clumped input (into the shared overflow records).
struct BinGeom {
  int shift, nbins, cap;
  size_t floats;
};
static BinGeom bin_geom(int T, int64_t n_rays, int cap_override) {
  BinGeom g;
  // bins of 2^kBinShift entries unless that needs more bins than the scatter's
  // LDS counters hold (a kBinShift of 12 -- 64 KiB of accumulators, two owner
  // workgroups per CU -- is DESIGN 4.4's measurement)
  const int want = T + 4 - kBinShift <= kScMaxBinsLog2 ? kBinShift : 13;
  g.shift = T + 4 < want ? T + 4 : want;
  g.nbins = 1 << (T + 4 - g.shift);
  const double rpb = (double)((n_rays + kBwdBlocks - 1) / kBwdBlocks);
  const double avg = rpb * (kSf * 4) * ldexp(1.0, g.shift - T);
  g.cap = cap_override > 0 ? cap_override : (int)(((int64_t)avg + 128 + 63) & ~(int64_t)63);
  // an odd multiple of 64 records: the regions' stride (16 B x cap) then has
  // as few factors of two as the 64-record granule allows.  Measured on
  // config 2 (scatter / owner): 320 224 / 225 us, 448 227 / 226, 384 233 /
  // 224, 256 247 / 237, 512 254 / 235 -- the 256 regions of a bin at a
  // power-of-two stride share memory channels
  if (cap_override <= 0 && ((g.cap >> 6) & 1) == 0) g.cap += 64;
  const size_t nrec = bin_records(g.nbins, g.cap, n_rays);
  g.floats = nrec * 5 + (size_t)kBwdBlocks * (g.nbins + 16) + ovf_book_words(g.nbins, n_rays) + 4;
  return g;
}
// Backward schedule: cfg->scatter 1 = float atomics (fused), 2 or 0 = binned
// (split).  The binned scatter keeps per-bin counters in LDS: nbins <=
// kScMaxBins (T <= 22); past that, and where a record's two x corners could
// leave one bin, the float-atomic schedule runs.  (The library reads no
// environment: every schedule choice is in hn_render_cfg.)
static int bwd_mode(const hn_render_cfg* c, int64_t n_rays) {
  if (!c) return kModeAtomic;
  const int want = c->scatter == 1 ? kModeAtomic : kModeSplit;
  const int T = c->grid.log2_hashmap_size;
  if (want != kModeSplit || (16ll << T) > (long long)kScMaxBins << 13) return kModeAtomic;
  // A record keeps its x1 corner's row as h(x0) ^ (2^nbits - 1), nbits =
  // ctz(~x0) + 1 <= bit_length(x0) + 1 (4 bits of the entry word), and assumes
  // both rows lie in one bin.  The cell index of a clamped point is at most
  // (bmax - bmin) / grid_size, so that must fit the bin (or the level, when a
  // bin holds whole levels: the xor is taken modulo 2^T).
  const int shift = bin_geom(T, n_rays, c->bin_cap).shift;
  if (shift < T) {
    double cells = 0.0;
    for (int l = 0; l < c->grid.n_levels; ++l)
      for (int a = 0; a < 3; ++a) {
        const double gs = c->grid.grid_size[l][a];
        const double n = gs > 0.0 ? ((double)c->grid.box_max[a] - c->grid.box_min[a]) / gs : 1e30;
        cells = n > cells ? n : cells;
      }
    int bits = 0;
    while (bits < 40 && ldexp(1.0, bits) <= cells + 1.0) ++bits;   // bit_length of the largest cell index
    if (bits + 1 > shift || bits + 1 > 15) return kModeAtomic;
  }
  return kModeSplit;
}

// A workspace is laid out by a running cursor, in floats from its base: take
// n floats at an alignment, get their offset.  Regions cannot overlap and the
// cursor's end is the size.
struct WsCursor {
  size_t at = 0;
  size_t take(size_t n, size_t align = 1) {
    const size_t o = (at + align - 1) & ~(align - 1);
    at = o + n;
    return o;
  }
};
template <class T>
static T* ws_at(void* workspace, size_t ofs) { return reinterpret_cast<T*>((float*)workspace + ofs); }

// The render workspace of (schedule, n rays), offsets in floats: the one place
// its layout is written down.  What the kernels index by themselves is tied
// to it here: render_lists_kernel and the binned render_bwd_kernel find the
// fine list 4 B behind B1K::lists and the scatter's 12 B behind that (a code
// per 16-sample group), a ray's marks are one word, ovf_place_kernel's repack
// writes both nets as [2][G_END], and ws_stamp's word lies within the counts.
constexpr size_t kListC = 4, kListF = 12, kListS = 12;   // list entries per ray: coarse, fine, the scatter's
constexpr size_t kListCounts = 8;                        // B1K::lmeta: 4 counts, then the stamp's words
static_assert(kListC == kSc / 16 && kListF == kSf / 16 && kListS == kSf / 16 && kMarkB == sizeof(float) &&
              kStampAt >= 4 && kStampAt + 3 <= (int)kListCounts, "the kernels' own offsets");
static_assert(G_END % 4 == 0 && W_END % 4 == 0 && kDcRay % 4 == 0, "every float4 region is 16-byte aligned");
struct WsLayout {
  size_t Pc, Pf, slab, dfeat, draw, marks, lmeta, lc, lf, ls, dfeat_f, bins, total;
};
static WsLayout ws_layout(int mode, const BinGeom& bg, int64_t n_rays) {
  const size_t n = n_rays > 0 ? (size_t)n_rays : 0;
  const bool binned = mode == kModeSplit;
  WsCursor c;
  WsLayout w;
  w.Pc = c.take(G_END);                                       // packed coarse net
  w.Pf = c.take(G_END);                                       // packed fine net
  w.slab = c.take((size_t)kBwdBlocks * kSlabSlots * W_END);   // dW slabs [256][4][9344]
  w.dfeat = c.take(n * kDcRay);                               // coarse-pass feature grads [n][64][32]
  w.draw = c.take(n * (kSc + kSf) * 4);                       // d raw [n][256][4]
  w.marks = c.take(n * kMarkB / sizeof(float));               // unit marks [n][kMarkB] u8 (B1K::uflags)
  w.lmeta = c.take(kListCounts);                              // the lists' counts, the training forward's stamp
  w.lc = c.take(kListC * n);                                  // the lists' group codes: coarse (B1K::lists),
  w.lf = c.take(kListF * n);                                  // fine,
  w.ls = c.take(kListS * n);                                  // the scatter's (ScK::slist)
  w.dfeat_f = c.take(binned ? n * kSf * 32 : 0, 4);           // binned: fine feature grads [n][6][1024]
  w.bins = c.take(binned ? bg.floats : 0);                    // binned: the records and their book (bin_geom)
  w.total = c.at;
  return w;
}

// The backward's plan for (cfg, n_rays), host arithmetic only: the schedule,
// and with it the workspace layout; for the binned schedule also the bin
// geometry and scatter_bins_kernel's dynamic LDS (the bins' counters, then
// the staging pool).
struct BwdPlan {
  int mode;          // kModeSplit (binned) or kModeAtomic
  BinGeom bg;        // binned only
  size_t sc_lds;     // binned only
  WsLayout ws;
  size_t bytes() const { return ws.total * sizeof(float); }
};
static BwdPlan bwd_plan(const hn_render_cfg* cfg, int64_t n_rays) {
  BwdPlan p{};
  p.mode = bwd_mode(cfg, n_rays);
  if (p.mode == kModeSplit) {
    p.bg = bin_geom(cfg->grid.log2_hashmap_size, n_rays, cfg->bin_cap);
    p.sc_lds = (size_t)((p.bg.nbins + 3) & ~3) * 8 + (size_t)kStPool * 20;
  }
  p.ws = ws_layout(p.mode, p.bg, n_rays);
  return p;
}

// The training forward's stamp: the 8-byte aligned word within lmeta[4..7]
static unsigned long long* ws_stamp(int32_t* lmeta) {
  return reinterpret_cast<unsigned long long*>((reinterpret_cast<uintptr_t>(lmeta + kStampAt) + 7) & ~(uintptr_t)7);
}

// The overflow book of a call's records (the kernels derive it alike)
static OvfBook host_ovf_book(float* bins, const BinGeom& bg, int64_t n_rays) {
  const size_t nrec = bin_records(bg.nbins, bg.cap, n_rays);
  return ovf_book(reinterpret_cast<uint32_t*>(bins + 4 * nrec), nrec, bg.nbins);
}

// The loss's upstream factors (hn_loss_bwd's with g_loss = 1): one definition
// for the training forward and the pre-pass, which must agree bitwise
static void loss_factors(float world, float sparse_w, int64_t n_rays, float& gm, float& sparse) {
  const float g = 1.f;
  gm = (g / world) / (float)(3 * n_rays);
  sparse = g * sparse_w;
}

// scatter_bins_kernel's dynamic LDS fits beside its static LDS, read once
// from the code object (a constant here would silently go stale
// if the static arrays grow).  Checked before anything is queued.
static bool sc_lds_fits(const BwdPlan& p) {
  static size_t fixed = 0;
  if (!fixed) {
    hipFuncAttributes at{};
    fixed = hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&scatter_bins_kernel)) == hipSuccess
                ? at.sharedSizeBytes : (size_t)16 * 1024;
  }
  return p.sc_lds + fixed <= (size_t)160 * 1024;
}

// hn_render_bwd_args.table_step / table_live: the fused table step of the
// binned owner pass
static int32_t check_table_step(const hn_render_cfg* cfg, const hn_render_bwd_args* a) {
  if (!a->table_step) return HN_OK;
  const int T = cfg->grid.log2_hashmap_size;
  const hn_radam_tensor& ts = *a->table_step;
  if (ts.n != ((int64_t)16 << T) * 2) return HN_E_SHAPE;
  if (!ts.p || !ts.m || !ts.v) return HN_E_NULL;
  if (a->table_live && (a->table_live_levels < 0 || a->table_live_levels > cfg->grid.n_levels || T < 6))
    return HN_E_SHAPE;
  return HN_OK;
}

// A backward's TV term (a->tv given): its gradient's factor, make_tv, the
// grid's levels and T; rec_fit: its records fit the binned scatter's overflow
// lists (ovf_per_block: every cube <= kTvRecMaxCube)
static int32_t check_tv(const hn_render_cfg* cfg, const hn_render_bwd_args* a, TvK& tvk, bool& rec_fit) {
  if (!a->g_tv) return HN_E_NULL;
  int nbf, nbb;
  if (int32_t st = make_tv(a->tv, tvk, nbf, nbb)) return st;
  if (a->tv->n_levels != cfg->grid.n_levels || a->tv->log2_hashmap_size != cfg->grid.log2_hashmap_size)
    return HN_E_SHAPE;
  rec_fit = a->tv->n_levels <= 16;
  for (int l = 0; l < a->tv->n_levels && rec_fit; ++l) rec_fit = a->tv->cube[l] <= kTvRecMaxCube;
  return HN_OK;
}

// The scatter's arguments every binned launch sets: the bins, and the TV
// term's records (tv NULL: none) -- tv_off[l] = first x-pair of level l
static void sc_bins_tv(ScK& sk, float* bins, const BinGeom& bg, const hn_tv_args* tv, const TvK& tvk) {
  sk.bins = bins;
  sk.bin_cap = bg.cap;
  sk.bin_shift = bg.shift;
  sk.nbins = bg.nbins;
  for (int l = 0; l <= 16; ++l) sk.tv_off[l] = 0;
  if (!tv) return;
  sk.tv = tvk;
  int off = 0;
  for (int l = 0; l < tv->n_levels; ++l) {
    sk.tv_off[l] = off;
    const int n1 = tv->cube[l] + 1;
    off += (n1 + 1) / 2 * n1 * n1;
  }
  for (int l = tv->n_levels; l <= 16; ++l) sk.tv_off[l] = off;
}

// The owner pass's arguments (bins [bin0, ...) of one launch)
static BinR owner_args(const hn_render_cfg* cfg, const hn_render_bwd_args* a, float* bins, const BinGeom& bg,
                       int bin0) {
  BinR r;
  r.bins = bins;
  r.n_rays = a->n_rays;
  r.nbins = bg.nbins;
  r.cap = bg.cap;
  r.shift = bg.shift;
  r.log2T = cfg->grid.log2_hashmap_size;
  r.d_table = a->d_table;
  r.overwrite = (a->d_table_mode & 1) != 0;
  r.fused = a->table_step != nullptr;
  if (r.fused) r.step = *a->table_step;
  r.live = r.fused ? a->table_live : nullptr;
  r.live_levels = r.live ? a->table_live_levels : 0;
  r.bin0 = bin0;
  return r;
}
static void launch_owner(const BinR& r, const BinGeom& bg, int n_bins, hipStream_t s) {
  hipLaunchKernelGGL(bin_reduce_kernel, dim3((unsigned)n_bins), dim3(kBinThreads),
                     (size_t)(2 << bg.shift) * sizeof(unsigned long long), s, r);
}

// What hn_render_fwd and hn_render_views share of their kernels' arguments; the
// nets' packed copies (Pc, Pf: their workspace's) are made here unless given
static int32_t field_args(const hn_render_cfg* cfg, const float* t_vals, const float* u, const float* table,
                          const hn_mlp& coarse, const hn_mlp& fine, int32_t weights_packed, void* workspace,
                          size_t ofs_c, size_t ofs_f, hipStream_t s, FieldK& f) {
  float *Pc = ws_at<float>(workspace, ofs_c), *Pf = ws_at<float>(workspace, ofs_f);
  if (int32_t st = weights_packed ? 0 : mlp_pack2_launch(&coarse, Pc, &fine, Pf, s)) return st;
  f = FieldK{make_grid_args(cfg->grid), cfg->white_bkgd, cfg->lindisp, t_vals, u, table, Pc, Pf};
  return HN_OK;
}

}  // namespace hn

using namespace hn;

extern "C" size_t hn_render_workspace_bytes(const hn_render_cfg* cfg, int64_t n_rays) {
  return bwd_plan(cfg, n_rays).bytes();
}

extern "C" int32_t hn_render_scatter_mode(const hn_render_cfg* cfg, int64_t n_rays) {
  return bwd_mode(cfg, n_rays) == kModeSplit ? 2 : 1;
}

extern "C" int32_t hn_device_faults(int32_t* faults, int32_t clear) {
  if (!faults) return HN_E_NULL;
  int32_t st = hip_status(hipMemcpyFromSymbol(faults, HIP_SYMBOL(g_hn_fault), sizeof(int32_t)));
  if (st || !clear || *faults == 0) return st;
  const int32_t zero = 0;
  return hip_status(hipMemcpyToSymbol(HIP_SYMBOL(g_hn_fault), &zero, sizeof(int32_t)));
}

// The current device's compute units, asked once per device (0: not known)
static int device_cus() {
  static std::atomic<int> cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  int n = cached[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 0) n = 0;
    cached[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}
// Which form of render_fwd_kernel a batch runs (hn_render_fwd.h; identical
// bits, so the choice is free).  The resident form gives a CU to 16 rays, the
// ring form spreads 4-ray workgroups over every CU: resident only where its
// workgroups fill the device, ceil(n_rays / 16) >= CUs.
static int fwd_pick_form(int64_t n_rays, int cus) {
  return cus > 0 && (n_rays + kFwdResWaves - 1) / kFwdResWaves >= cus ? 2 : 1;
}
// f(std::true_type or std::false_type) for a run-time b: one nesting level per
// boolean template parameter of a kernel, however many there are
template <class F>
static void with_bool(bool b, F&& f) { b ? f(std::true_type{}) : f(std::false_type{}); }
// render_fwd_kernel<kLoss, kNiT, kRes> of a call: the one place that picks the instantiation
static void launch_fwd(bool loss, bool ni64, bool res, int64_t n_rays, hipStream_t s, const RenderK& k) {
  const int bw = fwd_block_waves(res);
  const dim3 grid((unsigned)((n_rays + bw - 1) / bw)), block(64 * bw);
  with_bool(loss, [&](auto kLoss) {
    with_bool(ni64, [&](auto kNi64T) {
      with_bool(res, [&](auto kRes) {
        constexpr int ni = decltype(kNi64T)::value ? kNi64 : kNi;
        hipLaunchKernelGGL((render_fwd_kernel<decltype(kLoss)::value, ni, decltype(kRes)::value>), grid, block, 0, s,
                           k);
      });
    });
  });
}

extern "C" int32_t hn_render_fwd_pick(int64_t n_rays, int32_t* cus) {
  const int n = device_cus();
  if (cus) *cus = n;
  return fwd_pick_form(n_rays, n);
}

// The resident form's map from (workgroup, run slot) to rays, on the host:
// fwd_res_deal itself, with the scalar statement of the sort where the kernel
// uses ballots.  A run that starts past the batch's end has key 0, as in the
// kernel, whatever run_key says.
extern "C" int32_t hn_render_fwd_deal(int64_t n_rays, int64_t n_blocks, const uint8_t* run_key,
                                      int32_t* first_ray) {
  if (!first_ray) return HN_E_NULL;
  if (n_rays < 0 || n_blocks < 1 || n_blocks > (INT32_MAX / kFwdResWaves) || n_rays > n_blocks * kFwdResWaves)
    return HN_E_SHAPE;
  if (run_key)
    for (int64_t i = 0; i < n_blocks * kFwdResRuns; ++i)
      if (run_key[i] > kFwdResRunRays) return HN_E_SHAPE;
  for (int64_t b = 0; b < n_blocks; ++b) {
    const int x = (int)(b % kFwdResXcds);
    auto key_at = [&](int j) {
      const int64_t run = fwd_res_xcd_run(x, j);
      return run_key && run * kFwdResRunRays < n_rays ? (int)run_key[run] : 0;
    };
    for (int s = 0; s < kFwdResRuns; ++s)
      first_ray[b * kFwdResRuns + s] = (int32_t)(
          fwd_res_deal(n_blocks, b, s, [&](int nr, int pos) { return fwd_res_select(nr, pos, key_at); }) *
          kFwdResRunRays);
  }
  return HN_OK;
}

// The resident form's image of a net, on the host: res_src and res_at
// themselves (hn_mlp.h), the functions the kernel's copy and FragRes read
// through.
extern "C" int32_t hn_render_fwd_res_map(int32_t fine, int32_t* src, int64_t n_src, int32_t* at, int64_t n_at) {
  if (fine < 0 || fine > 1) return -HN_E_SHAPE;
  const int n = kResNetFloats;   // (the two nets' images are laid out alike)
  if ((src && n_src < n) || (at && n_at < G_B4 / 4)) return -HN_E_SHAPE;
  if (src)
    for (int i = 0; i < n; ++i) src[i] = res_src(i);
  if (at)
    for (int r = R_F0; r < R_B4; ++r)
      for (int t = 0; t < kRegOB[r] * reg_gpo(r); ++t)
        for (int lane = 0; lane < 64; ++lane) at[reg_off(r) / 4 + t * 64 + lane] = res_at(r, t, lane);
  return n;
}

extern "C" int32_t hn_render_fwd(const hn_render_cfg* cfg, const hn_render_fwd_args* a,
                                 void* workspace, size_t ws_bytes, void* stream) {
  return hn_render_fwd_form(cfg, a, 0, workspace, ws_bytes, stream);
}

extern "C" int32_t hn_render_fwd_form(const hn_render_cfg* cfg, const hn_render_fwd_args* a, int32_t form,
                                      void* workspace, size_t ws_bytes, void* stream) {
  int32_t st = check_cfg(cfg);
  if (st) return st;
  if (form < 0 || form > 2) return HN_E_SHAPE;
  if (!a) return HN_E_NULL;
  if (a->n_rays < 0) return HN_E_SHAPE;
  if (a->n_rays == 0) return HN_OK;
  if (!a->rays || !a->t_vals || !a->u || !a->table || !mlp_ok(a->coarse) || !mlp_ok(a->fine))
    return HN_E_NULL;
  if (cfg->perturb && !a->t_rand) return HN_E_NULL;
  if (!a->rgb || !a->depth || !a->acc || !a->sparsity || !a->rgb0 || !a->depth0 || !a->acc0 ||
      !a->sparsity0 || !a->z_std || !a->z_coarse || !a->z_fine || !a->raw_c || !a->raw_f ||
      !a->fine_src)
    return HN_E_NULL;
  if (!workspace) return HN_E_NULL;
  const BwdPlan plan = bwd_plan(cfg, a->n_rays);
  if (ws_bytes < plan.bytes()) return HN_E_WORKSPACE;
  // 64 importance samples: only the binned backward reads such a forward's
  // state, so a training forward (feat) on the float-atomic schedule is refused
  const bool ni64 = cfg->n_importance == kNi64;
  if (ni64 && a->feat && plan.mode != kModeSplit) return HN_E_SHAPE;
  if (a->loss) {   // the composite backward of the training loss done here (only target, world, sparse_w read)
    if (!a->loss->target) return HN_E_NULL;
    if (!(a->loss->world > 0.f)) return HN_E_SHAPE;
    if (plan.mode != kModeSplit) return HN_E_SHAPE;   // only the binned backward can skip its pre-pass
  }
  hipStream_t s = (hipStream_t)stream;
  RenderK k{};   // (no loss: no target, d raw, marks or stamp)
  const WsLayout& L = plan.ws;
  if ((st = field_args(cfg, a->t_vals, a->u, a->table, a->coarse, a->fine, a->weights_packed, workspace, L.Pc, L.Pf,
                       s, k.f)))
    return st;
  k.perturb = cfg->perturb;
  k.B = a->n_rays;
  k.rays = a->rays; k.t_rand = a->t_rand;
  k.noise_c = a->noise_c; k.noise_f = a->noise_f;
  k.rgb = a->rgb; k.depth = a->depth; k.acc = a->acc; k.sparsity = a->sparsity;
  k.rgb0 = a->rgb0; k.depth0 = a->depth0; k.acc0 = a->acc0; k.sparsity0 = a->sparsity0;
  k.z_std = a->z_std; k.z_coarse = a->z_coarse; k.z_fine = a->z_fine;
  k.raw_c = a->raw_c; k.raw_f = a->raw_f; k.fine_src = a->fine_src; k.feat = a->feat;
  // the saved features (32 KB + 6 KB per ray) go through L2 while the table
  // (16 x 2^T x 8 B) leaves room for them in the 256 MiB MALL, where the
  // backward finds them (config 2, T=19: forward 260.7 -> 253.6 us, step
  // -8 us); past it they are streamed (config 3, T=22, cached: forward
  // 633 -> 682 us)
  k.feat_nt = cfg->grid.log2_hashmap_size > 20;
  k.skip_dead = a->skip_dead_color != 0;
  const bool res = (form ? form : fwd_pick_form(a->n_rays, device_cus())) == 2;
  if (a->loss) {
    k.ltarget = a->loss->target;
    loss_factors(a->loss->world, a->loss->sparse_w, a->n_rays, k.lgm, k.lsparse);
    k.draw = ws_at<float>(workspace, L.draw);
    k.uflags = ws_at<uint8_t>(workspace, L.marks);
    k.stamp = ws_stamp(ws_at<int32_t>(workspace, L.lmeta));
  }
  launch_fwd(a->loss != nullptr, ni64, res, a->n_rays, s, k);
  return hip_status(hipGetLastError());
}

// Workspace of hn_render_views / hn_render_image (offsets in floats; the fixed
// grid's, so the same for both importance counts): both nets' packed weights |
// one slot per wave of the persistent grid (its current ray's two coarse
// feature tiles, ImageK::slots)
struct ImageWs {
  size_t Pc, Pf, slots, total;
};
static ImageWs image_ws_layout() {
  WsCursor c;
  ImageWs w;
  w.Pc = c.take(G_END);
  w.Pf = c.take(G_END);
  w.slots = c.take((size_t)kImgBlocks * kImgBlockWaves * kImgSlotFloats);
  w.total = c.at;
  return w;
}

extern "C" size_t hn_render_image_workspace_bytes(const hn_render_cfg* cfg) {
  return check_image_cfg(cfg) ? 0 : image_ws_layout().total * sizeof(float);
}
extern "C" size_t hn_render_views_workspace_bytes(const hn_render_cfg* cfg) {
  return check_cfg(cfg) ? 0 : image_ws_layout().total * sizeof(float);
}

// render_image_kernel<kNiT, kNdc> of a cfg and a launch: the one place that picks the instantiation
static void launch_image(const hn_render_cfg* cfg, hipStream_t s, const ImageK& k) {
  const dim3 grid(kImgBlocks), block(64 * kImgBlockWaves);
  with_bool(cfg->n_importance == kNi64, [&](auto kNi64T) {
    with_bool(k.ndc != 0, [&](auto kNdc) {
      constexpr int ni = decltype(kNi64T)::value ? kNi64 : kNi;
      hipLaunchKernelGGL((render_image_kernel<ni, decltype(kNdc)::value>), grid, block, 0, s, k);
    });
  });
}

// The whole-image renderer behind hn_render_views and hn_render_image(_variant)
// (cfg checked by the entry point, which has made its own refusals): every
// check, then the launch
static int32_t render_views(const hn_render_cfg* cfg, const hn_image_args* a, int32_t ndc, float ndc_sx,
                            float ndc_sy, int32_t variant, void* workspace, size_t ws_bytes, void* stream) {
  int32_t st;
  if (!a) return HN_E_NULL;
  if (cfg->perturb) return HN_E_SHAPE;   // the stratified jitter is the training forward's
  if (a->H <= 0 || a->W <= 0 || a->n_views < 0 || (a->pose_stride != 12 && a->pose_stride != 16)) return HN_E_SHAPE;
  if (variant < 0 || variant > (kImgReencode | kImgRowMajor)) return HN_E_SHAPE;
  if (ndc < 0 || ndc > 1) return HN_E_SHAPE;
  if (a->n_views == 0) return HN_OK;
  if (!a->poses || !a->t_vals || !a->u || !a->table || !mlp_ok(a->coarse) || !mlp_ok(a->fine)) return HN_E_NULL;
  if (!a->rgb || !a->depth || !a->acc) return HN_E_NULL;
  if (!workspace) return HN_E_NULL;
  const ImageWs L = image_ws_layout();
  if (ws_bytes < L.total * sizeof(float)) return HN_E_WORKSPACE;
  ImageK k;
  k.Hb = ((uint32_t)a->H + 1) / 2;
  k.Wb = ((uint32_t)a->W + 1) / 2;
  // the ray groups' index is 32 bits wide (an 8-view batch of 16384 x 16384 images still fits)
  if ((uint64_t)a->H * (uint64_t)a->W > 0x7fffffffull) return HN_E_SHAPE;
  const uint64_t groups = (variant & kImgRowMajor) ? ((uint64_t)a->n_views * a->H * a->W + 3) / 4
                                                   : (uint64_t)a->n_views * k.Hb * k.Wb;
  if (groups > 0x7fffffffull) return HN_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  if ((st = field_args(cfg, a->t_vals, a->u, a->table, a->coarse, a->fine, a->weights_packed, workspace, L.Pc, L.Pf,
                       s, k.f)))
    return st;
  k.variant = variant;
  k.n_views = a->n_views; k.H = a->H; k.W = a->W; k.pose_stride = a->pose_stride;
  k.groups = (uint32_t)groups;
  k.fx = a->fx; k.fy = a->fy; k.cx = a->cx; k.cy = a->cy; k.near = a->near; k.far = a->far;
  k.ndc = ndc; k.sx = ndc_sx; k.sy = ndc_sy;
  k.poses = a->poses;
  k.slots = (variant & kImgReencode) ? nullptr : ws_at<float>(workspace, L.slots);
  k.rgb = a->rgb; k.depth = a->depth; k.acc = a->acc; k.rays = a->rays;
  launch_image(cfg, s, k);
  return hip_status(hipGetLastError());
}

extern "C" int32_t hn_render_views(const hn_render_cfg* cfg, const hn_view_args* a, void* workspace,
                                   size_t ws_bytes, void* stream) {
  const int32_t st = check_cfg(cfg);
  if (st) return st;
  if (!a) return HN_E_NULL;
  return render_views(cfg, &a->image, a->ndc, a->ndc_sx, a->ndc_sy, a->variant, workspace, ws_bytes, stream);
}

extern "C" int32_t hn_render_image_variant(const hn_render_cfg* cfg, const hn_image_args* a, int32_t variant,
                                           void* workspace, size_t ws_bytes, void* stream) {
  const int32_t st = check_image_cfg(cfg);
  if (st) return st;
  return render_views(cfg, a, 0, 0.f, 0.f, variant, workspace, ws_bytes, stream);
}

extern "C" int32_t hn_render_image(const hn_render_cfg* cfg, const hn_image_args* a, void* workspace,
                                   size_t ws_bytes, void* stream) {
  return hn_render_image_variant(cfg, a, 0, workspace, ws_bytes, stream);
}

extern "C" int32_t hn_render_bins(const hn_render_cfg* cfg, int64_t n_rays, int32_t* shift) {
  if (!cfg || !shift) return 0;
  *shift = 0;
  if (check_cfg(cfg)) return 0;
  const BwdPlan plan = bwd_plan(cfg, n_rays);
  if (plan.mode != kModeSplit) return 0;
  *shift = plan.bg.shift;
  return plan.bg.nbins;
}

extern "C" int32_t hn_render_bwd_owner(const hn_render_cfg* cfg, const hn_render_bwd_args* a, void* workspace,
                                       size_t ws_bytes, int32_t bin_lo, int32_t bin_hi, void* stream) {
  int32_t st = check_cfg(cfg);
  if (st) return st;
  if (!a || !workspace) return HN_E_NULL;
  if (!a->owner_defer || a->n_rays <= 0) return HN_E_SHAPE;
  const BwdPlan plan = bwd_plan(cfg, a->n_rays);
  if (plan.mode != kModeSplit) return HN_E_SHAPE;
  if (!a->d_table && !a->table_step) return HN_E_NULL;
  if (ws_bytes < plan.bytes()) return HN_E_WORKSPACE;
  if (bin_lo < 0 || bin_hi > plan.bg.nbins || bin_lo > bin_hi) return HN_E_SHAPE;
  if (bin_lo == bin_hi) return HN_OK;
  launch_owner(owner_args(cfg, a, ws_at<float>(workspace, plan.ws.bins), plan.bg, bin_lo), plan.bg,
               bin_hi - bin_lo, (hipStream_t)stream);
  return hip_status(hipGetLastError());
}

// hn_render_bwd with no rays and a TV term (ABI 14): a data-parallel rank that
// drew no rays still carries the TV term (train.dp_loss puts it on rank 0,
// run_nerf.py:551-555 / :626-635).  Its gradient goes through the same TV
// records, overflow placement and exact fixed-point owner pass as a rendering
// rank's (scatter_bins_kernel with no units and no slab reduction), so it is
// bitwise reproducible where hn_tv_bwd's float atomics are not.
static int32_t tv_only_bwd(const hn_render_cfg* cfg, const hn_render_bwd_args* a, void* workspace,
                           size_t ws_bytes, hipStream_t s) {
  if (!a->g_tv || (!a->d_table && !a->table_step) || !workspace) return HN_E_NULL;
  if (a->d_table_mode < 0 || a->d_table_mode > 3 || a->owner_defer || a->mlp_step || a->repack || a->loss)
    return HN_E_SHAPE;
  const BwdPlan plan = bwd_plan(cfg, 0);
  if (plan.mode != kModeSplit) return HN_E_SHAPE;
  int32_t st = check_table_step(cfg, a);
  if (st) return st;
  TvK tvk;
  bool rec_fit;
  if ((st = check_tv(cfg, a, tvk, rec_fit))) return st;
  if (!rec_fit) return HN_E_SHAPE;
  if (ws_bytes < plan.bytes()) return HN_E_WORKSPACE;
  if (!sc_lds_fits(plan)) return HN_E_SHAPE;
  const BinGeom& bg = plan.bg;
  float* bins = ws_at<float>(workspace, plan.ws.bins);
  // the overflow book starts empty (render_comp_bwd_kernel's zero_ovf_book
  // on a rendering rank): total, per-bin spills, placement cursors
  const OvfBook ob = host_ovf_book(bins, bg, 0);
  if ((st = hip_status(hipMemsetAsync(ob.cnt, 0, (1 + 2 * (size_t)bg.nbins) * sizeof(uint32_t), s)))) return st;
  ScK sk{};
  sk.g = make_grid_args(cfg->grid);
  sk.B = 0;
  sk.g_tv = a->g_tv;
  sc_bins_tv(sk, bins, bg, a->tv, tvk);
  sk.slab = nullptr;   // no MLP gradients: the caller's stay untouched
  hipLaunchKernelGGL(scatter_bins_kernel, dim3(kBwdBlocks), dim3(64 * kScWaves), plan.sc_lds, s, sk);
  if ((st = hip_status(hipGetLastError()))) return st;
  const BinR r = owner_args(cfg, a, bins, bg, 0);   // (a->n_rays is 0 here)
  hipLaunchKernelGGL(ovf_place_kernel, dim3(kBwdBlocks), dim3(kPlaceThreads), 0, s, r, PackK{}, MortonK{},
                     NdcK{}, (unsigned)kBwdBlocks);
  if ((st = hip_status(hipGetLastError()))) return st;
  launch_owner(r, bg, bg.nbins, s);
  return hip_status(hipGetLastError());
}

// The composite pre-pass of either schedule: a wave per (ray, pass), and a
// workgroup ahead of them for the loss value where the call forms one
static void launch_prepass(const B1K& k, hipStream_t s) {
  hipLaunchKernelGGL(render_comp_bwd_kernel, dim3((unsigned)((2 * k.B + kFwdWaves - 1) / kFwdWaves + (k.lout ? 1 : 0))),
                     dim3(64 * kFwdWaves), 0, s, k);
}

// The binned schedule (hn_bwd_binned.h): pre-pass, lists, MLP backward,
// scatter into records (+ the TV term's, tv != NULL; + the dW slabs'
// reduction and the MLP steps), overflow placement (+ the repack), owner pass
// unless deferred to hn_render_bwd_owner.  nk: the next batch's job (NextK;
// validated, no workgroups without one) in the lists and placement launches,
// ndc its NDC step.
static int32_t bwd_binned(const hn_render_cfg* cfg, const hn_render_bwd_args* a, const BwdPlan& plan, const B1K& k,
                          const hn_tv_args* tv, const TvK& tvk, NextK& nk, const NdcK& ndc, void* workspace,
                          hipStream_t s) {
  int32_t st;
  // prepass_done: the training forward left d raw and the marks; the lists
  // kernel checks its stamp and takes the pre-pass's side jobs in one extra
  // workgroup (dense_bwd = 1 runs the same kernel, listing every group)
  const int prepass = a->prepass_done ? 1 : 0;
  if (!prepass) launch_prepass(k, s);
  // the backward's work lists (from the marks)
  const int64_t nlb = (a->n_rays + kListThreads - 1) / kListThreads;
  // (+ the next batch's tile counts and uniform draws, dispatched behind them)
  nk.first = (unsigned)(nlb < kListMaxBlocks ? nlb : kListMaxBlocks) + prepass;
  hipLaunchKernelGGL(render_lists_kernel, dim3(nk.first + (nk.m.n ? nk.m.blocks + uni_blocks(nk.u) : 0u)),
                     dim3(kListThreads), 0, s, k, prepass ? ws_stamp(k.lmeta) : nullptr, nk);
  if ((st = hip_status(hipGetLastError()))) return st;
  hipLaunchKernelGGL((render_bwd_kernel<kSwVmcnt, kModeSplit>), dim3(kBwdBlocks), dim3(64 * kB1Waves),
                     (size_t)kB1LdsF * sizeof(float), s, k);
  if ((st = hip_status(hipGetLastError()))) return st;
  ScK sk;
  sk.g = k.g;
  sk.B = a->n_rays;
  sk.rays = a->rays;
  sk.draw = k.draw;
  sk.scramble = k.scramble;
  sk.skip_zero = k.skip_zero;
  sk.lmeta = k.lmeta;
  sk.slist = k.skip_zero ? ws_at<int32_t>(workspace, plan.ws.ls) : nullptr;   // the scatter's group list
  sk.z_fine = a->z_fine;
  sk.fine_src = a->fine_src;
  sk.dfeat_f = k.dfeat_f;
  sk.dfeat_c = k.dfeat;
  sk.g_tv = a->g_tv;
  sc_bins_tv(sk, k.bins, plan.bg, tv, tvk);
  sk.slab = k.slab;
  sk.dc = a->d_coarse;
  sk.df = a->d_fine;
  sk.overwrite_mlp = (a->d_table_mode & 2) ? 1 : 0;
  sk.has_mstep = a->mlp_step != nullptr;
  for (int t = 0; t < 10; ++t) sk.mstep[t] = sk.has_mstep ? a->mlp_step[t] : hn_radam_tensor{};
  if (k.sf == kSf)
    hipLaunchKernelGGL(scatter_bins_kernel, dim3(kBwdBlocks), dim3(64 * kScWaves), plan.sc_lds, s, sk);
  else
    hipLaunchKernelGGL(scatter_bins_kernel64, dim3(kBwdBlocks), dim3(64 * kScWaves), plan.sc_lds, s, sk);
  if ((st = hip_status(hipGetLastError()))) return st;
  const BinR r = owner_args(cfg, a, k.bins, plan.bg, 0);
  PackK pk{};
  unsigned pblocks = 0;
  if (a->repack) {   // validated: mlp_step given
    pk.c = a->coarse;
    pk.f = a->fine;
    pk.P = ws_at<float>(workspace, plan.ws.Pc);   // [2][G_END]: Pc, then Pf
    pblocks = (unsigned)((2 * G_END + kPlaceThreads - 1) / kPlaceThreads);
  }
  // (+ the next batch's rays: every tile's count is in place since the lists launch)
  const unsigned own = (unsigned)kBwdBlocks + pblocks;
  hipLaunchKernelGGL(ovf_place_kernel, dim3(own + (nk.m.n ? nk.m.blocks : 0u)), dim3(kPlaceThreads), 0, s, r, pk,
                     nk.m, ndc, own);
  if ((st = hip_status(hipGetLastError()))) return st;
  if (!a->owner_defer) {
    launch_owner(r, plan.bg, plan.bg.nbins, s);
    if ((st = hip_status(hipGetLastError()))) return st;
  }
  return HN_OK;
}

// The float-atomic fused schedule (hn_bwd_atomic.h): the table gradient is
// accumulated by atomics, so an overwriting call zeroes it first; pre-pass,
// the fused MLP backward + scatter, the dW slabs' reduction.
static int32_t bwd_atomic(const hn_render_cfg* cfg, const hn_render_bwd_args* a, const B1K& k, hipStream_t s) {
  int32_t st;
  const int T = cfg->grid.log2_hashmap_size;
  if (a->d_table_mode & 1) {
    const size_t tb = ((size_t)16 << T) * 2 * sizeof(float);
    if ((st = hip_status(hipMemsetAsync(a->d_table, 0, tb, s)))) return st;
  }
  launch_prepass(k, s);
  const size_t lds = (size_t)kB1LdsF * sizeof(float);
  // 16 levels x 2^T x 8 B >= 256 MiB from T = 21: the table no longer fits the MALL
  if (T >= 21)
    hipLaunchKernelGGL((render_bwd_kernel<kSwVmcntBig, kModeAtomic>), dim3(kBwdBlocks), dim3(64 * kB1Waves), lds,
                       s, k);
  else
    hipLaunchKernelGGL((render_bwd_kernel<kSwVmcnt, kModeAtomic>), dim3(kBwdBlocks), dim3(64 * kB1Waves), lds, s,
                       k);
  if ((st = hip_status(hipGetLastError()))) return st;
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(kSlabVBlocks), dim3(64 * kSlabGroups), 0, s, k.slab, kBwdBlocks,
                     a->d_coarse, a->d_fine, (a->d_table_mode & 2) ? 1 : 0);
  return hip_status(hipGetLastError());
}

// What hn_render_bwd's checks settle for its launches
struct BwdCall {
  BwdPlan plan;
  TvK tvk;
  // TV term: records of the binned scatter (tv_rec), or hn_tv_bwd into d_table (tv_atomic)
  const hn_tv_args *tv_rec = nullptr, *tv_atomic = nullptr;
  NextK nk{};   // the next batch's job (none: no workgroups)
  NdcK ndc{};   // ... and its NDC step (none: world rays)
};

// Every check of hn_render_bwd: host work only, so a refused call queues
// nothing.  (A call with no rays is left to tv_only_bwd's checks.)
static int32_t check_bwd(const hn_render_cfg* cfg, const hn_render_bwd_args* a, void* workspace, size_t ws_bytes,
                         const hn_ray_ndc* next_ndc, BwdCall& c) {
  int32_t st = check_cfg(cfg);
  if (st) return st;
  if (!a) return HN_E_NULL;
  if (a->n_rays < 0) return HN_E_SHAPE;
  if (next_ndc && !a->next_batch) return HN_E_SHAPE;   // an NDC step of no job
  // the next batch rides the lists and placement launches of a backward that runs both
  if (a->next_batch && (a->n_rays == 0 || a->owner_defer)) return HN_E_SHAPE;
  if (a->n_rays == 0) return HN_OK;
  if (!a->rays || !a->table || !mlp_ok(a->coarse) || !mlp_ok(a->fine)) return HN_E_NULL;
  if (!a->z_coarse || !a->z_fine || !a->raw_c || !a->raw_f || !a->fine_src || !a->feat)
    return HN_E_NULL;
  if ((!a->d_table && !a->table_step) || !grad_ok(a->d_coarse) || !grad_ok(a->d_fine)) return HN_E_NULL;
  if (a->d_table_mode < 0 || a->d_table_mode > 3) return HN_E_SHAPE;
  if (!workspace) return HN_E_NULL;
  c.plan = bwd_plan(cfg, a->n_rays);
  const bool binned = c.plan.mode == kModeSplit;
  if (ws_bytes < c.plan.bytes()) return HN_E_WORKSPACE;
  if (cfg->n_importance == kNi64 && !binned) return HN_E_SHAPE;   // the float-atomic schedule is 64 + 128 only
  if (a->next_batch) {   // hn_sample_batch_morton's checks and codes
    if (!binned) return HN_E_SHAPE;
    const hn_next_batch& nb = *a->next_batch;
    if ((st = make_uni(nb.seed, nb.draws, nb.n_draws, c.nk.u))) return st;
    if ((st = make_morton(nb.sampler, nb.image, nb.c2w, nb.n_rays, nb.rays, nb.target, nb.workspace, nb.ws_bytes,
                          c.nk.m)))
      return st;
    if (c.nk.m.n && (st = make_ndc(next_ndc, c.ndc))) return st;
  }
  if (a->loss) {   // ABI 13: the training loss formed by the pre-pass (hn_render_loss)
    const hn_render_loss& L = *a->loss;
    if (!L.target || !L.rgb || !L.rgb0 || !L.sparsity || !L.sparsity0 || !L.out || (L.n_tv && !L.tv))
      return HN_E_NULL;
    if (L.n_tv < 0 || !(L.world > 0.f)) return HN_E_SHAPE;
  }
  // d raw and marks from the training forward: the binned schedule with the
  // loss formed here, no explicit upstream gradients
  if (a->prepass_done && (!binned || !a->loss || a->g_raw_f || a->g_rgb || a->g_rgb0)) return HN_E_SHAPE;
  // the fused table step lives in the binned scatter's owner pass
  if (a->table_step && !binned) return HN_E_SHAPE;
  if ((st = check_table_step(cfg, a))) return st;
  if (a->tv) {
    bool rec_fit;
    if ((st = check_tv(cfg, a, c.tvk, rec_fit))) return st;
    if (binned && rec_fit) {
      c.tv_rec = a->tv;
    } else {
      if (a->table_step || !a->d_table) return HN_E_SHAPE;
      c.tv_atomic = a->tv;
    }
  }
  if (a->owner_defer && !binned) return HN_E_SHAPE;
  if (a->repack && !a->mlp_step) return HN_E_SHAPE;
  if (a->mlp_step) {   // the MLP steps live in the binned scatter's slab reduction
    if (!binned) return HN_E_SHAPE;
    static constexpr int64_t numel[5] = {W_S1, W_C0 - W_S1, W_C1 - W_C0, W_C2 - W_C1, W_END - W_C2};
    for (int t = 0; t < 10; ++t) {
      const hn_radam_tensor& r = a->mlp_step[t];
      if (!r.p || !r.m || !r.v) return HN_E_NULL;
      if (r.n != numel[t % 5]) return HN_E_SHAPE;
    }
  }
  if (binned && !sc_lds_fits(c.plan)) return HN_E_SHAPE;   // bins beyond the LDS counters' room
  return HN_OK;
}

// The MLP backward's arguments of a checked call
static B1K fill_b1k(const hn_render_cfg* cfg, const hn_render_bwd_args* a, const BwdPlan& plan, void* workspace) {
  const WsLayout& L = plan.ws;
  const bool binned = plan.mode == kModeSplit;
  B1K k{};   // (no loss: none of its inputs, factors 0)
  k.B = a->n_rays;
  if (a->n_rays > 1) {   // else scramble 0
    int bits = 2;
    while ((1ll << bits) < a->n_rays) bits += 2;
    k.scramble = bits / 2;
  }
  k.white = cfg->white_bkgd;
  k.rays = a->rays; k.noise_c = a->noise_c; k.noise_f = a->noise_f;
  k.Pc = ws_at<float>(workspace, L.Pc); k.Pf = ws_at<float>(workspace, L.Pf);
  k.z_coarse = a->z_coarse; k.z_fine = a->z_fine; k.raw_c = a->raw_c; k.raw_f = a->raw_f;
  k.feat = a->feat;
  k.g_rgb = a->g_rgb; k.g_depth = a->g_depth; k.g_acc = a->g_acc; k.g_sparsity = a->g_sparsity;
  k.g_rgb0 = a->g_rgb0; k.g_depth0 = a->g_depth0; k.g_acc0 = a->g_acc0;
  k.g_sparsity0 = a->g_sparsity0; k.g_raw_f = a->g_raw_f;
  k.slab = ws_at<float>(workspace, L.slab);
  k.dfeat = ws_at<float>(workspace, L.dfeat);
  k.draw = ws_at<float>(workspace, L.draw);
  k.uflags = ws_at<uint8_t>(workspace, L.marks);
  k.lmeta = ws_at<int32_t>(workspace, L.lmeta);
  k.lists = ws_at<int32_t>(workspace, L.lc);   // (the kernels find the fine list behind the coarse one)
  k.skip_zero = cfg->dense_bwd ? 0 : 1;
  k.sf = kSc + cfg->n_importance;
  if (a->loss) {
    const hn_render_loss& l = *a->loss;
    loss_factors(l.world, l.sparse_w, a->n_rays, k.lgm, k.lsparse);
    k.ltarget = l.target; k.lrgb = l.rgb; k.lrgb0 = l.rgb0; k.lsp = l.sparsity; k.lsp0 = l.sparsity0;
    k.ltv = l.n_tv ? l.tv : nullptr;
    k.n_tv = l.n_tv;
    k.lworld = l.world; k.lsparse_w = l.sparse_w; k.ltv_w = l.tv_w;
    k.lout = l.out;
  }
  k.g = make_grid_args(cfg->grid);
  k.fine_src = a->fine_src;
  k.d_table = a->d_table;
  k.bins = binned ? ws_at<float>(workspace, L.bins) : nullptr;
  k.bin_cap = plan.bg.cap;
  k.bin_shift = plan.bg.shift;
  k.nbins = plan.bg.nbins;
  k.dfeat_f = binned ? ws_at<float>(workspace, L.dfeat_f) : nullptr;
  return k;
}

extern "C" int32_t hn_render_bwd(const hn_render_cfg* cfg, const hn_render_bwd_args* a,
                                 void* workspace, size_t ws_bytes, void* stream) {
  return hn_render_bwd_ndc(cfg, a, workspace, ws_bytes, nullptr, stream);
}

extern "C" int32_t hn_render_bwd_ndc(const hn_render_cfg* cfg, const hn_render_bwd_args* a, void* workspace,
                                     size_t ws_bytes, const hn_ray_ndc* next_ndc, void* stream) {
  BwdCall c;
  int32_t st = check_bwd(cfg, a, workspace, ws_bytes, next_ndc, c);
  if (st) return st;
  hipStream_t s = (hipStream_t)stream;
  if (a->n_rays == 0) return a->tv ? tv_only_bwd(cfg, a, workspace, ws_bytes, s) : HN_OK;
  const B1K k = fill_b1k(cfg, a, c.plan, workspace);
  // the weights' packed copies, then one schedule; then, under either, a TV
  // term that is not in the records: hn_tv_bwd's atomics into d_table
  const WsLayout& L = c.plan.ws;
  if (!a->weights_packed && (st = mlp_pack2_launch(&a->coarse, ws_at<float>(workspace, L.Pc), &a->fine,
                                                   ws_at<float>(workspace, L.Pf), s)))
    return st;
  if ((st = c.plan.mode == kModeSplit ? bwd_binned(cfg, a, c.plan, k, c.tv_rec, c.tvk, c.nk, c.ndc, workspace, s)
                                      : bwd_atomic(cfg, a, k, s)))
    return st;
  if (c.tv_atomic) return hn_tv_bwd(c.tv_atomic, a->g_tv, a->d_table, stream);
  return HN_OK;
}

// ---- the ray gradient (hn_bwd_rays.h) ----------------------------------------
// Scratch of hn_render_bwd_rays, offsets in floats: its own packed copies of
// both nets | d raw [n][256][4] and the marks [n] (the composite pre-pass
// writes both) | the units' partial sums [n][8][22].  Nothing of it is read
// after the call, and it shares nothing with a render workspace.
struct RaysWs {
  size_t Pc, Pf, draw, marks, part, total;
};
static RaysWs rays_ws_layout(int64_t n_rays) {
  const size_t n = n_rays > 0 ? (size_t)n_rays : 0;
  WsCursor c;
  RaysWs w;
  w.Pc = c.take(G_END);
  w.Pf = c.take(G_END);
  w.draw = c.take(n * (kSc + kSf) * 4, 4);
  w.marks = c.take(n * kMarkB / sizeof(float));
  w.part = c.take(n * kTilesPerRay * kRayPart);
  w.total = c.at;
  return w;
}

extern "C" size_t hn_render_bwd_rays_workspace_bytes(const hn_render_cfg* cfg, int64_t n_rays) {
  return check_cfg(cfg) || n_rays < 0 ? 0 : rays_ws_layout(n_rays).total * sizeof(float);
}

extern "C" int32_t hn_render_bwd_rays(const hn_render_cfg* cfg, const hn_render_bwd_args* a, void* scratch,
                                      size_t bytes, float* d_rays, void* stream) {
  int32_t st = check_cfg(cfg);
  if (st) return st;
  if (!a) return HN_E_NULL;
  if (a->n_rays < 0) return HN_E_SHAPE;
  if (a->loss || a->prepass_done) return HN_E_SHAPE;   // the upstream gradients are the g_* arrays
  if (a->n_rays == 0) return HN_OK;
  if (!a->rays || !a->table || !mlp_ok(a->coarse) || !mlp_ok(a->fine)) return HN_E_NULL;
  if (!a->z_coarse || !a->z_fine || !a->raw_c || !a->raw_f || !a->fine_src || !a->feat) return HN_E_NULL;
  if (!d_rays || !scratch) return HN_E_NULL;
  const RaysWs L = rays_ws_layout(a->n_rays);
  if (bytes < L.total * sizeof(float)) return HN_E_WORKSPACE;
  if ((uint64_t)a->n_rays * kTilesPerRay / kRayWaves > 0x7fffffffull) return HN_E_SHAPE;   // the grid's x extent
  hipStream_t s = (hipStream_t)stream;
  float *Pc = ws_at<float>(scratch, L.Pc), *Pf = ws_at<float>(scratch, L.Pf);
  if ((st = mlp_pack2_launch(&a->coarse, Pc, &a->fine, Pf, s))) return st;
  // the composite pre-pass, as hn_render_bwd launches it: d raw (and the marks, unused here)
  B1K b{};
  b.B = a->n_rays;
  b.white = cfg->white_bkgd;
  b.rays = a->rays; b.noise_c = a->noise_c; b.noise_f = a->noise_f;
  b.z_coarse = a->z_coarse; b.z_fine = a->z_fine; b.raw_c = a->raw_c; b.raw_f = a->raw_f;
  b.g_rgb = a->g_rgb; b.g_depth = a->g_depth; b.g_acc = a->g_acc; b.g_sparsity = a->g_sparsity;
  b.g_rgb0 = a->g_rgb0; b.g_depth0 = a->g_depth0; b.g_acc0 = a->g_acc0; b.g_sparsity0 = a->g_sparsity0;
  b.g_raw_f = a->g_raw_f;
  b.fine_src = a->fine_src;
  b.draw = ws_at<float>(scratch, L.draw);
  b.uflags = ws_at<uint8_t>(scratch, L.marks);
  b.sf = kSc + cfg->n_importance;
  launch_prepass(b, s);
  if ((st = hip_status(hipGetLastError()))) return st;
  RaysK k{};
  k.B = a->n_rays;
  k.sf = b.sf;
  k.nt = (kSc + b.sf) / 32;
  k.rays = a->rays;
  k.Pc = Pc; k.Pf = Pf;
  k.z_coarse = a->z_coarse; k.z_fine = a->z_fine;
  k.feat = a->feat;
  k.draw = b.draw;
  k.table = a->table;
  k.g = make_grid_args(cfg->grid);
  k.part = ws_at<float>(scratch, L.part);
  const int64_t units = a->n_rays * kTilesPerRay;
  hipLaunchKernelGGL(render_bwd_rays_kernel, dim3((unsigned)((units + kRayWaves - 1) / kRayWaves)),
                     dim3(64 * kRayWaves), 0, s, k);
  if ((st = hip_status(hipGetLastError()))) return st;
  RaysR r{};
  r.B = a->n_rays;
  r.nt = k.nt; r.sf = k.sf; r.white = cfg->white_bkgd;
  r.rays = a->rays; r.noise_c = a->noise_c; r.noise_f = a->noise_f;
  r.z_coarse = a->z_coarse; r.z_fine = a->z_fine; r.raw_c = a->raw_c; r.raw_f = a->raw_f;
  r.g_rgb = a->g_rgb; r.g_depth = a->g_depth; r.g_acc = a->g_acc; r.g_sparsity = a->g_sparsity;
  r.g_rgb0 = a->g_rgb0; r.g_depth0 = a->g_depth0; r.g_acc0 = a->g_acc0; r.g_sparsity0 = a->g_sparsity0;
  r.part = k.part;
  r.d_rays = d_rays;
  hipLaunchKernelGGL(render_bwd_rays_reduce_kernel, dim3((unsigned)((a->n_rays + kRayWaves - 1) / kRayWaves)),
                     dim3(64 * kRayWaves), 0, s, r);
  return hip_status(hipGetLastError());
}

// ---- density queries (hn_density.h) ------------------------------------------
// Every check of hn_density_points / hn_density_lattice but the point count's,
// before any launch.
static int32_t density_check(const hn_grid* g, const hn_mlp* w, const float* table, const float* sigma,
                             const uint32_t* occ) {
  if (!g || !w || !table || !mlp_ok(*w) || (!sigma && !occ)) return HN_E_NULL;
  if (int32_t st = check_grid(g)) return st;
  return g->n_levels != 16 ? HN_E_SHAPE : HN_OK;   // encode_tile's 16 levels
}
// Pack the net into the workspace and launch density_kernel<kLattice> over k.n points.
template <bool kLattice>
static int32_t density_launch(const hn_grid* g, const hn_mlp* w, const float* table, DensityK& k, void* workspace,
                              size_t ws_bytes, hipStream_t s) {
  if (!workspace) return HN_E_NULL;
  if (ws_bytes < hn_mlp_workspace_bytes()) return HN_E_WORKSPACE;
  float* P = (float*)workspace;
  if (int32_t st = mlp_pack_launch(w, P, s)) return st;
  k.g = make_grid_args(*g);
  k.table = table;
  k.P = P;
  const int64_t tiles = (k.n + 31) / 32;
  const int cus = device_cus();
  const int64_t resident = (int64_t)(cus > 0 ? cus : 256) * kDenWgPerCu;
  const int64_t blocks = std::min<int64_t>((tiles + kDenWaves - 1) / kDenWaves, resident);
  hipLaunchKernelGGL(density_kernel<kLattice>, dim3((unsigned)blocks), dim3(64 * kDenWaves), 0, s, k);
  return hip_status(hipGetLastError());
}

extern "C" int32_t hn_density_points(const hn_grid* g, const hn_mlp* w, const float* table, const float* x, int64_t n,
                                     float threshold, float* sigma, uint32_t* occ, void* workspace, size_t ws_bytes,
                                     void* stream) {
  if (int32_t st = density_check(g, w, table, sigma, occ)) return st;
  if (n < 0 || n > HN_DENSITY_MAX_POINTS) return HN_E_SHAPE;
  if (n == 0) return HN_OK;
  if (!x) return HN_E_NULL;
  DensityK k{};
  k.x = x;
  k.n = n;
  k.threshold = threshold;
  k.sigma = sigma;
  k.occ = occ;
  return density_launch<false>(g, w, table, k, workspace, ws_bytes, (hipStream_t)stream);
}

extern "C" int32_t hn_density_lattice(const hn_grid* g, const hn_mlp* w, const float* table, const hn_lattice* lat,
                                      float threshold, float* sigma, uint32_t* occ, void* workspace, size_t ws_bytes,
                                      void* stream) {
  if (!lat) return HN_E_NULL;
  if (int32_t st = density_check(g, w, table, sigma, occ)) return st;
  int64_t n = 1;
  for (int a = 0; a < 3; ++a) {   // compared before the multiply: n stays <= HN_DENSITY_MAX_POINTS, no overflow
    if (lat->dims[a] <= 0 || lat->dims[a] > HN_DENSITY_MAX_POINTS / n) return HN_E_SHAPE;
    n *= lat->dims[a];
  }
  DensityK k{};
  k.n = n;
  for (int a = 0; a < 3; ++a) {
    k.lo[a] = lat->lo[a];
    k.step[a] = lat->step[a];
  }
  k.nx = (uint32_t)lat->dims[0];
  k.ny = (uint32_t)lat->dims[1];
  k.threshold = threshold;
  k.sigma = sigma;
  k.occ = occ;
  return density_launch<true>(g, w, table, k, workspace, ws_bytes, (hipStream_t)stream);
}
