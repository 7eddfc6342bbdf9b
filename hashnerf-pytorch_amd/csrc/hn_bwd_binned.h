// hn_bwd_binned.h -- the binned backward schedule (kModeSplit): every
// benchmark line and nearly every test runs it.  Its kernels, in launch
// order after render_comp_bwd_kernel's pre-pass:
//   render_lists_kernel   lists of the 16-sample groups with a nonzero d raw
//                         (+ the next batch's tile counts and uniform draws)
//   render_bwd_kernel     <kSwVmcnt, kModeSplit>: 1,024 waves on equal slices
//                         of the coarse and fine lists (b1_groups), feature
//                         grads stored per point, one dW slab per run of waves
//   scatter_bins_kernel   the feature grads as records per bin (run heads'
//                         x-pairs, staged through LDS), the TV term's
//                         records, then the dW slabs' reduction with the
//                         NeRFSmall RAdam steps
//   ovf_place_kernel      spilled records bucketed by bin (+ the repack,
//                         + the next batch's rays)
//   bin_reduce_kernel     the owner pass: exact fixed-point sums per bin, the
//                         table gradient written once, or the fused table step
// No float atomic reaches memory and every sum has a fixed order, so the
// gradients are bitwise reproducible.
#pragma once
#include "hn_mlp_bwd.h"
#include "hn_sampler.h"

namespace hn {

// hn_render_bwd_args.next_batch: the next step's Morton draw and uniform
// draws (hn_sampler.h), run by workgroups appended to the two small launches
// of this schedule -- pass 1 and the uniforms behind the lists kernel's own
// workgroups, pass 2 behind the placement kernel's, the scatter and MLP
// kernels between them being the boundary the passes need.  `first` = the
// launch's own workgroups (its workgroups from `first` on belong to the job;
// without a job there are none).
struct NextK {
  MortonK m;
  UniK u;
  unsigned first;
};

// ---- binned table-gradient scatter ------------------------------------------
// The memory-side float-atomic rate (~20 G requests/s, one per 64-B segment
// of a wave-instruction) bounds the atomic scatter.  The binned scatter sends
// no float atomic to memory: each run head's x-pair of a corner row becomes
// one 20-B record {4 sums: (x0 f0, x0 f1, x1 f0, x1 f1), entry word}, written
// into the region of its bin (2^bin_shift consecutive table entries,
// level-major); bin_reduce_kernel then owns each bin and writes its slice of
// the gradient once.  Entry word = (l << T) + h(x0) | nbits << 28: the x1
// corner's row is h(x0) ^ ((2^nbits - 1) & mask), since the x prime is 1 and
// x1 = x0 + 1 differs from x0 in its trailing ones and the bit above (nbits
// <= 11 for cells <= 1024, so both rows fall in one 2^13-entry bin).
// Layout (floats from bins): vals f32x4 [nbins][kBwdBlocks][cap] (a bin's
// regions are contiguous for its owner) then the overflow lists
// [kBwdBlocks][ovf_per_block]; idx u32 over the same record index; counts u32
// [nbins][kBwdBlocks]; largest |value| per level f32 [16][kBwdBlocks] (the
// owner's fixed-point scale); then the overflow book (OvfBook).  The producer
// counts its records per bin in LDS (ds_add_rtn); a record past its region's
// capacity goes to the block's own overflow list (one more LDS counter), so
// spilling costs no global atomic.  A block's list holds every record the
// block can make (64 samples x 16 levels x 4 corner rows per unit): clumped
// input (a scene box inside the sample range, where every out-of-box sample
// clamps onto the box surface; the coarse levels of a T = 22 table) spills
// but never runs out.  ovf_place_kernel buckets the spilled records by bin so
// that each owner reads only its own.

// Record r in memory: the values [nrec] f32x4 then the words [nrec] u32.
// Measured and removed (round 2): groups of 4 records = 4 value quads
// then their 4 entry words (80 B), a record's value and word in one line and
// one write stream per region -- measured slower on config 2 (scatter +5 us,
// owner +6.5 us, two A/B pairs on one box): the owner's value loads then span
// 80-B strides instead of dense 1-KiB runs.  Either way the records take
// 5 * nrec floats from `bins` and the book words follow at bins + 5 * nrec
// (ovf_book's idx base = bins + 4 * nrec).
HN_DEV size_t rec_vofs(size_t r) { return 4 * r; }
HN_DEV size_t rec_wofs(size_t r, size_t nrec) { return 4 * nrec + r; }
// A record store.  The staged pool's runs of records (whole lines, read
// once by the owner pass) are written nontemporally; the direct stores (partial
// lines, scattered over the regions) go through L2 as usual, where their
// lines fill up.  Measured (config 2): direct stores nontemporal too, scatter
// 0.197 -> 0.321 ms; staged runs only, scatter and owner both faster (the L2s
// hold fewer dirty record lines to write back).
template <bool kStaged = false>
HN_DEV void rec_put(float* bins, size_t r, size_t nrec, f32x4 v, uint32_t w) {
  f32x4* pv = reinterpret_cast<f32x4*>(bins + rec_vofs(r));
  uint32_t* pw = reinterpret_cast<uint32_t*>(bins) + rec_wofs(r, nrec);
  if (kStaged) {
    __builtin_nontemporal_store(v, pv);
    __builtin_nontemporal_store(w, pw);
  } else {
    *pv = v;
    *pw = w;
  }
}
struct BinW {
  float* bins;
  size_t nrec;
  unsigned long long* lcnt;   // LDS [nbins]: records of the bin (low 32 bits: the slot
                              // counter), records of it in the current staging phase (high 32)
  uint32_t* lovf;      // LDS: this block's overflow records
  size_t base;         // first record of this block's region of bin 0
  size_t stride;       // records between a block's regions of consecutive bins
  size_t ovf_base;     // first record of this block's overflow list
  uint32_t n_ovf;      // its length
  uint32_t cap, shift;
};

__host__ __device__ inline int64_t sc_units_per_block(int64_t n_rays) {   // scatter_bins_kernel: 3 units per ray
  return (3 * (n_rays > 0 ? n_rays : 1) + kBwdBlocks - 1) / kBwdBlocks;
}
// TV records (the scatter blocks' share of the x-pairs, cubes <= kTvRecMaxCube):
// at most L x ((c + 2) / 2) x (c + 1)^2 pairs over the 256 blocks
constexpr int kTvRecMaxCube = 50;
constexpr size_t kTvRecPerBlock = (16 * ((kTvRecMaxCube + 2) / 2) * (kTvRecMaxCube + 1) * (kTvRecMaxCube + 1) +
                                   kBwdBlocks - 1) / kBwdBlocks;
// a producer's overflow list holds everything it can write: its units' render
// records (64 samples x 16 levels x 4 corner rows each) plus its TV share
__host__ __device__ inline size_t ovf_per_block(int64_t n_rays) {
  return (size_t)sc_units_per_block(n_rays) * 64 * 64 + kTvRecPerBlock;
}
__host__ __device__ inline size_t bin_records(int nbins, int cap, int64_t n_rays) {
  return (size_t)kBwdBlocks * nbins * cap + (size_t)kBwdBlocks * ovf_per_block(n_rays);
}
// Overflow book, u32 words after the counts and level maxima (idx + nrec +
// kBwdBlocks * (nbins + 16)): total spilled, spilled per bin, placement
// cursors, first slot per bin, the scatter blocks' slab-block counter,
// spilled per producer block, record ids (relative to the first overflow
// record) bucketed by bin.  All of it lives in the call's workspace, so
// concurrent hn_render_bwd calls with their own workspaces share nothing.
struct OvfBook {
  uint32_t *cnt, *per_bin, *cur, *first, *slab_next, *blk, *ids;
};
__host__ __device__ inline size_t ovf_book_words(int nbins, int64_t n_rays) {
  return 2 + 3 * (size_t)nbins + kBwdBlocks + (size_t)kBwdBlocks * ovf_per_block(n_rays);
}
__host__ __device__ inline OvfBook ovf_book(uint32_t* idx, size_t nrec, int nbins) {
  OvfBook o;
  o.cnt = idx + nrec + (size_t)kBwdBlocks * (nbins + 16);
  o.per_bin = o.cnt + 1;
  o.cur = o.per_bin + nbins;
  o.first = o.cur + nbins;
  o.slab_next = o.first + nbins;
  o.blk = o.slab_next + 1;
  o.ids = o.blk + kBwdBlocks;
  return o;
}

// max(|a|, |b|, m) for m >= 0 as one v_max3_f32 with abs modifiers: the
// compiler's fmaxf in IEEE mode first quiets each input (v_max_f32 x, x), two
// extra instructions per value.  Plain VALU operands (no MFMA or DPP result
// read here), so the asm needs no hazard padding; the values are finite (a
// non-finite one has already set the fault bit).
HN_DEV float max3_abs(float a, float b, float m) {
  float r;
  asm("v_max3_f32 %0, |%1|, |%2|, %3" : "=v"(r) : "v"(a), "v"(b), "v"(m));
  return r;
}

// Segmented suffix sum over runs of samples in one voxel along a 16-lane
// DPP row: lane pp absorbs lane pp + d iff no
// run head lies in (pp, pp + d]; pm = the row's head mask.  s1..s8:
// wave-uniform "some run is longer than 1 / 2 / 4 / 8" (steps skipped when
// no row needs them; a lane whose row does not, absorbs nothing).
// v + (same ? o : 0) is computed as fma(o, same, v): fma(o, 1, v) rounds
// like v + o, and fma(o, 0, v) = v (up to the sign of a zero v, which no
// record value carries into the owner's integer sums).
// All 4 corner rows of a level at once (the runs, and so `same`, are the
// rows' common ones), each step 16 v_fmac_f32_dpp: left to the compiler, the
// fma is packed into v_pk_fma_f32, which cannot take a DPP source, with a
// v_mov_b32_dpp per value (r05: scatter 0.213 -> 0.202 ms).
#define HN_SEG_FMAC(C, E, D) \
  "v_fmac_f32_dpp %[v" #C #E "], %[v" #C #E "], %[sf] row_shl:" #D " row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
// The steps as one asm block with wave-uniform branches inside (n = steps
// to run): the 16 values enter and leave once, without the copies the
// compiler puts at the joins of separately branched blocks.  Step d's `same`
// is computed in the block (v_cmp writes vcc, s_nop 1 before the v_cndmask
// reads it, as the compiler does); its 4 instructions also give the first
// DPP read its 2 wait states.
#define HN_SEG_SAME(M)                                                                                       \
  "v_lshrrev_b32 %[t], %[sh], %[pm]\n"                                                                       \
  "v_and_b32 %[t], " #M ", %[t]\n"                                                                           \
  "v_cmp_eq_u32 vcc, 0, %[t]\n"                                                                              \
  "s_nop 1\n"                                                                                                \
  "v_cndmask_b32_e64 %[sf], 0, 1.0, vcc\n"
#define HN_SEG_BODY(D)                                                                                       \
  HN_SEG_FMAC(0, 0, D) HN_SEG_FMAC(0, 1, D) HN_SEG_FMAC(0, 2, D) HN_SEG_FMAC(0, 3, D) HN_SEG_FMAC(1, 0, D)    \
  HN_SEG_FMAC(1, 1, D) HN_SEG_FMAC(1, 2, D) HN_SEG_FMAC(1, 3, D) HN_SEG_FMAC(2, 0, D) HN_SEG_FMAC(2, 1, D)    \
  HN_SEG_FMAC(2, 2, D) HN_SEG_FMAC(2, 3, D) HN_SEG_FMAC(3, 0, D) HN_SEG_FMAC(3, 1, D) HN_SEG_FMAC(3, 2, D)    \
  HN_SEG_FMAC(3, 3, D)
HN_DEV void seg_sum16(float (&v)[4][4], uint32_t pm, int pp, bool s1, bool s2, bool s4, bool s8) {
  // wave-uniform (from ballots); readfirstlane keeps it in an SGPR
  const int n = __builtin_amdgcn_readfirstlane(s1 ? (s2 ? (s4 ? (s8 ? 4 : 3) : 2) : 1) : 0);
  float t, sf;
  asm("s_cmp_eq_u32 %[n], 0\n s_cbranch_scc1 Lseg_end%=\n"
      HN_SEG_SAME(1) HN_SEG_BODY(1)
      "s_cmp_eq_u32 %[n], 1\n s_cbranch_scc1 Lseg_end%=\n"
      HN_SEG_SAME(3) HN_SEG_BODY(2)
      "s_cmp_eq_u32 %[n], 2\n s_cbranch_scc1 Lseg_end%=\n"
      HN_SEG_SAME(15) HN_SEG_BODY(4)
      "s_cmp_eq_u32 %[n], 3\n s_cbranch_scc1 Lseg_end%=\n"
      HN_SEG_SAME(0xff) HN_SEG_BODY(8)
      "Lseg_end%=:\n"
      : [v00] "+v"(v[0][0]), [v01] "+v"(v[0][1]), [v02] "+v"(v[0][2]), [v03] "+v"(v[0][3]),
        [v10] "+v"(v[1][0]), [v11] "+v"(v[1][1]), [v12] "+v"(v[1][2]), [v13] "+v"(v[1][3]),
        [v20] "+v"(v[2][0]), [v21] "+v"(v[2][1]), [v22] "+v"(v[2][2]), [v23] "+v"(v[2][3]),
        [v30] "+v"(v[3][0]), [v31] "+v"(v[3][1]), [v32] "+v"(v[3][2]), [v33] "+v"(v[3][3]),
        [t] "=&v"(t), [sf] "=&v"(sf)
      : [n] "s"(n), [sh] "v"((uint32_t)pp + 1u), [pm] "v"(pm)
      : "vcc", "scc");
}
#undef HN_SEG_SAME
#undef HN_SEG_BODY
#undef HN_SEG_FMAC

// round(v * 2^S) as int64 without f64 arithmetic: x = v * 2^S is exact in fp32
// (|x| < 2^47, a power-of-2 scale), a = trunc(x / 2^16) is an exact integer
// (|a| < 2^31),
// b = x - a * 2^16 exact with |b| < 2^16, and round(x) = a * 2^16 + rint(b)
// (ties to even agree: a * 2^16 is even).
HN_DEV long long fx_of(float v, float scale) {
  const float x = v * scale;
  const float a = truncf(x * 0x1p-16f);
  const float b = __builtin_fmaf(-a, 0x1p16f, x);
  return ((long long)(int32_t)a << 16) + (long long)(int32_t)rintf(b);
}

// A run head's record: the x-pair (x0 = cx, x1 = cx + 1) of corner row (yy, zz)
// (the y / z coordinates times their primes) at level l.  rec_slot takes the
// record's slot in its bin (LDS counter); rec_store writes it -- split so a
// caller can have several counter round trips in flight.
struct RecSlot {
  uint32_t word, bin, slot, pj;   // pj: the record's index among the bin's records of the staging phase
};
// staged = count the record in the bin's staging-phase half too (one 64-bit
// LDS add returns both counts: the staging index needs no separate read of
// the phase's first slot)
constexpr unsigned long long kCntRec = 1ull, kCntStaged = (1ull << 32) | 1ull;
HN_DEV RecSlot rec_slot(const BinW& bw, uint32_t l, uint32_t log2T, uint32_t cx, uint32_t yy, uint32_t zz,
                        unsigned long long inc = kCntRec) {
  const uint32_t mask = (1u << log2T) - 1u;
  const uint32_t flat = (l << log2T) + ((cx ^ yy ^ zz) & mask);
  const uint32_t nbits = (uint32_t)__builtin_ctz(~cx) + 1u;
  RecSlot r;
  r.word = flat | (nbits << 28);
  r.bin = flat >> bw.shift;
  const unsigned long long old =
      __hip_atomic_fetch_add(bw.lcnt + r.bin, inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  r.slot = (uint32_t)old;
  r.pj = (uint32_t)(old >> 32);
  return r;
}
HN_DEV void rec_store(const BinW& bw, const RecSlot& rs, const float (&v)[4]) {
  size_t r = bw.base + (size_t)rs.bin * bw.stride + rs.slot;
  bool ok = true;
  if (rs.slot >= bw.cap) {
    const uint32_t o = __hip_atomic_fetch_add(bw.lovf, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    ok = o < bw.n_ovf;   // always, by the list's size
    r = bw.ovf_base + o;
    if (!ok) __hip_atomic_fetch_or(&g_hn_fault, kFaultBins, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (ok) {
    rec_put(bw.bins, r, bw.nrec, f32x4{v[0], v[1], v[2], v[3]}, rs.word);
  }
}

// Voxel of one (point, level) for the split scatter: the cell from cell_floor
// (the forward's), the weights by the reference's IEEE divisions.
HN_DEV void voxel_cw_sc(const GridArgs& g, const float* gsl, const float pt[3], const float xc[3], int l,
                        int32_t cell[3], float w[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float gs = gsl[3 * l + a];
    const int32_t i = cell_floor(xc[a] - g.bmin[a], gs, gsl[kGsRcp + 3 * l + a]);
    const float vmin = (float)i * gs + g.bmin[a];
    const float vmax = vmin + gs;
    w[a] = div_rn(pt[a] - vmin, vmax - vmin);
    cell[a] = i;
  }
}

// ---- the table-gradient scatter as its own kernel --------------------------
// render_bwd_kernel stores each tile's feature grads; scatter_bins_kernel
// then runs the scatter at full occupancy (16 waves per CU).  A wave's unit is
// four listed 16-sample groups (dense_bwd: a third of one ray's 192 fine
// samples), lane = sample: its point o + d z, its grads (fine + coarse twin,
// in that order), its voxel computed once per level; per corner row the
// x-pair sums over runs of samples in one voxel (16-lane rows) and one record
// per run head.  Block b is producer b of the record layout (kBwdBlocks
// blocks).
constexpr int kScWaves = 16;
constexpr int kScMaxBinsLog2 = 13;
constexpr int kScMaxBins = 1 << kScMaxBinsLog2;   // LDS counters (32 KiB): T <= 22 at 2^13 entries per bin
constexpr int kBinShift = 13;   // preferred log2 entries per bin (bin_geom)

// Record staging: level-major phases across the block's waves (all 16 waves
// take level l of their units, then the block syncs), each head lane's record
// put into an LDS pool at (bin of the level, slot - the bin's first slot of the
// phase) and the pool flushed by the block in slot order: a bin's records of
// the phase leave as contiguous runs (one 16-B value and one word per lane,
// consecutive lanes on consecutive slots) instead of 64 scattered 16-B and 4-B
// stores per instruction.  Records past the pool's share of their bin (2^kStLog2
// records over the level's bins) or past the region's capacity are stored
// directly.  The slot of every record is the same as without staging, so the
// record buffer, and the owner's sums, are identical.  Measured (r03g, config
// 2): WRITE_SIZE 548 -> 395 MB per launch for 352 MB of records (1.56x ->
// 1.12x), backward launch time unchanged (0.813 / 0.814 vs 0.813 / 0.812 ms):
// the scatter waits on its own dependency chains (SQ_WAIT_INST_ANY 44% of its
// wave cycles), not on the write traffic.
constexpr int kStLog2 = 12, kStPool = 1 << kStLog2;   // 64 KiB of values + 16 KiB of words
constexpr int kStMinLog2C = 3;                          // fewer than 8 records per bin: no staging
struct StPhase {
  int b0, log2c;   // first bin of the phase's levels, log2 pool records per bin (< kStMinLog2C: direct)
  int nbl;         // bins of the phase's levels
};
// a staging phase: levels l .. l + 2^lg2n - 1 (their bins are consecutive;
// several levels per phase only where every level owns whole bins)
HN_DEV StPhase st_phase(int l, int log2T, int shift, int lg2n = 0) {
  StPhase ph;
  ph.b0 = (int)(((uint32_t)l << log2T) >> shift);
  const int lg = log2T > shift ? log2T - shift : 0;
  ph.nbl = 1 << (lg + lg2n);
  ph.log2c = kStLog2 - lg - lg2n;
  return ph;
}
// log2 levels per staging phase where the pool still holds 8 records per bin
// (one block barrier pair per phase; r05h: 1 level 0.984-0.987 ms per step,
// 2: 0.988-1.005, 4: 1.012-1.014, 8: 1.037-1.039)
constexpr int kScLpp = 1;

// kFineT: the ray's fine samples (kSf, or kSf64 with 64 importance samples) --
// the stride of the caller's z_fine and fine_src, and the dense form's units
// per ray; a textual shape of the one definition in hn_scatter_bins_def.h, which
// is included for scatter_bins_kernel (kSf) and scatter_bins_kernel64 (kSf64).
// (dfeat_f, d raw and the lists keep kSf's strides.)
#define HN_SC_KERNEL scatter_bins_kernel
#define HN_SC_FINE kSf
#include "hn_scatter_bins_def.h"
#undef HN_SC_KERNEL
#undef HN_SC_FINE
#define HN_SC_KERNEL scatter_bins_kernel64
#define HN_SC_FINE kSf64
#include "hn_scatter_bins_def.h"
#undef HN_SC_KERNEL
#undef HN_SC_FINE

// ---- the MLP backward over the work lists -----------------------------------
// The coarse and fine tiles share one code path (the pass is a runtime flag:
// weights, d raw offset, tile index and destination are selects), so the
// kernel holds ONE copy of b1_tile: ~25 KB of code, under the 64 KB
// instruction cache two CUs share.
// A tile whose 32 samples all have d raw = 0 (raw2outputs' backward gives
// exactly that to every sample with relu(sigma) = 0: alpha = 0, weight 0,
// run_nerf_helpers.py:577-628) has an exactly zero MLP backward: zero
// feature grads, and it adds 0 to every dW accumulator.  Such tiles are
// skipped -- the same results (an accumulator plus exact zeros is unchanged)
// for ~2/3 of the tiles of a trained scene (config 2: 57 % of the coarse and
// 70 % of the fine tiles, scripts/zero_grad_frac.py).
// Nothing is stored for them: the scatter kernel reads a sample's feature
// grads only where its own d raw (or its coarse twin's) is nonzero.  The
// weight ring is aligned to the tile period, so a skipped unit leaves it
// ready for the next one.  The composite pre-pass marks the tiles with a
// nonzero d raw (B1K::uflags), and the waves run lists of the marked tiles
// (render_bwd_kernel): the same loop shape as over every tile (a per-tile
// test inside the loop made the register allocator spill).
// One MLP tile of two listed 16-sample groups (round 6): points 0-15 group
// code ca, 16-31 group cb (codes ray << 4 | group; cb < 0: none, those lanes
// run with d raw 0 and store nothing).  Each lane's ray gives its own SH
// columns, and color_net.0's SH half is formed for both groups' rays at once
// (column p of that product is point p's ray), kept in LDS per group.  The
// two groups are often of different rays; every per-point input (features,
// masks, d raw) is read at the point's own place in the ray's tiles and its
// feature grads are written there, so the dW products and grads are those of
// the dense form's tiles, grouped differently.
HN_DEV void b1_groups(const B1K& k, int ca, int cb, bool fine, float* X, DW& dw, WRing& wr) {
  const int lane = lane_id();
  const int p = lane & 31, h = lane >> 5;
  const bool none = p >= 16 && cb < 0;
  const int code = p < 16 || cb < 0 ? ca : cb;
  const int64_t ray = code >> 4;
  const int i = 16 * (code & 15) + (p & 15);          // the point within its pass
  float4 dr = *reinterpret_cast<const float4*>(k.draw + ((size_t)ray * (kSc + kSf) + (fine ? kSc : 0) + i) * 4);
  if (none) dr = make_float4(0.f, 0.f, 0.f, 0.f);
  const float* P = opaque_ptr(fine ? k.Pf : k.Pc);
  Ray r;
  load_ray(k.rays, ray, r);
  const C0Sh c0sh = c0sh_setup<true>(P, r, X, lane);
  // the point's place in the saved tiles: tile (pass offset + i / 32), lane (i % 32) + 32 h
  const int ctile = (fine ? kSc / 32 : 0) + (i >> 5), pl = (i & 31) + 32 * h;
  const float* fb = k.feat + (size_t)ray * HN_RENDER_FEAT_PER_RAY;
  f32x16 feat;
  {
    const f32x4* t = reinterpret_cast<const f32x4*>(fb + (size_t)ctile * 1024);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const f32x4 v = __builtin_nontemporal_load(t + 64 * c + pl);
      feat[4 * c] = v.x; feat[4 * c + 1] = v.y; feat[4 * c + 2] = v.z; feat[4 * c + 3] = v.w;
    }
  }
  uint32_t sm[3];
  {
    const uint32_t* t = reinterpret_cast<const uint32_t*>(fb + kTilesPerRay * 1024) + ctile * kMaskWordsPerTile;
#pragma unroll
    for (int j = 0; j < 3; ++j) sm[j] = __builtin_nontemporal_load(t + 64 * j + pl);
  }
  const f32x16 dfeat = b1_tile(P, wr, X, feat, c0sh, dr, dw, sm);
  // this point's feature grads (the saved-feature tile order of both passes)
  if (!none) {
    f32x4* dst = fine ? reinterpret_cast<f32x4*>(k.dfeat_f + ((size_t)ray * (kSf / 32) + (i >> 5)) * 1024)
                      : reinterpret_cast<f32x4*>(k.dfeat + (size_t)ray * kDcRay + (size_t)(i >> 5) * 1024);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const f32x4 v = f32x4{dfeat[4 * c], dfeat[4 * c + 1], dfeat[4 * c + 2], dfeat[4 * c + 3]};
      __builtin_nontemporal_store(v, dst + 64 * c + pl);   // read once, by the scatter
    }
  }
}

// The binned scatter's overflow book starts empty (count, per bin, cursors,
// the scatter blocks' slab-block counter): reset by workgroup 0 of the first
// kernel of the backward.
HN_DEV void zero_ovf_book(const B1K& k) {
  const size_t nrec = bin_records(k.nbins, k.bin_cap, k.B);
  uint32_t* o = ovf_book(reinterpret_cast<uint32_t*>(k.bins + 4 * nrec), nrec, k.nbins).cnt;
  for (int i = threadIdx.x; i < 1 + 2 * k.nbins; i += blockDim.x) o[i] = 0u;
  if (threadIdx.x == 0) o[1 + 3 * k.nbins] = 0u;   // the scatter kernel's slab-block counter (ob.slab_next)
}

// The backward's work lists (round 6), from the composite pre-pass's marks
// (B1K::uflags; every group with dense_bwd): the coarse and the fine 16-sample
// groups with a nonzero d raw (the MLP backward's) and the fine groups with
// feature grads (the scatter's), each in ray order, as
// codes (ray << 4 | 16-sample group); their lengths and the MLP waves' coarse / fine
// split.  Workgroup w writes the codes of rays [w R, (w + 1) R): it counts
// the marks of every earlier ray itself (a few loads per thread; no
// workgroup waits for another), then takes 256 rays at a time, one per
// thread, with a block-wide prefix of their counts.  (One 1,024-thread
// workgroup for the whole batch took 14 us; computed redundantly by every
// block of the kernels that use the lists it cost the MLP backward ~28 us.)
constexpr int kListThreads = 256;
constexpr int kListMaxBlocks = 64;
static_assert(kListMaxBlocks + 1 <= (int)kStampCount, "the stamp's low byte counts the lists kernel's workgroups");
// What one workgroup's atomic add saw of the forward's stamp: valid for
// n_rays when it is that stamp plus the adds of at most the other workgroups;
// the workgroup that saw all the others' clears it.
HN_DEV bool stamp_check(unsigned long long* stamp, unsigned long long seen, int64_t n_rays, int n_groups) {
  const bool ok = (seen & ~kStampCount) == stamp_word(n_rays) && (int)(seen & kStampCount) < n_groups;
  if (ok && (int)(seen & kStampCount) == n_groups - 1) *stamp = 0ull;
  return ok;
}
HN_DEV int list_block_scan(int v, int* sh) {   // inclusive scan over the workgroup; sh: 4 ints of LDS
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  __syncthreads();   // sh free (its previous use is complete)
  if (lane == 63) sh[wave] = v;
  __syncthreads();
  for (int q = 0; q < wave; ++q) v += sh[q];
  return v;
}
HN_DEV int list_block_sum(int v, int* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}
// stamp (hn_render_bwd_args.prepass_done; NULL otherwise): the training
// forward wrote d raw and the marks, no pre-pass ran, and this is the
// backward's first kernel.  One extra workgroup, dispatched first, takes the
// pre-pass's two side jobs (the overflow book, the loss value).  Every
// workgroup checks the forward's stamp with one atomic add (asked for at
// once, looked at after the counting loop, which reads marks inside the
// workspace whatever they hold); without a stamp for these n_rays the kernel
// raises kFaultPrepass, leaves the lists alone and reports them empty.  The
// workgroup whose add came last clears the stamp: one backward per training
// forward.
__global__ __launch_bounds__(kListThreads) void render_lists_kernel(B1K k, unsigned long long* stamp, NextK nk) {
  static_assert(kListThreads == 256, "list_block_scan: 4 waves");
  if (blockIdx.x >= nk.first) {   // the next batch: dispatched behind the lists' own workgroups
    const unsigned j = blockIdx.x - nk.first;
    if (j < nk.m.blocks)
      morton_count_block<kListThreads>(nk.m, j);
    else
      uniform_block<kListThreads>(nk.u, j - nk.m.blocks);
    return;
  }
  __shared__ int sh[3][4];
  __shared__ int stamp_ok;
  const int t = threadIdx.x;
  int bx = (int)blockIdx.x, nbx = (int)nk.first;
  unsigned long long seen = 0ull;
  if (stamp) {
    if (t == 0) seen = __hip_atomic_fetch_add(stamp, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (bx == 0) {
      zero_ovf_book(k);   // binned scatter: no overflow records yet
      loss_fwd_block<kListThreads>(k.lrgb, k.lrgb0, k.ltarget, k.lsp, k.lsp0, k.B, k.ltv, k.n_tv, k.lworld,
                                   k.lsparse_w, k.ltv_w, k.lout);
      if (t == 0 && !stamp_check(stamp, seen, k.B, nbx)) {
        raise_fault(kFaultPrepass);
        for (int i = 0; i < 4; ++i) k.lmeta[i] = 0;   // no units: the kernels behind this one touch no ray
      }
      return;
    }
    --bx;
    --nbx;
  }
  // bits [coarse groups (4), -, fine groups (12), the scatter's groups (12)];
  // a 128-sample fine pass has 8 of each (bits 8-15, 20-27)
  const uint32_t dense = k.sf == kSf ? 0xffffff0fu : 0x0ff0ff0fu;
  auto mword = [&](int64_t r) -> uint32_t {
    return k.skip_zero ? *reinterpret_cast<const uint32_t*>(k.uflags + kMarkB * r) : dense;
  };
  const int64_t R = (k.B + nbx - 1) / nbx;
  const int64_t ra = (int64_t)bx * R, rb = ra + R < k.B ? ra + R : k.B;
  // the counts of the rays before this workgroup's range, and of all rays
  int bc = 0, bf = 0, bs = 0, tc = 0, tf = 0, ts = 0;
  for (int64_t r = t; r < k.B; r += kListThreads) {
    const uint32_t w = mword(r);
    const int c = __builtin_popcount(w & 15u), f = __builtin_popcount((w >> 8) & 0xfffu),
              g = __builtin_popcount(w >> 20);
    tc += c; tf += f; ts += g;
    if (r < ra) { bc += c; bf += f; bs += g; }
  }
  if (stamp && t == 0) stamp_ok = stamp_check(stamp, seen, k.B, nbx + 1) ? 1 : 0;
  int64_t xc = list_block_sum(bc, sh[0]), xf = list_block_sum(bf, sh[1]), xs = list_block_sum(bs, sh[2]);
  if (stamp && !stamp_ok) return;   // (written before list_block_sum's barriers)
  const int64_t Nc = list_block_sum(tc, sh[0]), Nf = list_block_sum(tf, sh[1]), Ns = list_block_sum(ts, sh[2]);
  int32_t* lc = k.lists;
  int32_t* lf = lc + 4 * k.B;
  int32_t* ls = lf + 12 * k.B;
  for (int64_t r0 = ra; r0 < rb; r0 += kListThreads) {
    const int64_t r = r0 + t;
    const uint32_t w = r < rb ? mword(r) : 0u;
    const int c = __builtin_popcount(w & 15u), f = __builtin_popcount((w >> 8) & 0xfffu),
              g = __builtin_popcount(w >> 20);
    const int ic = list_block_scan(c, sh[0]), jf = list_block_scan(f, sh[1]), ks = list_block_scan(g, sh[2]);
    int64_t oc = xc + ic - c, of = xf + jf - f, os = xs + ks - g;
    for (int i = 0; i < 4; ++i)
      if ((w >> i) & 1u) lc[oc++] = (int32_t)(r << 4) | i;
    for (int i = 0; i < 12; ++i)
      if ((w >> (8 + i)) & 1u) lf[of++] = (int32_t)(r << 4) | i;
    for (int i = 0; i < 12; ++i)
      if ((w >> (20 + i)) & 1u) ls[os++] = (int32_t)(r << 4) | i;
    xc += list_block_sum(c, sh[0]);
    xf += list_block_sum(f, sh[1]);
    xs += list_block_sum(g, sh[2]);
  }
  if (bx == 0 && t == 0) {
    const int G = kB1Waves * kBwdBlocks;
    int gc = Nc > 0 ? G : 0;   // MLP waves on the coarse list, in proportion to the lists
    if (Nc > 0 && Nf > 0) {
      gc = (int)((2 * (int64_t)G * Nc + Nc + Nf) / (2 * (Nc + Nf)));
      gc = gc < 1 ? 1 : (gc > G - 1 ? G - 1 : gc);
    }
    k.lmeta[0] = (int32_t)Nc;
    k.lmeta[1] = (int32_t)Nf;
    k.lmeta[2] = (int32_t)Ns;
    k.lmeta[3] = gc;
  }
}

// render_bwd_kernel<kSwVmcnt, kModeSplit>, the binned schedule's (only)
// instantiation of the MLP-backward kernel (declared in hn_mlp_bwd.h): the MLP
// backward over balanced tile lists (round 6).  The 16-sample groups with a
// nonzero d raw (the composite pre-pass's marks; all of them with dense_bwd)
// form two lists in ray order -- coarse groups, then fine groups,
// render_lists_kernel -- and the kB1Waves x nb MLP waves g = 4 * block + wave
// split them: the first gsplit waves the coarse list, the others the fine
// list, in contiguous slices of equal length (gsplit in proportion to the two
// lists).  Every wave then runs ~1/1024 of the work, whatever the scene leaves
// nonzero; each wave keeps one net's dW.  A tile is two consecutive listed
// groups (b1_groups).  A wave reads its codes 64 at a time (one vector load;
// the tile loop takes them by readlane).
// Then the block's waves g0 .. g0 + 3 -- the coarse net below gsplit, the
// fine one from there -- sum each run of same-net waves into its first wave
// (wave order, through `red`: the block's LDS), which alone stores slab g;
// scatter_bins_kernel's slab reduction sums these leaders' slabs in g order:
// deterministic (the split is a function of the marks alone).
// The LDS (kB1LdsF floats at launch, laid out in hn_mlp_bwd.h): this schedule
// uses the waves' operand images X, and all of it as `red`; the staged grid
// sizes and the zeroed flags behind the images are not read here.
template <>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void render_bwd_kernel<kSwVmcnt, kModeSplit>(B1K k) {
  extern __shared__ f32x4 smem4[];
  f32x4* const red = smem4;
  float* smem = reinterpret_cast<float*>(smem4);
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  float* X = smem + wave * kRRows * kXS;
  float* gsl = smem + kB1GslF;
  int* sync = reinterpret_cast<int*>(gsl + kGsLds);
  stage_grid_sizes(k.g, gsl);
  if (threadIdx.x < kSyncInts) sync[threadIdx.x] = 0;
  __syncthreads();
  const int64_t nb = gridDim.x, B = k.B;
  const int blk = (int)blockIdx.x;
  DW dw;
  dw_zero(dw);
  WRing wr;
  const int wv = __builtin_amdgcn_readfirstlane(wave);    // wave-uniform (SGPR)
  const int64_t Nc = __builtin_amdgcn_readfirstlane(k.lmeta[0]), Nf = __builtin_amdgcn_readfirstlane(k.lmeta[1]);
  const int gc = __builtin_amdgcn_readfirstlane(k.lmeta[3]);
  static_assert(kB1Waves == 4 && kSlabSlots == kB1Waves, "slab_reduce_block's run leaders: 4 waves per block");
  const int G = kB1Waves * (int)nb, g_me = blk * kB1Waves + wv;
  const bool fine = g_me >= gc;                            // wave-uniform
  const int64_t N = fine ? Nf : Nc;
  const int gi = fine ? g_me - gc : g_me, GG = fine ? G - gc : gc;
  // slices of whole group pairs (a tile = two consecutive listed groups)
  const int64_t NP = (N + 1) / 2;
  const int64_t lo = GG ? 2 * ((int64_t)gi * NP / GG) : 0, hi2 = GG ? 2 * ((int64_t)(gi + 1) * NP / GG) : 0;
  const int64_t hi = hi2 < N ? hi2 : N;
  const int32_t* L = k.lists + (fine ? 4 * B : 0);
  wring_prime(wr, fine ? k.Pf : k.Pc, lane);
  for (int64_t c0 = lo; c0 < hi; c0 += 64) {   // lo even: pairs never straddle
    const int cnt = (int)(hi - c0 < 64 ? hi - c0 : 64);
    const int codes = lane < cnt ? L[c0 + lane] : -1;
    for (int j = 0; j < cnt; j += 2) {
      const int ca = __builtin_amdgcn_readlane(codes, j);
      const int cb = j + 1 < cnt ? __builtin_amdgcn_readlane(codes, j + 1) : -1;
      b1_groups(k, ca, cb, fine, X, dw, wr);
    }
  }
  const int g0 = blk * kB1Waves;
  for (int w = 1; w < kB1Waves; ++w) {
    const bool w_leads = g0 + w == gc;                  // first fine wave of the block
    int ldr = 0;                                        // the leader of wave w
    if (g0 + w >= gc && g0 < gc) ldr = gc - g0;         // a fine wave behind the block's coarse ones
    __syncthreads();
    if (!w_leads && wv == w) dw_to_lds(dw, red, lane);
    __syncthreads();
    if (!w_leads && wv == ldr) dw_add_lds(dw, red, lane);
  }
  const bool leader = wv == 0 || g_me == gc;
  if (leader) dw_flush(dw, k.slab + (size_t)g_me * W_END, lane);
}

// Owner pass of the binned scatter: workgroup b sums every record of bin b
// (the regions of all kBwdBlocks producers, then the overflow records that
// belong to it) and writes its slice of 2^shift entries of the table
// gradient once: = (overwrite) or +=.  Every entry is written by exactly one
// workgroup.
//
// The sums are exact integer sums.  On gfx950 ds_add_f32 runs ~20x slower than
// integer LDS atomics (config 2: ~600 us for the bins' 71 M float adds, against
// ~145 us with ds_add_u32 on the same addresses, ~125 us for the record loads
// alone), and a bin's records are heavily duplicated (surfaces: e.g. 37.5 K
// records on 2.9 K distinct entries at level 8), which defeats claiming
// entries for plain read-modify-writes.  So each value is converted to a
// 64-bit fixed-point integer in units of 2^(E - 40), E the exponent of the
// bin's largest |value| (every value < 2^41 units, 2^20 of them < 2^61), and
// added with ds_add_u64; the slice is converted back (one rounding to fp32).
// Integer adds are associative, so the gradient is bitwise reproducible, and
// every entry keeps full fp32 precision down to 2^-16 of the bin's largest
// contribution (2^-40 absolute resolution below that).  Measured on recorded
// config 2 bins (scripts/bin_stats.py): median relative error 1e-8 (fp32
// sequential sums 6e-9 .. 2e-8); the worst entries, at |g| ~ 1e-17 with a bin
// maximum ~ 5e-7, within 8e-3 -- where fp32 atomics cannot resolve them
// either once a larger contribution has been added.
constexpr int kBinThreads = 1024;
constexpr int kSliceF4 = 4;   // float4s of a 2^13-entry slice per thread (2 x 2^13 floats / 4 / 1024)
// The fused step's optimizer-state loads: 0 in the epilogue; 1 at kernel
// start.  Measured on one box (config 2): 207.5 vs 214.8 / 204.5 us; loaded
// after the setup 238 us, after the thread's last record fetch 217 us (64
// VGPR spills): vmcnt waits are in order, so an earlier issue only moves the
// wait to the first records.
static_assert(kSliceF4 * kBinThreads * 4 >= (2 << 13), "bins are at most 2^13 entries (bin_geom)");
constexpr int kBrDepth = 4;   // records per thread and fetch group (two groups in flight)
constexpr int kBrChunks = 8192;   // table entries (16 KiB of LDS): bins of up to 512 K records


// acc: [feature][entry] (entry e's accumulators 8 B apart per feature: a
// wave's random entries spread over twice the LDS banks of [entry][feature])
HN_DEV void bin_add(unsigned long long* acc, uint32_t se, const f32x4 v, uint32_t w, uint32_t sel,
                    uint32_t tmask, float scale) {
  const uint32_t e0 = w & 0x0fffffffu & sel;
  const uint32_t e1 = e0 ^ (((1u << (w >> 28)) - 1u) & tmask);
  const long long q[4] = {fx_of(v.x, scale), fx_of(v.y, scale), fx_of(v.z, scale), fx_of(v.w, scale)};
  __hip_atomic_fetch_add(acc + e0, (unsigned long long)q[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_add(acc + se + e0, (unsigned long long)q[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_add(acc + e1, (unsigned long long)q[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_add(acc + se + e1, (unsigned long long)q[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Buckets the spilled records by bin.  Block j handles producer block j's
// overflow list: it scans the per-bin spill counts (block 0 publishes the
// first slot of each bin), counts its own records per bin in LDS, reserves one
// range per touched bin with a single global atomic, and places the record
// ids through LDS cursors (spilled records clump into few bins: per-record
// global cursors serialise on them).  Returns at once when nothing spilled
// (the usual case).
constexpr int kPlaceThreads = 1024;   // 256 measured the same (r05: the launch, not its work)
// The stepped NeRFSmall weights' MFMA copies (hn_render_bwd_args.repack):
// extra workgroups of the placement launch, which runs after the scatter
// kernel's slab reduction has stepped every weight (mlp_pack2_kernel's values)
struct PackK {
  hn_mlp c, f;
  float* P;   // [2][G_END]: the workspace's packed copies (hn_render_fwd's Pc, Pf)
};
static_assert(kPlaceThreads == kMortonThreads, "morton_emit_block: one thread per Morton index of a tile");
// next / first: the next batch's pass 2 in the workgroups from `first` on
// (NextK; first = the placement and repack workgroups), ndc = that batch's
// NDC step (hn_next_batch.ndc): only this pass forms rays
__global__ __launch_bounds__(kPlaceThreads) void ovf_place_kernel(BinR k, PackK pk, MortonK next, NdcK ndc,
                                                                  unsigned first) {
  if (blockIdx.x >= first) {
    morton_emit_block(next, ndc, blockIdx.x - first);
    return;
  }
  if (blockIdx.x >= kBwdBlocks) {
    const int idx = (int)(blockIdx.x - kBwdBlocks) * kPlaceThreads + (int)threadIdx.x;
    if (idx < 2 * G_END) pk.P[idx] = idx < G_END ? pack_value(pk.c, idx) : pack_value(pk.f, idx - G_END);
    return;
  }
  __shared__ uint32_t cur[kScMaxBins], lc[kScMaxBins];
  __shared__ uint32_t part[kPlaceThreads];
  const size_t nrec = bin_records(k.nbins, k.cap, k.n_rays);
  uint32_t* idx = const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(k.bins + 4 * nrec));
  const OvfBook ob = ovf_book(idx, nrec, k.nbins);
  if (*ob.cnt == 0u) return;
  const uint32_t mine = ob.blk[blockIdx.x];
  if (mine == 0u && blockIdx.x != 0) return;   // block 0 publishes `first`
  const int per = (k.nbins + kPlaceThreads - 1) / kPlaceThreads, t = threadIdx.x;
  uint32_t sum = 0;
  for (int j = 0; j < per; ++j) {
    const int bb = t * per + j;
    if (bb < k.nbins) {
      sum += ob.per_bin[bb];
      lc[bb] = 0u;
    }
  }
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < kPlaceThreads; d <<= 1) {   // inclusive scan of the thread sums
    const uint32_t v = t >= d ? part[t - d] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t run = part[t] - sum;
  for (int j = 0; j < per; ++j) {
    const int bb = t * per + j;
    if (bb < k.nbins) {
      cur[bb] = run;
      if (blockIdx.x == 0) ob.first[bb] = run;
      run += ob.per_bin[bb];
    }
  }
  const size_t o0 = (size_t)blockIdx.x * ovf_per_block(k.n_rays);   // this list, relative to the overflow
  const size_t l0 = (size_t)kBwdBlocks * k.nbins * k.cap + o0;   // first record of this list
  const uint32_t* words = reinterpret_cast<const uint32_t*>(k.bins);
  auto bin_of = [&](uint32_t s) { return (words[rec_wofs(l0 + s, nrec)] & 0x0fffffffu) >> k.shift; };
  for (uint32_t s = t; s < mine; s += kPlaceThreads)
    __hip_atomic_fetch_add(lc + bin_of(s), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
  for (int j = 0; j < per; ++j) {
    const int bb = t * per + j;
    if (bb < k.nbins && lc[bb])
      cur[bb] += __hip_atomic_fetch_add(ob.cur + bb, lc[bb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  for (uint32_t s = t; s < mine; s += kPlaceThreads) {
    const uint32_t pos = __hip_atomic_fetch_add(cur + bin_of(s), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    ob.ids[pos] = (uint32_t)(o0 + s);
  }
}

// Records of the bin, flattened over the producers' regions: thread i takes
// records i, i + 1024, ... (4 at a time, independent loads in flight) and
// finds each one's region by binary search over the LDS prefix of the
// regions' counts.
__global__ __launch_bounds__(kBinThreads) void bin_reduce_kernel(BinR k) {
  extern __shared__ f32x4 acc4[];
  __shared__ uint32_t pre[kBwdBlocks + 1];
  __shared__ uint32_t wsum[kBwdBlocks / 64], wmax[kBwdBlocks / 64];
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(acc4);
  const int n4 = (2 << k.shift) / 2;   // f32x4 = 2 accumulators
  const uint32_t b = (uint32_t)k.bin0 + blockIdx.x;
  const size_t e0 = (size_t)b << (k.shift + 1);   // first float of the slice
  const int nd4 = (2 << k.shift) / 4;             // float4s of the slice (<= 4 per thread)
  // fused step on a coarse level: the row pairs no gradient can reach (their
  // moments are zero, so the dense update leaves p, m, v bitwise unchanged)
  // are neither loaded nor stored (table_live; T=19: levels 0-6)
  const uint32_t* lw = nullptr;
  if (k.fused && k.live && k.shift <= k.log2T && (int)(((uint32_t)b << k.shift) >> k.log2T) < k.live_levels)
    lw = k.live + (((size_t)b << k.shift) >> 6);
  auto live_at = [&](int i) { return lw == nullptr || ((lw[i >> 5] >> (i & 31)) & 1u) != 0u; };
  for (int i = threadIdx.x; i < n4; i += kBinThreads) acc4[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const size_t nrec = bin_records(k.nbins, k.cap, k.n_rays);
  const uint32_t* words = reinterpret_cast<const uint32_t*>(k.bins);
  const uint32_t* idx = reinterpret_cast<const uint32_t*>(k.bins + 4 * nrec);   // book base
  const uint32_t* cnt = idx + nrec;
  const float* mxs = reinterpret_cast<const float*>(cnt + (size_t)kBwdBlocks * k.nbins);   // [16][blocks]
  const OvfBook obk = ovf_book(const_cast<uint32_t*>(idx), nrec, k.nbins);
  const uint32_t n_ovf = *obk.cnt;
  static_assert(kBwdBlocks == 256 && kBinThreads >= 256, "one count per thread of waves 0-3");
  // levels of this bin: one, or all 16 when the whole table is one bin
  const int lev0 = (int)(((uint32_t)b << k.shift) >> k.log2T);
  const int nlev = k.shift > k.log2T ? 1 << (k.shift - k.log2T) : 1;
  uint32_t n = 0;
  float mx = 0.f;
  if (threadIdx.x < kBwdBlocks) {
    const uint32_t c = cnt[(size_t)b * kBwdBlocks + threadIdx.x];
    n = c < (uint32_t)k.cap ? c : (uint32_t)k.cap;
    for (int l = lev0; l < lev0 + nlev; ++l) mx = fmaxf(mx, mxs[l * kBwdBlocks + threadIdx.x]);
  }
  const uint32_t inc = (uint32_t)wave_incl_sum((double)n);   // exact: counts < 2^53
  const float wmx = wave_max_f32(mx);
  if (threadIdx.x < kBwdBlocks && (threadIdx.x & 63) == 63) {
    wsum[threadIdx.x >> 6] = inc;
    wmax[threadIdx.x >> 6] = wmx;
  }
  __syncthreads();
  if (threadIdx.x < kBwdBlocks) {
    uint32_t add = 0;
    for (int q = 0; q < (int)(threadIdx.x >> 6); ++q) add += wsum[q];
    pre[threadIdx.x + 1] = inc + add;
  }
  if (threadIdx.x == 0) pre[0] = 0;
  // bin scale: every record value (overflow records included: the producers
  // take every record) is below 2^(E+1) -> below 2^41 units
  const float bmx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  const int E = ilogbf(bmx > 0.f ? bmx : 1.f);
  // 2^(40 - E) as fp32 (E >= -126 + ... : the scale stays a normal float for
  // every E in [-87, 127]; smaller maxima use 2^127, still < 2^41 units)
  const int S = 40 - (E < -126 ? -126 : E);
  const float scale = ldexpf(1.f, S > 127 ? 127 : S);
  __syncthreads();
  const uint32_t total = pre[kBwdBlocks];
  const uint32_t sel = (1u << k.shift) - 1u, tmask = (1u << k.log2T) - 1u, se = 1u << k.shift;
  // region of the first record of every 64-record chunk: a record's region is
  // then a short forward walk from its chunk's (regions hold ~24-114 records)
  // instead of an 8-step binary search
  __shared__ uint16_t first_reg[kBrChunks];
  const bool tab = ((total + 63) >> 6) <= (uint32_t)kBrChunks;   // uniform
  if (tab) {
    for (uint32_t c = threadIdx.x; c < ((total + 63) >> 6); c += kBinThreads) {
      const uint32_t r = c << 6;
      int lo = 0;
#pragma unroll
      for (int st = kBwdBlocks / 2; st >= 1; st >>= 1)
        if (pre[lo + st] <= r) lo += st;
      first_reg[c] = (uint16_t)lo;
    }
    __syncthreads();
  }
  const size_t bbase = (size_t)b * kBwdBlocks * k.cap;
  // records r0 + q * 1024 (lane-consecutive: coalesced loads), each found in
  // the regions' prefix from its 64-record chunk's first region (a binary
  // search per record measured slower; both faster than one search per 4
  // lane-consecutive records with their 64-B-strided loads); the next group
  // of records is loaded before the current one is added
  auto fetch = [&](uint32_t r0, f32x4 (&v)[kBrDepth], uint32_t (&w)[kBrDepth]) {
#pragma unroll
    for (int q = 0; q < kBrDepth; ++q) {
      const uint32_t r = r0 + q * kBinThreads;
      if (r < total) {
        int lo = 0;   // largest p with pre[p] <= r
        if (tab) {
          lo = first_reg[r >> 6];
          while (pre[lo + 1] <= r) ++lo;   // r < total = pre[kBwdBlocks]: stops by lo = 255
        } else
        {
#pragma unroll
          for (int st = kBwdBlocks / 2; st >= 1; st >>= 1)
            if (pre[lo + st] <= r) lo += st;
        }
        const size_t rec = bbase + (size_t)lo * k.cap + (r - pre[lo]);
        v[q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(k.bins + rec_vofs(rec)));   // read once
        w[q] = __builtin_nontemporal_load(words + rec_wofs(rec, nrec));
      }
    }
  };
  auto add = [&](uint32_t r0, const f32x4 (&v)[kBrDepth], const uint32_t (&w)[kBrDepth]) {
#pragma unroll
    for (int q = 0; q < kBrDepth; ++q)
      if (r0 + q * kBinThreads < total) {
        bin_add(acc, se, v[q], w[q], sel, tmask, scale);
      }
  };
  f32x4 va[kBrDepth], vb[kBrDepth];
  uint32_t wa[kBrDepth], wb[kBrDepth];
  uint32_t r0 = threadIdx.x;
  if (r0 < total) fetch(r0, va, wa);
  for (; r0 < total; r0 += 2 * kBrDepth * kBinThreads) {
    const uint32_t r1 = r0 + kBrDepth * kBinThreads;
    if (r1 < total) fetch(r1, vb, wb);
    add(r0, va, wa);
    if (r1 >= total) break;
    if (r1 + kBrDepth * kBinThreads < total) fetch(r1 + kBrDepth * kBinThreads, va, wa);
    add(r1, vb, wb);
  }
  if (n_ovf) {   // this bin's spilled records (bucketed by ovf_place_kernel)
    const size_t ob = (size_t)kBwdBlocks * k.nbins * k.cap;
    const uint32_t lo = obk.first[b], hi = lo + obk.per_bin[b];
    for (uint32_t s = lo + threadIdx.x; s < hi; s += kBinThreads) {
      const uint32_t o = obk.ids[s];
      bin_add(acc, se, *reinterpret_cast<const f32x4*>(k.bins + rec_vofs(ob + o)), words[rec_wofs(ob + o, nrec)],
              sel, tmask, scale);
    }
  }
  __syncthreads();
  const double inv = 1.0 / (double)scale;
  float4* dst = k.d_table ? reinterpret_cast<float4*>(k.d_table + e0) : nullptr;
  if (k.fused && dst == nullptr) {
    // fused step: the thread's live flags, then all of its p, m, v loads in
    // flight at once (one HBM round trip instead of one per float4: the
    // pass 90.5 -> 88.6 us on config 2)
    bool lv[kSliceF4];
#pragma unroll
    for (int j = 0; j < kSliceF4; ++j) {
      const int i = threadIdx.x + j * kBinThreads;
      lv[j] = i < nd4 && live_at(i);
    }
    f32x4 p4[kSliceF4], m4[kSliceF4], v4[kSliceF4];
#pragma unroll
    for (int j = 0; j < kSliceF4; ++j) {
      const int i = threadIdx.x + j * kBinThreads;
      if (lv[j]) {
        p4[j] = reinterpret_cast<const f32x4*>(k.step.p + e0)[i];
        m4[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(k.step.m + e0) + i);
        v4[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(k.step.v + e0) + i);
      }
    }
#pragma unroll
    for (int j = 0; j < kSliceF4; ++j) {
      const int i = threadIdx.x + j * kBinThreads;
      if (i >= nd4) break;
      float4 a;
      a.x = (float)((double)(long long)acc[2 * i] * inv);
      a.y = (float)((double)(long long)acc[se + 2 * i] * inv);
      a.z = (float)((double)(long long)acc[2 * i + 1] * inv);
      a.w = (float)((double)(long long)acc[se + 2 * i + 1] * inv);
      if (!lv[j]) {
        if (a.x != 0.f || a.y != 0.f || a.z != 0.f || a.w != 0.f)
          __hip_atomic_fetch_or(&g_hn_fault, kFaultDeadRow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        continue;
      }
      float4 p{p4[j][0], p4[j][1], p4[j][2], p4[j][3]}, m{m4[j][0], m4[j][1], m4[j][2], m4[j][3]},
          v{v4[j][0], v4[j][1], v4[j][2], v4[j][3]};
      radam_elem(k.step, p.x, a.x, m.x, v.x);
      radam_elem(k.step, p.y, a.y, m.y, v.y);
      radam_elem(k.step, p.z, a.z, m.z, v.z);
      radam_elem(k.step, p.w, a.w, m.w, v.w);
      __builtin_nontemporal_store(f32x4{m.x, m.y, m.z, m.w}, reinterpret_cast<f32x4*>(k.step.m + e0) + i);
      __builtin_nontemporal_store(f32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4*>(k.step.v + e0) + i);
      if (k.step.mode != 0) reinterpret_cast<f32x4*>(k.step.p + e0)[i] = f32x4{p.x, p.y, p.z, p.w};
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < kSliceF4; ++j) {   // entries 2i, 2i + 1
    const int i = threadIdx.x + j * kBinThreads;
    if (i >= nd4) break;
    float4 a;
    a.x = (float)((double)(long long)acc[2 * i] * inv);
    a.y = (float)((double)(long long)acc[se + 2 * i] * inv);
    a.z = (float)((double)(long long)acc[2 * i + 1] * inv);
    a.w = (float)((double)(long long)acc[se + 2 * i + 1] * inv);
    if (dst) {
      if (!k.overwrite) {
        const float4 d = dst[i];
        a.x = a.x + d.x; a.y = a.y + d.y; a.z = a.z + d.z; a.w = a.w + d.w;
      }
      dst[i] = a;
    }
    if (k.fused && !live_at(i)) {   // a dead pair: its gradient is a structural zero
      if (a.x != 0.f || a.y != 0.f || a.z != 0.f || a.w != 0.f)
        __hip_atomic_fetch_or(&g_hn_fault, kFaultDeadRow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (k.fused) {   // RAdam on these 4 table elements (radam_kernel's update, same op forms)
      f32x4* pp = reinterpret_cast<f32x4*>(k.step.p + e0) + i;
      f32x4* pm = reinterpret_cast<f32x4*>(k.step.m + e0) + i;
      f32x4* pv = reinterpret_cast<f32x4*>(k.step.v + e0) + i;
      // m and v are nontemporal (next read by the next step's owner pass);
      // p stays cached: the next forward gathers it (p nontemporal too
      // measured the forward +10 us)
      const f32x4 p4 = *pp, m4 = __builtin_nontemporal_load(pm), v4 = __builtin_nontemporal_load(pv);
      float4 p{p4[0], p4[1], p4[2], p4[3]}, m{m4[0], m4[1], m4[2], m4[3]}, v{v4[0], v4[1], v4[2], v4[3]};
      radam_elem(k.step, p.x, a.x, m.x, v.x);
      radam_elem(k.step, p.y, a.y, m.y, v.y);
      radam_elem(k.step, p.z, a.z, m.z, v.z);
      radam_elem(k.step, p.w, a.w, m.w, v.w);
      __builtin_nontemporal_store(f32x4{m.x, m.y, m.z, m.w}, pm);
      __builtin_nontemporal_store(f32x4{v.x, v.y, v.z, v.w}, pv);
      if (k.step.mode != 0) *pp = f32x4{p.x, p.y, p.z, p.w};
    }
  }
}

}  // namespace hn

