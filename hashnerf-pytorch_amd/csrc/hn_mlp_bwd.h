// hn_mlp_bwd.h -- the MLP backward of one 32-point tile, shared by both
// backward schedules of render_bwd_kernel, and what becomes of its dW.
// One wave per SIMD (4 per CU, 512 registers each): the wave keeps ALL twelve
// 32x32 weight-gradient blocks of its network as MFMA accumulators (DW: 192
// registers, AGPR-resident) for the whole kernel, so a tile's dW costs only
// its MFMAs -- no per-tile LDS accumulation.  The operands of the dW products
// (the point index on the MFMA k axis) come from per-wave LDS images of bf16
// split parts read back transposed (the weight-gradient operand images
// below).  The weight fragments stream through a register ring (WRing) that
// runs across GEMM and tile boundaries.  ReLU masks are kept as bits.  The
// composite backward (d raw per sample) comes from a full-occupancy pre-pass
// (render_comp_bwd_kernel).
// b1_tile is the tile and c0sh_setup its rays' set-up; which tiles a wave
// runs, and where their feature grads go, is the schedule's (b1_groups in
// hn_bwd_binned.h, b1_unit in hn_bwd_atomic.h).  After the kernel, dw_flush
// stores a wave's accumulators to its dW slab and slab_reduce_block sums the
// slabs in a fixed order.
#pragma once
#include "hn_render_args.h"

namespace hn {

// render_bwd_kernel's LDS (both instantiations are launched with kB1LdsF
// floats): per wave the weight-gradient operand images (9 x 4 KiB) in a slab
// of kRRows x kXS floats, then the atomic schedule's hand-off ring, voxel
// buffer and flags, and the staged grid sizes.
constexpr int kXS = 36;
constexpr int kRRows = 260;
constexpr int kB1Waves = 4;
constexpr int kMW = kB1Waves - 1;                          // MLP waves; wave kMW scatters
constexpr int kB1Img = kMW * kRRows * kXS;                 // floats (112,320 B)
// Fine-tile hand-off ring (MLP waves -> scatter wave): per slot the tile's
// feature grads [32 points][kXS] ([f][level], coarse twin added), the 32
// sample depths and the ray origin / direction.
constexpr int kSlots = 8;
constexpr int kSlotZ = 32 * kXS, kSlotR = kSlotZ + 32, kSlotF = kSlotR + 8;
constexpr int kVoxF = 16 * 16 * 8;                         // scatter wave's voxel buffer
constexpr int kSyncInts = 5 + 2 * kSlots;
constexpr int kB1GslF = kB1Img + kSlots * kSlotF + kVoxF;   // float offset of the staged grid sizes, then sync
constexpr int kB1LdsF = kB1GslF + kGsLds + kSyncInts;
static_assert(kB1LdsF * 4 <= 160 * 1024, "LDS budget");
// dW slabs in the workspace: [kBwdBlocks][kSlabSlots][W_END], slot 0 the
// block's coarse dW, slots 1-3 its fine MLP waves' dW (slab_reduce_kernel)
constexpr int kSlabSlots = 4;
static_assert(kRRows * kXS % 4 == 0 && kXS % 4 == 0 && kSlotF % 4 == 0, "b128 alignment");

// The MLP-backward kernel: one persistent block per CU, 4 waves, kB1LdsF floats
// of LDS.  Each schedule defines its own body -- the primary template is the
// atomic schedule's (hn_bwd_atomic.h), <kSwVmcnt, kModeSplit> the binned
// schedule's explicit specialisation (hn_bwd_binned.h) -- so neither reads a
// line of the other.
template <int CAP, int MODE>
__global__ void render_bwd_kernel(B1K k);

struct DW {
  f32x16 c2[2], c1[4], c0[2], s1[2], s0[2];
};

// ---- weight-gradient operand images --------------------------------------
// A 32 x 32 tile of a layer's activations or output grads (rows = features,
// columns = the tile's points; D layout in registers) is staged as its first
// two split-f32 parts (hn_common.h: p0 = bf16(x), p1 = bf16(x - p0), the NS = 2
// split of the dW products) in a per-wave image [32 points][32 features] of
// bf16 per part (64-B point rows).  The parts come from the split the tile
// already gets as the B operand of the next GEMM of the chain (gemm_w with
// an image sink), so the dW products need no split of their own.
// dW[o][i] = sum_p G[o][p] X[i][p] contracts the point index (X's column),
// so both operands are read back transposed by ds_read_b64_tr_b16: lane l
// gets feature l & 31 of 4 consecutive points per read.  The 8-byte feature
// quads of point p sit at quad f4 ^ ((p >> 1) & 7): the quad writes of a
// D-layout tile are 2-way (the minimum for 64 lanes x 8 B on 32 banks), the
// transposed reads conflict-free.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int kImgBlk = 4096;   // bytes per tile image: 2 parts x 2 KiB
// tile images per wave: features | h0 (2) | [sh16 | sigma | geo15] | c0 (2) |
// c1 (2) | rgb grads; the grads of the backward reuse c1 (dc1, then ds1) and
// c0 (dc0, then dh0) once those are consumed
enum : int { kBF = 0, kBH0 = 1, kBC0in = 3, kBC0 = 4, kBC1 = 6, kBDR = 8, kNImg = 9 };
static_assert(kNImg * kImgBlk <= kRRows * kXS * 4, "images fit the per-wave LDS");

HN_DEV uint32_t img_off(int blk, int part, int p, int f4) {
  return (uint32_t)(blk * kImgBlk + part * 2048 + p * 64 + ((f4 ^ ((p >> 1) & 7)) << 3));
}
HN_DEV void put_quad(char* Xb, int blk, int part, int p, int f4, uint32_t lo, uint32_t hi) {
  *reinterpret_cast<uint2*>(Xb + img_off(blk, part, p, f4)) = uint2{lo, hi};
}
// Parts 0 and 1 of one split B chunk (elements j = D registers 8c' + j of
// lane (p, h): rows 16c' + 4h + j for j < 4, 16c' + 8 + 4h + j - 4 after) to
// quads f4b + h and f4b + 2 + h (f4b = 4c' + the tile's feature offset / 4).
template <int NS>
HN_DEV void put_parts(char* Xb, int blk, int f4b, const SP<NS>& s, int lane) {
  static_assert(NS >= 2, "the images hold two parts");
  const int p = lane & 31, h = lane >> 5;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const u32x4 w = __builtin_bit_cast(u32x4, s.p[q]);
    put_quad(Xb, blk, q, p, f4b + h, w[0], w[1]);
    put_quad(Xb, blk, q, p, f4b + 2 + h, w[2], w[3]);
  }
}
// A D-layout tile not split by any GEMM of the chain (c1): split and stage it.
HN_DEV void put_tile(char* Xb, int blk, const f32x16& v, int lane) {
#pragma unroll
  for (int c = 0; c < 2; ++c) put_parts<2>(Xb, blk, 4 * c, splitn<2>([&](int j) { return v[8 * c + j]; }), lane);
}

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
HN_DEV s16x4 ds_read_tr(const char* a) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(reinterpret_cast<uintptr_t>(a)));
}
// Operand of K = 16 chunk cc (points 16cc .. 16cc + 15) of image tile blk,
// part q: lane l holds feature l & 31 at points 16cc + 8h + j (element j).
HN_DEV bf16x8 img_operand(const char* Xb, int blk, int q, int cc, int lane) {
  const int g = (lane >> 4) & 3, i = lane & 15, h = lane >> 5;
  const int f4 = 4 * (g & 1) + (i & 3), pt = 16 * cc + 8 * h + (i >> 2);
  const s16x4 lo = ds_read_tr(Xb + img_off(blk, q, pt, f4));
  const s16x4 hi = ds_read_tr(Xb + img_off(blk, q, pt + 4, f4));
  const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

// acc[NB * a + b] += sum over the tile's 32 points of A(ablk[a]) B(bblk[b])^T
// (two K = 16 chunks, 2-part products in mfma_split's order)
template <int NA, int NB>
HN_DEV void wgrad_n(const char* Xb, const int (&ablk)[NA], const int (&bblk)[NB], f32x16* acc, int lane) {
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
    SP<2> a[NA], b[NB];
#pragma unroll
    for (int j = 0; j < NA; ++j)
#pragma unroll
      for (int q = 0; q < 2; ++q) a[j].p[q] = img_operand(Xb, ablk[j], q, cc, lane);
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int q = 0; q < 2; ++q) b[j].p[q] = img_operand(Xb, bblk[j], q, cc, lane);
#pragma unroll
    for (int ja = 0; ja < NA; ++ja)
#pragma unroll
      for (int jb = 0; jb < NB; ++jb) acc[NB * ja + jb] = mfma_split<2>(a[ja], b[jb], acc[NB * ja + jb]);
  }
}

template <int I, int N, typename F>
HN_DEV void static_for(F&& f) {
  if constexpr (N > 0) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N - 1>(f);
  }
}

// A weight-gradient block's operands read into registers ahead of its
// products (WgOps), and the products then issued in the gaps of a later
// data-path GEMM (WgX, gemm_w's `xt`): the image reads leave before
// that GEMM's own image writes (a wave's LDS accesses execute in order), and
// the products -- the same ones, per accumulator in the same order as
// wgrad_n's -- keep the matrix pipe busy while the chain waits on its own
// results and splits.  NoX: no extra products.
template <int NA, int NB>
struct WgOps {
  SP<2> a[2][NA], b[2][NB];   // [K = 16 chunk cc][operand]
};
template <int NA, int NB>
HN_DEV void wg_load(WgOps<NA, NB>& o, const char* Xb, const int (&ablk)[NA], const int (&bblk)[NB], int lane) {
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
#pragma unroll
    for (int j = 0; j < NA; ++j)
#pragma unroll
      for (int q = 0; q < 2; ++q) o.a[cc][j].p[q] = img_operand(Xb, ablk[j], q, cc, lane);
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int q = 0; q < 2; ++q) o.b[cc][j].p[q] = img_operand(Xb, bblk[j], q, cc, lane);
  }
}
struct NoX {
  static constexpr int per(int) { return 0; }
  template <int C>
  HN_DEV void run() const {}
};
// the 2 * NA * NB products of a WgOps (cc-major, as wgrad_n) spread over NC chunks
template <int NA, int NB, int NC>
struct WgX {
  const WgOps<NA, NB>& o;
  f32x16* acc;
  static constexpr int P = 2 * NA * NB;
  static constexpr int lo(int c) { return c * P / NC; }
  static constexpr int per(int c) { return 3 * (lo(c + 1) - lo(c)); }   // MFMAs at chunk c
  template <int C>
  HN_DEV void run() const {
    static_for<lo(C), lo(C + 1) - lo(C)>([&](auto pc) {
      constexpr int p = decltype(pc)::value, cc = p / (NA * NB), ja = p % (NA * NB) / NB, jb = p % NB;
      acc[NB * ja + jb] = mfma_split<2>(o.a[cc][ja], o.b[cc][jb], acc[NB * ja + jb]);
    });
  }
};

// ---- weight-fragment stream ----------------------------------------------
// A tile's 15 data-path GEMMs read their packed A-fragment groups (one 1-KiB
// dwordx4 load per wave: 4 f32 k-steps, or one bf16 part of 8 k-steps) in a
// fixed order (92 groups at kSplitF = 3, kSplitB = 2), padded to a
// multiple of the ring depth so that the ring lines up with the tile period.
// The ring keeps the next 8 groups (~16 bf16 MFMAs with their splits) in
// flight across GEMM, tile and unit boundaries: no GEMM starts on an exposed
// L2 latency at one wave per SIMD.  Depth 4 measured 484 us for the config-2
// MLP backward, 8: 460 us.  The two output blocks of a GEMM are paired
// (kSegs, gemm_w's NB = 2): one B split per chunk for both, two independent
// accumulator chains (515 -> 484 us together with wgrad_n's shared splits).
struct GemmSeg {
  int r, ob;   // region (hn_mlp.h), output block; ob = -1: both blocks, chunk by chunk
};
constexpr GemmSeg kSegs[] = {{R_F0, -1}, {R_F1, 0}, {R_F2G, -1}, {R_F3, -1}, {R_B4, -1},
                             {R_B3, -1}, {R_B2G, 0}, {R_B1, -1}, {R_B0, 0}};
constexpr int kNSegs = sizeof(kSegs) / sizeof(kSegs[0]);
// kSplitR: parts the backward's forward recompute uses of the forward
// regions' kSplitF packed parts (the leading parts of a split are the same
// for every part count, so the recompute streams only groups q < kSplitR of
// each chunk).  3 = the forward's own products (bit-identical activations).
constexpr int kSplitR = 2;
constexpr int seg_ns(const GemmSeg& g) {   // parts this stream uses per chunk (0: f32)
  return g.r < R_B4 && reg_ns(g.r) > kSplitR ? kSplitR : reg_ns(g.r);
}
constexpr int seg_gpo(const GemmSeg& g) { return seg_ns(g) ? seg_ns(g) * kRegKS[g.r] / 8 : kRegKS[g.r] / 4; }
constexpr int seg_groups(const GemmSeg& g) { return seg_gpo(g) * (g.ob < 0 ? 2 : 1); }
constexpr int seg_start(int i) {   // first group of segment i in the stream
  int n = 0;
  for (int j = 0; j < i; ++j) n += seg_groups(kSegs[j]);
  return n;
}
constexpr int kTileGroups = seg_start(kNSegs), kRing = 8;   // ring depth: 4 measured 484 us, 8: 460 us (above)
constexpr int kTilePeriod = (kTileGroups + kRing - 1) / kRing * kRing;   // pad groups keep slots static
// A paired segment streams chunk c of block 0 (its NS groups; f32: one
// group), then chunk c of block 1, then chunk c + 1 ...
constexpr int group_off(int idx) {
  idx %= kTilePeriod;
  if (idx >= kTileGroups) idx = 0;              // pad groups re-read group 0
  for (const GemmSeg& g : kSegs) {
    const int n = reg_gpo(g.r), u = seg_gpo(g);   // packed / streamed groups per block
    const int per = seg_ns(g) ? seg_ns(g) : 1, pk = reg_ns(g.r) ? reg_ns(g.r) : 1;   // per chunk
    if (g.ob >= 0) {
      if (idx < u) return reg_off(g.r) + (g.ob * n + pk * (idx / per) + idx % per) * 256;
    } else if (idx < 2 * u) {
      const int c = idx / (2 * per), ob = idx / per % 2, q = idx % per;
      return reg_off(g.r) + (ob * n + pk * c + q) * 256;
    }
    idx -= seg_groups(g);
  }
  return 0;
}
static_assert(group_off(kTileGroups - 1) == G_B0 + (reg_gpo(R_B0) - 1) * 256, "GEMM sequence");
static_assert(kSplitF != 3 || kSplitFC != 3 || kSplitB != 2 || kSplitR != 3 ||
              (kTileGroups == 92 && G_END == 30208), "layout");

struct WRing {
  f32x4 b[kRing];
};

// Weight-fragment group load: frag_load (hn_common.h, raw buffer load with a
// scalar offset).
HN_DEV f32x4 wload(const float* P, int off, int lane) {
  return frag_load(P, off, lane);
}

// (offsets are constexpr-evaluated: left to the optimiser, the region
// arithmetic of group_off stays as scalar loops in the kernel)
HN_DEV void wring_prime(WRing& w, const float* P, int lane) {
  static_for<0, kRing>([&](auto jc) {
    constexpr int j = decltype(jc)::value, off = group_off(j);
    w.b[j] = wload(P, off, lane);
  });
}
template <int IDX>
HN_DEV f32x4 wring_take(WRing& w, const float* P, int lane) {
  constexpr int off = group_off(IDX + kRing);
  const f32x4 a = w.b[IDX % kRing];
  w.b[IDX % kRing] = wload(P, off, lane);
  return a;
}

// The next chunk's B split (VALU) is issued in the gaps of this
// chunk's MFMAs (sched_group_barrier: one MFMA, then V VALU) instead of after
// them; the same splits and the same MFMA order, so results are unchanged.
// Measured (r03g, config 2, two runs each on one box): backward launch
// 0.812 -> 0.789 ms, step 1.159 -> 1.134 ms; the kernel's 24 VGPR spills go to 0.
// The same pipelining in the forward's gemm (round 3, removed) changed
// nothing there (render_fwd 0.304 ms either way).
// (VALU per MFMA slot, 2-part splits: 7 for one block, 4 for a pair.  Measured
// round 4, r04sw: 5 / 3 took render_bwd_kernel from 0.2343 to 0.2426 ms,
// 10 / 6 to 0.2364 ms.)
template <int NMFMA, int NVALU>
HN_DEV void swp_pattern() {
  static_for<0, NMFMA>([&](auto) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);       // one MFMA
    __builtin_amdgcn_sched_group_barrier(0x002, NVALU, 0);   // then VALU
  });
}

// acc[b] += A(block b of segment SEG of the stream) . B for the segment's NB
// output blocks (2: a paired segment -- one B split per chunk for both blocks,
// and two independent accumulator chains); bval(s) = B operand of f32 k-step s.
// IMG >= 0: chunk c's first two B parts also go to image tile IMG + c / 2 at
// quad offset F4B + 4 (c % 2) (put_parts; Xb = the wave's images).
// XT: extra independent MFMAs issued after chunk c's own (WgX; NoX: none),
// their VALU slots sharing the next chunk's split (kSplitV VALU per split).
template <int NS, bool PAIR>
constexpr int kSplitV = NS == 3 ? 36 : (PAIR ? 24 : 21);
constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }
template <int SEG, int NB, int IMG = -1, int F4B = 0, typename BF, typename XT = NoX>
HN_DEV void gemm_w(WRing& w, const float* P, f32x16* acc, int lane, BF bval, char* Xb = nullptr,
                   const XT& xt = XT{}) {
  constexpr int R = kSegs[SEG].r, KS = kRegKS[R], NS = seg_ns(kSegs[SEG]), START = seg_start(SEG);
  static_assert(NB == (kSegs[SEG].ob < 0 ? 2 : 1), "a paired segment yields both blocks, any other one");
  static_assert(IMG < 0 || NS >= 2, "image sinks take split B operands");
  // chunk c's A parts off the ring: block 0's NS groups, then block 1's
  auto take = [&](auto cc, SP<NS>(&a)[NB]) {
    static_for<0, NB * NS>([&](auto ic) {
      constexpr int c = decltype(cc)::value, i = decltype(ic)::value;
      a[i / NS].p[i % NS] = as_bf16x8(wring_take<START + NB * NS * c + i>(w, P, lane));
    });
  };
  if constexpr (NS > 0 && KS > 8) {   // split-f32, next chunk's split in the MFMA gaps
    constexpr int NC = KS / 8;
    SP<NS> b = splitn<NS>([&](int j) { return bval(j); });
    __builtin_amdgcn_sched_barrier(0);
    static_for<0, NC>([&](auto cc) {
      constexpr int c = decltype(cc)::value;
      SP<NS> a[NB];
      take(cc, a);
      if constexpr (IMG >= 0) put_parts<NS>(Xb, IMG + c / 2, F4B + 4 * (c % 2), b, lane);
      mfma_split<NS, NB>(a, b, acc);
      xt.template run<c>();
      if constexpr (c + 1 < NC) {
        b = splitn<NS>([&](int j) { return bval(8 * (c + 1) + j); });
        constexpr int M = NB * NS + XT::per(c);
        constexpr int V = NB == 2 ? (NS == 3 ? 3 : 4) : (NS == 3 ? 6 : 7);   // VALU per MFMA slot (above)
        swp_pattern<M, XT::per(c) ? ceil_div(kSplitV<NS, NB == 2>, M) : V>();
      }
      __builtin_amdgcn_sched_barrier(0);
    });
  } else if constexpr (NS > 0) {                // split-f32: NS groups per block and K = 16 chunk
    static_for<0, KS / 8>([&](auto cc) {
      constexpr int c = decltype(cc)::value;
      SP<NS> a[NB];
      take(cc, a);
      const SP<NS> b = splitn<NS>([&](int j) { return bval(8 * c + j); });
      if constexpr (IMG >= 0) put_parts<NS>(Xb, IMG + c / 2, F4B + 4 * (c % 2), b, lane);
      mfma_split<NS, NB>(a, b, acc);
      xt.template run<c>();
      __builtin_amdgcn_sched_barrier(0);
    });
  } else {
    static_for<0, KS / 4>([&](auto gc) {
      constexpr int g = decltype(gc)::value;
      f32x4 a[NB];
      static_for<0, NB>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        a[b] = wring_take<START + NB * g + b>(w, P, lane);
      });
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = mfma(a[b][j], bval(4 * g + j), acc[b]);
      xt.template run<g>();
      __builtin_amdgcn_sched_barrier(0);
    });
  }
}

constexpr int seg_of(int r) {   // first stream segment of region r
  for (int i = 0; i < kNSegs; ++i)
    if (kSegs[i].r == r) return i;
  return -1;
}
// acc[0..1] += both output blocks of region R . B: one paired segment, or
// a segment per block (the image sink on the first)
template <int R, int IMG = -1, int F4B = 0, typename BF, typename XT = NoX>
HN_DEV void gemm2(WRing& w, const float* P, f32x16 acc[2], int lane, BF bval, char* Xb = nullptr,
                  const XT& xt = XT{}) {
  constexpr int S = seg_of(R);
  if constexpr (kSegs[S].ob < 0) {
    gemm_w<S, 2, IMG, F4B>(w, P, acc, lane, bval, Xb, xt);
  } else {
    static_assert(std::is_same<XT, NoX>::value, "extra products go to paired segments");
    gemm_w<S, 1, IMG, F4B>(w, P, acc, lane, bval, Xb);
    gemm_w<S + 1, 1>(w, P, acc + 1, lane, bval);
  }
}

// ReLU with its mask bits, in integer forms that keep no lane masks
// live (the compare forms held 16+ SGPR-pair masks across the GEMMs and
// spilled them to VGPR lanes): relu = the bits with the sign-extended sign
// cleared (v > 0 ? v : 0 for every non-NaN v, -0 -> +0), bit = relu > 0 from
// the relu's bits, and the gradient masked by AND with the sign-extended bit.
// (No inline asm here: an asm operand that is an MFMA result gets none of the
// MFMA-to-VALU wait states the compiler inserts for its own instructions.)
HN_DEV void relu_bits(f32x16& v, uint32_t& m, int ob) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const uint32_t b = __float_as_uint(v[r]);
    const uint32_t u = b & ~(uint32_t)((int32_t)b >> 31);
    m |= min(u, 1u) << (16 * ob + r);
    v[r] = __uint_as_float(u);
  }
}
HN_DEV void mask_bits(f32x16& g, uint32_t m, int ob) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const uint32_t keep = (uint32_t)__builtin_amdgcn_sbfe((int)m, 16 * ob + r, 1);   // 0 or ~0
    g[r] = __uint_as_float(__float_as_uint(g[r]) & keep);
  }
}

// Ordering of a wave's own LDS image writes and transposed reads inside a
// tile.  The LDS unit executes one wave's ds instructions in order, so a read
// issued after a write sees it (also another lane's) and a write after a read
// does not overwrite what the read returns: only the compiler must keep the
// program order: a compiler barrier (the reads' own lgkmcnt waits stay)
// instead of s_waitcnt lgkmcnt(0) at each hand-over (lds_fence_wave), which
// also waits for every write still in flight (measured equal, round 3).
HN_DEV void tile_lds_order() {
  asm volatile("" ::: "memory");
}

// color_net.0 applied to the ray's sh features (the same for every point of
// the ray): its 64 rows are kept in the wave's LDS slab after the
// images (read back as the c0 accumulators' seed, 8 broadcast ds_read_b128
// per tile) instead of 32 VGPRs live across the unit's tiles.
constexpr int kC0shF = kNImg * kImgBlk / 4;   // float offset in the wave's slab
static_assert(kC0shF + 128 <= kRRows * kXS, "c0sh (two groups' rays) fits the per-wave slab");
struct C0Sh {
  const float* lds;
};
HN_DEV void c0sh_seed(const C0Sh& c, f32x16 (&c0)[2], int h) {
#pragma unroll
  for (int ob = 0; ob < 2; ++ob)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(c.lds + 32 * ob + row_of(4 * g, h));
#pragma unroll
      for (int j = 0; j < 4; ++j) c0[ob][4 * g + j] = v[j];
    }
}

// The set-up of a tile's rays ahead of b1_tile.  The SH part of color_net.0's
// input (each lane's ray gives its point's columns: features 8h .. 8h + 7 of
// the [sh16 | sigma | geo15] image) goes to the kBC0in image; color_net.0 is
// applied to the SH features (column p of that product is point p's ray; bit-
// identical to starting each point's chain with it) and its 64 rows are kept
// at X + kC0shF.  kGroups false: one ray for the 32 points, column 0 (lanes 0
// and 32 store).  true: points 0-15 and 16-31 are of two rays, columns 0 and
// 16, 64 floats apart; a lane's C0Sh is its own group's.
template <bool kGroups>
HN_DEV C0Sh c0sh_setup(const float* P, const Ray& r, float* X, int lane) {
  const int p = lane & 31, h = lane >> 5;
  float sh8[8], shx8[8];
  ray_sh(r, h, sh8, shx8);
  const SP<2> sp = splitn<2>([&](int j) { return shx8[j]; });
  // point p's 64-B row first, then the swizzled quad in it (img_off's sum in this order)
  char* Xp = reinterpret_cast<char*>(X) + 64 * p;
  const int sw = (p >> 1) & 7;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const u32x4 w = __builtin_bit_cast(u32x4, sp.p[q]);
    put_quad(Xp, kBC0in, q, 0, (2 * h) ^ sw, w[0], w[1]);
    put_quad(Xp, kBC0in, q, 0, (2 * h + 1) ^ sw, w[2], w[3]);
  }
  float* cl = X + kC0shF;
  const int grp = kGroups ? 64 * (p >> 4) : 0;   // the lane's group's rows
#pragma unroll
  for (int ob = 0; ob < 2; ++ob) {
    const f32x16 v = gemm<R_F2S>(P, ob, zero16(), lane, [&](int s) { return sh8[s]; });
    if ((kGroups ? p & 15 : p) == 0)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<f32x4*>(cl + grp + 32 * ob + row_of(4 * g, h)) =
            f32x4{v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
  }
  lds_fence_wave();
  return C0Sh{cl + grp};
}

// One 32-point tile: recompute the forward (features from the cache), then
// the MLP backward; dW into the wave's accumulators, d feature to dst.
HN_DEV f32x16 b1_tile(const float* __restrict__ P, WRing& wr, float* X, const f32x16& feat,
                      const C0Sh& c0sh, float4 dr, DW& dw, const uint32_t (&sm)[3]) {
  const int lane = lane_id();   // opaque: lane-derived LDS addresses are not hoisted out of the loop
  const int h = lane >> 5;
  char* Xb = reinterpret_cast<char*>(X);
  uint32_t mh0 = sm[0], mc0 = sm[1], mc1 = sm[2], mdead = 0;
#define HN_RELU(v, m, ob) relu_bits(v, mdead, ob)
  // ---- forward recompute (models.py:151-174); each GEMM stages its B
  // operand's parts as a dW operand image ----
  f32x16 h0[2] = {zero16(), zero16()};
  gemm2<R_F0, kBF>(wr, P, h0, lane, [&](int s) { return feat[s]; }, Xb);
  HN_RELU(h0[0], mh0, 0);
  HN_RELU(h0[1], mh0, 1);
  f32x16 s1 = zero16();
  gemm_w<seg_of(R_F1), 1, kBH0>(wr, P, &s1, lane, [&](int s) { return h0[s >> 4][s & 15]; }, Xb);
  f32x16 c0[2];
  c0sh_seed(c0sh, c0, h);
  // s1 rows 0..15 = [sigma | geo15] -> features 16..31 of [sh16 | sigma | geo15]
  gemm2<R_F2G, kBC0in, 4>(wr, P, c0, lane, [&](int s) { return s1[s]; }, Xb);
  HN_RELU(c0[0], mc0, 0);
  HN_RELU(c0[1], mc0, 1);
  {
    f32x16 c1[2] = {zero16(), zero16()};
    gemm2<R_F3, kBC0>(wr, P, c1, lane, [&](int s) { return c0[s >> 4][s & 15]; }, Xb);
    HN_RELU(c1[0], mc1, 0);
    HN_RELU(c1[1], mc1, 1);
    put_tile(Xb, kBC1, c1[0], lane);
    put_tile(Xb, kBC1 + 1, c1[1], lane);
  }
  if (h == 0) {   // rgb grads: features 0..2 of the kBDR tile (features >= 3 are never stored)
    const SP<2> d = splitn<2>([&](int j) { return j == 0 ? dr.x : j == 1 ? dr.y : j == 2 ? dr.z : 0.f; });
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const u32x4 w = __builtin_bit_cast(u32x4, d.p[q]);
      put_quad(Xb, kBDR, q, lane & 31, 0, w[0], w[1]);
    }
  }
  tile_lds_order();
  // Each layer's weight-gradient products run inside the NEXT data-path GEMM
  // (WgX): its operands are read here, before that GEMM's image writes, and
  // its MFMAs fill the chain's gaps -- per accumulator the same products in
  // the same order as the separate wgrad_n form of round 4 (bitwise-equal dW;
  // step 0.988 -> 0.980 ms, r05i).
  // ---- color_net.2 (dW rows >= 3 are discarded) inside color_net.2^T ----
  WgOps<1, 2> w_c2;
  {
    const int ab[1] = {kBDR}, bb[2] = {kBC1, kBC1 + 1};
    wg_load(w_c2, Xb, ab, bb, lane);
  }
  const float dy2[2] = {h ? dr.y : dr.x, h ? 0.f : dr.z};
  f32x16 dc1[2] = {zero16(), zero16()};
  gemm2<R_B4>(wr, P, dc1, lane, [&](int s) { return s < 2 ? dy2[s] : 0.f; }, nullptr, WgX<1, 2, 1>{w_c2, dw.c2});
  mask_bits(dc1[0], mc1, 0);
  mask_bits(dc1[1], mc1, 1);
  // ---- color_net.1 (dc1 image over c1) ----
  f32x16 dc0[2] = {zero16(), zero16()};
  gemm2<R_B3, kBC1>(wr, P, dc0, lane, [&](int s) { return dc1[s >> 4][s & 15]; }, Xb);
  mask_bits(dc0[0], mc0, 0);
  mask_bits(dc0[1], mc0, 1);
  tile_lds_order();
  // ---- color_net.0 (dc0 image over c0; B = [sh16 | sigma | geo15]), color_net.1's dW inside ----
  WgOps<2, 2> w_c1;
  {
    const int ab[2] = {kBC1, kBC1 + 1}, bb[2] = {kBC0, kBC0 + 1};
    wg_load(w_c1, Xb, ab, bb, lane);            // dw.c1[2 * nb + kb]
  }
  f32x16 ds1 = zero16();
  gemm_w<seg_of(R_B2G), 1, kBC0>(wr, P, &ds1, lane, [&](int s) { return dc0[s >> 4][s & 15]; }, Xb,
                                 WgX<2, 2, 4>{w_c1, dw.c1});
  if (h == 0) ds1[0] = dr.w;                    // row 0 = sigma (A row 0 is zero)
  tile_lds_order();
  // ---- sigma_net.1 (ds1 image over dc1's first tile; rows 16..31 discarded), color_net.0's dW inside ----
  WgOps<2, 1> w_c0;
  {
    const int ab[2] = {kBC0, kBC0 + 1}, bb[1] = {kBC0in};
    wg_load(w_c0, Xb, ab, bb, lane);
  }
  f32x16 dh0[2] = {zero16(), zero16()};
  gemm2<R_B1, kBC1>(wr, P, dh0, lane, [&](int s) { return ds1[s]; }, Xb, WgX<2, 1, 1>{w_c0, dw.c0});
  mask_bits(dh0[0], mh0, 0);
  mask_bits(dh0[1], mh0, 1);
  tile_lds_order();
  // ---- sigma_net.0 (dh0 image over dc0), sigma_net.1's dW inside ----
  WgOps<1, 2> w_s1;
  {
    const int ab[1] = {kBC1}, bb[2] = {kBH0, kBH0 + 1};
    wg_load(w_s1, Xb, ab, bb, lane);
  }
  f32x16 dfeat = zero16();
  gemm_w<seg_of(R_B0), 1, kBC0>(wr, P, &dfeat, lane, [&](int s) { return dh0[s >> 4][s & 15]; }, Xb,
                                WgX<1, 2, 4>{w_s1, dw.s1});
  tile_lds_order();
  {
    const int ab[2] = {kBC0, kBC0 + 1}, bb[1] = {kBF};
    wgrad_n<2, 1>(Xb, ab, bb, dw.s0, lane);
  }
  static_for<kTileGroups, kTilePeriod - kTileGroups>([&](auto gc) {   // pad groups: keep the ring
    (void)wring_take<decltype(gc)::value>(wr, P, lane);                 // aligned with the tile
  });
  tile_lds_order();                             // image reads done before any later writes
  (void)mdead;
#undef HN_RELU
  return dfeat;
}

// Coarse-pass feature grads, per ray: 64 samples x 32 features (workspace-internal)
constexpr size_t kDcRay = (size_t)kSc * 32;
// dW(coarse) (+)= sum_b slab[b][0], dW(fine) (+)= sum_b (slab[b][1] +
// slab[b][2] + slab[b][3]).  64 consecutive elements per block, kSlabGroups
// slab-groups per element (8 loads in flight per thread, ~18 waves per CU: the
// read is latency bound otherwise), LDS combine in a fixed order, so the sums
// are deterministic given the slabs.
constexpr int kSlabGroups = 16;
constexpr int kSlabIlp = 8;   // slab loads in flight per thread (a power of 2)
// One slab-reduce block's 64 elements (vblock): the arithmetic of every
// element is fixed (the group partials, then the pairwise combines), so the
// sums are the same whichever kernel runs it (slab_reduce_kernel, or the
// binned scatter's tail).  1024 threads; part[16][64] in LDS.
// ms (binned scatter, optional): the ten NeRFSmall tensors' RAdam steps
// ([network_fn's 5 | network_fine's 5], hn_mlp order), applied to each element
// with its final gradient (radam_kernel's update) where that is formed.
HN_DEV void slab_reduce_block(const float* __restrict__ slab, int n_blocks, const hn_mlp_grad& dc,
                              const hn_mlp_grad& df, int overwrite, int vblock, float (*part)[64],
                              const hn_radam_tensor* ms = nullptr, const int32_t* gsplit = nullptr) {
  const int lane = threadIdx.x & 63;
  const int e = vblock * 64 + lane;
  const int grp = threadIdx.x >> 6;
  const bool fine = e >= W_END;
  const int i = fine ? e - W_END : e;
  // the slabs summed for this element.  gsplit (the binned schedule's
  // balanced lists): the MLP waves g = 4 * block + wave run the coarse net for
  // g < *gsplit, the fine net from there, and each block's waves of one net
  // are summed into the first of them before the store, so only these run
  // leaders hold a slab -- coarse: the waves 4j < gs; fine: gs, then the waves
  // 4j > gs.  Otherwise (block, slot) pairs, slot 0 (coarse) or 1..3 (fine),
  // flattened
  const int gs = gsplit ? *gsplit : 0;
  const int per = fine ? kSlabSlots - 1 : 1;
  const int n_lead = fine ? (kSlabSlots * n_blocks) / 4 - gs / 4 : (gs + 3) / 4;
  const int n_slabs = gsplit ? n_lead : n_blocks * per;
  auto slab_at = [&](int q) {
    if (gsplit) {
      const int g = !fine ? 4 * q : (gs % 4 == 0 ? gs + 4 * q : (q == 0 ? gs : 4 * (gs / 4 + q)));
      return slab[(size_t)g * W_END + i];
    }
    const int b = q / per, slot = fine ? 1 + q % per : 0;
    return slab[((size_t)b * kSlabSlots + slot) * W_END + i];
  };
  float s = 0.f;
  if (e < 2 * W_END) {
    float acc[kSlabIlp];
#pragma unroll
    for (int u = 0; u < kSlabIlp; ++u) acc[u] = 0.f;
    int q = grp;
    for (; q + (kSlabIlp - 1) * kSlabGroups < n_slabs; q += kSlabIlp * kSlabGroups)
#pragma unroll
      for (int u = 0; u < kSlabIlp; ++u) acc[u] += slab_at(q + kSlabGroups * u);
    for (; q < n_slabs; q += kSlabGroups) acc[0] += slab_at(q);
#pragma unroll
    for (int w = kSlabIlp / 2; w >= 1; w /= 2)   // pairwise, fixed order
#pragma unroll
      for (int u = 0; u < w; ++u) acc[u] = acc[u] + acc[u + w];
    s = acc[0];
  }
  part[grp][lane] = s;
  __syncthreads();
  if (grp == 0 && e < 2 * W_END) {
    float t[kSlabGroups];
#pragma unroll
    for (int g = 0; g < kSlabGroups; ++g) t[g] = part[g][lane];
#pragma unroll
    for (int w = kSlabGroups / 2; w >= 1; w /= 2)
#pragma unroll
      for (int g = 0; g < w; ++g) t[g] = t[g] + t[g + w];
    s = t[0];
    const hn_mlp_grad& d = fine ? df : dc;
    const int ly = i < W_S1 ? 0 : i < W_C0 ? 1 : i < W_C1 ? 2 : i < W_C2 ? 3 : 4;   // the torch tensor
    const int j = i - (ly == 0 ? 0 : ly == 1 ? W_S1 : ly == 2 ? W_C0 : ly == 3 ? W_C1 : W_C2);
    float* dst = (ly == 0 ? d.sigma0 : ly == 1 ? d.sigma1 : ly == 2 ? d.color0 : ly == 3 ? d.color1 : d.color2) + j;
    const float gv = overwrite ? s : *dst + s;
    *dst = gv;
    if (ms) {
      const hn_radam_tensor& r = ms[(fine ? 5 : 0) + ly];
      float p = r.p[j], m = r.m[j], v = r.v[j];
      radam_elem(r, p, gv, m, v);
      r.m[j] = m;
      r.v[j] = v;
      if (r.mode != 0) r.p[j] = p;
    }
  }
}
constexpr int kSlabVBlocks = (2 * W_END + 63) / 64;

// ---- a wave's dW accumulators to memory -------------------------------------
// acc[base + n*ld + k] = D[n - n0][k - k0] for n < nmax, k < kmax: every dW
// element belongs to exactly one (block, lane, register) of the twelve blocks.
HN_DEV void dw_block(float* acc, int base, int ld, int n0, int nmax, int k0, int kmax, const f32x16& d,
                     int lane) {
  const int i = lane & 31, h = lane >> 5;
  const int kk = k0 + i;
  if (kk >= kmax) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + row_of(r, h);
    if (n < nmax) acc[base + n * ld + kk] = d[r];
  }
}

// color_net.0's dW block: its columns are the image features [sh16 | sigma |
// geo15] (b1_tile): feature 16 (sigma, no weight) is dropped, 17..31 are
// weight columns 16..30.
HN_DEV void dw_block_c0(float* acc, int nb, const f32x16& d, int lane) {
  const int i = lane & 31, h = lane >> 5;
  if (i == 16) return;
  const int col = i < 16 ? i : i - 1;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float* dst = acc + W_C0 + (32 * nb + row_of(r, h)) * 31 + col;
    *dst = d[r];
  }
}

HN_DEV void dw_flush(const DW& dw, float* acc, int lane) {
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) dw_block(acc, W_C2, 64, 0, 3, 32 * kb, 64, dw.c2[kb], lane);
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) dw_block(acc, W_C1, 64, 32 * nb, 64, 32 * kb, 64, dw.c1[2 * nb + kb], lane);
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) dw_block_c0(acc, nb, dw.c0[nb], lane);
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) dw_block(acc, W_S1, 64, 0, 16, 32 * kb, 64, dw.s1[kb], lane);
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) dw_block(acc, W_S0, 32, 32 * nb, 64, 0, 32, dw.s0[nb], lane);
}

HN_DEV void dw_zero(DW& dw) {
#pragma unroll
  for (int j = 0; j < 2; ++j) dw.c2[j] = dw.c0[j] = dw.s1[j] = dw.s0[j] = zero16();
#pragma unroll
  for (int j = 0; j < 4; ++j) dw.c1[j] = zero16();
}

// A block's MLP waves can sum their dW before the slab store (the binned
// schedule does): a wave's 12 accumulator blocks through LDS as
// [block][quad][lane] f32x4 (48 KiB; conflict-free b128 accesses), added by
// the first wave of the block that runs the same net, in wave order.
template <typename F>
HN_DEV void dw_each(DW& dw, F&& f) {
#pragma unroll
  for (int j = 0; j < 2; ++j) f(dw.c2[j], j);
#pragma unroll
  for (int j = 0; j < 4; ++j) f(dw.c1[j], 2 + j);
#pragma unroll
  for (int j = 0; j < 2; ++j) f(dw.c0[j], 6 + j);
#pragma unroll
  for (int j = 0; j < 2; ++j) f(dw.s1[j], 8 + j);
#pragma unroll
  for (int j = 0; j < 2; ++j) f(dw.s0[j], 10 + j);
}
HN_DEV void dw_to_lds(DW& dw, f32x4* L, int lane) {
  dw_each(dw, [&](f32x16& v, int b) {
#pragma unroll
    for (int q = 0; q < 4; ++q) L[(b * 4 + q) * 64 + lane] = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
  });
}
HN_DEV void dw_add_lds(DW& dw, const f32x4* L, int lane) {
  dw_each(dw, [&](f32x16& v, int b) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 t = L[(b * 4 + q) * 64 + lane];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * q + j] = v[4 * q + j] + t[j];
    }
  });
}

}  // namespace hn

