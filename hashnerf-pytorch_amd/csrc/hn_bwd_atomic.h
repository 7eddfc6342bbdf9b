// hn_bwd_atomic.h -- the float-atomic fused backward schedule (kModeAtomic):
// the only one for T > 22 and for grids whose cell index does not fit a bin,
// and the reference of the binned schedule's tests.
// One persistent block per CU owns rays blockIdx.x + i * gridDim.x.  A coarse
// unit is one ray's 2 coarse tiles, a fine unit 2 of a ray's 6 fine tiles
// (b1_unit).  Wave 0 first runs the block's coarse units and publishes each
// ray's coarse feature grads; waves 0-2 then take fine units from an LDS work
// counter and hand every fine tile's feature grads through an LDS ring
// (Ring, ring_put) to wave 3, which only scatters: trilinear backward + float
// atomics into the table gradient (ring_drain, scatter_slot,
// scatter_level_x).  Every wait is bounded (spin_until, wait_flag) and ends
// in a device fault bit, not a hang.  slab_reduce_kernel then sums the
// blocks' dW slabs.
#pragma once
#include "hn_mlp_bwd.h"

namespace hn {

// Scatter of one fine tile's table gradient (embedding_dense_backward of
// hash_encoding.py:106 + trilinear backward).  A fine sample that is one of
// the 64 coarse samples (fine_src < 64) is the same point in both passes: its
// coarse-pass feature grads (written by the coarse kernel) are added first,
// so every unique point is scattered once (25 % fewer atomics).
//
// Lane layout: lane = 16 * (2 * xi + f) + point, 16 points per pass.  One
// atomic wave-instruction covers corners (0,j,k) and (1,j,k) of both features
// of 16 points: h(x+1) differs from h(x) only in low bits (prime 1 on x), so
// 7/8 of the x-pairs fall in one 64-byte segment and the four dwords of a
// point go out as ~1 memory request instead of 2 (the float-atomic path is
// request-rate bound for random rows).  Points are consecutive samples along
// the ray and sit along a 16-lane DPP row, so a run of samples inside one
// voxel is summed by a segmented suffix sum of row shifts (no LDS round
// trips, no branches) and only the run head issues atomics.

// Atomic wave-instructions the scatter wave may have in flight before it
// issues a level's 4 (-1: no cap).  Uncapped, its atomics crowd the CU's
// vector-memory pipeline and the MLP waves' weight loads stall behind them
// (backward 1.59 ms at config 2); capped too tightly, the scatter wave waits
// on atomic latency.  Measured with the f32-MFMA MLP (scripts/variants.sh):
// 1: 1.59 ms, 2: 1.56, 4: 1.496, 6: 1.508.  With the split-f32 MLP and
// Morton-ordered batches (scripts/variants_env.sh, two runs each): 4: 1.282 /
// 1.278 ms, 8: 1.258 / 1.252, 12: 1.275 / 1.274.
// The cap when the table does not fit the 256 MiB MALL (T >= 21): config 3
// (T=22, B=8192) measured 2.93 / 2.94 ms at cap 8 and 2.82 / 2.82 ms at 4.
// (kSwVmcnt = 8, kSwVmcntBig = 4, hn_render_args.h.)
// One level of the scatter for the 16 points of a pass; v = this lane's
// point's voxel {cell x, cell y * PY, cell z * PZ, w x, y, z} from the compact
// pass (the prime products are precomputed there: (c + 1) * P = c * P + P,
// and c -> c * P is a bijection, so run heads compare the products).
template <int CAP>   // in-flight atomic cap: kSwVmcnt, or kSwVmcntBig for a table beyond the MALL
HN_DEV void scatter_level_x(const GridArgs& g, float* __restrict__ dtable, const f32x4 v0, const float2 v1,
                            uint32_t l, float gl, int lane) {
  const int pp = lane & 15, xi = lane >> 5;
  const int f = (lane >> 4) & 1;
  const uint32_t cx = (uint32_t)__float_as_int(v0.x), y0 = (uint32_t)__float_as_int(v0.y),
                 z0 = (uint32_t)__float_as_int(v0.z);
  const float w[3] = {v0.w, v1.x, v1.y};
  const uint32_t mask = (1u << g.log2T) - 1u;
  const uint32_t hx = cx + (uint32_t)xi;
  const uint32_t y1 = y0 + kPrimeY, z1 = z0 + kPrimeZ;
  // d feat / d e_c = ((g * fz) * fy) * fx  (trilerp_bwd order), c = 4*xi + jk
  const float fx = xi ? w[0] : 1.f - w[0];
  const float gz0 = gl * (1.f - w[2]), gz1 = gl * w[2];
  float cv[4];
  cv[0] = (gz0 * (1.f - w[1])) * fx;   // j=0 k=0
  cv[1] = (gz1 * (1.f - w[1])) * fx;   // j=0 k=1
  cv[2] = (gz0 * w[1]) * fx;           // j=1 k=0
  cv[3] = (gz1 * w[1]) * fx;           // j=1 k=1
  const uint32_t q0 = dpp_u<kRowShr1>(cx), q1 = dpp_u<kRowShr1>(y0), q2 = dpp_u<kRowShr1>(z0);
  const bool head = pp == 0 || q0 != cx || q1 != y0 || q2 != z0;
  const uint32_t pm = (uint32_t)__ballot(head) & 0xffffu;   // every row sees the same points
  // Segmented suffix sum over runs of samples in one voxel: lane p absorbs
  // lane p+d iff no run starts in (p, p+d].  Step d is only needed when some
  // run is longer than d (k consecutive non-heads = a run of > k samples);
  // the tests are on the wave-uniform head mask, so skipped steps cost nothing.
  const uint32_t nz1 = ~pm & 0xfffeu, nz2 = nz1 & (nz1 >> 1), nz4 = nz2 & (nz2 >> 2);
  auto seg_sum = [&](float (&v)[4]) {
    if (!nz1) return;
    auto absorb = [&](auto dc, int d) {
      const bool same = pp + d < 16 && ((pm >> (pp + 1)) & ((1u << d) - 1u)) == 0u;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float o = dpp_f<decltype(dc)::value>(v[c]);
        v[c] = same ? v[c] + o : v[c];
      }
    };
    absorb(std::integral_constant<int, kRowShl<1>>{}, 1);
    if (nz2) {
      absorb(std::integral_constant<int, kRowShl<2>>{}, 2);
      if (nz4) {
        absorb(std::integral_constant<int, kRowShl<4>>{}, 4);
        if (nz4 & (nz4 >> 4)) absorb(std::integral_constant<int, kRowShl<8>>{}, 8);
      }
    }
  };
  seg_sum(cv);
  if (head) {
    const uint32_t row0 = l << g.log2T;
    const uint32_t hh[4] = {(hx ^ y0 ^ z0) & mask, (hx ^ y0 ^ z1) & mask, (hx ^ y1 ^ z0) & mask,
                            (hx ^ y1 ^ z1) & mask};
    // cap the atomics in flight (they share the CU's vector-memory pipeline
    // with the MLP waves' weight loads); waiting only here, after this
    // level's VALU, overlaps the wait with it
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CAP) : "memory");
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float* dst = reinterpret_cast<float*>(reinterpret_cast<char*>(dtable) +
                                            (row0 + hh[c]) * 8u + 4u * f);
      atomic_add_f32(dst, cv[c]);
    }
  }
}



// ---- fine-tile hand-off ring ----------------------------------------------
// The MLP waves never issue an atomic and the scatter wave never issues a
// global load: a load behind outstanding atomics waits for all of them
// (in-order vmcnt), so mixing the two in one wave exposes the atomic latency.
// Protocol (LDS ints, single consumer): a producer takes ticket t, waits until
// slot t % kSlots has been consumed t / kSlots times, fills it and publishes
// ready[slot] = t + 1; the consumer takes tickets in order.  The producer
// holding the oldest unconsumed ticket never waits, so the ring cannot
// deadlock.  Flags are relaxed LDS atomics ordered by lgkmcnt(0) fences (an
// acquire / release would also wait vmcnt(0), draining the atomics).
struct Ring {
  float* slots;
  int* tick;    // next ticket
  int* ready;   // [kSlots] ticket + 1 of the slot's contents
  int* freed;   // [kSlots] times consumed
  const float* gsl;
};

// A bounded wait that runs out raises its fault bit (raise_fault,
// hn_render_args.h): a protocol bug ends in an error the host sees.
constexpr int kSpinCap = 1 << 22;   // iterations of >= 128 cycles: ~0.25 s

// Bounded spin on a workgroup-local flag.
HN_DEV void spin_until(int* flag, int need, int fault_bit) {
  bool ok = false;
  for (int it = 0; it < kSpinCap; ++it) {
    const int v = __builtin_amdgcn_readfirstlane(
        __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    if (v >= need) {
      ok = true;
      break;
    }
    __builtin_amdgcn_s_sleep(2);
  }
  if (!ok) raise_fault(fault_bit);
  asm volatile("" ::: "memory");
}

HN_DEV int lds_load(int* p) {
  return __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}

HN_DEV void ring_publish(int* flag, int v) {
  lds_fence_wave();                               // the slot's LDS accesses are done
  if (lane_id() == 0) __hip_atomic_store(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// A slot: the tile's feature grads [32 points][kXS] ([f][level]), the coarse
// twin's grads added (tw, lane (point, feature h)), depths and the ray.
HN_DEV void fill_slot(float* S, const Ray& r, float z, const f32x16& dfeat, const f32x4 tw[4]) {
  const int lane = lane_id();
  const int p = lane & 31, h = lane >> 5;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int l = h ? tile_level(m, 1) : tile_level(m, 0);
    S[p * kXS + l] = dfeat[2 * m];
    S[p * kXS + 16 + l] = dfeat[2 * m + 1];
  }
  lds_fence_wave();
  // fine grad + twin grad: the order of the former two-kernel scatter
  f32x4* g4 = reinterpret_cast<f32x4*>(S + p * kXS + 16 * h);
#pragma unroll
  for (int c = 0; c < 4; ++c) g4[c] = g4[c] + tw[c];
  if (h == 0) S[kSlotZ + p] = z;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      S[kSlotR + a] = r.o[a];
      S[kSlotR + 3 + a] = r.d[a];
    }
  }
  lds_fence_wave();
}

// The table-gradient scatter of one slot (embedding_dense_backward of
// hash_encoding.py:106 + trilinear backward); V = 2048-float voxel buffer.
template <int CAP>
HN_DEV void scatter_slot(const B1K& k, const float* S, float* V, const float* gsl) {
  const int lane = lane_id();
  const int pp = lane & 15, f = (lane >> 4) & 1, lq = lane >> 4;
  Ray r;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r.o[a] = S[kSlotR + a];
    r.d[a] = S[kSlotR + 3 + a];
  }
#pragma unroll
  for (int grp = 0; grp < 2; ++grp) {
    float pt[3], xc[3];
    ray_point(r, S[kSlotZ + 16 * grp + pp], pt);
#pragma unroll
    for (int a = 0; a < 3; ++a) xc[a] = clamp_t(pt[a], k.g.bmin[a], k.g.bmax[a]);
    // compact pass: lane (row lq, point pp) computes levels lq, lq+4, lq+8,
    // lq+12 once, instead of every (x offset, feature) row repeating the divisions
    if (grp) lds_fence_wave();                  // previous pass's voxel reads done
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int l = 4 * b + lq;
      int32_t cell[3];
      float w[3];
      voxel_cw(k.g, gsl, pt, xc, l, cell, w);
      float* dst = V + (l * 16 + pp) * 8;
      *reinterpret_cast<f32x4*>(dst) = f32x4{__int_as_float(cell[0]), __uint_as_float((uint32_t)cell[1] * kPrimeY),
                                              __uint_as_float((uint32_t)cell[2] * kPrimeZ), w[0]};
      *reinterpret_cast<float2*>(dst + 4) = make_float2(w[1], w[2]);
    }
    lds_fence_wave();
    float gl[16];
    const f32x4* src4 = reinterpret_cast<const f32x4*>(S + (16 * grp + pp) * kXS + 16 * f);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const f32x4 v = src4[c];
      gl[4 * c] = v.x; gl[4 * c + 1] = v.y; gl[4 * c + 2] = v.z; gl[4 * c + 3] = v.w;
    }
    // voxel entries are read one level ahead (one wave per SIMD: nothing
    // else hides the LDS latency)
    const float* vs = V + pp * 8;
    f32x4 v0 = *reinterpret_cast<const f32x4*>(vs);
    float2 v1 = *reinterpret_cast<const float2*>(vs + 4);
#pragma unroll
    for (int l = 0; l < 16; ++l) {
      const f32x4 c0 = v0;
      const float2 c1 = v1;
      if (l < 15) {
        v0 = *reinterpret_cast<const f32x4*>(vs + (l + 1) * 128);
        v1 = *reinterpret_cast<const float2*>(vs + (l + 1) * 128 + 4);
      }
      scatter_level_x<CAP>(k.g, k.d_table, c0, c1, l, gl[l], lane);
      if ((l & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
  }
  lds_fence_wave();                             // slot and voxel reads done
}

// Producer: one fine tile.  A fine sample that is one of the 64 coarse
// samples (fine_src < 64) is the same point in both passes: its coarse-pass
// grads are added, so every unique point is scattered once.  z / src: this
// lane's point's depth and fine_src (prefetched per unit).
HN_DEV void ring_put(const B1K& k, const Ring& q, float* X, const Ray& r, int64_t ray, float z, int src,
                     const f32x16& dfeat) {
  const int lane = lane_id();
  const int h = lane >> 5;
  const bool twin = src < kSc;
  const f32x4* dc =
      reinterpret_cast<const f32x4*>(k.dfeat + (size_t)ray * kDcRay + (size_t)(twin ? src : 0) * 32 + 16 * h);
  f32x4 tw[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) tw[c] = twin ? dc[c] : f32x4{0.f, 0.f, 0.f, 0.f};
  int t = 0;
  if (lane == 0) t = atomicAdd(q.tick, 1);
  t = __builtin_amdgcn_readfirstlane(t);
  const int s = t % kSlots;
  spin_until(&q.freed[s], t / kSlots, kFaultSlot);
  float* S = q.slots + s * kSlotF;
  fill_slot(S, r, z, dfeat, tw);
  ring_publish(&q.ready[s], t + 1);
}

// Consumer: takes tickets in order until every one of the n_tiles fine tiles
// has a ticket.  tick only grows and a tile takes its ticket before it is
// handed over, so tick == n_tiles with t >= tick means no ticket t will ever
// come.
template <int CAP>
HN_DEV void ring_drain(const B1K& k, const Ring& q, float* V, int n_tiles) {
  for (int t = 0;; ++t) {
    const int s = t % kSlots;
    bool have = false, done = false;
    for (int it = 0; it < kSpinCap; ++it) {
      if (lds_load(&q.ready[s]) >= t + 1) {
        have = true;
        break;
      }
      const int tk = lds_load(q.tick);
      if (tk >= n_tiles && t >= tk) {
        done = true;
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
    if (!have && !done) raise_fault(kFaultDrain);   // tiles left unscattered
    asm volatile("" ::: "memory");
    if (!have) break;
    const float* S = q.slots + s * kSlotF;
    scatter_slot<CAP>(k, S, V, q.gsl);
    ring_publish(&q.freed[s], t / kSlots + 1);
  }
}

HN_DEV void wait_flag(int* flag, int need) {
  for (int it = 0; it < kSpinCap; ++it) {
    if (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) >= need) return;
    __builtin_amdgcn_s_sleep(8);
  }
  raise_fault(kFaultCoarse);
}

// One work unit: composite backward of the ray (:541/:558 chain), then 2 tiles.
// Fine units hand each tile to the scatter wave; before the first hand-off
// they wait until wave 0 has published this ray's coarse feature grads
// (*done >= need)
template <int S>
HN_DEV void b1_unit(const B1K& k, int64_t ray, int part, float* X, DW& dw, WRing& wr, const Ring* ring,
                    int* done = nullptr, int need = 0) {
  const int lane = lane_id();
  constexpr bool fine = S == kSf;
  const int p = lane & 31, h = lane >> 5;
  Ray r;
  load_ray(k.rays, ray, r);
  const int tile0 = 2 * part;                   // tile within this pass
  const float* drs = k.draw + ((size_t)ray * (kSc + kSf) + (fine ? kSc : 0) + 32 * tile0 + p) * 4;
  float4 dr[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) dr[t] = *reinterpret_cast<const float4*>(drs + 128 * t);
  const float* P = opaque_ptr(fine ? k.Pf : k.Pc);
  const C0Sh c0sh = c0sh_setup<false>(P, r, X, lane);
  const int ctile = (fine ? kSc / 32 : 0) + tile0;
  float zq[2] = {0.f, 0.f};
  int srcq[2] = {0, 0};
  if constexpr (fine) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      zq[t] = k.z_fine[ray * kSf + 32 * (tile0 + t) + p];
      srcq[t] = k.fine_src[ray * kSf + 32 * (tile0 + t) + p];
    }
  }
  f32x16 feat, featn;
  load_feat(k.feat, ray, ctile, lane, feat);
  load_feat(k.feat, ray, ctile + 1, lane, featn);
  static_for<0, 2>([&](auto tc) {   // unrolled: the ring's slots and the per-tile arrays stay static
    constexpr int t = decltype(tc)::value;
    uint32_t sm[3] = {0u, 0u, 0u};
    load_masks(k.feat, ray, ctile + t, lane, sm);
    const f32x16 dfeat = b1_tile(P, wr, X, t ? featn : feat, c0sh, dr[t], dw, sm);
    const int qbase = 32 * (tile0 + t);
    if constexpr (fine) {
      if (t == 0) wait_flag(done, need);       // the coarse twin grads are written
      ring_put(k, *ring, X, r, ray, zq[t], srcq[t], dfeat);
    } else {
      // coarse: per-point feature grads [point][feature f][level] for the fine
      // units' ring hand-off (lane half h holds levels tile_level(m, h))
      float* dst = k.dfeat + (size_t)ray * kDcRay + (size_t)(qbase + p) * 32;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int l = h ? tile_level(m, 1) : tile_level(m, 0);
        dst[l] = dfeat[2 * m];
        dst[16 + l] = dfeat[2 * m + 1];
      }
    }
  });
}

// render_bwd_kernel<CAP, kModeAtomic>: the primary template of the
// MLP-backward kernel (declared in hn_mlp_bwd.h; the binned schedule
// specialises it).  LDS: per wave the operand images X, the ring's slots, the
// scatter wave's voxel buffer V, the staged grid sizes, and sync: [0] coarse
// rays done, [1] fine units taken, [2] ring tickets, [5..) the slots' ready
// and freed counts.
// The waves' roles are the file header's; wave 3 only scatters because the
// table gradient is bound by the memory-side float-atomic rate, so the MLP
// work runs under it.  Every wave that waits, waits on a wave of its own
// workgroup: co-resident.
template <int CAP, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void render_bwd_kernel(B1K k) {
  static_assert(MODE == kModeAtomic, "the binned schedule has its own specialisation");
  extern __shared__ f32x4 smem4[];
  float* smem = reinterpret_cast<float*>(smem4);
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  float* X = smem + wave * kRRows * kXS;
  float* slots = smem + kB1Img;
  float* V = slots + kSlots * kSlotF;
  float* gsl = V + kVoxF;                        // [voxel buffer | grid sizes | sync]
  int* sync = reinterpret_cast<int*>(gsl + kGsLds);
  stage_grid_sizes(k.g, gsl);
  if (threadIdx.x < kSyncInts) sync[threadIdx.x] = 0;
  __syncthreads();
  const Ring ring{slots, &sync[2], &sync[5], &sync[5 + kSlots], gsl};
  const int64_t nb = gridDim.x;
  const int n_rays = k.B > (int64_t)blockIdx.x ? (int)((k.B - 1 - blockIdx.x) / nb + 1) : 0;
  // ray of the block's i-th unit: a contiguous chunk per block when the
  // batch divides evenly, so the rays in flight at one time across the chip
  // are far apart in a spatially ordered batch (concurrent atomics on the
  // same rows serialize at the memory side); strided otherwise
  const bool chunked = k.B % nb == 0;
  auto block_ray = [&](int64_t i) -> int64_t {
    if (!chunked) return (int64_t)blockIdx.x + i * nb;
    // a fixed pseudo-random permutation of the batch scatters both the rays in
    // flight across the chip (one per block) and a block's consecutive rays
    uint32_t x = (uint32_t)((int64_t)blockIdx.x * (k.B / nb) + i);
    if (k.scramble) {
      do {
        x = feistel(x, k.scramble, 0x5bd1e995u);
      } while ((int64_t)x >= k.B);
    }
    return (int64_t)x;
  };
  DW dw;
  dw_zero(dw);
  WRing wr;
  if (wave == kMW) {
    ring_drain<CAP>(k, ring, V, 2 * kSf / 64 * n_rays);
  } else {
    if (wave == 0) {
      wring_prime(wr, k.Pc, lane);
      for (int i = 0; i < n_rays; ++i) {
        b1_unit<kSc>(k, block_ray(i), 0, X, dw, wr, nullptr);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this ray's feature grads are in L2
        if (lane == 0) __hip_atomic_store(&sync[0], i + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      dw_flush(dw, k.slab + (size_t)blockIdx.x * kSlabSlots * W_END, lane);   // slot 0: coarse
      dw_zero(dw);
    }
    wring_prime(wr, k.Pf, lane);
    for (;;) {
      int u = 0;
      if (lane == 0) u = atomicAdd(&sync[1], 1);
      u = __builtin_amdgcn_readfirstlane(u);
      if (u >= 3 * n_rays) break;
      b1_unit<kSf>(k, block_ray(u / 3), u % 3, X, dw, wr, &ring, &sync[0], u / 3 + 1);
    }
    // every MLP wave stores its fine dW to its own slab slot (waves 0-2 ->
    // slots 1-3), inside this branch: the accumulators must not be live in
    // the scatter wave's code (a spill there would wait vmcnt(0), i.e. drain
    // its atomics).  Formerly the waves summed into one LDS image with LDS
    // atomics after waiting for wave 0: ~0.1 M cycles of the kernel's tail.
    dw_flush(dw, k.slab + ((size_t)blockIdx.x * kSlabSlots + (wave + 1)) * W_END, lane);
  }
}

// The blocks' dW slabs summed into the weight gradients (slab_reduce_block's
// fixed order).
__global__ __launch_bounds__(64 * kSlabGroups) void slab_reduce_kernel(const float* __restrict__ slab, int n_blocks,
                                                                       hn_mlp_grad dc, hn_mlp_grad df, int overwrite) {
  __shared__ float part[kSlabGroups][64];
  slab_reduce_block(slab, n_blocks, dc, df, overwrite, blockIdx.x, part);
}

}  // namespace hn

