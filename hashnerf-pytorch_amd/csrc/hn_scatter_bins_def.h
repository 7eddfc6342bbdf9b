// hn_scatter_bins_def.h -- scatter_bins_kernel's definition (hn_bwd_binned.h
// says what it does), included once per fine-pass shape (no include guard) with
//   HN_SC_KERNEL  the kernel's name
//   HN_SC_FINE    the ray's fine samples (kSf or kSf64): the stride of the
//                 caller's z_fine and fine_src, and the dense form's units per ray
// A textual shape, not a template or an inlined body: either of those changed
// the register allocation of the kSf kernel, which this way stays the kernel
// it was before the second shape, instruction for instruction.
__global__ __launch_bounds__(64 * kScWaves) void HN_SC_KERNEL(ScK k) {
  // dynamic LDS: the bins' record counters, then the staging pool
  // (the host's BwdPlan::sc_lds)
  extern __shared__ __attribute__((aligned(16))) uint32_t sc_dyn[];
  unsigned long long* const bcnt = reinterpret_cast<unsigned long long*>(sc_dyn);   // BinW::lcnt
  __shared__ float gsl[kGsLds], lvmx[16];
  __shared__ uint32_t lovf;
  __shared__ uint32_t lvmxl[16 * 64];
  for (int i = threadIdx.x; i < 16 * 64; i += blockDim.x) lvmxl[i] = 0u;
  // wave-uniform work-unit arithmetic (u, ray = u / 3, u % 3, act) on the scalar unit
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = lane_id();
  for (int i = threadIdx.x; i < k.nbins; i += blockDim.x) bcnt[i] = 0ull;
  if (threadIdx.x < 16) lvmx[threadIdx.x] = 0.f;
  if (threadIdx.x == 0) lovf = 0u;
  stage_grid_sizes(k.g, gsl);
  __syncthreads();
  BinW bw;
  const size_t nrec = bin_records(k.nbins, k.bin_cap, k.B);
  bw.bins = k.bins;
  bw.nrec = nrec;
  uint32_t* const book = reinterpret_cast<uint32_t*>(k.bins + 4 * nrec);
  const OvfBook ob = ovf_book(book, nrec, k.nbins);
  bw.lovf = &lovf;
  bw.n_ovf = (uint32_t)ovf_per_block(k.B);
  bw.lcnt = bcnt;
  bw.base = (size_t)blockIdx.x * k.bin_cap;
  bw.stride = (size_t)kBwdBlocks * k.bin_cap;
  bw.ovf_base = (size_t)kBwdBlocks * k.nbins * k.bin_cap + (size_t)blockIdx.x * bw.n_ovf;

  bw.cap = (uint32_t)k.bin_cap;
  bw.shift = (uint32_t)k.bin_shift;
  // The block's units.  With exact-zero skipping: its slice of the list of
  // fine 16-sample groups that have feature grads to scatter
  // (render_lists_kernel, from the composite pre-pass's marks), the list in
  // ray order and cut into equal slices over the blocks -- every block the
  // same share of the work, whatever the scene leaves nonzero; a wave's unit
  // is four consecutive groups of the slice, one per 16-lane run row (often of
  // different rays; runs never cross rows, so the records are the dense
  // form's).  Otherwise (dense_bwd) every unit is a third of one ray's fine
  // samples, the rays permuted as the MLP backward's (unit_ray).
  const bool use_list = k.slist != nullptr;
  int64_t u0 = 0, u1 = 0;
  int64_t s0 = 0, s1 = 0;   // this block's slice of the group list
  if (use_list) {
    const int64_t Ns = __builtin_amdgcn_readfirstlane(k.lmeta[2]);
    s0 = (int64_t)blockIdx.x * Ns / gridDim.x;
    s1 = (int64_t)(blockIdx.x + 1) * Ns / gridDim.x;
    u1 = (s1 - s0 + 3) / 4;   // a unit = four consecutive groups of the slice, one per 16-lane row
  } else {
    const int64_t units = (HN_SC_FINE / 64) * k.B;   // 64-sample units: 3 per ray, 2 with a 128-sample fine pass
    const int64_t per = (units + gridDim.x - 1) / gridDim.x;
    u0 = (int64_t)blockIdx.x * per;
    u1 = u0 + per < units ? u0 + per : units;
  }
  const int pp = lane & 15;
  // the staging pool: 80 KiB
  uint32_t* const st_raw = sc_dyn + 2 * ((k.nbins + 3) & ~3);   // 16-B aligned after the counters
  f32x4* const stv = reinterpret_cast<f32x4*>(st_raw);
  uint32_t* const stw = st_raw + 4 * kStPool;
  __shared__ uint32_t stfl[2][kStPool >> kStMinLog2C];   // per phase parity: first staged slot per bin
  const int log2T = (int)k.g.log2T, sh = k.bin_shift;
  // first staged slot of each bin of level l (the bins' counts so far, capped)
  // (stfl alternates between phases: par = the phase's parity)
  int par = 0;
  auto st_init = [&](const StPhase& ph, int pr) {
    if (ph.log2c < kStMinLog2C) return;
    for (int i = threadIdx.x; i < ph.nbl; i += blockDim.x) {
      const unsigned long long c = bcnt[ph.b0 + i];
      stfl[pr][i] = min((uint32_t)c, bw.cap);
      bcnt[ph.b0 + i] = c & 0xffffffffull;   // the phase's count from 0 (no atomics in flight on it now)
    }
  };
  // the pool's records of level l to their regions, in slot order
  auto st_flush = [&](const StPhase& ph) {
    if (ph.log2c < kStMinLog2C) return;
    const uint32_t c = 1u << ph.log2c;
    for (int p = threadIdx.x; p < kStPool; p += blockDim.x) {
      const int bl = p >> ph.log2c, b = ph.b0 + bl;
      const uint32_t j = (uint32_t)p & (c - 1u), f = stfl[par][bl];
      const uint32_t end = min(min((uint32_t)bcnt[b], bw.cap), f + c);
      if (f + j < end) {
        const size_t r = bw.base + (size_t)b * bw.stride + f + j;
        rec_put<true>(bw.bins, r, bw.nrec, stv[p], stw[p]);
      }
    }
  };
  const int64_t n_it = (u1 - u0 + kScWaves - 1) / kScWaves;   // the same for every wave of the block
  // one unit's inputs: its ray, point and (fine + coarse twin) grads of one level
  struct Unit {
    bool act;
    Ray r;
    float pt[3], xc[3];
    const float* tb;   // the sample's fine grads (tile order), or null: exactly zero
    const float* tw;   // its coarse twin's grads, or null (none, or exactly zero)
    float g0, g1;      // the current level's two feature grads (fine + coarse twin)
  };
  bool bad = false;   // a non-finite grad or point seen by this lane
  // dense_bwd: a fixed pseudo-random permutation of the batch (ScK::scramble),
  // so the units without any gradient (below) spread evenly over the blocks
  auto unit_ray = [&](int64_t j) -> int64_t {
    uint32_t x = (uint32_t)j;
    if (k.scramble) {
      do {
        x = feistel(x, k.scramble, 0x5bd1e995u);
      } while ((int64_t)x >= k.B);
    }
    return (int64_t)x;
  };
  // unit u0 + wave + it * kScWaves: its ray, the lane's sample point and grad rows
  auto unit_base = [&](int64_t it) {
    Unit q;
    const int64_t u = u0 + wave + it * kScWaves;
    q.act = u < u1;
    q.g0 = q.g1 = 0.f;
    q.tb = q.tw = nullptr;
    if (q.act) {
      int64_t ray;
      int i;   // the lane's fine sample
      bool none = false;   // a second tile that does not exist: no grads
      if (use_list) {
        // row r of the unit: group s0 + 4 u + r, a group of 16 consecutive
        // samples of one ray -- the run rows are the dense form's, so the
        // records are too (minus the all-zero ones)
        const int64_t gj = s0 + 4 * u + (lane >> 4);
        const int c0 = k.slist[s0 + 4 * u];
        const int code = gj < s1 ? k.slist[gj] : c0;
        none = gj >= s1;
        ray = code >> 4;
        i = 16 * (code & 15) + (lane & 15);
      } else {
        ray = unit_ray(u / (HN_SC_FINE / 64));
        i = 64 * (int)(u % (HN_SC_FINE / 64)) + lane;
      }
      {
        const float* rb = k.rays + 11 * ray;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          q.r.o[a] = rb[a];
          q.r.d[a] = rb[3 + a];
        }
      }
      ray_point(q.r, k.z_fine[ray * HN_SC_FINE + i], q.pt);
#pragma unroll
      for (int a = 0; a < 3; ++a) q.xc[a] = clamp_t(q.pt[a], k.g.bmin[a], k.g.bmax[a]);
      bad |= !(fabsf((q.pt[0] + q.pt[1]) + q.pt[2]) <= 3.402823466e38f);
      // a sample whose d raw is exactly zero has exactly zero feature grads (the
      // MLP backward did not store them: the lists' skip); the same for
      // its coarse twin
      const float* dr = k.draw + (size_t)ray * (kSc + kSf) * 4;
      if (!none && (!k.skip_zero || draw_nonzero(*reinterpret_cast<const float4*>(dr + 4 * (kSc + i)))))
        q.tb = k.dfeat_f + ((size_t)ray * (kSf / 32) + (i >> 5)) * 1024 + 4 * (i & 31);
      const int src = k.fine_src[ray * HN_SC_FINE + i];
      if (!none && src < kSc && (!k.skip_zero || draw_nonzero(*reinterpret_cast<const float4*>(dr + 4 * src))))
        q.tw = k.dfeat_c + (size_t)ray * kDcRay + (size_t)(src >> 5) * 1024 + 4 * (src & 31);
      // no lane with a gradient: the unit writes no record (wave-uniform)
      q.act = __ballot(q.tb != nullptr || q.tw != nullptr) != 0ull;
    }
    return q;
  };
  // level l's grads = elements 2 (l & 1) .. of level pair l / 2 (tile_level:
  // chunk lp / 2 of lane half lp % 2); a coarse twin adds its coarse grads
  // (fine + twin, in that order); no twin: the fine grads as they are.  (Loading
  // level l + 1's while level l runs measured no faster, r05g.)
  auto unit_grads = [&](Unit& q, int l) {
    if (!q.act) return;
    const int lp = l >> 1, o = 4 * (64 * (lp >> 1) + 32 * (lp & 1)) + 2 * (l & 1);
    float2 gq = q.tb ? *reinterpret_cast<const float2*>(q.tb + o) : make_float2(0.f, 0.f);
    if (q.tw) {
      const float2 t = *reinterpret_cast<const float2*>(q.tw + o);
      gq = make_float2(gq.x + t.x, gq.y + t.y);
    }
    q.g0 = gq.x;
    q.g1 = gq.y;
    bad |= !(fabsf(gq.x + gq.y) <= 3.402823466e38f);
  };
  // The records of one level of a unit: voxel, run heads, per corner row the
  // x-pair sums over runs of samples in one voxel (16-lane rows), then each
  // head lane's record into the staging pool, or stored directly (slots from
  // the LDS counters)
  auto level = [&](const Unit& q, const int l, const StPhase& ph) {
    if (!q.act) return;
    const bool staged = ph.log2c >= kStMinLog2C;
    int32_t cell[3];
    float w[3];
    voxel_cw_sc(k.g, gsl, q.pt, q.xc, l, cell, w);
    const uint32_t cx = (uint32_t)cell[0], y0 = (uint32_t)cell[1] * kPrimeY, z0 = (uint32_t)cell[2] * kPrimeZ;
    const uint32_t q0 = dpp_u<kRowShr1>(cx), q1 = dpp_u<kRowShr1>(y0), q2 = dpp_u<kRowShr1>(z0);
    bool head = pp == 0 || q0 != cx || q1 != y0 || q2 != z0;
    const uint64_t hb = __ballot(head);
    const uint32_t pm = ((uint32_t)(hb >> (lane & 48)) & 0xffffu) | 0x10000u;   // + virtual head 16 (seg_same)
    // lane 0 of every row is a head, so these never carry across rows
    const uint64_t nz1 = ~hb & 0xfffefffefffefffeull, nz2 = nz1 & (nz1 >> 1), nz4 = nz2 & (nz2 >> 2);
    const bool s1 = nz1 != 0ull, s2 = nz2 != 0ull, s4 = nz4 != 0ull, s8 = (nz4 & (nz4 >> 4)) != 0ull;
    const float az = 1.f - w[2], ay = 1.f - w[1], ax = 1.f - w[0];
    // d feat / d e_c = ((g * wz) * wy) * wx (trilerp_bwd's order)
    // the two features as one packed pair (v_pk_mul_f32: the same fp32
    // products, half the instructions; the asm below would otherwise leave
    // them unpacked)
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 g2 = {q.g0, q.g1};
    const f2 gz[2] = {g2 * az, g2 * w[2]};   // [k] (features f0, f1)
    float vmax = 0.f;   // largest |record value| of the level: the owner's fixed-point scale
    float v[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = c >> 1, kk = c & 1;
      const float wy = j ? w[1] : ay;
      const f2 a = gz[kk] * wy;
      const f2 x0 = a * ax, x1 = a * w[0];
      v[c][0] = x0.x; v[c][1] = x0.y; v[c][2] = x1.x; v[c][3] = x1.y;
    }
    seg_sum16(v, pm, pp, s1, s2, s4, s8);
#pragma unroll
    for (int c = 0; c < 4; ++c) vmax = max3_abs(v[c][2], v[c][3], max3_abs(v[c][0], v[c][1], vmax));
    RecSlot rs[4];
    // a run whose four sums are exactly zero (samples without gradient, or a
    // zero trilinear weight) adds nothing to the owner's integer sums: no
    // record (the same table gradient bitwise; not with dense_bwd)
    bool put[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
      put[c] = head && (!k.skip_zero || ((__float_as_uint(v[c][0]) | __float_as_uint(v[c][1]) |
                                           __float_as_uint(v[c][2]) | __float_as_uint(v[c][3])) << 1) != 0u);
    if (head) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {   // 4 counter round trips in flight
        const int j = c >> 1, kk = c & 1;
        if (put[c])
          rs[c] = rec_slot(bw, (uint32_t)l, (uint32_t)log2T, cx, j ? y0 + kPrimeY : y0, kk ? z0 + kPrimeZ : z0,
                           staged ? kCntStaged : kCntRec);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (!put[c]) continue;
        // staged index = the record's place among the bin's records of this
        // phase (its slot minus the phase's first slot whenever slot < cap)
        const uint32_t bl = rs[c].bin - (uint32_t)ph.b0, j = rs[c].pj;
        if (staged && rs[c].slot < bw.cap && j < (1u << ph.log2c)) {
          const int qq = (int)((bl << ph.log2c) + j);
          stv[qq] = f32x4{v[c][0], v[c][1], v[c][2], v[c][3]};
          stw[qq] = rs[c].word;
          continue;
        }
        rec_store(bw, rs[c], v[c]);
      }
    }
    __hip_atomic_fetch_max(&lvmxl[l * 64 + lane], __float_as_uint(vmax), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
  };
  // staging phases of 2^lpp levels where each level owns whole bins and the
  // pool still holds >= 2^kStMinLog2C records per bin (T=19: 2 levels per
  // phase, 32 records per bin; T=22: 1 level, 8 per bin)
  const int lg_bins = log2T - sh;   // log2 bins per level
  const int lpp = lg_bins < 0 ? 0 : max(0, min(kScLpp, kStLog2 - kStMinLog2C - lg_bins));
  auto phase_of = [&](int l) { return st_phase(l, log2T, sh, l + (1 << lpp) <= 16 ? lpp : 0); };
  st_init(phase_of(0), par);
  __syncthreads();
  // the levels unit by unit (each unit's ray and rows loaded once), their
  // records through the staging pool, one phase per (unit round, level group)
  for (int64_t it = 0; it < n_it; ++it) {
    Unit q = unit_base(it);
    for (int l = 0; l < 16;) {
      const StPhase ph = phase_of(l);
      const int np = l + (1 << lpp) <= 16 ? 1 << lpp : 1;
      for (int j = 0; j < np; ++j, ++l) {
        unit_grads(q, l);
        level(q, l, ph);
      }
      __syncthreads();   // the phase's records are in the pool, its counts final
      st_flush(ph);
      // the next phase's bins (other parity), counts unchanged by the flush
      const int ln = l < 16 ? l : (it + 1 < n_it ? 0 : 16);
      if (ln < 16) st_init(phase_of(ln), par ^ 1);
      __syncthreads();   // the pool is free again
      par ^= 1;
    }
  }
  // non-finite inputs (NaN / Inf in a grad or the point): one test per lane
  if (__ballot(bad) != 0ull && lane == 0)
    __hip_atomic_fetch_or(&g_hn_fault, kFaultNonFinite, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (k.tv_off[16] > 0) {
    // The TV term's table gradient: one record per x-pair (x0, x0 + 1) of cube
    // vertices of one (y, z) row, d TV_l / d e (tv_grad) scaled by g_tv[l] /
    // cube, through the same region / overflow path as the render records
    // (so the owner pass sums render + TV exactly and the table step stays fused)
    const int total = k.tv_off[16], per = (total + (int)gridDim.x - 1) / (int)gridDim.x;
    const int q0 = (int)blockIdx.x * per, q1 = q0 + per < total ? q0 + per : total;
    const uint32_t T = (uint32_t)k.g.log2T;
    for (int q = q0 + (int)threadIdx.x; q < q1; q += (int)blockDim.x) {
      int l = 0;
      while (l + 1 < k.tv.L && q >= k.tv_off[l + 1]) ++l;
      const int c = k.tv.cube[l], n1 = c + 1, np = (n1 + 1) / 2, loc = q - k.tv_off[l];
      const int ip = loc % np, j = (loc / np) % n1, kk = loc / (np * n1);
      const uint32_t x0 = (uint32_t)(k.tv.mv[3 * l] + 2 * ip), y = (uint32_t)(k.tv.mv[3 * l + 1] + j),
                     z = (uint32_t)(k.tv.mv[3 * l + 2] + kk);
      const float scale = k.g_tv[l] / (float)c;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int f = 0; f < 2; ++f) v[f] = scale * tv_grad(k.tv, l, c, 2 * ip, j, kk, x0, y, z, f);
      if (2 * ip + 1 <= c)
#pragma unroll
        for (int f = 0; f < 2; ++f) v[2 + f] = scale * tv_grad(k.tv, l, c, 2 * ip + 1, j, kk, x0 + 1u, y, z, f);
      const float chk = (v[0] + v[1]) + (v[2] + v[3]);
      if (!(fabsf(chk) <= 3.402823466e38f))
        __hip_atomic_fetch_or(&g_hn_fault, kFaultNonFinite, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const float vmax = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
      __hip_atomic_fetch_max(reinterpret_cast<uint32_t*>(&lvmx[l]), __float_as_uint(vmax), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
      const RecSlot rs = rec_slot(bw, (uint32_t)l, T, x0, y * kPrimeY, z * kPrimeZ);
      rec_store(bw, rs, v);
    }
  }
  __syncthreads();
  if (wave == 0) {   // lane = level: the max of its 64 lane slots
    const int l = lane & 15, q = lane >> 4;
    uint32_t m = 0u;
    for (int j = 0; j < 16; ++j) m = max(m, lvmxl[l * 64 + 16 * q + j]);
    __hip_atomic_fetch_max(reinterpret_cast<uint32_t*>(&lvmx[l]), m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  uint32_t* cnt = book + nrec + blockIdx.x;
  for (int i = threadIdx.x; i < k.nbins; i += blockDim.x) {
    const uint32_t c = (uint32_t)bcnt[i];
    cnt[(size_t)i * kBwdBlocks] = c;
    if (c > bw.cap)   // spilled records of bin i (ovf_place_kernel's bucket sizes)
      __hip_atomic_fetch_add(ob.per_bin + i, c - bw.cap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  float* mxo = reinterpret_cast<float*>(book + nrec + (size_t)kBwdBlocks * k.nbins) + blockIdx.x;
  if (threadIdx.x < 16) mxo[threadIdx.x * kBwdBlocks] = lvmx[threadIdx.x];
  if (threadIdx.x == 0) {
    const uint32_t n = lovf < bw.n_ovf ? lovf : bw.n_ovf;
    ob.blk[blockIdx.x] = n;
    if (n) __hip_atomic_fetch_add(ob.cnt, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (k.slab) {   // the dW slabs are complete (the MLP-backward kernel ran before this one)
    float(*part)[64] = reinterpret_cast<float(*)[64]>(stv);   // the staging pool is free now
    static_assert(kStPool * 20 >= sizeof(float) * kSlabGroups * 64 && 64 * kScWaves == 64 * kSlabGroups,
                  "slab-reduce blocks inside the scatter blocks");
    // the 292 slab blocks go to the scatter blocks as they finish (a counter
    // reset by render_comp_bwd_kernel): the sums do not depend on who runs them
    __shared__ int vb_sh;
    for (;;) {
      __syncthreads();   // part and vb_sh are free (the pool's last readers, or the previous combine)
      if (threadIdx.x == 0)
        vb_sh = (int)__hip_atomic_fetch_add(ob.slab_next, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      const int vb = vb_sh;
      if (vb >= kSlabVBlocks) break;
      slab_reduce_block(k.slab, kBwdBlocks, k.dc, k.df, k.overwrite_mlp, vb, part, k.has_mstep ? k.mstep : nullptr,
                        k.lmeta + 3);
    }
  }
}
