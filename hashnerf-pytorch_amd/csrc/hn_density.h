// hn_density.h -- density queries: raw sigma (NeRFSmall's column 3, the value
// before raw2outputs' ReLU) of the field at caller-given points or on a regular
// lattice the kernel generates itself, and/or the occupancy bits sigma >
// threshold.  Only what sigma needs runs: encode_tile and the two sigma GEMMs
// (gemm_src<R_F0>, relu16, gemm_src<R_F1>), the operations of
// mlp_fwd_tile_src's first part in its order on the same packed fragments, so a
// point's sigma is bitwise the forward's.  Nothing per point but the answers is
// written: 4 B (sigma) and/or 1 bit (occupancy).
#pragma once
#include "hn_render_args.h"

namespace hn {

// Persistent workgroups of kDenWaves waves, kDenWgPerCu per compute unit (16
// waves per CU = 4 per SIMD, the render forward's occupancy); a wave runs one
// 32-point tile at a time.
constexpr int kDenWaves = 8;
constexpr int kDenWgPerCu = 2;
// The workgroup's LDS copy of the net: the resident image's prefix (the map at
// kResRegs, hn_mlp.h) up to its third region -- exactly R_F0 and R_F1's kept
// rows, read through FragRes like the render forward's resident form.
constexpr int kDenResFloats = res_reg_off(R_F2G);
static_assert(kResRegs[0] == R_F0 && kResRegs[1] == R_F1 && kResRegs[2] == R_F2G && kDenResFloats * 4 == 18432 &&
                  kDenResFloats % 4 == 0,
              "the sigma regions are the resident image's first two");

struct DensityK {
  GridArgs g;
  const float* table;
  const float* P;        // the packed net
  const float* x;        // [n][3] (points) or unused (lattice)
  int64_t n;
  float lo[3], step[3];  // lattice: coordinate on axis a = lo[a] + (float)i_a * step[a]
  uint32_t nx, ny;       // lattice: flat index q = (iz * ny + iy) * nx + ix
  float threshold;
  float* sigma;          // [n] or NULL
  uint32_t* occ;         // [(n + 31) / 32] or NULL: bit q & 31 of word q >> 5 = sigma[q] > threshold
};

// A flat lattice index as (ix, iy, iz), moved by a fixed number of points
// without a division per move.
struct LatticeAt {
  uint32_t ix, iy;
  uint64_t iz;
};
HN_DEV LatticeAt lattice_at(uint64_t q, uint32_t nx, uint32_t ny) {
  const uint64_t r = q / nx;
  return LatticeAt{(uint32_t)(q - r * nx), (uint32_t)(r % ny), r / ny};
}
// at + d, d = lattice_at(a count of points): each sum is below twice its dim, so one carry each
HN_DEV LatticeAt lattice_add(LatticeAt at, const LatticeAt& d, uint32_t nx, uint32_t ny) {
  uint64_t x = (uint64_t)at.ix + d.ix, y = (uint64_t)at.iy + d.iy;
  if (x >= nx) { x -= nx; ++y; }
  at.iz += d.iz;
  if (y >= ny) { y -= ny; ++at.iz; }
  at.ix = (uint32_t)x;
  at.iy = (uint32_t)y;
  return at;
}

// kLattice = false: point q is x[q].  kLattice = true: point q of the lattice.
// Tile t is points 32 t .. 32 t + 31 (it may wrap rows); workgroup b's wave w
// runs tiles (b + i gridDim.x) kDenWaves + w: at any time the device works on
// one contiguous run of the flat index, a workgroup on 256 consecutive points.
// No atomics, nothing accumulated: a second launch writes the same bits.
template <bool kLattice>
__global__ __launch_bounds__(64 * kDenWaves) void density_kernel(DensityK k) {
  __shared__ __attribute__((aligned(16))) float res[kDenResFloats];
  __shared__ float gsl[kGsLds];
  stage_grid_sizes(k.g, gsl);
  {
    // dwordx4 j of the image from the packed net's dwordx4 res_src / 4, as the
    // render forward's resident form copies its image
    constexpr int kN4 = kDenResFloats / 4;
    const f32x4* src = reinterpret_cast<const f32x4*>(k.P);
    f32x4* dst = reinterpret_cast<f32x4*>(res);
#pragma unroll
    for (int i = 0; i < (kN4 + 64 * kDenWaves - 1) / (64 * kDenWaves); ++i) {
      const int j = i * 64 * kDenWaves + (int)threadIdx.x;
      if (j < kN4) dst[j] = src[res_src(4 * j) >> 2];
    }
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int p = lane & 31, h = lane >> 5;
  const FragRes net{k.P, res};
  const int64_t n_tiles = (k.n + 31) >> 5;
  const int64_t stride = (int64_t)gridDim.x * kDenWaves;
  int64_t tile = (int64_t)blockIdx.x * kDenWaves + wave;
  LatticeAt at{}, step{};
  if constexpr (kLattice) {
    at = lattice_at((uint64_t)tile * 32u, k.nx, k.ny);
    step = lattice_at((uint64_t)stride * 32u, k.nx, k.ny);
  }
  for (; tile < n_tiles; tile += stride) {
    const int64_t q = tile * 32 + p;
    const bool valid = q < k.n;
    float pt[3];
    if constexpr (kLattice) {
      // the lane's point: p steps along x from the tile's first, carried into y and z
      // (a lane past n forms coordinates past the lattice: no memory is addressed by them)
      const uint32_t r = at.ix + (uint32_t)p;   // dims < 2^31: no wrap
      const uint32_t cx = r / k.nx;
      const uint32_t s = at.iy + cx;
      const uint32_t cy = s / k.ny;
      const float idx[3] = {(float)(r - cx * k.nx), (float)(s - cy * k.ny), (float)(at.iz + cy)};
#pragma unroll
      for (int a = 0; a < 3; ++a) pt[a] = __fadd_rn(k.lo[a], __fmul_rn(idx[a], k.step[a]));
      at = lattice_add(at, step, k.nx, k.ny);
    } else {
      const float* xp = k.x + 3 * (valid ? q : k.n - 1);
#pragma unroll
      for (int a = 0; a < 3; ++a) pt[a] = xp[a];
    }
    f32x16 feat;
    encode_tile(k.g, gsl, k.table, pt, h, feat);
    // sigma_net.0: 32 -> 64, ReLU; sigma_net.1: 64 -> 16 (row 0 = sigma): mlp_fwd_tile_src's first part
    f32x16 h0[2];
#pragma unroll
    for (int ob = 0; ob < 2; ++ob) {
      h0[ob] = gemm_src<R_F0>(net, ob, zero16(), lane, [&](int s) { return feat[s]; });
      relu16(h0[ob]);
    }
    const f32x16 s1 = gemm_src<R_F1>(net, 0, zero16(), lane, [&](int s) { return h0[s >> 4][s & 15]; });
    const bool own = lane < 32 && valid;   // row 0 of the D tile sits on lanes 0-31
    if (k.sigma != nullptr && own) __builtin_nontemporal_store(s1[0], k.sigma + q);
    if (k.occ != nullptr) {
      const uint32_t word = (uint32_t)__ballot(own && s1[0] > k.threshold);
      if (lane == 0) k.occ[tile] = word;
    }
  }
}

}  // namespace hn
