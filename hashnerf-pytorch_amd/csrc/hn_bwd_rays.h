// hn_bwd_rays.h -- the gradient of a fused forward with respect to its rays
// (hn_render_bwd_rays): pose refinement on the saved state of hn_render_fwd.
// near, far and the sampling draws are constants and the importance samples
// are detached (run_nerf_helpers.py:546), so no d z reaches the ray and, with
// the sums over the ray's 64 coarse points (coarse net, coarse z) and its fine
// points (fine net, fine z),
//   d o       = sum_k dx_k
//   d d       = sum_k z_k dx_k + d|d| d / |d|      (0 where |d| = 0)
//   d viewdir = J_sh(viewdir)^T sum_k dsh_k
// dx_k = hn_encode_bwd_input's closed form (level_dx) on the point's feature
// gradient, dsh_k = color_net.0's input gradient on its 16 SH columns, d|d| =
// composite_bwd_inputs' sum of each pass.  Launch order, after the composite
// pre-pass (render_comp_bwd_kernel, unchanged) has written d raw:
//   render_bwd_rays_kernel         one wave per (ray, 32-point tile): the MLP
//                                  backward's data path, dx per point, 22 partial
//                                  sums per unit
//   render_bwd_rays_reduce_kernel  one wave per ray: the partials in tile order,
//                                  d|d| of both passes, J_sh, d_rays [B][11]
// No atomics and no sum across waves: every sum has a fixed order, so d_rays
// is bitwise repeatable.
#pragma once
#include "hn_mlp_bwd.h"

namespace hn {

// Partial sums of one unit: [dx 3 | z dx 3 | dsh 16]
constexpr int kRayPart = 22;
constexpr int kRayWaves = 4;   // units (waves) per workgroup of either kernel

struct RaysK {
  int64_t B;
  int32_t nt;           // 32-point tiles per ray: 2 coarse + 6 (or 4) fine, the saved-feature tile order
  int32_t sf;           // fine samples per ray (the stride of z_fine)
  const float* rays;
  const float *Pc, *Pf;
  const float *z_coarse, *z_fine;
  const float* feat;    // the forward's saved state: only its ReLU mask words are read
  const float* draw;    // [B][64 + 192][4] d raw (the pre-pass's)
  const float* table;
  GridArgs g;
  float* part;          // [B][kTilesPerRay][kRayPart]
};

// v summed over the lanes l ^ 1 .. l ^ top (a butterfly of ds_bpermute moves:
// the same order on every launch)
template <int TOP>
HN_DEV float lanes_sum(float v, int lane) {
#pragma unroll
  for (int o = 1; o <= TOP; o <<= 1) v += shfl_from(v, lane ^ o);
  return v;
}

__global__ __launch_bounds__(64 * kRayWaves) void render_bwd_rays_kernel(RaysK k) {
  __shared__ float gsl[kGsLds];
  stage_grid_sizes(k.g, gsl);
  __syncthreads();
  const int lane = lane_id();
  const int64_t unit = (int64_t)blockIdx.x * kRayWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (unit >= k.B * kTilesPerRay) return;
  const int64_t ray = unit / kTilesPerRay;
  const int tile = (int)(unit % kTilesPerRay);
  if (tile >= k.nt) return;   // a 4-tile fine pass: no unit, its partials are never read
  const bool fine = tile >= kSc / 32;
  const int p = lane & 31, h = lane >> 5;
  const int i = 32 * (fine ? tile - kSc / 32 : tile) + p;   // the point within its pass
  const float4 dr = *reinterpret_cast<const float4*>(k.draw + ((size_t)ray * (kSc + kSf) + (fine ? kSc : 0) + i) * 4);
  float* out = k.part + (size_t)unit * kRayPart;
  // no gradient reaches any of the 32 points: exact zeros, and neither the
  // masks nor anything else a skip_dead_color forward left unwritten is read
  if (__ballot(draw_nonzero(dr)) == 0ull) {
    if (lane < kRayPart) out[lane] = 0.f;
    return;
  }
  uint32_t sm[3];
  load_masks(k.feat, ray, tile, lane, sm);
  // The data path of the tile's MLP backward (mlp_bwd_tile, nothing at its dW
  // points): d raw -> d feature [32 per point, the feature tile's D layout] and
  // d sh [16 per point].  The ReLU decisions are the forward's own, from its
  // saved mask words sm = [h0 | c0 | c1], so no activation is recomputed and no
  // feature read.
  f32x16 dfeat, dsh;
  mlp_bwd_tile(
      opaque_ptr(fine ? k.Pf : k.Pc), dr, [&](f32x16& v, int l, int ob) { mask_bits(v, sm[l], ob); },
      [](auto, const f32x16*) {}, dfeat, &dsh, lane);
  // the point, and its d x over this lane half's eight levels
  Ray r;
  load_ray(k.rays, ray, r);
  const float z = fine ? k.z_fine[ray * k.sf + i] : k.z_coarse[ray * kSc + i];
  float pt[3], xc[3];
  ray_point(r, z, pt);
#pragma unroll
  for (int a = 0; a < 3; ++a) xc[a] = clamp_t(pt[a], k.g.bmin[a], k.g.bmax[a]);
  const uint32_t mask = (1u << k.g.log2T) - 1u;
  float v[6 + 8] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const uint32_t l = h ? tile_level(m, 1) : tile_level(m, 0);
    const float gs[3] = {gsl[3 * l], gsl[3 * l + 1], gsl[3 * l + 2]};
    const uint32_t row0 = l << k.g.log2T;
    level_dx(pt, xc, gs, k.g.bmin, mask, make_float2(dfeat[2 * m], dfeat[2 * m + 1]),
             [&](uint32_t hr) { return ld_row(k.table, (row0 + hr) * 8u); }, v);
    if ((m & (kEncGroup - 1)) == kEncGroup - 1) __builtin_amdgcn_sched_barrier(0);   // <= 16 gathers in flight
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) v[3 + a] = z * v[a];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[6 + j] = dsh[j];
  // dx and z dx over the wave; each lane half's eight SH rows over its 32 points
#pragma unroll
  for (int j = 0; j < 6; ++j) v[j] = lanes_sum<32>(v[j], lane);
#pragma unroll
  for (int j = 6; j < 14; ++j) v[j] = lanes_sum<16>(v[j], lane);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 6; ++j) out[j] = v[j];
  }
  if (p == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) out[6 + row_of(j, h)] = v[6 + j];
  }
}

// What the second pass reads beside the partials: the composite backward's
// inputs of both passes (the pre-pass's own), for d |d|.
struct RaysR {
  int64_t B;
  int32_t nt, sf, white;
  const float* rays;
  const float *noise_c, *noise_f;
  const float *z_coarse, *z_fine, *raw_c, *raw_f;
  const float *g_rgb, *g_depth, *g_acc, *g_sparsity, *g_rgb0, *g_depth0, *g_acc0, *g_sparsity0;
  const float* part;
  float* d_rays;        // [B][11]: [d o | d d | 0 0 | d viewdir]
};

// d loss / d |d| of one pass of one ray (composite_bwd_inputs' sum)
template <int N>
HN_DEV float pass_dnorm(const float* raw, const float* z, const float* noise, int S, float dnorm, bool white,
                        const CompGrad& g, int lane) {
  CompSamples<N> cs;
  composite_samples<N>(raw, z, noise, S, dnorm, cs, lane);
  CompTotals t;
  composite_totals<N>(cs, t);
  return composite_bwd_inputs<N>(cs, t, z, S, dnorm, white, g, nullptr, nullptr, lane);
}

HN_DEV void pass_grad(CompGrad& g, int64_t ray, const float* grgb, const float* gacc, const float* gdep,
                      const float* gent) {
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

__global__ __launch_bounds__(64 * kRayWaves) void render_bwd_rays_reduce_kernel(RaysR k) {
  const int lane = lane_id();
  const int64_t ray = (int64_t)blockIdx.x * kRayWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (ray >= k.B) return;
  Ray r;
  load_ray(k.rays, ray, r);
  const bool white = k.white != 0;
  CompGrad g;
  pass_grad(g, ray, k.g_rgb0, k.g_acc0, k.g_depth0, k.g_sparsity0);
  const float dn_c = pass_dnorm<kSc / 64>(k.raw_c + ray * kSc * 4, k.z_coarse + ray * kSc,
                                          k.noise_c ? k.noise_c + ray * kSc : nullptr, kSc, r.dnorm, white, g, lane);
  pass_grad(g, ray, k.g_rgb, k.g_acc, k.g_depth, k.g_sparsity);
  const int S = k.sf;
  const float* rawf = k.raw_f + ray * S * 4;
  const float* zf = k.z_fine + ray * S;
  const float* nf = k.noise_f ? k.noise_f + ray * S : nullptr;
  const float dn_f = S == kSf ? pass_dnorm<kSf / 64>(rawf, zf, nf, S, r.dnorm, white, g, lane)
                              : pass_dnorm<kSf64 / 64>(rawf, zf, nf, S, r.dnorm, white, g, lane);
  // column `lane` of the ray's partials, tile by tile
  float s = 0.f;
  if (lane < kRayPart)
    for (int t = 0; t < k.nt; ++t) s += k.part[((size_t)ray * kTilesPerRay + t) * kRayPart + lane];
  float dxs[6], go[16];
#pragma unroll
  for (int j = 0; j < 6; ++j) dxs[j] = shfl_from(s, j);
#pragma unroll
  for (int j = 0; j < 16; ++j) go[j] = shfl_from(s, 6 + j);
  if (lane == 0) {
    float dv[3];
    sh16_bwd(r.vd[0], r.vd[1], r.vd[2], go, dv);
    // torch.norm's backward: g d / |d|, zero where |d| = 0 (each pass as hn_composite_bwd_inputs forms it)
    const float sc = r.dnorm > 0.f ? dn_c / r.dnorm : 0.f, sf = r.dnorm > 0.f ? dn_f / r.dnorm : 0.f;
    float* o = k.d_rays + 11 * ray;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      o[a] = dxs[a];
      o[3 + a] = dxs[3 + a] + (sc * r.d[a] + sf * r.d[a]);
      o[8 + a] = dv[a];
    }
    o[6] = o[7] = 0.f;
  }
}

}  // namespace hn
