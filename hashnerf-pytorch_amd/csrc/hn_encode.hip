// hn_encode.hip -- standalone hash-grid encoding (fwd/bwd) and SH encoding,
// with the gradients w.r.t. the points and directions.
//
// Replaces HashEmbedder.forward (embedding/hash_encoding.py:84-110), its
// autograd (embedding_dense_backward per level) and SHEncoder.forward
// (embedding/spherical_harmonic.py:65-103).  One thread per (point, level):
// the 8 corner gathers of a level are independent 8-byte loads, consecutive
// threads write consecutive 8-byte feature pairs (coalesced [N][L*2] rows).
#include "hn_common.h"

namespace hn {

__global__ __launch_bounds__(256) void encode_fwd_kernel(GridArgs g, const float* __restrict__ x,
                                                         int64_t n, const float* __restrict__ table,
                                                         float* __restrict__ feat,
                                                         uint8_t* __restrict__ keep) {
  const int L = g.n_levels;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= n * L) return;
  const int64_t p = tid / L;
  const int l = (int)(tid - p * L);
  const float xp[3] = {x[3 * p], x[3 * p + 1], x[3 * p + 2]};
  float xc[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) xc[a] = clamp_t(xp[a], g.bmin[a], g.bmax[a]);
  const uint32_t mask = (1u << g.log2T) - 1u;
  Voxel v;
  voxel_level(xp, xc, g.gs[l], g.bmin, mask, v);
  float f0, f1;
  encode_level(table + ((size_t)l << g.log2T) * 2, v, f0, f1);
  *reinterpret_cast<float2*>(feat + (size_t)p * (2 * L) + 2 * l) = make_float2(f0, f1);
  if (keep != nullptr && l == 0) {
    // hash_encoding.py:66,109: the mask of the LAST level, taken after the
    // level-0 clamp => only NaN coordinates fail when L > 1.
    bool k = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float ref = (L > 1) ? xc[a] : xp[a];
      k = k && (ref == clamp_t(ref, g.bmin[a], g.bmax[a]));
    }
    keep[p] = k ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void encode_bwd_kernel(GridArgs g, const float* __restrict__ x,
                                                         int64_t n, const float* __restrict__ dfeat,
                                                         float* __restrict__ dtable) {
  const int L = g.n_levels;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= n * L) return;
  const int64_t p = tid / L;
  const int l = (int)(tid - p * L);
  const float xp[3] = {x[3 * p], x[3 * p + 1], x[3 * p + 2]};
  float xc[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) xc[a] = clamp_t(xp[a], g.bmin[a], g.bmax[a]);
  const uint32_t mask = (1u << g.log2T) - 1u;
  Voxel v;
  voxel_level(xp, xc, g.gs[l], g.bmin, mask, v);
  const float2 gd = *reinterpret_cast<const float2*>(dfeat + (size_t)p * (2 * L) + 2 * l);
  float c0[8], c1[8];
  trilerp_bwd(gd.x, v.w, c0);
  trilerp_bwd(gd.y, v.w, c1);
  float* base = dtable + ((size_t)l << g.log2T) * 2;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    atomic_add_f32(base + 2 * (size_t)v.h[c], c0[c]);
    atomic_add_f32(base + 2 * (size_t)v.h[c] + 1, c1[c]);
  }
}

// d f / d w of trilerp for one feature's 8 corner values, times the upstream
// g: autograd's nested-lerp derivatives (hash_encoding.py:145-161 backwards:
// z, then y, then x), added to dw[3].
HN_DEV void trilerp_bwd_w(float g, const float e[8], const float w[3], float dw[3]) {
  const float ax = 1.f - w[0], ay = 1.f - w[1];
  const float c00 = e[0] * ax + e[4] * w[0];
  const float c01 = e[1] * ax + e[5] * w[0];
  const float c10 = e[2] * ax + e[6] * w[0];
  const float c11 = e[3] * ax + e[7] * w[0];
  const float c0 = c00 * ay + c10 * w[1];
  const float c1 = c01 * ay + c11 * w[1];
  const float g0 = g * (1.f - w[2]), g1 = g * w[2];      // d / d c0, d / d c1
  dw[2] += g * (c1 - c0);
  dw[1] += g0 * (c10 - c00) + g1 * (c11 - c01);
  dw[0] += (g0 * ay) * (e[4] - e[0]) + (g1 * ay) * (e[5] - e[1]) +
           (g0 * w[1]) * (e[6] - e[2]) + (g1 * w[1]) * (e[7] - e[3]);
}

// One level's share of d loss / d x for one point: voxel_level's cell and
// weights, the 8 corner rows, both features' d f / d w, over vmax - vmin
// (d w_a / d x_a = 1 / (vmax_a - vmin_a), hash_encoding.py:143).  row(h) loads
// the level's table row h as a float2.
template <typename Row>
HN_DEV void level_dx(const float xp[3], const float xc[3], const float gs[3], const float bmin[3], uint32_t mask,
                     float2 gd, Row row, float dx[3]) {
  Voxel v;
  uint32_t cell[3];
  voxel_level_cell(xp, xc, gs, bmin, mask, v, cell);     // voxel_level's ops
  float e0[8], e1[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float2 t = row(v.h[c]);
    e0[c] = t.x;
    e1[c] = t.y;
  }
  float dw[3] = {0.f, 0.f, 0.f};
  trilerp_bwd_w(gd.x, e0, v.w, dw);
  trilerp_bwd_w(gd.y, e1, v.w, dw);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float vmin = (float)(int32_t)cell[a] * gs[a] + bmin[a];   // vmax - vmin as voxel_level forms it
    dx[a] += dw[a] / ((vmin + gs[a]) - vmin);
  }
}

// L = 16: one thread per (point, level) like encode_fwd_kernel; the 16 levels
// of a point are 16 consecutive lanes, whose three partial sums are reduced
// by xor shuffles inside that group.  Every lane reaches the shuffles: lanes
// past n * 16 contribute zeros.
__global__ __launch_bounds__(256) void encode_bwd_input16_kernel(GridArgs g, const float* __restrict__ x,
                                                                 int64_t n, const float* __restrict__ table,
                                                                 const float* __restrict__ dfeat,
                                                                 float* __restrict__ dx) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = tid < n * 16;
  const int64_t p = tid >> 4;
  const int l = (int)(tid & 15);
  float d[3] = {0.f, 0.f, 0.f};
  if (live) {
    const float xp[3] = {x[3 * p], x[3 * p + 1], x[3 * p + 2]};
    float xc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) xc[a] = clamp_t(xp[a], g.bmin[a], g.bmax[a]);
    const uint32_t mask = (1u << g.log2T) - 1u;
    const float2 gd = *reinterpret_cast<const float2*>(dfeat + (size_t)p * 32 + 2 * l);
    const uint32_t row0 = (uint32_t)l << g.log2T;        // (16 << 24) * 8 bytes fits 32 bits
    level_dx(xp, xc, g.gs[l], g.bmin, mask, gd, [&](uint32_t h) { return ld_row(table, (row0 + h) * 8u); }, d);
  }
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] += __shfl_xor(d[a], m, 16);
  }
  if (live && l == 0) {
    dx[3 * p] = d[0];
    dx[3 * p + 1] = d[1];
    dx[3 * p + 2] = d[2];
  }
}

// Any other level count (1 .. HN_MAX_LEVELS): one thread per point, the
// levels in a loop.
__global__ __launch_bounds__(256) void encode_bwd_input_kernel(GridArgs g, const float* __restrict__ x,
                                                               int64_t n, const float* __restrict__ table,
                                                               const float* __restrict__ dfeat,
                                                               float* __restrict__ dx) {
  const int L = g.n_levels;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const float xp[3] = {x[3 * p], x[3 * p + 1], x[3 * p + 2]};
  float xc[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) xc[a] = clamp_t(xp[a], g.bmin[a], g.bmax[a]);
  const uint32_t mask = (1u << g.log2T) - 1u;
  float d[3] = {0.f, 0.f, 0.f};
  for (int l = 0; l < L; ++l) {
    const float2 gd = *reinterpret_cast<const float2*>(dfeat + (size_t)p * (2 * L) + 2 * l);
    const float* table_l = table + ((size_t)l << g.log2T) * 2;
    level_dx(xp, xc, g.gs[l], g.bmin, mask, gd,
             [&](uint32_t h) { return *reinterpret_cast<const float2*>(table_l + 2 * (size_t)h); }, d);
  }
  dx[3 * p] = d[0];
  dx[3 * p + 1] = d[1];
  dx[3 * p + 2] = d[2];
}

// d sh16 / d (x, y, z) contracted with the upstream go[16].
HN_DEV void sh16_bwd(float x, float y, float z, const float go[16], float d[3]) {
  const float C1 = 0.4886025119029199f;
  const float C2_0 = 1.0925484305920792f, C2_1 = -1.0925484305920792f,
              C2_2 = 0.31539156525252005f, C2_3 = -1.0925484305920792f,
              C2_4 = 0.5462742152960396f;
  const float C3_0 = -0.5900435899266435f, C3_1 = 2.890611442640554f,
              C3_2 = -0.4570457994644658f, C3_3 = 0.3731763325901154f,
              C3_4 = -0.4570457994644658f, C3_5 = 1.445305721320277f,
              C3_6 = -0.5900435899266435f;
  const float xx = x * x, yy = y * y, zz = z * z;
  const float xy = x * y, yz = y * z, xz = x * z;
  const float g4 = C2_0 * go[4], g5 = C2_1 * go[5], g6 = C2_2 * go[6], g7 = C2_3 * go[7], g8 = C2_4 * go[8];
  const float g9 = C3_0 * go[9], g10 = C3_1 * go[10], g11 = C3_2 * go[11], g12 = C3_3 * go[12],
              g13 = C3_4 * go[13], g14 = C3_5 * go[14], g15 = C3_6 * go[15];
  d[0] = -C1 * go[3] + g4 * y - 2.f * g6 * x + g7 * z + 2.f * g8 * x
         + 6.f * g9 * xy + g10 * yz - 2.f * g11 * xy - 6.f * g12 * xz
         + g13 * (4.f * zz - 3.f * xx - yy) + 2.f * g14 * xz + 3.f * g15 * (xx - yy);
  d[1] = -C1 * go[1] + g4 * x + g5 * z - 2.f * g6 * y - 2.f * g8 * y
         + 3.f * g9 * (xx - yy) + g10 * xz + g11 * (4.f * zz - xx - 3.f * yy) - 6.f * g12 * yz
         - 2.f * g13 * xy - 2.f * g14 * yz - 6.f * g15 * xy;
  d[2] = C1 * go[2] + g5 * y + 4.f * g6 * z + g7 * x
         + g10 * xy + 8.f * g11 * yz + g12 * (6.f * zz - 3.f * xx - 3.f * yy)
         + 8.f * g13 * xz + g14 * (xx - yy);
}

__global__ __launch_bounds__(256) void sh_bwd_kernel(const float* __restrict__ dirs, const float* __restrict__ dout,
                                                     int64_t n, float* __restrict__ ddirs) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  float go[16];
  const float4* src = reinterpret_cast<const float4*>(dout + 16 * p);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 t = src[i];
    go[4 * i] = t.x; go[4 * i + 1] = t.y; go[4 * i + 2] = t.z; go[4 * i + 3] = t.w;
  }
  float d[3];
  sh16_bwd(dirs[3 * p], dirs[3 * p + 1], dirs[3 * p + 2], go, d);
  ddirs[3 * p] = d[0];
  ddirs[3 * p + 1] = d[1];
  ddirs[3 * p + 2] = d[2];
}

__global__ __launch_bounds__(256) void sh_fwd_kernel(const float* __restrict__ d, int64_t n,
                                                     float* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  float o[16];
  sh16(d[3 * p], d[3 * p + 1], d[3 * p + 2], o);
  float4* dst = reinterpret_cast<float4*>(out + 16 * p);
#pragma unroll
  for (int i = 0; i < 4; ++i) dst[i] = make_float4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
}

static int32_t check_grid(const hn_grid* g) {
  if (!g) return HN_E_NULL;
  if (g->n_levels < 1 || g->n_levels > HN_MAX_LEVELS) return HN_E_SHAPE;
  if (g->n_features != 2) return HN_E_SHAPE;
  if (g->log2_hashmap_size < 1 || g->log2_hashmap_size > 24) return HN_E_SHAPE;
  return HN_OK;
}

}  // namespace hn

using namespace hn;

extern "C" int32_t hn_encode_fwd(const hn_grid* g, const float* x, int64_t n, const float* table,
                                 float* feat, uint8_t* keep_mask, void* stream) {
  int32_t st = check_grid(g);
  if (st) return st;
  if (n < 0) return HN_E_SHAPE;
  if (n == 0) return HN_OK;
  if (!x || !table || !feat) return HN_E_NULL;
  const int64_t total = n * g->n_levels;
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(encode_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     make_grid_args(*g), x, n, table, feat, keep_mask);
  return hip_status(hipGetLastError());
}

extern "C" int32_t hn_encode_bwd(const hn_grid* g, const float* x, int64_t n, const float* dfeat,
                                 float* dtable, void* stream) {
  int32_t st = check_grid(g);
  if (st) return st;
  if (n < 0) return HN_E_SHAPE;
  if (n == 0) return HN_OK;
  if (!x || !dfeat || !dtable) return HN_E_NULL;
  const int64_t total = n * g->n_levels;
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(encode_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     make_grid_args(*g), x, n, dfeat, dtable);
  return hip_status(hipGetLastError());
}

extern "C" int32_t hn_sh_fwd(const float* dirs, int64_t n, float* out, void* stream) {
  if (n < 0) return HN_E_SHAPE;
  if (n == 0) return HN_OK;
  if (!dirs || !out) return HN_E_NULL;
  hipLaunchKernelGGL(sh_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, dirs, n, out);
  return hip_status(hipGetLastError());
}

extern "C" int32_t hn_encode_bwd_input(const hn_grid* g, const float* x, int64_t n, const float* table,
                                       const float* dfeat, float* dx, void* stream) {
  int32_t st = check_grid(g);
  if (st) return st;
  if (n < 0) return HN_E_SHAPE;
  if (n == 0) return HN_OK;
  if (!x || !table || !dfeat || !dx) return HN_E_NULL;
  if (g->n_levels == 16) {
    hipLaunchKernelGGL(encode_bwd_input16_kernel, dim3((unsigned)((n * 16 + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, make_grid_args(*g), x, n, table, dfeat, dx);
  } else {
    hipLaunchKernelGGL(encode_bwd_input_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, make_grid_args(*g), x, n, table, dfeat, dx);
  }
  return hip_status(hipGetLastError());
}

extern "C" int32_t hn_sh_bwd(const float* dirs, const float* dout, int64_t n, float* ddirs, void* stream) {
  if (n < 0) return HN_E_SHAPE;
  if (n == 0) return HN_OK;
  if (!dirs || !dout || !ddirs) return HN_E_NULL;
  hipLaunchKernelGGL(sh_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, dirs, dout, n, ddirs);
  return hip_status(hipGetLastError());
}

extern "C" int32_t hn_abi_version(void) { return HN_ABI_VERSION; }

extern "C" const char* hn_status_string(int32_t s) {
  switch (s) {
    case HN_OK: return "ok";
    case HN_E_NULL: return "required pointer is NULL";
    case HN_E_SHAPE: return "unsupported shape/configuration";
    case HN_E_WORKSPACE: return "workspace too small";
    default: break;
  }
  if (s >= HN_E_HIP) return hipGetErrorString((hipError_t)(s - HN_E_HIP));
  return "unknown status";
}
