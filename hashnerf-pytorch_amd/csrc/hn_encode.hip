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
