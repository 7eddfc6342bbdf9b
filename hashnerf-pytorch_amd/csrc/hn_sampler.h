// hn_sampler.h -- the Morton ray sampler's and the uniform draws' device code
// (hn_sample_batch_morton), as workgroup bodies with a block index of their
// own: hn_train.hip's two sampler kernels are thin wrappers of them, and the
// binned render backward (hn_bwd_binned.h) runs the same bodies for the NEXT
// step's batch as extra workgroups of its two small launches
// (hn_render_bwd_args.next_batch) -- the same functions on the same seeds, so
// the drawn values are bitwise those of the stand-alone entry point.
#pragma once
#include "hn_common.h"

namespace hn {

// ---------------------------------------------------------------------------
// The per-image draw in Morton order of its pixels (window-relative row,
// column): pixel x is drawn iff perm^-1(x) < n, so walking the Morton indices of the
// window and compacting the drawn ones lists the draw's set in that order with
// no sort.  Two passes with a kernel boundary between them: per-tile counts,
// then prefix + tile scan + emit.  A tile is kMortonThreads Morton indices.
// ---------------------------------------------------------------------------
constexpr int kMortonThreads = 1024;
HN_DEV uint32_t compact_bits16(uint32_t v) {
  v &= 0x55555555u;
  v = (v | (v >> 1)) & 0x33333333u;
  v = (v | (v >> 2)) & 0x0f0f0f0fu;
  v = (v | (v >> 4)) & 0x00ff00ffu;
  v = (v | (v >> 8)) & 0x0000ffffu;
  return v;
}
// Morton index m -> drawn pixel (window-relative linear index) or ~0u
HN_DEV uint32_t morton_drawn(const hn_ray_sampler& s, int half, int64_t n, uint32_t m) {
  const uint32_t row = compact_bits16(m >> 1), col = compact_bits16(m);
  if (row >= (uint32_t)s.crop_h || col >= (uint32_t)s.crop_w) return ~0u;
  const uint32_t M = (uint32_t)s.crop_h * (uint32_t)s.crop_w;
  const uint32_t x = row * (uint32_t)s.crop_w + col;
  uint32_t y = x;
  do {   // inverse of the cycle-walked permutation
    y = feistel_inv(y, half, s.seed);
  } while (y >= M);
  return (int64_t)y < n ? x : ~0u;
}

// torch.rand on the CUDA/HIP default generator, restated (ATen's
// distribution_elementwise_grid_stride_kernel with hiprand's Philox4x32-10,
// unroll 4): element li of a draw comes from thread idx = li % T of torch's
// launch (T threads), its call it = li / (4T) and component (li / T) % 4 --
// Philox of counter (offset / 4 + it, subsequence idx) under key = seed,
// mapped by rocrand's 2^-32 + v * 2^-32 to (0, 1], and 1 -> 0 (uniform_'s
// bound reversal).
struct UniK {
  uint32_t key[2];
  int n;
  int64_t start[HN_UNIFORM_MAX_DRAWS + 1];   // element prefix of the draws
  hn_uniform_draw d[HN_UNIFORM_MAX_DRAWS];
};
HN_DEV uint32_t philox_component(uint64_t ctr, uint64_t sub, uint32_t k0, uint32_t k1, int comp) {
  uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = (uint32_t)sub, c3 = (uint32_t)(sub >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return comp == 0 ? c0 : comp == 1 ? c1 : comp == 2 ? c2 : c3;
}
// global element g of the UniK's draws
HN_DEV void uniform_elem(const UniK& u, int64_t g) {
  int j = 0;
  while (j + 1 < u.n && g >= u.start[j + 1]) ++j;
  const hn_uniform_draw& d = u.d[j];
  const int64_t li = g - u.start[j];
  const uint64_t T = (uint64_t)d.threads, idx = (uint64_t)li % T, rem = (uint64_t)li / T;
  const uint32_t v = philox_component(d.offset / 4 + (rem >> 2), idx, u.key[0], u.key[1], (int)(rem & 3));
  const float x = 0x1p-32f + (float)v * 0x1p-32f;
  d.out[li] = x == 1.f ? 0.f : x;
}
// elements [b, b + 1) * kMortonThreads of the draws, by a workgroup of kThreads
template <int kThreads>
HN_DEV void uniform_block(const UniK& u, unsigned b) {
  for (int i = threadIdx.x; i < kMortonThreads; i += kThreads) {
    const int64_t g = (int64_t)b * kMortonThreads + i;
    if (g < u.start[u.n]) uniform_elem(u, g);
  }
}

// One Morton draw: the arguments of sample_morton's two passes
struct MortonK {
  hn_ray_sampler s;
  const float* image;
  const float* c2w;
  int half;          // the Feistel network's half width (bits)
  int64_t n;         // rays drawn
  uint32_t n_idx;    // Morton indices that cover the window (4^k)
  unsigned blocks;   // tiles: ceil(n_idx / kMortonThreads)
  int* counts;       // [blocks] drawn pixels per tile (the workspace)
  float* rays;       // [n][11]
  float* target;     // [n][3]
};

// Pass 1, tile b: its number of drawn pixels.  Every thread of a workgroup of
// kThreads (a divisor of kMortonThreads) calls it.
template <int kThreads>
HN_DEV void morton_count_block(const MortonK& k, unsigned b) {
  static_assert(kMortonThreads % kThreads == 0, "every thread makes the same number of rounds");
  int c = 0;
  for (int i = threadIdx.x; i < kMortonThreads; i += kThreads) {
    const uint32_t m = b * kMortonThreads + i;
    const bool sel = m < k.n_idx && morton_drawn(k.s, k.half, k.n, m) != ~0u;
    c += __syncthreads_count(sel);
  }
  if (threadIdx.x == 0) k.counts[b] = c;
}

// The ray of pixel (row py, column px) as render() packs it
// (ray_util.py:62-80, run_nerf_helpers.py:355-368): out[11] = [o3 d3 near far
// viewdir3].  Every ray a sampler or the image renderer makes comes from here,
// float32 operation for float32 operation.
HN_DEV void pixel_ray(float fx, float fy, float cx, float cy, float near, float far, const float* __restrict__ c2w,
                      int px, int py, float out[11]) {
  // dirs = [(i - cx) / fx, -(j - cy) / fy, -1]; rays_d = sum(dirs * c2w[:3,:3], -1)
  const float d0 = ((float)px - cx) / fx;
  const float d1 = -(((float)py - cy) / fy);
  const float d2 = -1.f;
  float d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    d[a] = d0 * c2w[4 * a] + d1 * c2w[4 * a + 1] + d2 * c2w[4 * a + 2];
    out[a] = c2w[4 * a + 3];
    out[3 + a] = d[a];
  }
  out[6] = near;
  out[7] = far;
  const float nrm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
#pragma unroll
  for (int a = 0; a < 3; ++a) out[8 + a] = d[a] / nrm;
}

// render()'s NDC step on a packed ray (run_nerf_helpers.py:349 get_ndc_rays(H,
// W, K[0][0], 1., o, d), ray_util.py:96-142): out[0:6] rewritten, near, far
// and the view direction (taken from the world direction before this step)
// left alone.  Every operation below is one separately rounded float32
// operation in torch's order (the library is built with -ffp-contract=off), so
// the result is rays.get_ndc_rays' bit for bit.  The near plane is render()'s
// constant 1.: torch evaluates 2. * near / o_z as reciprocal(o_z) * 2., which
// is 2 / o_z bit for bit only because doubling is exact -- another plane needs
// that restated.  sx, sy: the Python scalars -1. / (W / (2. * focal)) and
// -1. / (H / (2. * focal)), focal = K[0][0] (the reference's quirk: not cx, cy
// or fy), formed in float64 by the caller and passed as float32.  A ray with
// d_z = 0 gets whatever non-finite values these operations give.
HN_DEV void ndc_ray(float sx, float sy, float out[11]) {
  const float t = -(1.f + out[2]) / out[5];
  float o[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float td = t * out[3 + a];
    o[a] = out[a] + td;
  }
  const float ox_oz = o[0] / o[2], oy_oz = o[1] / o[2];
  const float o2 = 1.f + 2.f / o[2];
  const float dx_dz = out[3] / out[5], dy_dz = out[4] / out[5];
  out[0] = sx * ox_oz;
  out[1] = sy * oy_oz;
  out[2] = o2;
  out[3] = sx * (dx_dz - ox_oz);
  out[4] = sy * (dy_dz - oy_oz);
  out[5] = 1.f - o2;
}

// A sampler's NDC step (hn_ray_ndc): a kernel argument of its own beside the
// draw's, so `on` is wave-uniform (a scalar branch) and the structs of the
// world-ray draw -- and the kernels that only count, which never form a ray
// -- stay as they are.  on = 0: world rays.
struct NdcK {
  int on;
  float sx, sy;
};

HN_DEV void emit_ray(const hn_ray_sampler& s, const float* __restrict__ image, const float* __restrict__ c2w,
                     const NdcK& ndc, uint32_t x, int64_t r, float* __restrict__ rays,
                     float* __restrict__ target) {
  const int py = s.crop_y0 + (int)(x / (uint32_t)s.crop_w);
  const int px = s.crop_x0 + (int)(x % (uint32_t)s.crop_w);
  float ray[11];
  pixel_ray(s.fx, s.fy, s.cx, s.cy, s.near, s.far, c2w, px, py, ray);
  if (ndc.on) ndc_ray(ndc.sx, ndc.sy, ray);
#pragma unroll
  for (int a = 0; a < 11; ++a) rays[11 * r + a] = ray[a];
  const float* px3 = image + 3 * ((size_t)py * s.W + px);
#pragma unroll
  for (int a = 0; a < 3; ++a) target[3 * r + a] = px3[a];
}

// Pass 2, tile b (after every tile's pass 1: a kernel boundary): the rays of
// its drawn pixels, behind those of the earlier tiles.  Every thread of a
// workgroup of exactly kMortonThreads calls it.
HN_DEV void morton_emit_block(const MortonK& k, const NdcK& ndc, unsigned b) {
  __shared__ int part[kMortonThreads / 64 + 1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // rays drawn by the earlier tiles
  uint32_t pre = 0;
  for (uint32_t q = tid; q < b; q += kMortonThreads) pre += (uint32_t)k.counts[q];
  pre = wave_sum(pre);
  if (lane == 0) part[wave] = (int)pre;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int w = 0; w < kMortonThreads / 64; ++w) base += part[w];
  __syncthreads();
  const uint32_t m = b * kMortonThreads + tid;
  const uint32_t x = m < k.n_idx ? morton_drawn(k.s, k.half, k.n, m) : ~0u;
  const bool sel = x != ~0u;
  const uint64_t bal = __ballot(sel);
  if (lane == 0) part[wave] = __popcll(bal);
  __syncthreads();
  int off = base;
  for (int w = 0; w < wave; ++w) off += part[w];
  if (!sel) return;
  const int64_t r = off + __popcll(bal & ((1ull << lane) - 1ull));
  emit_ray(k.s, k.image, k.c2w, ndc, x, r, k.rays, k.target);
}

// ---------------------------------------------------------------------------
// use_batching ray pool: position q of the epoch's shuffle -> its ray (11
// floats at `out`) and target colour (3 at `tgt`).  hn_sample_pool writes the
// positions in order, hn_sample_pool_ordered in Morton order of their keys --
// the same function, so the same 14 floats.
// ---------------------------------------------------------------------------
HN_DEV void pool_ray(const hn_ray_pool& p, const float* __restrict__ images, const float* __restrict__ poses,
                     const int32_t* __restrict__ ids, int half, uint32_t q, float* __restrict__ out,
                     float* __restrict__ tgt) {
  const uint32_t hw = (uint32_t)p.H * (uint32_t)p.W;
  const uint32_t N = (uint32_t)p.n_images * hw;
  uint32_t x = q;
  do {
    x = feistel(x, half, p.seed);
  } while (x >= N);
  const int img = ids[x / hw];
  const uint32_t pix = x % hw;
  const int py = (int)(pix / (uint32_t)p.W), px = (int)(pix % (uint32_t)p.W);
  const float* c = poses + (size_t)img * p.pose_stride;
  // dirs = [(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -1] (float64: K is)
  const double d0 = ((double)px - p.cx) / p.fx;
  const double d1 = -((double)py - p.cy) / p.fy;
  const double d2 = -1.0;
  float d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {   // np.sum(dirs[..., None, :] * c2w[:3, :3], -1): ((p0 + p1) + p2)
    d[a] = (float)((d0 * (double)c[4 * a] + d1 * (double)c[4 * a + 1]) + d2 * (double)c[4 * a + 2]);
    out[a] = c[4 * a + 3];
    out[3 + a] = d[a];
  }
  out[6] = p.near;
  out[7] = p.far;
  const float nrm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);   // render(): viewdirs (:350)
#pragma unroll
  for (int a = 0; a < 3; ++a) out[8 + a] = d[a] / nrm;
  const float* px3 = images + 3 * (((size_t)img * p.H + py) * p.W + px);
#pragma unroll
  for (int a = 0; a < 3; ++a) tgt[a] = px3[a];
}

// The ray a pool draw hands out: pool_ray's, then render()'s NDC step where
// the draw asks for one (the target, near, far and the view direction stay
// the world ray's)
HN_DEV void pool_ray_final(const hn_ray_pool& p, const float* __restrict__ images, const float* __restrict__ poses,
                           const int32_t* __restrict__ ids, int half, const NdcK& ndc, uint32_t q, float r[11],
                           float t[3]) {
  pool_ray(p, images, poses, ids, half, q, r, t);
  if (ndc.on) ndc_ray(ndc.sx, ndc.sy, r);
}
// ... written to row `row` of a batch
HN_DEV void pool_ray_store(const float r[11], const float t[3], size_t row, float* __restrict__ rays,
                           float* __restrict__ target) {
#pragma unroll
  for (int a = 0; a < 11; ++a) rays[11 * row + a] = r[a];
#pragma unroll
  for (int a = 0; a < 3; ++a) target[3 * row + a] = t[a];
}

// One ordered pool draw (hn_sample_pool_ordered)
struct PoolOrderK {
  hn_ray_pool p;
  const float* images;
  const float* poses;
  const int32_t* ids;
  int64_t start;
  int n;             // rays, 1 .. HN_POOL_ORDER_MAX
  int padded;        // n rounded up to a power of two
  int half;          // the Feistel network's half width (bits)
  float box_min[3], box_max[3];
  float* rays;       // [n][11]
  float* target;     // [n][3]
  uint32_t* keys;    // [n] or nullptr
};

// The 30-bit Morton key of a ray's mid-depth point, clamped to the box; every
// operation a float32 one (the library is built with -ffp-contract=off).
HN_DEV uint32_t spread_bits10(uint32_t v) {   // bit k -> bit 3k
  v &= 0x3ffu;
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}
HN_DEV uint32_t pool_key(const PoolOrderK& k, const float* r) {
  const float tm = 0.5f * (k.p.near + k.p.far);
  uint32_t key = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float pt = r[a] + r[3 + a] * tm;
    float u = (pt - k.box_min[a]) / (k.box_max[a] - k.box_min[a]);
    u = fminf(fmaxf(u, 0.f), 1.f);   // fmaxf(NaN, 0) = 0
    const int c = min((int)(u * 1024.f), 1023);
    key |= spread_bits10((uint32_t)c) << a;
  }
  return key;
}

// The whole draw, by ONE workgroup of exactly kMortonThreads: keys, a bitonic
// sort of key << 13 | i in LDS (all words distinct, so the network's result is
// the unique ascending (key, i) order), then the rays of the sorted positions.
// A compare-exchange stage of stride j gives thread t the pair (lo, lo | j),
// lo = t with a zero inserted at bit log2 j: for j >= 32 the 32 lanes of a
// half-wave read 32 consecutive 8-byte words, one 256-byte bank row, without a
// conflict; for j < 32 they span two rows, a 2-way conflict -- 5 of the 13
// strides.  The layout stays linear: what the sort costs is a pass over the
// array per stage (DESIGN 4.6 has the phase times and what was tried).
constexpr int kPoolIdxBits = 13;
static_assert((1 << kPoolIdxBits) == HN_POOL_ORDER_MAX, "key << 13 | i holds every position of a batch");
// With an NDC step the key is that of the final (NDC) ray, under the pool's
// near and far as for a world ray.
HN_DEV void pool_order_block(const PoolOrderK& k, const NdcK& ndc) {
  __shared__ uint64_t w[HN_POOL_ORDER_MAX];
  const int tid = threadIdx.x;
  for (int i = tid; i < k.padded; i += kMortonThreads) {
    uint64_t word = ~0ull;   // the padding sorts behind every ray
    if (i < k.n) {
      float r[11], t[3];
      pool_ray_final(k.p, k.images, k.poses, k.ids, k.half, ndc, (uint32_t)(k.start + i), r, t);
      word = ((uint64_t)pool_key(k, r) << kPoolIdxBits) | (uint64_t)i;
    }
    w[i] = word;
  }
  __syncthreads();
  for (int len = 2; len <= k.padded; len <<= 1) {
    for (int j = len >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (k.padded >> 1); t += kMortonThreads) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const uint64_t a = w[lo], b = w[hi];
        if ((a > b) == ((lo & len) == 0)) {
          w[lo] = b;
          w[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int j = tid; j < k.n; j += kMortonThreads) {
    const uint64_t word = w[j];
    const uint32_t i = (uint32_t)word & (uint32_t)(HN_POOL_ORDER_MAX - 1);
    float r[11], t[3];
    pool_ray_final(k.p, k.images, k.poses, k.ids, k.half, ndc, (uint32_t)(k.start + i), r, t);
    pool_ray_store(r, t, (size_t)j, k.rays, k.target);
    if (k.keys) k.keys[j] = (uint32_t)(word >> kPoolIdxBits);
  }
}

// ---------------------------------------------------------------------------
// Host side: a draw's geometry and checks, shared by hn_sample_batch_morton
// and hn_render_bwd's next-batch job (which validates before it queues
// anything).
// ---------------------------------------------------------------------------
// Morton-window geometry: 4^k indices cover the window, kMortonThreads per tile.
inline bool morton_geometry(const hn_ray_sampler* s, uint32_t& n_idx, unsigned& blocks) {
  if (s->crop_h <= 0 || s->crop_w <= 0 || s->crop_h > HN_SAMPLER_MORTON_MAX || s->crop_w > HN_SAMPLER_MORTON_MAX)
    return false;
  int k = 0;
  while ((1 << k) < s->crop_h || (1 << k) < s->crop_w) ++k;
  n_idx = 1u << (2 * k);
  blocks = (unsigned)((n_idx + kMortonThreads - 1) / kMortonThreads);
  return true;
}

// A draw's NDC step: none without an hn_ray_ndc; scalars that are not finite
// or are zero (no focal length gives them) are refused.
inline int32_t make_ndc(const hn_ray_ndc* n, NdcK& k) {
  k = NdcK{0, 0.f, 0.f};
  if (!n) return HN_OK;
  if (!std::isfinite(n->sx) || !std::isfinite(n->sy) || n->sx == 0.f || n->sy == 0.f) return HN_E_SHAPE;
  k = NdcK{1, n->sx, n->sy};
  return HN_OK;
}

inline int32_t make_uni(uint64_t seed, const hn_uniform_draw* draws, int32_t n_draws, UniK& u) {
  if (n_draws < 0 || n_draws > HN_UNIFORM_MAX_DRAWS) return HN_E_SHAPE;
  if (n_draws && !draws) return HN_E_NULL;
  u.key[0] = (uint32_t)seed;
  u.key[1] = (uint32_t)(seed >> 32);
  u.n = n_draws;
  u.start[0] = 0;
  for (int j = 0; j < n_draws; ++j) {
    const hn_uniform_draw& d = draws[j];
    if (d.numel < 0 || (d.numel && d.threads <= 0) || (d.offset & 3)) return HN_E_SHAPE;
    if (d.numel && !d.out) return HN_E_NULL;
    u.d[j] = d;
    u.start[j + 1] = u.start[j] + d.numel;
  }
  return HN_OK;
}
// tiles of kMortonThreads elements over the draws
inline unsigned uni_blocks(const UniK& u) {
  return (unsigned)((u.start[u.n] + kMortonThreads - 1) / kMortonThreads);
}

// sample_morton's checks, in its order; HN_OK with k.n == 0 for an empty draw
// (nothing to launch), else k filled in.
inline int32_t make_morton(const hn_ray_sampler* s, const float* image, const float* c2w, int64_t n_rays,
                           float* rays, float* target, void* workspace, size_t ws_bytes, MortonK& k) {
  k.n = 0;
  k.blocks = 0;
  if (!s) return HN_E_NULL;
  if (n_rays < 0) return HN_E_SHAPE;
  if (n_rays == 0) return HN_OK;
  if (!image || !c2w || !rays || !target) return HN_E_NULL;
  if (s->H <= 0 || s->W <= 0 || s->crop_h <= 0 || s->crop_w <= 0 || s->crop_y0 < 0 || s->crop_x0 < 0 ||
      s->crop_y0 + s->crop_h > s->H || s->crop_x0 + s->crop_w > s->W)
    return HN_E_SHAPE;
  uint32_t n_idx;
  unsigned blocks;
  if (!morton_geometry(s, n_idx, blocks)) return HN_E_SHAPE;
  const uint64_t M = (uint64_t)s->crop_h * (uint64_t)s->crop_w;
  if ((uint64_t)n_rays > M) return HN_E_SHAPE;   // without replacement
  if (!workspace) return HN_E_NULL;
  if (ws_bytes < (size_t)blocks * sizeof(int)) return HN_E_WORKSPACE;
  int bits = 2;
  while ((1ull << bits) < M) bits += 2;
  k.s = *s;
  k.image = image;
  k.c2w = c2w;
  k.half = bits / 2;
  k.n = n_rays;
  k.n_idx = n_idx;
  k.blocks = blocks;
  k.counts = static_cast<int*>(workspace);
  k.rays = rays;
  k.target = target;
  return HN_OK;
}

}  // namespace hn
