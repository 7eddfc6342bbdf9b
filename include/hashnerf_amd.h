/*
 * hashnerf_amd.h -- C ABI of the MI355X (gfx950) HashNeRF hot path.
 *
 * Plain pointers + sizes, no torch types.  Every pointer is a DEVICE pointer
 * (HBM, fp32, contiguous, row-major) unless documented otherwise; config
 * structs are HOST pointers read at call time.  `stream` is a hipStream_t
 * passed as void*.  The library never allocates or frees, and synchronises
 * only in hn_device_faults: scratch comes in through `workspace`; outputs are
 * caller-allocated.
 * Gradient outputs named d* are ACCUMULATED (+=) so the caller zeroes them,
 * mirroring autograd's .grad accumulation.  Return value: 0 on success,
 * a positive HN_E_* code for argument errors, or a hipError_t + 1000.
 *
 * Each entry point cites the reference interface it replaces
 * (mache102/HashNeRF-pytorch, file:line).
 */
#ifndef HASHNERF_AMD_H
#define HASHNERF_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 14 also covers three additive fields appended at the end of their structs,
 * where zero / NULL keeps the earlier behaviour: hn_render_fwd_args.loss,
 * hn_render_bwd_args.prepass_done and .next_batch (a caller built against the shorter structs
 * must zero-fill the args, as every caller of this ABI does), the samplers'
 * NDC step (hn_ray_ndc with hn_sample_rays_ndc, hn_sample_rays_morton_ndc,
 * hn_sample_batch_morton_ndc, hn_sample_pool_ndc, hn_sample_pool_ordered_ndc
 * and, for the next-batch job, hn_render_bwd_ndc), and the additive
 * entry points hn_sample_pool_ordered, hn_render_image (with its
 * hn_render_image_workspace_bytes and hn_render_image_variant),
 * hn_render_views (with hn_render_views_workspace_bytes),
 * hn_render_fwd_form, hn_render_fwd_pick, hn_render_fwd_deal and
 * hn_render_fwd_res_map, and the input gradients
 * hn_encode_bwd_input, hn_sh_bwd and hn_composite_bwd_inputs. */
#define HN_ABI_VERSION 14
#define HN_MAX_LEVELS 32

enum {
  HN_OK = 0,
  HN_E_NULL = 1,        /* required pointer is NULL */
  HN_E_SHAPE = 2,       /* unsupported size (e.g. n_levels, n_samples) */
  HN_E_WORKSPACE = 3,   /* workspace too small */
  HN_E_HIP = 1000       /* + hipError_t */
};

/* Hash-grid description (embedding/hash_encoding.py:14-57).  grid_size is
 * (box_max - box_min) / resolution_l evaluated on the host in fp32 exactly as
 * hash_encoding.py:72/:101 do, so the device sees bit-identical cell sizes.
 * Table layout in HBM: [n_levels][2^log2_hashmap_size][n_features] fp32
 * (the stacked `embeddings.{l}.weight` tensors). */
typedef struct hn_grid {
  int32_t n_levels;            /* L <= HN_MAX_LEVELS (16) */
  int32_t n_features;          /* F, must be 2 */
  int32_t log2_hashmap_size;   /* T, 1..24 */
  int32_t reserved;
  float box_min[3];
  float box_max[3];
  float grid_size[HN_MAX_LEVELS][3];
} hn_grid;

/* NeRFSmall weights (models.py:96-149; num_layers=2, hidden 64, geo 15,
 * num_layers_color=3): torch nn.Linear layout [out][in], no biases. */
typedef struct hn_mlp {
  const float* sigma0;   /* sigma_net.0.weight [64][32] */
  const float* sigma1;   /* sigma_net.1.weight [16][64] */
  const float* color0;   /* color_net.0.weight [64][31]  (in = [sh16 | geo15]) */
  const float* color1;   /* color_net.1.weight [64][64] */
  const float* color2;   /* color_net.2.weight [3][64] */
} hn_mlp;

typedef struct hn_mlp_grad {
  float* sigma0; float* sigma1; float* color0; float* color1; float* color2;  /* += */
} hn_mlp_grad;

#define HN_MLP_PARAMS 9344          /* 2048 + 1024 + 1984 + 4096 + 192 */
#define HN_MLP_PACKED_FLOATS 30208  /* MFMA fragment-ordered copy (split-f32 bf16 parts), per net */

int32_t hn_abi_version(void);
const char* hn_status_string(int32_t status);
/* Sticky device fault word.  The persistent render backward synchronises its
 * waves through bounded LDS waits; a wait that runs out (a protocol failure,
 * never expected) sets a bit here instead of hanging the GPU: 1 ring slot,
 * 2 ring drain (tiles left unscattered), 4 coarse-grad flag, 8 dW buffer,
 * 16 binned-scatter overflow records exhausted (gradient records lost),
 * 32 a NaN / Inf feature gradient or sample point reached the binned scatter
 * (its exact fixed-point sums cannot carry it; the reference's autograd would
 * propagate it into the table gradient), 64 a gradient on a row pair table_live
 * marks dead (hn_render_bwd_args).
 * Nonzero means the gradients of the launches since the last clear are
 * invalid.  This is the one entry point that synchronises (a blocking copy
 * from the device); call it at points where the host syncs anyway.
 * *faults = the word; clear != 0 resets it. */
int32_t hn_device_faults(int32_t* faults, int32_t clear);

/* ---- L1 encodings --------------------------------------------------------
 * HashEmbedder.forward (hash_encoding.py:84-110): x[n][3] -> feat[n][L*F],
 * keep_mask[n] (uint8, may be NULL).  Corners from the clamped point, trilinear
 * weights from the unclamped point, every level hashed (SURVEY 8a traps 1-3). */
int32_t hn_encode_fwd(const hn_grid* g, const float* x, int64_t n, const float* table,
                      float* feat, uint8_t* keep_mask, void* stream);
/* Autograd of the above (embedding_dense_backward x L): dtable += scatter. */
int32_t hn_encode_bwd(const hn_grid* g, const float* x, int64_t n, const float* dfeat,
                      float* dtable, void* stream);
/* SHEncoder.forward, degree 4 (embedding/spherical_harmonic.py:65-103):
 * dirs[n][3] -> out[n][16]. */
int32_t hn_sh_fwd(const float* dirs, int64_t n, float* out, void* stream);
/* Gradients with respect to the inputs of the two encodings (additive under
 * ABI 14): what autograd gives the reference for x.requires_grad_().
 * hn_encode_bwd_input: autograd of trilinear_interp (hash_encoding.py:130-163)
 * through w = (x - vmin) / (vmax - vmin) (:143): dx[n][3] (overwritten) =
 * sum over levels and their two features of dfeat * d f / d w_a / (vmax_a -
 * vmin_a).  The weights come from the unclamped point and the cell from the
 * clamped one, as in hn_encode_fwd; nothing flows through floor or the clamp
 * (:69, :74), so a point outside the box gets the same formula.  No atomics:
 * dx is bitwise repeatable. */
int32_t hn_encode_bwd_input(const hn_grid* g, const float* x, int64_t n, const float* table,
                            const float* dfeat, float* dx, void* stream);
/* hn_sh_bwd: the derivatives of the 16 polynomials of SHEncoder.forward
 * (spherical_harmonic.py:65-103): dirs[n][3], dout[n][16] -> ddirs[n][3]
 * (overwritten). */
int32_t hn_sh_bwd(const float* dirs, const float* dout, int64_t n, float* ddirs, void* stream);

/* ---- L2 NeRFSmall (MFMA) ------------------------------------------------
 * NeRFSmall.forward (models.py:151-174): x[n][48] = [feat32 | sh16] ->
 * out[n][4] = [rgb3 | sigma].  workspace >= hn_mlp_workspace_bytes(). */
size_t hn_mlp_workspace_bytes(void);
int32_t hn_mlp_fwd(const hn_mlp* w, const float* x, int64_t n, float* out,
                   void* workspace, size_t ws_bytes, void* stream);
/* Backward: dx[n][48] (overwritten; may be NULL), dw (+=). */
int32_t hn_mlp_bwd(const hn_mlp* w, const float* x, const float* dout, int64_t n,
                   float* dx, const hn_mlp_grad* dw, void* workspace, size_t ws_bytes,
                   void* stream);

/* ---- L3 volume rendering --------------------------------------------------
 * raw2outputs (run_nerf_helpers.py:577-628), n_samples <= 256 per ray:
 * raw[n_rays][S][4], z[n_rays][S], rays_d[n_rays][3], noise[n_rays][S] or NULL
 * -> rgb[n_rays][3], disp, acc, depth, entropy [n_rays], weights[n_rays][S]. */
int32_t hn_composite_fwd(const float* raw, const float* z, const float* rays_d,
                         const float* noise, int64_t n_rays, int32_t n_samples,
                         int32_t white_bkgd, float* rgb, float* disp, float* acc,
                         float* weights, float* depth, float* entropy, void* stream);
/* Backward w.r.t. raw (overwritten): upstream grads of rgb[n][3], acc[n],
 * depth[n], entropy[n], weights[n][S] (any may be NULL = 0). */
int32_t hn_composite_bwd(const float* raw, const float* z, const float* rays_d,
                         const float* noise, int64_t n_rays, int32_t n_samples,
                         int32_t white_bkgd, const float* g_rgb, const float* g_acc,
                         const float* g_depth, const float* g_entropy,
                         const float* g_weights, float* d_raw, void* stream);
/* Backward w.r.t. z and rays_d (additive under ABI 14; both overwritten,
 * either may be NULL), from the same inputs and upstream gradients: z through
 * dists = z[i+1] - z[i] (:590-592) and depth = sum(w z) / sum(w) (:617),
 * rays_d through dists * ||rays_d|| (:593) -- every other output depends on
 * them through alpha = 1 - exp(-relu(sigma) * dists) (:596, :607) alone.
 * d_z[n_rays][S], d_rays_d[n_rays][3]. */
int32_t hn_composite_bwd_inputs(const float* raw, const float* z, const float* rays_d,
                                const float* noise, int64_t n_rays, int32_t n_samples,
                                int32_t white_bkgd, const float* g_rgb, const float* g_acc,
                                const float* g_depth, const float* g_entropy,
                                const float* g_weights, float* d_z, float* d_rays_d,
                                void* stream);
/* sample_pdf (run_nerf_helpers.py:264-307) with u given:
 * bins[n_rays][nb], weights[n_rays][nb-1], u[n_rays][ns] -> out[n_rays][ns];
 * nb <= 256. */
int32_t hn_sample_pdf(const float* bins, const float* weights, const float* u,
                      int64_t n_rays, int32_t n_bins, int32_t n_samples, float* out,
                      void* stream);

/* ---- fused render_rays (run_nerf_helpers.py:464-574) ---------------------
 * One kernel for the whole forward of a ray batch (coarse 64 -> composite ->
 * sample_pdf 128 -> sort -> fine 192 -> composite) and one for its backward.
 * Hash grid must have L=16, F=2; N_samples=64; N_importance=128, or 64 (the
 * LLFF configurations: sample_pdf 64 -> sort -> fine 128).  Below, Ni =
 * n_importance and Sf = 64 + Ni: the caller's per-ray tensors are sized by the
 * cfg (u [B][Ni]; noise_f, z_fine, fine_src [B][Sf]; raw_f, g_raw_f
 * [B][Sf][4]; the sizes written at the fields are those of Ni = 128), `feat`
 * keeps HN_RENDER_FEAT_PER_RAY per ray (opaque; the tail a 4-tile fine pass
 * does not use is not written), and hn_render_workspace_bytes(Ni = 64) <=
 * that of Ni = 128.  Ni = 64 trains on the binned backward only: where
 * hn_render_scatter_mode is not 2 (scatter = 1, T > 22, the box-geometry
 * fallback), hn_render_fwd with feat != NULL and hn_render_bwd return
 * HN_E_SHAPE before any launch; the inference forward (feat == NULL) runs for
 * every T.  The whole-image kernel renders both counts through hn_render_views;
 * its earlier entry points stay 64 + 128 only: hn_render_image(_variant) return
 * HN_E_SHAPE and hn_render_image_workspace_bytes 0 for Ni = 64. */
typedef struct hn_render_cfg {
  hn_grid grid;
  int32_t n_samples;      /* 64 */
  int32_t n_importance;   /* 128 or 64 */
  int32_t white_bkgd;
  int32_t lindisp;
  int32_t perturb;        /* 1: stratified jitter from t_rand */
  int32_t scatter;        /* backward table-gradient scatter: 0 auto (= binned where the
                             table allows it), 1 float atomics, 2 binned (records +
                             exact per-bin owner pass; T <= 22).  The library reads no
                             environment variables (ABI 14). */
  int32_t bin_cap;        /* binned scatter: records per (producer block, bin) region, a
                             multiple of 64; 0 = sized from the batch.  Small values
                             exercise the shared overflow records (tests). */
  int32_t dense_bwd;      /* ABI 14 (in ABI 12-13's merge_levels slot, whose merged coarse-level
                             records were removed): 0 = the backward skips the samples whose
                             d raw is exactly zero (relu(sigma) = 0: alpha = 0, weight 0), whose
                             feature and weight gradients are exactly zero -- the same results
                             up to the sign of zero; 1 = every sample computed (A/B, tests) */
} hn_render_cfg;

#define HN_RENDER_FEAT_PER_RAY 9728   /* (64 + 192) points x 16 levels x 2 features, then the
                                         MLPs' ReLU masks of those points (ABI 10) */

/* ABI 13: the training loss fused into hn_render_bwd (the trainer's step;
 * replaces its hn_loss_fwd_bwd launch).  The loss is run_nerf.py:612-636
 * under train.dp_loss's data-parallel rule:
 *   loss = (mse(rgb) + mse(rgb0)) / world + sparse_w * sum(entropy + entropy0)
 *          + tv_w * sum(tv)
 * With hn_render_bwd_args.loss set, the backward's composite pre-pass forms
 * the upstream gradients itself from the forward's outputs (hn_loss_bwd's op
 * forms with g_loss = 1; the g_* arguments are not read) and one of its
 * workgroups reduces the loss value into out[4] = loss, mse, mse0, sum of
 * entropies (hn_loss_fwd's fp64 sums, another thread count).  The TV term's
 * gradient still comes in as tv / g_tv (= tv_w per level). */
typedef struct hn_render_loss {
  const float* target;      /* [B][3] */
  const float* rgb; const float* rgb0;            /* the forward's [B][3] outputs */
  const float* sparsity; const float* sparsity0;  /* the forward's [B] entropies */
  const float* tv;          /* [n_tv] per-level TV values (hn_tv_fwd), or NULL */
  int32_t n_tv;
  float world, sparse_w, tv_w;
  float* out;               /* [4] */
} hn_render_loss;

typedef struct hn_render_fwd_args {
  int64_t n_rays;
  const float* rays;        /* [B][11] = [o3 d3 near far viewdir3] (run_nerf_helpers.py:509-512) */
  const float* t_vals;      /* [64]   torch.linspace(0,1,64) (:514) */
  const float* t_rand;      /* [B][64] jitter (:528) or NULL if !perturb */
  const float* u;           /* [B][128] importance uniforms (:276) */
  const float* noise_c;     /* [B][64] or NULL (raw_noise_std = 0) */
  const float* noise_f;     /* [B][192] or NULL */
  const float* table;       /* [16][2^T][2] */
  hn_mlp coarse;            /* network_fn */
  hn_mlp fine;              /* network_fine */
  /* outputs (render_rays ret, :560-568) */
  float* rgb; float* depth; float* acc; float* sparsity;        /* fine: [B][3],[B],[B],[B] */
  float* rgb0; float* depth0; float* acc0; float* sparsity0;    /* coarse */
  float* z_std;             /* [B] */
  /* saved for backward (also returned: raw = raw_f) */
  float* z_coarse;          /* [B][64] */
  float* z_fine;            /* [B][192] */
  float* raw_c;             /* [B][64][4] */
  float* raw_f;             /* [B][192][4] */
  uint8_t* fine_src;        /* [B][192]: coarse index of each fine sample, 255 = importance */
  float* feat;              /* [B][HN_RENDER_FEAT_PER_RAY] hash features of the 64 + 192
                               evaluated points and their ReLU masks (MFMA-tile order,
                               opaque); NULL = not kept (inference); required by hn_render_bwd */
  int32_t weights_packed;   /* ABI 13: nonzero = `workspace` already holds both nets' packed MFMA
                               copies of these weights (an hn_render_bwd with repack wrote them and the
                               weights are unchanged since): no packing launch */
  int32_t skip_dead_color;  /* ABI 14: nonzero (and no noise for that pass) = a tile of 32 samples
                               whose raw sigmas are all <= 0 -- alpha 0 and weight 0 at every sample,
                               so its colours enter no output and no gradient -- skips the colour
                               net: raw_c / raw_f rgb of those samples are written as 0 (rgb, depth,
                               acc, the entropies and every gradient unchanged), and such fine
                               tiles' features and ReLU masks are not stored in `feat` (no d raw of
                               theirs is nonzero, so the binned dense_bwd = 0 backward, which runs
                               lists of the nonzero groups, never reads them).  Only that backward
                               may follow: hn_render_scatter_mode == 2 and dense_bwd = 0.  The
                               float-atomic schedule and a dense_bwd = 1 backward load every tile,
                               so either one of this state is invalid.  0 = every sample's raw
                               rgb computed (the reference's `raw` output), every tile stored */
  const hn_render_loss* loss;   /* additive under ABI 14 (NULL = the forward as before): the training loss
                               whose gradient the following hn_render_bwd takes (of this struct only target,
                               world and sparse_w are read here).  Each ray's forward wave then also runs
                               the composite backward of its two passes and leaves d raw and the work
                               marks in `workspace`, with a stamp for n_rays; the one hn_render_bwd that
                               follows on this workspace sets prepass_done and launches no pre-pass --
                               bitwise the same gradients.  Binned scatter only (hn_render_scatter_mode
                               == 2, else HN_E_SHAPE).  Every output of the forward is unchanged */
} hn_render_fwd_args;

typedef struct hn_render_bwd_args {
  int64_t n_rays;
  const float* rays;
  const float* noise_c; const float* noise_f;
  const float* table;
  hn_mlp coarse; hn_mlp fine;
  const float* z_coarse; const float* z_fine; const float* raw_c; const float* raw_f;
  const uint8_t* fine_src;  /* from the forward */
  const float* feat;        /* from the forward (saved hash features) */
  int32_t weights_packed;   /* nonzero: `workspace` is the one hn_render_fwd used and the weights
                               are unchanged since, so its packed MFMA copies are reused */
  int32_t d_table_mode;     /* bit 0 clear: d_table += gradient (as every d* output); set: d_table =
                               gradient (every entry written, the caller need not zero it).
                               bit 1 set: d_coarse / d_fine = their gradients likewise (ABI 8) */
  /* upstream grads (NULL = 0) */
  const float* g_rgb; const float* g_depth; const float* g_acc; const float* g_sparsity;
  const float* g_rgb0; const float* g_depth0; const float* g_acc0; const float* g_sparsity0;
  const float* g_raw_f;     /* [B][192][4] or NULL */
  /* gradient outputs (+=) */
  float* d_table;           /* [16][2^T][2]; may be NULL when table_step is given */
  hn_mlp_grad d_coarse; hn_mlp_grad d_fine;
  /* Optional fused optimizer step (binned scatter only, else HN_E_SHAPE): the
   * owner pass applies this RAdam step (hn_radam_step's per-element update,
   * g = the table gradient of this backward) to the table right where it forms
   * the gradient; p / m / v are the table and its moments, g is ignored.
   * NULL = no step (the gradient goes to d_table). */
  const struct hn_radam_tensor* table_step;
  /* Optional total-variation term (loss.py:11-43; run_nerf.py:626-635) in the same
   * backward (ABI 9): tv = the TV args of the hn_tv_fwd call (host), g_tv = device
   * [L] upstream gradients of its per-level values.  With the binned scatter and
   * cubes <= 50 its gradient goes into the bins as records (so table_step stays
   * fused); otherwise it is added to d_table (hn_tv_bwd; table_step not allowed).
   * NULL = no TV term.
   * ABI 14: n_rays == 0 with a TV term (a data-parallel rank that drew no rays,
   * run_nerf.py:551-555, still carries the TV term) runs the TV term alone through
   * the same records and exact owner pass -- bitwise reproducible, unlike
   * hn_tv_bwd's float atomics; only cfg, tv, g_tv, d_table (or table_step),
   * d_table_mode and the workspace (hn_render_workspace_bytes(cfg, 0)) are read,
   * the MLP gradients are not touched, owner_defer must be 0.  The binned scatter
   * is required (else HN_E_SHAPE: use hn_tv_bwd).  n_rays == 0 without a TV term
   * does nothing. */
  const struct hn_tv_args* tv;
  const float* g_tv;
  /* Optional with table_step (ABI 11): the live row pairs of the table's leading
   * table_live_levels levels, a device bitmap over the flat [level][row] index:
   * bit (R >> 1) & 31 of word R >> 6 covers rows R and R + 1.  A clear bit
   * promises that neither row can ever receive a gradient (render or TV: level l's
   * corners lie in [0, res_l + 1]^3 once the point is clamped to the box,
   * hash_encoding.py:66-76, so the other rows of a level with (res_l + 2)^3 < 2^T
   * are structural zeros) and that their moments are zero; the fused step then
   * neither loads nor stores p / m / v there -- the dense update would leave them
   * bitwise unchanged.  A nonzero gradient on a clear pair sets fault bit 64.
   * NULL = every row stepped. */
  const uint32_t* table_live;
  int32_t table_live_levels;
  /* ABI 12, binned scatter only: nonzero = stop before the owner pass; the
   * caller then runs it per range of bins with hn_render_bwd_owner (e.g. to
   * start each range's gradient exchange while the next range is reduced).
   * The workspace must not be touched in between. */
  int32_t owner_defer;
  const hn_render_loss* loss;   /* ABI 13: NULL, or the training loss formed here (above) */
  const struct hn_radam_tensor* mlp_step;   /* ABI 13 (binned scatter only, else HN_E_SHAPE): NULL, or [10] the
                               NeRFSmall tensors' RAdam steps (network_fn's sigma_net.0, sigma_net.1,
                               color_net.0, color_net.1, color_net.2, then network_fine's; g unused),
                               applied where each weight's final gradient is formed (hn_radam_step's
                               per-element update; the gradient is still written to d_coarse / d_fine) */
  int32_t repack;           /* ABI 13, with mlp_step: then write the stepped weights' packed MFMA copies
                               into `workspace` (in the overflow-placement launch), so the next
                               hn_render_fwd on this workspace may set weights_packed */
  int32_t prepass_done;     /* additive under ABI 14 (0 = as before): the hn_render_fwd of these rays on this
                               workspace ran with the same `loss` (target, world, sparse_w), so d raw and
                               the marks are in the workspace and the composite pre-pass is not launched.
                               Needs the binned scatter, `loss` (its value is still reduced here) and no
                               g_rgb / g_rgb0 / g_raw_f (else HN_E_SHAPE).  The first kernel checks the
                               forward's stamp on the device: absent, for another n_rays, or already used
                               by a backward, it sets fault bit 128 (hn_device_faults) and the launch
                               computes no ray's gradient */
  const struct hn_next_batch* next_batch;   /* additive under ABI 14 (NULL = as before): the next step's batch
                               (hn_next_batch below: hn_sample_batch_morton's arguments) drawn inside this
                               backward's two small launches.  Binned scatter with its owner pass here only:
                               HN_E_SHAPE with the float-atomic schedule, with n_rays == 0 and with owner_defer.
                               Checked as hn_sample_batch_morton checks it, with its return codes, before
                               anything is queued */
} hn_render_bwd_args;

/* The binned scatter's bins for this cfg and batch: returns their number (0:
 * the float-atomic schedule, no bins) and sets *shift: bin b holds the table
 * entries (flat level-major rows) [b << shift, (b + 1) << shift). */
int32_t hn_render_bins(const hn_render_cfg* cfg, int64_t n_rays, int32_t* shift);
/* The owner pass of hn_render_bwd (owner_defer set) over bins [bin_lo,
 * bin_hi): writes (or steps, with table_step) exactly those bins' slices of
 * the table gradient.  Same cfg / args / workspace as the deferred call. */
int32_t hn_render_bwd_owner(const hn_render_cfg* cfg, const hn_render_bwd_args* a, void* workspace,
                            size_t ws_bytes, int32_t bin_lo, int32_t bin_hi, void* stream);

/* ---- L4 hash-table total variation (loss.py:11-43), all levels at once ---
 * Level l samples the cube of (cube[l]+1)^3 grid vertices starting at
 * min_vertex[l] (device int32 [L][3], the reference's torch.randint draw),
 * hashes them like hash_encoding.py:112-128 and sums squared differences of
 * the entries along x, y and z, divided by cube[l]. */
typedef struct hn_tv_args {
  int32_t n_levels;
  int32_t log2_hashmap_size;
  int32_t cube[HN_MAX_LEVELS];
  const int32_t* min_vertex;   /* device [L][3] */
  const float* table;          /* device [L][2^T][2] */
} hn_tv_args;
/* tv[L] (device) is overwritten with the per-level TV values. */
int32_t hn_tv_fwd(const hn_tv_args* a, float* tv, void* stream);
/* dtable += sum_l g_tv[l] * d tv_l / d table  (g_tv: device [L]). */
int32_t hn_tv_bwd(const hn_tv_args* a, const float* g_tv, float* dtable, void* stream);

/* ---- L4 RAdam step (radam.py:28-94) over many tensors in one launch -----
 * Per element, in the op forms of torch's CPU kernels (bit-exact on the
 * reference's trace):
 *   v = fma((1-beta2)*g, g, v*beta2) ; m = fma(1-beta1, g, m*beta1)
 *   mode 2 (N_sma >= 5): p = fma(neg_wd_lr, p, p) (if wd); p += (neg_step_lr*m)/(sqrt(v)+eps)
 *   mode 1 (step_size > 0, N_sma < 5): p = fma(neg_wd_lr, p, p) (if wd); p = fma(neg_step_lr, m, p)
 *   mode 0: moments only (the reference's first steps at beta2=0.99).
 * Scalars are the fp32 values torch would use (host computes N_sma/step_size). */
#define HN_RADAM_MAX_TENSORS 16
typedef struct hn_radam_tensor {
  float* p; const float* g; float* m; float* v; int64_t n;
  float beta1, beta2, one_minus_beta1, one_minus_beta2, eps, neg_wd_lr, neg_step_lr;
  int32_t mode;
  int32_t has_wd;
  int32_t reserved;
} hn_radam_tensor;
int32_t hn_radam_step(const hn_radam_tensor* ts, int32_t n_tensors, void* stream);

/* ---- L5 training-step driver (run_nerf.py:576-636) -----------------------
 * Device ray sampler: n_rays DISTINCT pixels of one training image drawn
 * without replacement (np.random.choice(..., replace=False) at
 * run_nerf.py:595; here a seeded Feistel permutation of the crop window with
 * cycle walking), the rays of ray_util.py:62-80 for them, and their target
 * colours.  rays[n][11] = [o3 d3 near far viewdir3] (the ray batch render()
 * builds, run_nerf_helpers.py:355-368); target[n][3]. */
typedef struct hn_ray_sampler {
  int32_t H, W;                        /* image size */
  int32_t crop_y0, crop_x0, crop_h, crop_w;   /* sampling window (precrop, :584-593) */
  float fx, fy, cx, cy;                /* intrinsics K */
  float near, far;
  uint64_t seed;                       /* per step and rank */
} hn_ray_sampler;
int32_t hn_sample_rays(const hn_ray_sampler* s, const float* image, const float* c2w, int64_t n_rays,
                       float* rays, float* target, void* stream);
/* The same draw (same set for the same seed) listed in Morton order of its
 * pixels (window-relative row, column), so consecutive rays are spatial
 * neighbours: hn_render_fwd gives consecutive ray groups to one XCD and they
 * share its L2.  Pixel x is drawn iff perm^-1(x) < n_rays, so the Morton walk
 * of the window compacts the draw in order, without a sort.  Window sides up
 * to HN_SAMPLER_MORTON_MAX; workspace = hn_sample_rays_morton_workspace_bytes. */
#define HN_SAMPLER_MORTON_MAX 4096
size_t hn_sample_rays_morton_workspace_bytes(const hn_ray_sampler* s);
int32_t hn_sample_rays_morton(const hn_ray_sampler* s, const float* image, const float* c2w, int64_t n_rays,
                              float* rays, float* target, void* workspace, size_t ws_bytes, void* stream);

/* ABI 13: torch.rand on the device's default generator, restated bit for bit
 * (render_rays' draws, run_nerf_helpers.py:528 t_rand and :276 via :548 u):
 * ATen's uniform_ kernel runs `threads` = blockDim x gridDim threads of
 * hiprand Philox4x32-10 (key = seed, subsequence = thread, counter = offset / 4
 * + call), four values per call, element li from thread li % threads, call
 * li / (4 threads), component (li / threads) % 4; value 2^-32 + v 2^-32, with
 * 1 mapped to 0.  The caller supplies the generator's seed and each draw's
 * offset and threads as torch would use them (and advances the generator). */
typedef struct hn_uniform_draw {
  float* out;               /* [numel] */
  int64_t numel;
  int64_t threads;          /* torch's launch for this numel: 256 x min(ceil(numel / 256), CUs x 2048 / 256) */
  uint64_t offset;          /* the generator's philox offset at this draw (a multiple of 4) */
} hn_uniform_draw;
#define HN_UNIFORM_MAX_DRAWS 4
int32_t hn_uniform_philox(uint64_t seed, const hn_uniform_draw* draws, int32_t n_draws, void* stream);
/* hn_sample_rays_morton with the step's uniform draws made in its first
 * launch (one launch less than the sampler + torch.rand's own launches). */
int32_t hn_sample_batch_morton(const hn_ray_sampler* s, const float* image, const float* c2w, int64_t n_rays,
                               float* rays, float* target, void* workspace, size_t ws_bytes, uint64_t seed,
                               const hn_uniform_draw* draws, int32_t n_draws, void* stream);

/* The samplers' NDC step (additive under ABI 14; the LLFF configurations,
 * run_nerf.py:270 with render()'s ndc=True): every sampler -- per image, the
 * next-batch job, the pool -- can hand out render()'s final ray in the launch
 * that forms the world ray.  The world ray is formed as without; then
 * get_ndc_rays(H, W, K[0][0], 1., o, d) (ray_util.py:96-142, the near plane
 * render() passes, run_nerf_helpers.py:349) rewrites rays[i][0:6], float32
 * operation for float32 operation as torch evaluates it, so those six floats
 * are torch's bit for bit.  rays[i][6:8] stay the caller's near / far,
 * rays[i][8:11] the normalised WORLD direction (render() takes viewdirs
 * before its NDC step, :350) and the target the pixel.
 *   sx = -1. / (W / (2. * focal)),  sy = -1. / (H / (2. * focal)),  focal = K[0][0]
 * formed in float64 by the caller and passed as float32 (hn_view_args.ndc_sx /
 * ndc_sy are the same two).  A scalar that is not finite or is zero:
 * HN_E_SHAPE, checked behind the call's other checks and before any launch.
 * A ray with d_z = 0 (parallel to the near plane) gets whatever non-finite
 * values those float operations give; no sampler looks for one (a non-finite
 * sample point raises fault bit 32 in the binned render backward).
 * ndc == NULL in any call below is the call without the suffix, bitwise; the
 * entry points without the suffix pass NULL. */
typedef struct hn_ray_ndc {
  float sx, sy;
} hn_ray_ndc;
int32_t hn_sample_rays_ndc(const hn_ray_sampler* s, const float* image, const float* c2w, int64_t n_rays,
                           float* rays, float* target, const hn_ray_ndc* ndc, void* stream);
int32_t hn_sample_rays_morton_ndc(const hn_ray_sampler* s, const float* image, const float* c2w, int64_t n_rays,
                                  float* rays, float* target, void* workspace, size_t ws_bytes,
                                  const hn_ray_ndc* ndc, void* stream);
int32_t hn_sample_batch_morton_ndc(const hn_ray_sampler* s, const float* image, const float* c2w, int64_t n_rays,
                                   float* rays, float* target, void* workspace, size_t ws_bytes, uint64_t seed,
                                   const hn_uniform_draw* draws, int32_t n_draws, const hn_ray_ndc* ndc,
                                   void* stream);

/* The same call as a job of hn_render_bwd (hn_render_bwd_args.next_batch): a
 * training loop's next batch depends on nothing its current step computes, so
 * the binned backward runs the sampler's two passes as extra workgroups of its
 * own two small launches, which a kernel boundary separates as the passes
 * need -- the tile counts and the uniform draws behind the work lists'
 * workgroups, the emit behind the overflow placement's -- instead of two
 * launches ahead of the next forward.  The fields are hn_sample_batch_morton's
 * arguments (sampler and draws: host pointers read at call time); every
 * output is bitwise that call's.  rays / target / the draws' outputs /
 * workspace must not be buffers the backward itself reads or writes. */
typedef struct hn_next_batch {
  const hn_ray_sampler* sampler;
  const float* image;
  const float* c2w;
  int64_t n_rays;
  float* rays;
  float* target;
  void* workspace;
  size_t ws_bytes;
  uint64_t seed;
  const hn_uniform_draw* draws;
  int32_t n_draws;
} hn_next_batch;
/* hn_render_bwd whose next-batch job hands out NDC rays (additive under ABI
 * 14): a->next_batch drawn as hn_sample_batch_morton_ndc(..., next_ndc, .)
 * draws it, bitwise, next_ndc checked as that call checks it, with its code,
 * before anything is queued.  hn_next_batch keeps its layout; next_ndc == NULL
 * is hn_render_bwd, which passes NULL.  next_ndc without a->next_batch:
 * HN_E_SHAPE.  The backward's own results do not depend on the job. */
int32_t hn_render_bwd_ndc(const hn_render_cfg* cfg, const hn_render_bwd_args* a, void* workspace, size_t ws_bytes,
                          const hn_ray_ndc* next_ndc, void* stream);

/* use_batching ray pool (run_nerf.py:505-521 builds rays_rgb from every training
 * pixel and shuffles it; :544-555 takes consecutive N_rand slices and reshuffles
 * after each epoch).  The pool is never materialised: position q of an epoch
 * maps to pool pixel perm(q) (a keyed, cycle-walked Feistel bijection of
 * [0, n_images * H * W), the epoch's shuffle; pool order is (image, row,
 * column) as rays_rgb's reshape), whose ray is get_rays_np's (ray_util.py:82-93:
 * float64 arithmetic, rounded to float32 as rays_rgb.astype(np.float32)) and
 * whose target is the image pixel.  Batch k of an epoch = positions
 * [k N_rand, min((k + 1) N_rand, pool size)): the caller passes start = k N_rand
 * and the batch length (the last batch of an epoch is short, as the
 * reference's slice).  rays[n][11] and target[n][3] as hn_sample_rays. */
typedef struct hn_ray_pool {
  int32_t n_images;       /* training images in the pool (image_ids[n_images]) */
  int32_t H, W;
  int32_t pose_stride;    /* floats between consecutive c2w matrices in `poses` (12 or 16) */
  double fx, fy, cx, cy;  /* intrinsics K, float64 as get_rays_np uses them */
  float near, far;
  uint64_t seed;          /* the epoch's shuffle key */
} hn_ray_pool;
/* images: device [n_all][H][W][3]; poses: device [n_all][.][4] (row-major
 * c2w, pose_stride floats apart); image_ids: device int32 [n_images] (i_train). */
int32_t hn_sample_pool(const hn_ray_pool* p, const float* images, const float* poses, const int32_t* image_ids,
                       int64_t start, int64_t n_rays, float* rays, float* target, void* stream);
/* The same batch -- pool positions [start, start + n_rays), every ray's 14
 * floats bitwise hn_sample_pool's -- listed in Morton order of the rays'
 * mid-depth points in the hash grid's box, so consecutive rays of the batch
 * are spatial neighbours as the per-image Morton sampler's are (a pool batch
 * comes from every training image, so pixel order cannot do it).  Position i
 * gets the 30-bit key of its float32 o = rays[i][0:3], d = rays[i][3:6] (every
 * operation a separately rounded float32 one):
 *   tm = 0.5f * (near + far);  pt_a = o[a] + d[a] * tm
 *   u_a = fminf(fmaxf((pt_a - box_min[a]) / (box_max[a] - box_min[a]), 0), 1)   (NaN -> 0)
 *   c_a = min((int)(u_a * 1024), 1023);  key bit 3k + a = bit k of c_a  (a = 0: x, k = 0..9)
 * and the rows are written in ascending (key, i): ties keep the shuffle's
 * order.  keys (device [n_rays], or NULL) receives each output row's key.
 * One launch, no workspace: one workgroup sorts the batch in LDS (so n_rays <=
 * HN_POOL_ORDER_MAX), further workgroups make the `draws` -- the values of
 * hn_uniform_philox(seed, draws, n_draws) bitwise.  box_min / box_max: host
 * float[3], read at call time.  n_rays == 0 is a no-op without a launch. */
#define HN_POOL_ORDER_MAX 8192
int32_t hn_sample_pool_ordered(const hn_ray_pool* p, const float* images, const float* poses,
                               const int32_t* image_ids, int64_t start, int64_t n_rays, const float* box_min,
                               const float* box_max, float* rays, float* target, uint32_t* keys, uint64_t seed,
                               const hn_uniform_draw* draws, int32_t n_draws, void* stream);
/* The two pool draws with the NDC step (hn_ray_ndc above; NULL = the calls
 * above, bitwise).  The ordered draw keys the FINAL ray: o and d in the key
 * formula above are the NDC ones, tm the mid-depth of the pool's near / far (0.5
 * for an LLFF pool), box the NDC box the hash grid has (bbox.py:44-75). */
int32_t hn_sample_pool_ndc(const hn_ray_pool* p, const float* images, const float* poses, const int32_t* image_ids,
                           int64_t start, int64_t n_rays, float* rays, float* target, const hn_ray_ndc* ndc,
                           void* stream);
int32_t hn_sample_pool_ordered_ndc(const hn_ray_pool* p, const float* images, const float* poses,
                                   const int32_t* image_ids, int64_t start, int64_t n_rays, const float* box_min,
                                   const float* box_max, float* rays, float* target, uint32_t* keys, uint64_t seed,
                                   const hn_uniform_draw* draws, int32_t n_draws, const hn_ray_ndc* ndc,
                                   void* stream);

/* Blender image preparation (load/load_blender.py:63, :78-86; run_nerf.py:259-262):
 * rgba: device uint8 [n][H][W][4] (the PNGs) -> out, float32:
 *   x = float32(u8 / 255.0)  (float64 division, as np.array(imgs) / 255.);
 *   half_res: 2 x 2 box mean (cv2.resize INTER_AREA to H/2 x W/2; H, W even);
 *   mode 0: RGBA [n][H'][W'][4] (what load_blender_data returns);
 *   mode 1: white background, rgb * a + (1 - a) -> [n][H'][W'][3] (float32
 *           arithmetic at full resolution, float64 after half_res as the
 *           reference's float64 half-res array, rounded to float32);
 *   mode 2: rgb only -> [n][H'][W'][3] (white_bkgd False). */
int32_t hn_blender_images(const uint8_t* rgba, int64_t n_images, int32_t H, int32_t W, int32_t half_res,
                          int32_t mode, float* out, void* stream);

/* Training loss (run_nerf.py:612-636 with the data-parallel rule of
 * SURVEY 8e): loss = (mse(rgb) + mse(rgb0)) / world + sparse_w * (sum sp + sum sp0)
 * + tv_w * sum tv.  rgb0/sp0/tv may be NULL.  out[4] (device) = loss, mse, mse0,
 * sum of entropies.  The backward writes the upstream gradients of the five
 * inputs in torch autograd's op order (mean/pow/div/mul backward), g_loss is
 * the device scalar d L_total / d loss. */
int32_t hn_loss_fwd(const float* rgb, const float* rgb0, const float* target, const float* sp,
                    const float* sp0, int64_t n_rays, const float* tv, int32_t n_tv, float world,
                    float sparse_w, float tv_w, float* out, void* stream);
int32_t hn_loss_bwd(const float* rgb, const float* rgb0, const float* target, int64_t n_rays,
                    int32_t n_tv, float world, float sparse_w, float tv_w, const float* g_loss,
                    float* g_rgb, float* g_rgb0, float* g_sp, float* g_sp0, float* g_tv, void* stream);
/* hn_loss_fwd and hn_loss_bwd in one launch (the trainer's step: the backward
 * does not depend on the loss value); out and the gradients bitwise those of
 * the two calls. */
int32_t hn_loss_fwd_bwd(const float* rgb, const float* rgb0, const float* target, const float* sp,
                        const float* sp0, int64_t n_rays, const float* tv, int32_t n_tv, float world,
                        float sparse_w, float tv_w, float* out, const float* g_loss, float* g_rgb,
                        float* g_rgb0, float* g_sp, float* g_sp0, float* g_tv, void* stream);

size_t hn_render_workspace_bytes(const hn_render_cfg* cfg, int64_t n_rays);
/* The table-gradient scatter hn_render_bwd runs for this configuration and
 * batch (1 float atomics, 2 binned), after cfg->scatter, the table size and
 * the box's cell counts. */
int32_t hn_render_scatter_mode(const hn_render_cfg* cfg, int64_t n_rays);
int32_t hn_render_fwd(const hn_render_cfg* cfg, const hn_render_fwd_args* a,
                      void* workspace, size_t ws_bytes, void* stream);
/* hn_render_fwd with the form of its kernel chosen by the caller (additive
 * under ABI 14; tests and A/B measurements), every output bitwise
 * hn_render_fwd's: 1 = 4-ray workgroups, every weight fragment through a
 * per-wave LDS ring; 2 = 16-ray workgroups that hold both nets' sigma layers
 * resident in LDS; 0 = hn_render_fwd, which picks 2 where ceil(n_rays / 16)
 * reaches the device's compute units and 1 below that.  Any other form:
 * HN_E_SHAPE, before anything is launched. */
int32_t hn_render_fwd_form(const hn_render_cfg* cfg, const hn_render_fwd_args* a, int32_t form,
                           void* workspace, size_t ws_bytes, void* stream);
/* The form (1 or 2) hn_render_fwd runs for n_rays on the current device;
 * *cus (optional) = the compute units that rule was stated against. */
int32_t hn_render_fwd_pick(int64_t n_rays, int32_t* cus);
/* Which rays the workgroups of form 2 take (additive under ABI 14; host only,
 * no device needed: the function the kernel calls, for tests and the cost
 * model of scripts/fwd_deal_model.py).  Workgroup b of n_blocks (the launch
 * uses ceil(n_rays / 16)) runs four runs of 4 consecutive rays;
 * first_ray[4 b + s] = the first ray of its run s, and every multiple of 4
 * below 16 n_blocks appears once.  run_key [4 n_blocks] (NULL = all equal):
 * per run of the batch the number of its rays, 0..4, whose target is not the
 * background colour, which the loss-mode forward counts itself; a run that
 * starts at or past n_rays counts 0.  Where n_blocks is a multiple of 32 and
 * at most 2048, XCD b % 8 owns the 64-ray segments = b % 8 (mod 8), sorts
 * their runs stably by descending key and deals them in rounds over its
 * n_blocks / 8 workgroups, even rounds forward and odd rounds backward; any
 * other grid takes one run from each quarter of its XCD's band of the batch
 * (of the batch, where n_blocks is no multiple of 8).  A key above 4,
 * n_rays > 16 n_blocks or n_blocks < 1: HN_E_SHAPE. */
int32_t hn_render_fwd_deal(int64_t n_rays, int64_t n_blocks, const uint8_t* run_key, int32_t* first_ray);
/* What a workgroup of form 2 holds of a packed net in LDS (additive under ABI
 * 14; host only, no device needed: the functions the kernel copies and reads
 * through, for the tests).  fine: 0 the coarse net, 1 the fine net (the two
 * are laid out alike).  Returns the floats of that net's image (the
 * workgroup's image is the coarse net's, then the fine net's): sigma_net.0,
 * rows 0-15 of sigma_net.1, color_net.0's geo half and rows 0-2 of
 * color_net.2.  src [n_src] (optional): for every float of the image
 * the index of the packed-net float it is a copy of.  at [n_at] (optional,
 * n_at >= 4608: one entry per 16-byte lane of the forward regions, the packed
 * float index / 4): the image's float offset of that lane's 4 floats, or -1
 * where the image does not hold them -- a region that is loaded at use
 * (color_net.1, color_net.0's SH half), or a lane the packing leaves zero (output rows 16-31 of sigma_net.1, 3-31 of
 * color_net.2), for which the kernel takes zero bits.  fine outside 0..1 or an
 * array too short: -HN_E_SHAPE. */
int32_t hn_render_fwd_res_map(int32_t fine, int32_t* src, int64_t n_src, int32_t* at, int64_t n_at);
int32_t hn_render_bwd(const hn_render_cfg* cfg, const hn_render_bwd_args* a,
                      void* workspace, size_t ws_bytes, void* stream);

/* ---- the gradient with respect to the rays (additive under ABI 14) --------
 * d loss / d rays [B][11] of the forward whose saved state `a` holds (pose
 * refinement: a pose's gradient follows by autograd of get_rays /
 * get_ndc_rays).  near, far and the sampling draws are constants and the
 * importance samples detached (run_nerf_helpers.py:546), so per ray
 *   columns 0:3  d o       = sum_k dx_k
 *   columns 3:6  d d       = sum_k z_k dx_k + d|d| d / |d|   (0 where |d| = 0)
 *   columns 6:8  near, far : written as 0 (no gradient is formed for them)
 *   columns 8:11 d viewdir = J_sh(viewdir)^T sum_k dsh_k
 * over the 64 coarse points (coarse net) and the fine points (fine net); dx_k
 * is hn_encode_bwd_input's closed form, d|d| hn_composite_bwd_inputs'.  Read
 * from `a`: n_rays, rays, noise_c / noise_f, table, both nets, z_coarse,
 * z_fine, raw_c, raw_f, fine_src, feat (its ReLU mask words) and the g_*
 * upstream gradients; every d* output, step and job field is ignored, `loss`
 * and `prepass_done` must be unset (HN_E_SHAPE).  Written: d_rays only (=, not
 * +=).  `scratch` (hn_render_bwd_rays_workspace_bytes; 0 for a cfg
 * hn_render_fwd refuses) belongs to this call alone -- the nets are packed
 * into it whatever weights_packed says -- and may be the caller's for any
 * other use afterwards; a render workspace is neither read nor written, so
 * hn_render_bwd of the same state may run before or after.  No float atomic:
 * bitwise repeatable.  A tile of 32 samples whose d raw are all exact zeros
 * reads none of the saved state, so a skip_dead_color forward's state is
 * accepted.  Every check precedes the first launch: NULL a / rays / table /
 * nets / saved tensors / feat / d_rays / scratch HN_E_NULL, scratch too small
 * HN_E_WORKSPACE, a cfg hn_render_fwd refuses HN_E_SHAPE; n_rays == 0: HN_OK,
 * nothing launched. */
size_t hn_render_bwd_rays_workspace_bytes(const hn_render_cfg* cfg, int64_t n_rays);
int32_t hn_render_bwd_rays(const hn_render_cfg* cfg, const hn_render_bwd_args* a, void* scratch, size_t bytes,
                           float* d_rays, void* stream);

/* ---- whole images from poses (additive under ABI 14) ----------------------
 * The evaluation renderer: run_nerf_helpers.py:310-392 render(H, W, K,
 * c2w=pose, ndc=False, use_viewdirs=True) with perturb = 0 and raw_noise_std =
 * 0, for every pose of a list as :395-459 render_path walks it -- one launch,
 * poses in and images out.  Pixel (row j, column i) of view v gets the ray of
 * hn_sample_rays for that pixel (ray_util.py:62-80, the normalised view
 * direction; the same float32 operations in the same order) and
 * hn_render_fwd's rgb / depth / acc for that ray bit for bit, under the same
 * hn_render_cfg (white_bkgd and lindisp honoured; perturb != 0 is
 * HN_E_SHAPE).  Tiles of 32 samples without density skip the colour net, as
 * hn_render_fwd_args.skip_dead_color (no noise here, so no output changes).
 * Nothing but the three images is written: no z, raw, coarse outputs,
 * entropies or features.  A fixed grid of workgroups loops over the rays --
 * 2 x 2 pixel blocks, 16 x 16 pixel tiles of them in Morton order, view after
 * view -- so the workspace (both nets' packed weights, and per resident wave
 * the two coarse feature tiles its ray's fine pass reuses) depends on cfg
 * only, not on H, W or n_views.
 * hn_render_image and hn_render_image_variant take 64 + 128 samples and world
 * rays only (cfg->n_importance = 64: HN_E_SHAPE); hn_render_views below is the
 * same host path and the same kernel for every configuration it covers.
 * H, W <= 0, n_views < 0, a pose_stride other than 12 or 16, or more than
 * 2^31 - 1 ray groups (4 rays): HN_E_SHAPE; n_views == 0: HN_OK without a launch. */
typedef struct hn_image_args {
  int32_t n_views, H, W;
  int32_t pose_stride;            /* floats between consecutive c2w matrices (12 or 16) */
  float fx, fy, cx, cy;           /* K, as hn_ray_sampler */
  float near, far;
  const float* poses;             /* device [n_views][3][4] row-major c2w */
  const float* t_vals;            /* device [64]  torch.linspace(0,1,64) */
  const float* u;                 /* device [128] ([cfg->n_importance] for hn_render_views) the det
                                     importance uniforms, the same for every ray */
  const float* table;
  hn_mlp coarse, fine;
  float* rgb;                     /* [n_views][H][W][3] */
  float* depth; float* acc;       /* [n_views][H][W] */
  float* rays;                    /* optional [n_views*H*W][11], pixel order (view, row, column); NULL = not written */
  int32_t weights_packed;         /* as hn_render_fwd_args */
} hn_image_args;
size_t  hn_render_image_workspace_bytes(const hn_render_cfg* cfg);
int32_t hn_render_image(const hn_render_cfg* cfg, const hn_image_args* a, void* workspace, size_t ws_bytes,
                        void* stream);
/* The same call with one of the design alternatives it was measured against
 * (scripts/render_image_ab.py), every output bitwise hn_render_image's:
 * variant bit 0 = every fine sample hash-encoded (no reuse of the coarse
 * twins' features), bit 1 = rays taken in (view, row, column) order, 4
 * consecutive pixels per workgroup.  0 = hn_render_image. */
int32_t hn_render_image_variant(const hn_render_cfg* cfg, const hn_image_args* a, int32_t variant,
                                void* workspace, size_t ws_bytes, void* stream);

/* ---- whole images for every fused configuration (additive under ABI 14) ---
 * hn_render_image's renderer for cfg->n_importance = 128 or 64 (any other
 * count: HN_E_SHAPE) and, with ndc = 1, for NDC rays: render(H, W, K,
 * c2w=pose, ndc=True, use_viewdirs=True), the LLFF configurations' evaluation
 * (near = 0, far = 1 are the caller's, as for any ray).  Everything said of
 * hn_render_image holds: the rays, the order, the grid, the outputs bit for
 * bit hn_render_fwd's on the same rays under the same cfg, the status codes,
 * every check before any launch.  image.u holds cfg->n_importance values.
 * ndc = 1: each pixel's ray goes through run_nerf_helpers.py:349
 * get_ndc_rays(H, W, K[0][0], 1., rays_o, rays_d) (ray_util.py:96-142) on the
 * device, float32 operation for float32 operation in torch's order: origin and
 * direction are rewritten, near, far and the view direction (normalised from
 * the world direction before that step, as render() does) are not; image.rays,
 * when given, receives these final rays.  The near plane is render()'s constant
 * 1.  ndc_sx = -1. / (W / (2. * focal)) and ndc_sy = -1. / (H / (2. * focal))
 * with focal = K[0][0], evaluated in double and rounded to float once (what
 * torch does with a Python scalar times a float32 tensor; the reference uses
 * H, W and fx here, not cx, cy or fy).  ndc = 0: both factors are ignored.  A
 * ray whose world direction has d_z = 0 gets the non-finite values those
 * operations give, and is then rendered as hn_render_fwd renders such a ray.
 * variant: hn_render_image_variant's bits, 0 = the shipped design.
 * ndc outside {0, 1} or a variant outside those bits: HN_E_SHAPE.
 * hn_render_views_workspace_bytes is the same for both counts and equals
 * hn_render_image_workspace_bytes of the 128 cfg (0 for a refused cfg). */
typedef struct hn_view_args {
  hn_image_args image;            /* u: device [cfg->n_importance] */
  int32_t ndc;                    /* 0 world rays, 1 NDC rays */
  float ndc_sx, ndc_sy;
  int32_t variant;
} hn_view_args;
size_t  hn_render_views_workspace_bytes(const hn_render_cfg* cfg);
int32_t hn_render_views(const hn_render_cfg* cfg, const hn_view_args* a, void* workspace, size_t ws_bytes,
                        void* stream);

/* ---- density queries (additive under ABI 14) -------------------------------
 * Raw sigma of one NeRFSmall over the hash grid -- NeRFSmall's column 3, the
 * value before the ReLU that raw2outputs applies -- at n points x [n][3], or
 * on a regular lattice the kernel generates itself: point q = (iz * ny + iy)
 * * nx + ix has the coordinate lo[a] + (float)i_a * step[a] on axis a, formed
 * as one f32 multiply and one f32 add (no FMA), so lo + arange(n, float32) *
 * step on the host gives the same bits.  Only the hash encoding and the two
 * sigma layers run; a point's sigma is bitwise what hn_encode_fwd + hn_mlp_fwd
 * (and the fused forward) give for it.  Outputs, each optional, at least one:
 *   sigma [n] f32;
 *   occ [(n + 31) / 32] u32: bit q & 31 of word q >> 5 = sigma[q] > threshold,
 *   the last word's bits past n are 0 (threshold is read only with occ).
 * Nothing is accumulated: a second call writes the same bits.  The grid must
 * have 16 levels; n and nx * ny * nz are at most HN_DENSITY_MAX_POINTS (2^31
 * tiles of 32 points).  workspace: hn_mlp_workspace_bytes() bytes, the net's
 * packed copy, written by the call.  Status, every check before any launch:
 * HN_E_NULL for a NULL g, w (or one of its tensors), table, lat, x (n > 0),
 * workspace, or both outputs NULL; HN_E_SHAPE for a grid that is not 16 levels
 * x 2 features with T in 1..24, n < 0, a dim <= 0 or a count past the bound;
 * HN_E_WORKSPACE for a short workspace.  n == 0 is HN_OK and launches nothing.
 * The library does not allocate or synchronise. */
#define HN_DENSITY_MAX_POINTS ((int64_t)1 << 36)
typedef struct hn_lattice {
  float lo[3];
  float step[3];
  int32_t dims[3];                /* nx, ny, nz */
  int32_t reserved;
} hn_lattice;
int32_t hn_density_points(const hn_grid* g, const hn_mlp* w, const float* table, const float* x, int64_t n,
                          float threshold, float* sigma, uint32_t* occ, void* workspace, size_t ws_bytes,
                          void* stream);
int32_t hn_density_lattice(const hn_grid* g, const hn_mlp* w, const float* table, const hn_lattice* lat,
                           float threshold, float* sigma, uint32_t* occ, void* workspace, size_t ws_bytes,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HASHNERF_AMD_H */
