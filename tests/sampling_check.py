"""Where a ray's samples are placed, judged without a left-out share (helper of
test_sampling_check_cpu.py and test_gpu_sampling.py; no GPU, no fixture).

Importance samples cannot be compared in z: near sample_pdf's `denom < 1e-5`
test (run_nerf_helpers.py:303) an ulp in the cdf moves a sample by a large part
of a bin, and a flip of the test by a whole bin.  They can be compared in cdf
space: a sample s drawn for u is right when the reference cdf F, piecewise
linear over the bins, has F(s) = u.  At a threshold flip |F(s) - u| < 1e-5
still holds, because the whole bin's mass is below 1e-5.

cdf_residual(bins, weights, u, samples) -> (residual, bound, inside), all fp64
torch on the CPU:

  F         the cdf of (weights + 1e-5) / sum, cdf[0] = 0, linear between bins;
  bin i     searchsorted(bins, s, right=True) - 1, clamped to [0, nb - 2];
  residual  |c0 + (s - b0) / (b1 - b0) * (c1 - c0) - u|.  Where s sits on a bin
            edge shared by zero-width bins F(s) is the interval from the cdf at
            the first of the equal edges to the cdf at the last (a sample drawn
            in a zero-width bin is that edge for every u of the bin), and the
            residual is u's distance from it: a zero-width bin passes if
            u is in [c0 - bound, c1 + bound];
  bound     1e-5 + 5e-6 + (c1 - c0) * 2 * ulp32(s) / (b1 - b0):
            1e-5   the reference's own denom < 1e-5 threshold (:303); below it
                   the sample collapses onto b0;
            5e-6   the fp32 rounding of the weights (expf), the normaliser and
                   the cdf's 63 entries (<= 6e-8 each, accumulating);
            last   the fp32 rounding of s itself (a product and a sum, each
                   within an ulp of s), carried through F's slope in the bin;
  inside    bins[0] <= s <= bins[-1].

The 5e-6 stands for weights that are the sampler's exact input, or whose sum is
near 1.  Where F's weights are recomputed in fp64 from a pass's raw output and
the sampler under test formed its own in fp32 (the fused forward, and the
reference's render_rays alike), each nonzero weight is (1 - exp(-x)) * T with
exp(-x) known to an ulp of a number below 1, 2^-24, however small the weight;
a cumulative sum of n of them is uncertain by E = n * 2^-24, and a cdf entry,
one such sum over another of total `mass`, by 2 E / mass.  A ray that grazes
the density has mass ~1e-3 and the term is ~1e-2 there; at mass 1 it is 7e-6.
cdf_residual(..., weights_err=E) adds it (raw_weights_err gives E); measured
on the oracle alone (its fp32 raw -> weights -> samples against the fp64 F of
the same raw, the sweep's natural batches): without the term the reference
itself reaches 3.5 bounds on the 0/1 jittered batch and 1.7 on the 2/6 det
one; with it 0.12 of the bound.

Rows whose bins decrease (a ray with near > far) are judged on -bins and -s.
None of the numbers is measured on a kernel.  Measured on the oracle alone
(test_sampling_check_cpu.py's sweep: 256 rays x 5 bound / lindisp settings x
{det, jittered} x 5 kinds of weights x 3 kinds of u, fp32 oracle.sample_pdf):
the largest residual / bound is 0.628, every sample inside (a bin of mass just
under 1e-5 beside a weight of 1: the threshold term alone; natural weights
reach 0.19).

rank_residual is the same for samples whose order of drawing is lost (the
forward's z_fine keeps them sorted): F does not decrease, so the k-th smallest
sample belongs to the k-th smallest u.

coarse_z_ref is run_nerf_helpers.py:514-536, the coarse z of render_rays, in
fp32 torch ops, op for op the text of oracle.render_rays.
"""
import torch

F64 = torch.float64
THRESHOLD = 1e-5      # sample_pdf's denom < 1e-5 (:303)
ROUNDING = 5e-6       # fp32 weights, normaliser, cdf; reference alone: 0.628 of the bound with this term


def ulp32(x):
    """Spacing of the fp32 numbers at |x| (fp64 tensor)."""
    a = x.to(torch.float32).abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).to(F64)


def reference_cdf(weights):
    """[B, nb - 1] weights -> [B, nb] fp64 cdf of (weights + 1e-5) / sum with cdf[0] = 0 (:266-269)."""
    w = weights.to(F64) + 1e-5
    pdf = w / w.sum(-1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    return torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)


def _flip_decreasing(bins, samples):
    bins, samples = bins.to(F64), samples.to(F64)
    sign = torch.where(bins[:, -1:] < bins[:, :1], -1.0, 1.0).to(F64)
    return bins * sign, samples * sign


def _eval_bin(bins, cdf, s, i, zero_width_end):
    """F at s within bin i, its bound there; a zero-width bin gives the cdf at
    its lower (0) or upper (1) edge."""
    b0, b1 = torch.gather(bins, 1, i), torch.gather(bins, 1, i + 1)
    c0, c1 = torch.gather(cdf, 1, i), torch.gather(cdf, 1, i + 1)
    width = b1 - b0
    flat = width <= 0
    safe = torch.where(flat, torch.ones_like(width), width)
    f = torch.where(flat, c1 if zero_width_end else c0, c0 + (s - b0) / safe * (c1 - c0))
    slope = torch.where(flat, torch.zeros_like(width), (c1 - c0) / safe)
    return f, THRESHOLD + ROUNDING + slope * 2.0 * ulp32(s)


def raw_weights_err(weights):
    """E [B]: the fp32 uncertainty of a cumulative sum of weights formed from a
    pass's raw output -- 2^-24 for each nonzero weight (the module's note)."""
    return 2.0 ** -24 * torch.count_nonzero(weights, dim=-1).to(F64)


def cdf_residual(bins, weights, u, samples, weights_err=None):
    """bins [B, nb], weights [B, nb - 1], u and samples [B, ns] (samples[b, k]
    drawn for u[b, k]) -> (residual, bound, inside), [B, ns] each.
    weights_err: None for exact weights, or E [B] (raw_weights_err)."""
    bins, s = _flip_decreasing(bins.detach().cpu(), samples.detach().cpu())
    u = u.detach().cpu().to(F64)
    cdf = reference_cdf(weights.detach().cpu())
    nb = bins.shape[-1]
    bins, s = bins.contiguous(), s.contiguous()
    hi = (torch.searchsorted(bins, s, right=True) - 1).clamp(0, nb - 2)
    lo = (torch.searchsorted(bins, s, right=False) - 1).clamp(0, nb - 2)   # == hi unless s is a bin edge
    f_hi, bound_hi = _eval_bin(bins, cdf, s, hi, 1)
    f_lo, bound_lo = _eval_bin(bins, cdf, s, lo, 0)
    f_lo = torch.minimum(f_lo, f_hi)
    below = u < f_lo
    residual = torch.where(below, f_lo - u, (u - f_hi).clamp_min(0.0))
    bound = torch.where(below, bound_lo, bound_hi)
    if weights_err is not None:
        mass = (weights.detach().cpu().to(F64) + 1e-5).sum(-1, keepdim=True)
        bound = bound + 2.0 * weights_err.detach().cpu().to(F64).reshape(-1, 1) / mass
    # (a NaN anywhere -- a mutant's 0 / 0 -- must not read as a pass)
    residual = torch.where(torch.isfinite(residual), residual, torch.full_like(residual, float("inf")))
    inside = (s >= bins[:, :1]) & (s <= bins[:, -1:])
    return residual, bound, inside


def rank_residual(bins, weights, u, samples, weights_err=None):
    """cdf_residual for samples in any order: the k-th smallest sample (along
    the bins' direction) against the k-th smallest u."""
    fb, fs = _flip_decreasing(bins.detach().cpu(), samples.detach().cpu())
    return cdf_residual(fb, weights, torch.sort(u.detach().cpu(), -1)[0], torch.sort(fs, -1)[0], weights_err)


def coarse_z_ref(rays, t_vals, t_rand, lindisp):
    """rays [B, >= 8] fp32 (near, far in columns 6, 7), t_vals [64], t_rand
    [B, 64] or None (perturb == 0) -> the coarse z [B, 64], fp32."""
    rays, t_vals = rays.detach().cpu(), t_vals.detach().cpu()
    bounds = torch.reshape(rays[..., 6:8], [-1, 1, 2])
    near, far = bounds[..., 0], bounds[..., 1]
    if not lindisp:
        z_vals = near * (1. - t_vals) + far * t_vals
    else:
        z_vals = 1. / (1. / near * (1. - t_vals) + 1. / far * t_vals)
    z_vals = z_vals.expand([rays.shape[0], t_vals.shape[0]])
    if t_rand is not None:
        mids = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
        upper = torch.cat([mids, z_vals[..., -1:]], -1)
        lower = torch.cat([z_vals[..., :1], mids], -1)
        z_vals = lower + (upper - lower) * t_rand.detach().cpu()
    return z_vals


SETTINGS = ("uniform", "per_ray", "zero_one", "lindisp", "lindisp_per_ray")


def ray_bounds(setting, n, g):
    """near, far [n, 1] of a bound setting (SETTINGS; the last two go with lindisp)."""
    if setting in ("uniform", "lindisp"):
        return torch.full((n, 1), 2.0), torch.full((n, 1), 6.0)
    if setting == "zero_one":
        return torch.zeros(n, 1), torch.ones(n, 1)
    return 0.5 + 2.5 * torch.rand(n, 1, generator=g), 4.0 + 5.0 * torch.rand(n, 1, generator=g)


def make_u(kind, n, ni, g):
    """[n, ni] importance uniforms: "random", "linspace" (the det draw, :279) or
    "edges": random with the columns 0, 1 - 2^-24 (the largest fp32 below 1) and 2^-32."""
    if kind == "linspace":
        return torch.linspace(0., 1., ni).expand(n, ni).contiguous()
    u = torch.rand(n, ni, generator=g)
    if kind == "edges":
        u[:, 0], u[:, 1], u[:, 2] = 0.0, 1.0 - 2.0 ** -24, 2.0 ** -32
    return u
