"""sampling_check.cdf_residual, the criterion test_gpu_sampling.py holds the
kernels' importance samples to, has teeth (CPU only):

* the reference passes it -- oracle.sample_pdf's own fp32 samples, over 256
  rays x {uniform 2/6, per-ray near/far, 0/1, lindisp 2/6, lindisp per-ray} x
  {det, jittered} x {zero, one-spike, two-spike, 1e-7-sized, natural weights}
  x {random u, linspace u, random u with columns 0, 2^-32 and 1 - 2^-24}, stay
  within 0.8 of the bound and inside the bins;
* mutants of sample_pdf fail it on every batch with natural weights, with no
  share of samples exempt;
* coarse_z_ref, the coarse z the GPU tests compare with, is bitwise the
  oracle's render_rays.
"""
import pytest
import torch

from sampling_check import SETTINGS, cdf_residual, coarse_z_ref, make_u, rank_residual, raw_weights_err, ray_bounds

B, T, NI = 256, 14, 128
BOX = (torch.tensor([-4.0, -4.0, -3.4]), torch.tensor([4.0, 4.0, 3.3]))
WEIGHTS = ("zero", "one_spike", "two_spike", "tiny", "natural")
U_KINDS = ("random", "linspace", "edges")
_BATCHES = {}


def batch(oracle, setting, jitter):
    """One coarse pass of the oracle: rays, t_rand, its z and weights.  Built once, left unchanged."""
    key = (setting, jitter)
    if key in _BATCHES:
        return _BATCHES[key]
    O = oracle
    g = torch.Generator().manual_seed(100 + 2 * SETTINGS.index(setting) + jitter)
    table = torch.rand(16, 2 ** T, 2, generator=g) - 0.5
    wc = O.init_nerf_small(g)
    K = [[555.5, 0., 200.], [0., 555.5, 200.], [0., 0., 1.]]
    ro, rd = O.get_rays(400, 400, K, O.pose_spherical(35.0, -30.0, 4.0)[:3, :4])
    sel = torch.randperm(400 * 400, generator=g)[:B]
    ro, rd = ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]
    near, far = ray_bounds(setting, B, g)
    rays = torch.cat([ro, rd, near, far, rd / torch.norm(rd, dim=-1, keepdim=True)], -1)
    t_rand = torch.rand(B, 64, generator=g) if jitter else None
    with torch.no_grad():
        ret = O.render_rays(rays, wc, None, table, BOX[0], BOX[1], O.level_resolutions(16, 16, 512), T,
                            N_importance=0, t_rand=t_rand, lindisp=setting.startswith("lindisp"))
    z = ret["z_vals0"]
    # the same weights in fp64 from the pass's fp32 raw, as the GPU test forms them
    w64 = O.raw2outputs(ret["raw0"].double(), z.double(), rd.double())[3][:, 1:-1].contiguous()
    _BATCHES[key] = dict(rays=rays, t_rand=t_rand, z=z, bins=.5 * (z[..., 1:] + z[..., :-1]),
                         weights=ret["weights0"], w64=w64, g=g)
    return _BATCHES[key]


def make_weights(kind, natural, g):
    """[B, 62] fp32 weights[..., 1:-1] of a kind."""
    n = B
    w = torch.zeros(n, 62)
    rows = torch.arange(n)
    if kind == "natural":
        return natural[:, 1:-1].contiguous()
    if kind == "tiny":
        return 1e-7 * torch.rand(n, 62, generator=g)
    if kind in ("one_spike", "two_spike"):
        w[rows, torch.randint(0, 62, (n,), generator=g)] = 1.0
    if kind == "two_spike":
        w[rows, torch.randint(0, 62, (n,), generator=g)] += 0.6
    return w


@pytest.mark.parametrize("jitter", [0, 1], ids=["det", "jittered"])
@pytest.mark.parametrize("setting", SETTINGS)
def test_reference_passes(oracle, setting, jitter):
    b = batch(oracle, setting, jitter)
    g = torch.Generator().manual_seed(7)
    worst = worst_raw = 0.0
    for wk in WEIGHTS:
        w = make_weights(wk, b["weights"], g)
        for uk in U_KINDS:
            u = make_u(uk, B, NI, g)
            s = oracle.sample_pdf(b["bins"], w, u)
            assert s.dtype == torch.float32
            res, bound, inside = cdf_residual(b["bins"], w, u, s)
            ratio = float((res / bound).max())
            worst = max(worst, ratio)
            assert bool(inside.all()), (wk, uk)
            assert bool((res <= bound).all()), (wk, uk, ratio)
            # the samples in any order, matched by rank
            perm = torch.argsort(torch.rand(B, NI, generator=g), -1)
            res, bound, inside = rank_residual(b["bins"], w, u, torch.gather(s, 1, perm))
            assert bool((res <= bound).all()) and bool(inside.all()), (wk, uk, "by rank")
            if wk == "natural":   # F from the raw output in fp64, the sampler's weights its own fp32 ones
                res, bound, inside = cdf_residual(b["bins"], b["w64"], u, s, raw_weights_err(b["w64"]))
                worst_raw = max(worst_raw, float((res / bound).max()))
                assert bool((res <= bound).all()) and bool(inside.all()), (uk, "weights from raw")
    print(f"{setting} jitter={jitter}: largest residual / bound {worst:.3f}, weights from raw {worst_raw:.3f}")
    assert worst <= 0.8 and worst_raw <= 0.8, (worst, worst_raw)


def test_reference_passes_reversed_and_degenerate_bins(oracle):
    """Rows the forward's odd rays make: decreasing bins (near > far) are judged
    on the negated axis, and all-equal bins (near == far: every sample is that
    value, F there is all of [0, 1])."""
    g = torch.Generator().manual_seed(11)
    z = torch.linspace(6., 2., 64).expand(B, 64) + 0.02 * torch.rand(B, 64, generator=g)
    bins = .5 * (z[..., 1:] + z[..., :-1])
    assert bool((bins[:, 1:] < bins[:, :-1]).all())
    for wk in ("zero", "one_spike", "two_spike", "tiny"):
        w = make_weights(wk, None, g)
        for uk in U_KINDS:
            u = make_u(uk, B, NI, g)
            s = oracle.sample_pdf(bins, w, u)
            for fn in (cdf_residual, rank_residual):
                res, bound, inside = fn(bins, w, u, s)
                assert bool((res <= 0.8 * bound).all()) and bool(inside.all()), (wk, uk, fn.__name__)
    flat = torch.full((4, 63), 3.25)
    u = make_u("edges", 4, NI, g)
    s = oracle.sample_pdf(flat, torch.rand(4, 62, generator=g), u)
    assert torch.equal(s, torch.full_like(s, 3.25))
    res, bound, inside = cdf_residual(flat, torch.rand(4, 62, generator=g), u, s)
    assert bool((res <= bound).all()) and bool(inside.all())
    res, bound, inside = cdf_residual(flat, torch.zeros(4, 62), u, s + 0.5)
    assert not bool(inside.any())


def mutant_sample_pdf(kind, bins, weights_full, u):
    """oracle.sample_pdf(bins, weights_full[..., 1:-1], u) (run_nerf_helpers.py:
    264-307 as render_rays calls it, :547-549) with one thing wrong."""
    weights = weights_full[..., :-2] if kind == "weights_slice" else weights_full[..., 1:-1]
    if kind != "no_epsilon":
        weights = weights + 1e-5
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    u = u.contiguous()
    if kind == "u_cap":
        u = u.clamp(max=0.99)
    inds = torch.searchsorted(cdf, u, right=(kind != "right_false"))
    below = torch.max(torch.zeros_like(inds - 1), inds - 1)
    above = torch.min((cdf.shape[-1] - 1) * torch.ones_like(inds), inds)
    g = torch.stack([below, above], -1)
    shape = [g.shape[0], g.shape[1], cdf.shape[-1]]
    cdf_g = torch.gather(cdf.unsqueeze(1).expand(shape), 2, g)
    gb = (g + 1).clamp(max=cdf.shape[-1] - 1) if kind == "bins_shift" else g
    bins_g = torch.gather(bins.unsqueeze(1).expand(shape), 2, gb)
    denom = cdf_g[..., 1] - cdf_g[..., 0]
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t = (u - cdf_g[..., 0]) / denom
    samples = bins_g[..., 0] + t * (bins_g[..., 1] - bins_g[..., 0])
    if kind == "last_bin_clamp":     # one sample per ray
        samples[:, 5] = bins[:, -1]
    return samples


MUTANTS = ("no_epsilon", "bins_shift", "last_bin_clamp", "u_cap", "weights_slice")


@pytest.mark.parametrize("kind", MUTANTS + ("none",))
def test_mutants_fail(oracle, kind):
    """Each mutant has a sample over the bound (or outside the bins) in every
    batch with natural weights, for every kind of u; the unmutated text
    (kind "none", bitwise oracle.sample_pdf) has none."""
    g = torch.Generator().manual_seed(13)
    for setting in SETTINGS:
        for jitter in (0, 1):
            b = batch(oracle, setting, jitter)
            w = b["weights"][:, 1:-1].contiguous()
            for uk in U_KINDS:
                u = make_u(uk, B, NI, g)
                s = mutant_sample_pdf(kind, b["bins"], b["weights"], u)
                for fn, raw in ((cdf_residual, 0), (rank_residual, 0), (rank_residual, 1)):
                    res, bound, inside = fn(b["bins"], b["w64"], u, s, raw_weights_err(b["w64"])) if raw else \
                        fn(b["bins"], w, u, s)
                    bad = int((~(res <= bound) | ~inside).sum())
                    if kind == "none":
                        assert torch.equal(s, oracle.sample_pdf(b["bins"], w, u))
                        assert bad == 0, (setting, jitter, uk, fn.__name__, bad)
                    else:
                        assert bad > 0, (setting, jitter, uk, fn.__name__, "mutant passes")


def test_searchsorted_side_is_not_observable(oracle):
    """searchsorted(..., right=False) in sample_pdf's text is no mutant: where u
    equals an interior cdf entry both sides draw the shared bin edge (t = 0 of
    the upper bin, t = 1 of the lower), u = 0 is caught by the clamp of
    `below`, and the + 1e-5 keeps fp32 cdf entries apart.  Its samples differ
    from the oracle's only by rounding, and the criterion, rightly, passes them."""
    g = torch.Generator().manual_seed(17)
    for setting in SETTINGS:
        b = batch(oracle, setting, 1)
        w = b["weights"][:, 1:-1].contiguous()
        for uk in U_KINDS:
            u = make_u(uk, B, NI, g)
            s = mutant_sample_pdf("right_false", b["bins"], b["weights"], u)
            ref = oracle.sample_pdf(b["bins"], w, u)
            width = (b["bins"][:, -1:] - b["bins"][:, :1]).abs()
            assert bool(((s - ref).abs() <= 1e-6 * width).all()), (setting, uk)
            res, bound, inside = cdf_residual(b["bins"], w, u, s)
            assert bool((res <= bound).all()) and bool(inside.all())


@pytest.mark.parametrize("jitter", [0, 1], ids=["det", "jittered"])
@pytest.mark.parametrize("setting", SETTINGS)
def test_coarse_z_ref_is_the_oracles(oracle, setting, jitter):
    b = batch(oracle, setting, jitter)
    z = coarse_z_ref(b["rays"], oracle.linspace_tvals(64), b["t_rand"], setting.startswith("lindisp"))
    assert z.dtype == torch.float32 and torch.equal(z, b["z"])
    assert bool((z[:, 1:] >= z[:, :-1]).all())
