"""Where the fused forward places each ray's samples, with no share of them
left out: the coarse z (coarse_z, hn_render_fwd.h), sample_pdf_wave and the
merge of the two runs (importance_sort: merge_sort_z<2> / merge_sort_z<1> and the
rank_sort_wave fallback), and the stand-alone hn_sample_pdf at its edges.

The other oracle tests allow 3 % of the fine z to be anything, because samples
cannot be compared in z (sample_pdf's `denom < 1e-5`, run_nerf_helpers.py:303).
Here every importance sample is judged in cdf space (tests/sampling_check.py:
|F(s) - u| within a bound made of the reference's threshold and fp32 rounding,
none of it measured on a kernel; test_sampling_check_cpu.py shows the oracle
passes it and five kinds of sampler bug do not).

States are built as gpu_support.blender_state does (T = 14, finest 512, the
blender box and camera), with t_vals, t_rand and u made on the CPU and
uploaded, so host and device see the same bits.  Bound settings
(sampling_check.SETTINGS): uniform 2/6, per-ray near in [0.5, 3] / far in
[4, 9], 0/1, and the first two again with lindisp.

Largest device residual / bound measured on an MI355X (each test prints its
own; the oracle alone reaches 0.12 with weights from raw and 0.63 with exact
ones), test_every_importance_sample at B = 67, the largest over the three
kinds of u, by bound setting in SETTINGS' order:

  ni = 128  natural 0.063 0.073 0.103 0.091 0.073   zero 0.010 0.016 0.006 0.009 0.010
            dense   0.014 0.020 0.021 0.022 0.025
  ni = 64   natural 0.063 0.068 0.103 0.089 0.071   zero 0.009 0.016 0.006 0.010 0.012
            dense   0.013 0.021 0.020 0.020 0.025

B = 1: 0.025, B = 130 in either form: 0.064, B = 256: 0.078; the ordinary rays
of the ties batch 0.044, its reversed rays 0.005.  hn_sample_pdf, the largest
over n_samples and the kinds of weights, by n_bins 2, 3, 9, 32, 33, 63, 256:
0.214 0.176 0.663 0.249 0.230 0.246 0.620 (the large ones are samples
collapsed onto a bin edge below the 1e-5 threshold, as the reference's are).
The coarse z is bitwise on both branches, lindisp included.
"""
import pytest
import torch

from gpu_support import BLENDER_BOX, OUT_KEYS, bits_equal, blender_nets, hf, rel_err
from sampling_check import SETTINGS, cdf_residual, coarse_z_ref, make_u, rank_residual, raw_weights_err, ray_bounds

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 14
BOX = BLENDER_BOX
SIGMA_SIGN = {"natural": 0, "zero": -1, "dense": 1}
U_KINDS = ("random", "linspace", "edges")
_SCENES = {}
_RAYS = {}


def scene(hn, weights):
    """Table and nets of a kind of weights (blender_nets' sigma_sign: -1 makes
    every raw sigma <= 0, a uniform pdf; +1 every one >= 0).  Built once."""
    if weights not in _SCENES:
        n = blender_nets(hn, T, 31 + SIGMA_SIGN[weights], sigma_sign=SIGMA_SIGN[weights])
        _SCENES[weights] = dict(emb=n.emb, mc=n.mc, mf=n.mf, table=n.emb.table.detach(),
                                ws=[w.detach() for w in list(n.mc.weights()) + list(n.mf.weights())])
    return _SCENES[weights]


def make_rays(hn, B, setting, seed=0):
    """[B, 11] rays on the CPU: the blender camera's, near and far of the setting."""
    key = (B, setting, seed)
    if key not in _RAYS:
        g = torch.Generator().manual_seed(1000 * seed + 10 * B + SETTINGS.index(setting))
        _, K = hn.rays.blender_intrinsics(400, 400)
        ro, rd = hn.get_rays(400, 400, K, hn.pose_spherical(30.0 + seed, -30.0, 4.0)[:3, :4].to(DEV))
        sel = torch.randperm(400 * 400, generator=g)[:B]
        ro, rd = ro.reshape(-1, 3).cpu()[sel], rd.reshape(-1, 3).cpu()[sel]
        near, far = ray_bounds(setting, B, g)
        _RAYS[key] = torch.cat([ro, rd, near, far, rd / torch.norm(rd, dim=-1, keepdim=True)], -1).contiguous()
    return _RAYS[key]


def forward(hn, rays, ni, lindisp, weights, u, t_rand, form=None):
    """One HF.render_fwd of CPU-made inputs; returns (out, state), the device fault word read."""
    HF = hf()
    sc = scene(hn, weights)
    cfg = HF.make_render_cfg(sc["emb"].grid(), True, lindisp, t_rand is not None, n_importance=ni, scatter="binned")
    t_vals = torch.linspace(0., 1., 64)
    out, st = HF.render_fwd(cfg, rays.to(DEV), t_vals.to(DEV), None if t_rand is None else t_rand.to(DEV),
                            u.to(DEV), None, None, sc["table"], sc["ws"], True, form=form)
    torch.cuda.synchronize()
    HF.L.check_device_faults()
    return out, st


def draws(B, ni, u_kind, perturb, seed):
    g = torch.Generator().manual_seed(seed)
    t_rand = torch.rand(B, 64, generator=g) if perturb else None
    return t_rand, make_u(u_kind, B, ni, g)


def coarse_weights(oracle, st, rays):
    """The coarse pass's weights[..., 1:-1] (:547) in fp64 from the device's own raw and z."""
    w = oracle.raw2outputs(st.raw_c.cpu().double(), st.z_c.cpu().double(), rays[:, 3:6].double())[3]
    return w[:, 1:-1].contiguous()


def split_fine(st, ni):
    """z_f / fine_src -> (importance samples [B, ni] in z_f's order, positions
    [B, 64] of the coarse samples); asserts the tags' structure."""
    zf, src = st.z_f.cpu(), st.fine_src.cpu().long()
    B = zf.shape[0]
    assert tuple(zf.shape) == (B, 64 + ni) and tuple(src.shape) == (B, 64 + ni)
    imp = src == 255
    assert bool(((src < 64) | imp).all())
    assert bool((imp.sum(1) == ni).all()), "not n_importance samples on every ray"
    pos = torch.full((B, 64), -1, dtype=torch.long)
    rows = torch.arange(B)[:, None].expand_as(src)
    pos[rows[~imp], src[~imp]] = torch.arange(64 + ni).expand_as(src)[~imp]
    assert bool((pos >= 0).all()), "a coarse index is missing from fine_src"
    return zf[imp].view(B, ni), pos


def check_samples(oracle, st, rays, u, ni, rows=None):
    """(b)'s assertions on a forward state; returns the largest residual / bound."""
    samples, pos = split_fine(st, ni)
    zf, zc = st.z_f.cpu(), st.z_c.cpu()
    sl = slice(None) if rows is None else rows
    # the coarse run is kept bitwise, in its own order
    assert torch.equal(torch.gather(zf, 1, pos)[sl], zc[sl])
    assert bool((pos[sl][:, 1:] > pos[sl][:, :-1]).all())
    bins = .5 * (zc[..., 1:] + zc[..., :-1])
    assert bins.dtype == torch.float32
    # (the kernel's own weights are fp32: raw_weights_err, sampling_check's note)
    w = coarse_weights(oracle, st, rays)[sl]
    res, bound, inside = rank_residual(bins[sl], w, u[sl], samples[sl], raw_weights_err(w))
    ratio = float((res / bound).max())
    assert bool(inside.all()), "an importance sample outside the bins"
    assert bool((res <= bound).all()), f"{int((res > bound).sum())} samples over the bound, worst {ratio:.3f} of it"
    return ratio


def check_z_std(out, st, ni, rows=None):
    """(c): z_std against the fp64 population std of the device's own importance samples."""
    samples, _ = split_fine(st, ni)
    sl = slice(None) if rows is None else rows
    s = samples[sl].double()
    ref = torch.std(s, dim=-1, unbiased=False)
    tol = 1e-6 * ref + 1e-6 * s.abs().max(-1)[0]
    err = (out["z_std"].cpu()[sl].double() - ref).abs()
    assert bool((err <= tol).all()), float((err / tol).max())


# ---- a. coarse z, bitwise ------------------------------------------------------
@pytest.mark.parametrize("B,form", [(1, None), (67, None), (130, "ring"), (130, "resident")])
@pytest.mark.parametrize("perturb", [0, 1], ids=["det", "jittered"])
@pytest.mark.parametrize("setting", SETTINGS)
def test_coarse_z_bitwise(hn, setting, perturb, B, form):
    """z_coarse equals run_nerf_helpers.py:514-536 in fp32 torch ops, bit for
    bit, on both branches of coarse_z and with bounds that differ between rays:
    the library is built with -ffp-contract=off and fp32 division is correctly
    rounded (hn_render_fwd.h's claim).  130 rays: more than one workgroup in
    either form, the last one partial."""
    lindisp = setting.startswith("lindisp")
    rays = make_rays(hn, B, setting)
    t_rand, u = draws(B, 128, "random", perturb, 5)
    out, st = forward(hn, rays, 128, lindisp, "natural", u, t_rand, form=form)
    ref = coarse_z_ref(rays, torch.linspace(0., 1., 64), t_rand, lindisp)
    zc = st.z_c.cpu()
    assert bits_equal(zc, ref), f"{int((zc != ref).sum())} coarse z differ, by up to {float((zc - ref).abs().max()):.3e}"
    assert bits_equal(out["z_coarse"].cpu(), ref)


# ---- b, c. every importance sample, z_std ----------------------------------------
def _sample_case(hn, oracle, ni, setting, weights, u_kind, B=67, form=None):
    lindisp = setting.startswith("lindisp")
    rays = make_rays(hn, B, setting)
    # det sampling goes with its own u (perturb == 0: linspace, :279)
    t_rand, u = draws(B, ni, u_kind, u_kind != "linspace", 9)
    out, st = forward(hn, rays, ni, lindisp, weights, u, t_rand, form=form)
    sig = st.raw_c[..., 3]
    if weights == "zero":
        assert bool((sig <= 0).all())
    elif weights == "dense":
        assert float((sig > 0).float().mean()) > 0.9
    ratio = check_samples(oracle, st, rays, u, ni)
    check_z_std(out, st, ni)
    print(f"residual/bound ni={ni} {setting} {weights} {u_kind} B={B} form={form}: {ratio:.3f}")
    return ratio


@pytest.mark.parametrize("u_kind", U_KINDS)
@pytest.mark.parametrize("weights", ["natural", "zero", "dense"])
@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("ni", [128, 64])
def test_every_importance_sample(hn, oracle, ni, setting, weights, u_kind):
    """Every ray has exactly n_importance samples tagged 255, all inside the
    bins, and the k-th smallest has F(s_k) = the k-th smallest u within the
    bound -- F from oracle.raw2outputs in fp64 on the device's raw_c / z_c; the
    64 coarse-tagged entries of z_f are z_c bitwise at increasing positions;
    z_std is the fp64 population std of those samples (rtol 1e-6 + 1e-6 max|z|:
    one rounding of an fp64 result to fp32, plus the cancellation floor)."""
    _sample_case(hn, oracle, ni, setting, weights, u_kind)


@pytest.mark.parametrize("ni,B,form", [(128, 1, None), (64, 1, None), (128, 130, "resident"), (64, 130, "resident"),
                                       (128, 130, "ring"), (128, 256, None), (64, 256, None)])
def test_every_importance_sample_other_batches(hn, oracle, ni, B, form):
    """The same at one ray, at more than one workgroup of either form and at 256
    rays (lindisp with per-ray bounds, natural weights, u with the edge columns)."""
    _sample_case(hn, oracle, ni, "lindisp_per_ray", "natural", "edges", B=B, form=form)


# ---- d. ties and the unsorted-coarse fallback ---------------------------------------
@pytest.mark.parametrize("weights", ["natural", "zero"])
@pytest.mark.parametrize("ni", [128, 64])
def test_ties_and_unsorted_coarse_fallback(hn, oracle, ni, weights):
    """One batch of 8 rays, perturb off: rays 0-1 with near == far, rays 2-3
    with near > far (the coarse run decreases, merge_sort_z returns false and
    rank_sort_wave sorts all the samples), rays 4-7 ordinary.

    near == far: all z_f are near bitwise, fine_src is [0..63, 255 x ni]
    (coarse first on ties), z_std is 0.  near > far: z_f does not decrease,
    each coarse index sits once at its own value, there are ni samples tagged
    255 inside the bins.  Their colours are the reference's own garbage
    (negative dists), and so, with density, are their coarse weights: alpha <=
    0 makes weights + 1e-5 negative, the "cdf" goes down as well as up, and no
    order of the sorted samples is implied.  The cdf criterion is therefore
    asserted on the reversed rays where every raw sigma is <= 0 (weights
    "zero": the uniform pdf over decreasing bins), and on the ordinary rays in
    both cases.  Ordinary rays give the bits they give in a batch without the
    odd rays, in either form of the kernel."""
    HF = hf()
    rays = make_rays(hn, 8, "uniform", seed=3).clone()
    rays[0, 6:8] = 4.0    # powers of two: near * (1 - t) + near * t is near exactly (the products are exact,
    rays[1, 6:8] = 2.0    # fl(1 - t) + t is within 2^-25 of 1 and rounds to it)
    rays[2, 6], rays[2, 7] = 6.0, 2.0
    rays[3, 6], rays[3, 7] = 5.5, 1.25
    _, u = draws(8, ni, "edges", 0, 21)
    ordinary = slice(4, 8)
    alone, st_alone = forward(hn, rays[ordinary], ni, False, weights, u[ordinary], None)
    for form in ("ring", "resident"):
        out, st = forward(hn, rays, ni, False, weights, u, None, form=form)
        HF.L.check_device_faults()
        zf, zc, src = st.z_f.cpu(), st.z_c.cpu(), st.fine_src.cpu().long()
        samples, pos = split_fine(st, ni)
        # near == far
        for r in (0, 1):
            assert bits_equal(zf[r], rays[r, 6].expand(64 + ni)), f"ray {r}"
            assert torch.equal(src[r], torch.cat([torch.arange(64), torch.full((ni,), 255)])), f"ray {r}"
            assert float(out["z_std"][r]) == 0.0
        # near > far
        rev = slice(2, 4)
        assert bool((zc[rev, 1:] < zc[rev, :-1]).all())
        assert bool((zf[rev, 1:] >= zf[rev, :-1]).all())
        assert torch.equal(torch.gather(zf, 1, pos)[rev], zc[rev])
        bins = .5 * (zc[..., 1:] + zc[..., :-1])
        assert bool(((samples[rev] <= bins[rev, :1]) & (samples[rev] >= bins[rev, -1:])).all())
        check_z_std(out, st, ni, rows=rev)
        if weights == "zero":
            assert bool((st.raw_c[rev, :, 3] <= 0).all())
            w = torch.zeros(2, 62, dtype=torch.float64)
            res, bound, inside = rank_residual(bins[rev], w, u[rev], samples[rev])
            assert bool((res <= bound).all()) and bool(inside.all()), float((res / bound).max())
            print(f"residual/bound reversed rays ni={ni} {form}: {float((res / bound).max()):.3f}")
        # ordinary rays: the criterion, and the bits of a batch of their own
        ratio = check_samples(oracle, st, rays, u, ni, rows=ordinary)
        check_z_std(out, st, ni, rows=ordinary)
        for k in OUT_KEYS:
            assert bits_equal(out[k][ordinary], alone[k]), f"{form}: {k} of an ordinary ray depends on the batch"
        assert torch.equal(st.fine_src[ordinary], st_alone.fine_src), form
        print(f"residual/bound ties ni={ni} {weights} {form}: {ratio:.3f}")


# ---- e. the stand-alone entry at its edges ---------------------------------------------
def _entry_weights(kind, B, nw, g):
    if kind == "zero":
        return torch.zeros(B, nw)
    if kind == "tiny":
        return 1e-7 * torch.rand(B, nw, generator=g)
    if kind == "random":
        return torch.rand(B, nw, generator=g)
    w = torch.zeros(B, nw)
    w[torch.arange(B), torch.randint(0, nw, (B,), generator=g)] = 1.0
    return w


@pytest.mark.parametrize("n_samples", [1, 64, 65, 200])
@pytest.mark.parametrize("n_bins", [2, 3, 9, 32, 33, 63, 256])
def test_sample_pdf_entry_edges(hn, n_bins, n_samples):
    """hn_sample_pdf against the same criterion, sample by sample (the entry
    keeps the order of u).  n_bins covers every branch of torch_row_sum (the
    tail only, nv < 4, the ILP path with and without remainder vectors, four
    weights per lane), n_samples one and more than one round of the wave, 5
    rays a partial last workgroup; weights zero, one spike (bins of mass just
    under the 1e-5 threshold beside it), 1e-7-sized and random; the last row's
    bins decrease.  Not compared bitwise with torch on the CPU at these widths:
    ATen's row-sum order depends on the host's vector ISA
    (test_gpu_parity keeps the bitwise fixture)."""
    HF = hf()
    B = 5
    g = torch.Generator().manual_seed(100 * n_bins + n_samples)
    worst = 0.0
    for kind in ("zero", "spike", "tiny", "random"):
        bins = 2.0 + 4.0 * torch.sort(torch.rand(B, n_bins, generator=g), -1)[0]
        bins[-1] = bins[-1].flip(0)
        w = _entry_weights(kind, B, n_bins - 1, g)
        u = torch.rand(B, n_samples, generator=g)
        if n_samples >= 3:
            u[:, 0], u[:, 1], u[:, 2] = 0.0, 1.0 - 2.0 ** -24, 2.0 ** -32
        s = HF.sample_pdf(bins.to(DEV), w.to(DEV), u.to(DEV))
        torch.cuda.synchronize()
        assert tuple(s.shape) == (B, n_samples)
        res, bound, inside = cdf_residual(bins, w, u, s)
        ratio = float((res / bound).max())
        worst = max(worst, ratio)
        assert bool(inside.all()), kind
        assert bool((res <= bound).all()), (kind, ratio)
    print(f"residual/bound entry n_bins={n_bins} n_samples={n_samples}: {worst:.3f}")


def test_sample_pdf_entry_no_samples(hn):
    HF = hf()
    g = torch.Generator().manual_seed(3)
    bins = torch.sort(torch.rand(5, 9, generator=g), -1)[0]
    s = HF.sample_pdf(bins.to(DEV), torch.rand(5, 8, generator=g).to(DEV), torch.empty(5, 0, device=DEV))
    torch.cuda.synchronize()
    assert tuple(s.shape) == (5, 0)
    HF.L.check_device_faults()


# ---- f. lindisp and per-ray bounds through the backward --------------------------------
def test_fused_step_lindisp_per_ray_bounds(hn, oracle):
    """One fused training step with lindisp = 1 and bounds that differ between
    rays (B = 67, white background, perturb on) against the oracle, as
    test_gpu_edges.test_fused_step_ragged_batches with its tolerances: forward
    rtol 1e-4 / atol 2e-5, loss rtol 1e-5, gradients 5e-4 relative norm.  The
    oracle's fine pass runs on the device's z_fine, whose samples
    test_every_importance_sample checks one by one."""
    import numpy as np
    O, HF = oracle, hf()
    B = 67
    n = blender_nets(hn, T, 41)
    emb, mc, mf = n.emb, n.mc, n.mf
    rb = make_rays(hn, B, "lindisp_per_ray", seed=4)
    assert rb[:, 6].unique().numel() == B and rb[:, 7].unique().numel() == B
    nq = hn.NetworkQuery(emb, hn.SHEncoder())
    HF.DEBUG_KEEP = True
    try:
        ret_d = hn.render_rays(rb.to(DEV), network_fn=mc, network_query_fn=nq, N_samples=64, retraw=True, lindisp=True,
                               perturb=1., N_importance=128, network_fine=mf, white_bkgd=True, pytest=True)
    finally:
        HF.DEBUG_KEEP = False
    z_fine = HF.LAST["z_fine"].cpu()
    assert tuple(z_fine.shape) == (B, 192)
    target = torch.rand(B, 3, generator=torch.Generator().manual_seed(2))
    loss, _ = hn.training_loss(ret_d["rgb_map"], ret_d, target.to(DEV), 1e-3)
    loss.backward()
    torch.cuda.synchronize()
    HF.L.check_device_faults()
    # pytest=True draws t_rand and u from np.random.seed(0) (run_nerf_helpers.py:531-534, :288-291)
    np.random.seed(0)
    t_rand = torch.tensor(np.random.rand(B, 64), dtype=torch.float32)
    np.random.seed(0)
    u = torch.tensor(np.random.rand(B, 128), dtype=torch.float32)
    tab = emb.table.detach().cpu().requires_grad_(True)
    wc = {k: v.detach().cpu().requires_grad_(True) for k, v in zip(O.MLP_KEYS, mc.weights())}
    wf = {k: v.detach().cpu().requires_grad_(True) for k, v in zip(O.MLP_KEYS, mf.weights())}
    ret = O.render_rays(rb, wc, wf, tab, BOX[0], BOX[1], O.level_resolutions(16, 16, 512), T,
                        t_rand=t_rand, u=u, white_bkgd=True, lindisp=True, z_fine=z_fine)
    assert bits_equal(HF.LAST["z_coarse"].cpu(), ret["z_vals0"].detach())
    for k in ("rgb_map", "depth_map", "acc_map", "rgb0", "sparsity_loss", "sparsity_loss0"):
        np.testing.assert_allclose(ret_d[k].detach().cpu().numpy(), ret[k].detach().numpy(), rtol=1e-4, atol=2e-5,
                                   err_msg=k)
    ref_loss = O.training_loss(ret, target, 1e-3)
    np.testing.assert_allclose(loss.item(), ref_loss.item(), rtol=1e-5, atol=1e-7)
    ref_loss.backward()

    assert torch.count_nonzero(tab.grad) > 0
    assert rel_err(emb.table.grad, tab.grad) <= 5e-4, rel_err(emb.table.grad, tab.grad)
    for w_dev, w_ref in ((mc.weights(), wc), (mf.weights(), wf)):
        for p, k in zip(w_dev, O.MLP_KEYS):
            assert rel_err(p.grad, w_ref[k].grad) <= 5e-4, (k, rel_err(p.grad, w_ref[k].grad))
