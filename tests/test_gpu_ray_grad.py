"""The fused ray gradient (hn_render_bwd_rays behind render_rays(...,
ray_grad="fused")): d loss / d ray_batch and a pose's gradient against autograd
of the fp32 oracle on the CPU, the fine pass on the device's own fine z; raw
noise against the unfused composition; exact zeros, repeatability, the forward
outputs, the parameters' gradients beside it, a frozen field, a
skip_dead_color state, and the refusals.  Comparisons are norm-relative over
all entries; each prints the device-against-fp32-oracle error beside the fp32
oracle's own error against the float64 one before it asserts.

The bar is the project's end-to-end 5e-4 (the MLP backward's data path runs on
the 2-part bf16 split), on the small scene: T = 14, finest 64, 37 rays."""
from importlib import import_module

import pytest
import torch

import ray_grad_cases as rc
from gpu_support import DEV, bits_equal, done, forward_kind, hf, kind_scene, rel_err

pytestmark = pytest.mark.gpu

TOL_E2E = 5e-4
B = 37                      # no multiple of 4 (the reduction's rays per workgroup) or 16
RAY_COLS = (("d o", slice(0, 3)), ("d d", slice(3, 6)), ("d viewdir", slice(8, 11)))


def render_module():
    return import_module("hashnerf_pytorch_amd.render")


def params(s):
    return [s.emb.table] + list(s.mc.weights()) + list(s.mf.weights())


def freeze(s, frozen=True):
    for p in params(s):
        p.requires_grad_(not frozen)
        p.grad = None


def fused_step(hn, s, rays, ni, white, target, **more):
    """One forward and backward of the training loss with ray_grad="fused", the
    forward's fine z recorded -> (ret, rays.grad, z_fine)."""
    HF = hf()
    rays = rays.to(DEV).requires_grad_(True)
    HF.DEBUG_KEEP = True
    try:
        ret = hn.render_rays(rays, ray_grad="fused", **rc.render_kw(s, ni, white, **more))
        z_fine = HF.LAST["z_fine"].clone()
    finally:
        HF.DEBUG_KEEP = False
        HF.LAST.clear()
    loss, _ = hn.training_loss(ret["rgb_map"], ret, target.to(DEV), rc.SPARSE_W)
    loss.backward()
    done()
    return ret, rays.grad, z_fine


def check_batch_grad(what, got, w32, w64):
    assert torch.isfinite(got).all()
    assert bool((got[:, 6:8] == 0).all()), "near / far columns are written as zeros"
    for name, cols in RAY_COLS:
        err, floor = rel_err(got[:, cols], w32[:, cols]), rel_err(w32[:, cols], w64[:, cols])
        print(f"[ray-grad] {what}: {name}: device vs fp32 oracle {err:.3e}, fp32 vs fp64 oracle {floor:.3e}")
        assert float(w32[:, cols].abs().max()) > 0
        assert err <= TOL_E2E, f"{what}: {name}: relative error {err:.3e}"


# ---- parity with the oracle --------------------------------------------------------
@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("ni", [128, 64])
def test_ray_gradient_matches_oracle_autograd(hn, oracle, ni, white):
    s = rc.scene(hn, dev=DEV)
    freeze(s)
    rays = rc.ray_batch(hn, B)
    target = torch.rand(B, 3, generator=torch.Generator().manual_seed(50))
    _, got, z_fine = fused_step(hn, s, rays, ni, white, target)
    assert z_fine.shape == (B, 64 + ni)
    w32, w64 = (rc.oracle_batch_grad(oracle, s, rays, ni, white, target, z_fine, dt)
                for dt in (torch.float32, torch.float64))
    check_batch_grad(f"64 + {ni}, white = {white}", got, w32, w64)


def test_out_of_box_rays(hn, oracle):
    """near 2, far 6 around a box of +-1: most samples of every ray lie outside
    it (clamped cells, unclamped weights)."""
    s = rc.scene(hn, half=1.0, dev=DEV)
    freeze(s)
    rays = rc.ray_batch(hn, B, seed=51)
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * torch.linspace(2., 6., 64)[None, :, None]
    assert float(((pts.abs() > 1.0).any(-1)).float().mean()) > 0.5
    target = torch.rand(B, 3, generator=torch.Generator().manual_seed(52))
    _, got, z_fine = fused_step(hn, s, rays, 128, True, target)
    w32, w64 = (rc.oracle_batch_grad(oracle, s, rays, 128, True, target, z_fine, dt)
                for dt in (torch.float32, torch.float64))
    check_batch_grad("box +-1, 64 + 128", got, w32, w64)


def test_pose_gradient_ndc_image(hn, oracle):
    """render(H, W, K, c2w=pose, ndc=True) of an 11 x 14 forward-facing camera,
    64 + 64: the pose's gradient through get_rays, get_ndc_rays, the view
    directions and the fused ray gradient."""
    HF = hf()
    s = rc.scene(hn, dev=DEV)
    freeze(s)
    target = torch.rand(rc.NDC_H, rc.NDC_W, 3, generator=torch.Generator().manual_seed(rc.NDC_TARGET_SEED))
    c2w = rc.NDC_POSE.to(DEV).requires_grad_(True)
    HF.DEBUG_KEEP = True
    try:
        rgb, _, _, ex = hn.render(rc.NDC_H, rc.NDC_W, rc.NDC_K, c2w=c2w, use_viewdirs=True, ndc=True, near=0., far=1.,
                                  ray_grad="fused", **rc.render_kw(s, 64, False))
        z_fine = HF.LAST["z_fine"].clone()
    finally:
        HF.DEBUG_KEEP = False
        HF.LAST.clear()
    loss, _ = hn.training_loss(rgb, ex, target.to(DEV), rc.SPARSE_W)
    loss.backward()
    done()
    assert z_fine.shape == (rc.NDC_H * rc.NDC_W, 128)
    w32, w64 = (rc.oracle_pose_grad(hn, oracle, s, rc.NDC_POSE, target, z_fine, dt)[0]
                for dt in (torch.float32, torch.float64))
    err, floor = rel_err(c2w.grad, w32), rel_err(w32, w64)
    print(f"[ray-grad] NDC 11 x 14, 64 + 64: c2w: device vs fp32 oracle {err:.3e}, fp32 vs fp64 oracle {floor:.3e}")
    assert torch.isfinite(c2w.grad).all() and float(c2w.grad.abs().max()) > 0
    assert err <= TOL_E2E, f"NDC 64 + 64: d loss / d c2w: relative error {err:.3e}"


# ---- raw noise ---------------------------------------------------------------------
def test_raw_noise_matches_the_unfused_composition(hn):
    """raw_noise_std > 0 under pytest=True: both paths draw the same noise."""
    s = rc.scene(hn, dev=DEV)
    freeze(s)
    target = torch.rand(B, 3, generator=torch.Generator().manual_seed(53)).to(DEV)
    got = []
    for ray_grad in ("fused", None):
        rays = rc.ray_batch(hn, B).to(DEV).requires_grad_(True)
        ret = hn.render_rays(rays, ray_grad=ray_grad, pytest=True, **rc.render_kw(s, 128, True, raw_noise_std=1.0))
        loss, _ = hn.training_loss(ret["rgb_map"], ret, target, rc.SPARSE_W)
        loss.backward()
        done()
        got.append((ret["rgb_map"].detach(), rays.grad))
    (rgb_f, g_f), (rgb_u, g_u) = got
    assert float((rgb_f - rgb_u).abs().max()) <= 1e-6, "the two forwards saw other samples"
    for name, cols in RAY_COLS:
        err = rel_err(g_f[:, cols], g_u[:, cols])
        print(f"[ray-grad] raw noise, 64 + 128: {name}: fused vs unfused {err:.3e}")
        assert float(g_u[:, cols].abs().max()) > 0
        assert err <= TOL_E2E, f"raw noise: {name}: relative error {err:.3e}"


# ---- exact zeros, shapes -----------------------------------------------------------
def test_rays_without_density_get_exact_zeros(hn):
    s = rc.scene(hn, dead=True, dev=DEV)
    freeze(s)
    target = torch.rand(B, 3, generator=torch.Generator().manual_seed(54))
    ret, got, _ = fused_step(hn, s, rc.ray_batch(hn, B), 128, True, target)
    assert float(ret["acc_map"].detach().max()) == 0 and float(ret["acc0"].detach().max()) == 0
    assert got.shape == (B, 11) and torch.isfinite(got).all()
    assert bool((got == 0).all())


def test_dead_ray_among_live_ones(hn):
    """One ray of a live batch with every sigma <= 0 (some exactly 0) in its
    saved raw outputs: exact zeros for it, the other rays' rows unchanged."""
    HF = hf()
    s = kind_scene(hn, B, "rand")
    cfg = HF.make_render_cfg(s.emb.grid(), True, False, True, scatter="binned")
    fwd, st = forward_kind(HF, s, cfg, False, False)
    grads = dict(g_rgb=2. * (fwd["rgb"] - s.target) / (3 * B), g_rgb0=2. * (fwd["rgb0"] - s.target) / (3 * B),
                 g_sparsity=torch.full((B,), 1e-3, device=DEV), g_sparsity0=torch.full((B,), 1e-3, device=DEV))
    live = HF.render_bwd_rays(st, grads)
    for raw in (st.raw_c, st.raw_f):
        raw[5, :, 3] = -raw[5, :, 3].abs()
        raw[5, ::7, 3] = 0.0
    got = HF.render_bwd_rays(st, grads)
    done()
    assert torch.isfinite(got).all() and float(live[5].abs().max()) > 0
    assert bool((got[5] == 0).all())
    keep = torch.arange(B, device=DEV) != 5
    assert bits_equal(got[keep], live[keep]) and float(got[keep][:, :6].abs().max()) > 0


def test_one_ray(hn):
    s = rc.scene(hn, dev=DEV)
    freeze(s)
    rays = rc.ray_batch(hn, B)
    target = torch.rand(B, 3, generator=torch.Generator().manual_seed(50))
    _, one, _ = fused_step(hn, s, rays[:1], 128, True, target[:1])
    assert one.shape == (1, 11) and torch.isfinite(one).all()
    assert float(one[:, :6].abs().min()) > 0 and float(one[:, 8:].abs().max()) > 0
    assert bool((one[:, 6:8] == 0).all())


@pytest.mark.parametrize("ni", [128, 64])
def test_two_calls_are_bitwise_equal(hn, ni):
    s = rc.scene(hn, dev=DEV)
    freeze(s)
    rays = rc.ray_batch(hn, B)
    target = torch.rand(B, 3, generator=torch.Generator().manual_seed(50))
    a, b = (fused_step(hn, s, rays, ni, True, target)[1] for _ in range(2))
    assert float(a.abs().max()) > 0 and bits_equal(a, b)


# ---- beside the rest of the fused path ---------------------------------------------
def test_forward_outputs_are_the_fused_kernels(hn):
    HF, R = hf(), render_module()
    s = rc.scene(hn, dev=DEV)
    freeze(s)
    rays = rc.ray_batch(hn, B).to(DEV)
    ret = hn.render_rays(rays.clone().requires_grad_(True), retraw=True, ray_grad="fused",
                         **rc.render_kw(s, 128, True))
    cfg = HF.make_render_cfg(s.emb.grid(), True, False, False, n_importance=128)
    u = torch.linspace(0., 1., 128, device=DEV).expand(B, 128)
    direct = HF.render_rays_fused(cfg, rays, R._linspace_cached(64, rays.device), None, u, None, None, s.emb.table,
                                  s.mc.weights(), s.mf.weights())
    done()
    names = ("rgb_map", "depth_map", "acc_map", "sparsity_loss", "rgb0", "depth0", "acc0", "sparsity_loss0", "z_std",
             "raw")
    assert set(ret) == set(names)
    for n, t in zip(names, direct):
        assert bits_equal(ret[n], t), n
    assert ret["rgb_map"].requires_grad


def test_parameter_gradients_are_bitwise_those_without_ray_grad(hn):
    s = rc.scene(hn, dev=DEV)
    target = torch.rand(B, 3, generator=torch.Generator().manual_seed(55)).to(DEV)
    got = []
    for on in (False, True):
        freeze(s, False)
        rays = rc.ray_batch(hn, B).to(DEV).requires_grad_(on)
        ret = hn.render_rays(rays, ray_grad="fused", **rc.render_kw(s, 128, True))
        loss, _ = hn.training_loss(ret["rgb_map"], ret, target, rc.SPARSE_W)
        loss.backward()
        done()
        assert (rays.grad is not None) == on
        got.append(([p.grad.clone() for p in params(s)], rays.grad))
    for i, (a, b) in enumerate(zip(got[0][0], got[1][0])):
        assert float(a.abs().max()) > 0
        assert bits_equal(a, b), f"parameter {i} (0 = table) with the ray gradient on"
    # and the ray gradient beside them is the frozen field's
    freeze(s)
    _, alone, _ = fused_step(hn, s, rc.ray_batch(hn, B), 128, True, target)
    assert bits_equal(got[1][1], alone)


def test_without_the_opt_in_rays_get_no_gradient_and_no_launch(hn, monkeypatch):
    """render_rays_fused without ray_grad (a direct caller, rays with grad, a
    trainable field): None for the rays and no render_bwd_rays, as before."""
    HF, R = hf(), render_module()
    s = rc.scene(hn, dev=DEV)
    freeze(s, False)
    called = []
    monkeypatch.setattr(HF, "render_bwd_rays", lambda *a, **k: called.append(1))
    rays = rc.ray_batch(hn, B).to(DEV).requires_grad_(True)
    cfg = HF.make_render_cfg(s.emb.grid(), True, False, False, n_importance=128)
    u = torch.linspace(0., 1., 128, device=DEV).expand(B, 128)
    out = HF.render_rays_fused(cfg, rays, R._linspace_cached(64, rays.device), None, u, None, None, s.emb.table,
                               s.mc.weights(), s.mf.weights())
    out[0].square().mean().backward()
    done()
    assert rays.grad is None and not called
    assert s.emb.table.grad is not None and float(s.emb.table.grad.abs().max()) > 0
    freeze(s)


def test_frozen_field_gets_no_gradient(hn, monkeypatch):
    HF = hf()
    s = rc.scene(hn, dev=DEV)
    freeze(s)
    called = []
    monkeypatch.setattr(HF, "render_bwd", lambda *a, **k: called.append(1))
    target = torch.rand(B, 3, generator=torch.Generator().manual_seed(50))
    _, got, _ = fused_step(hn, s, rc.ray_batch(hn, B), 128, True, target)
    assert float(got.abs().max()) > 0
    assert not called, "render_bwd (table gradient, MLP-weight and scatter work) ran for a frozen field"
    assert all(p.grad is None for p in params(s))


def test_skip_dead_color_state_is_safe(hn, monkeypatch):
    """A skip_dead_color forward stores neither features nor masks for tiles
    without density; on a NaN-prefilled state the ray gradient is finite and
    bitwise the plain state's."""
    HF = hf()
    s = kind_scene(hn, B, "rand")
    cfg = HF.make_render_cfg(s.emb.grid(), True, False, True, scatter="binned")
    real_empty = torch.empty

    def nan_empty(*a, **k):
        t = real_empty(*a, **k)
        return t.fill_(float("nan")) if t.dtype == torch.float32 else t
    out = {}
    for skip in (False, True):
        if skip:
            monkeypatch.setattr(torch, "empty", nan_empty)
        fwd, st = forward_kind(HF, s, cfg, False, skip)
        monkeypatch.undo()
        grads = dict(g_rgb=2. * (fwd["rgb"] - s.target) / (3 * B), g_rgb0=2. * (fwd["rgb0"] - s.target) / (3 * B),
                     g_sparsity=torch.full((B,), 1e-3, device=DEV), g_sparsity0=torch.full((B,), 1e-3, device=DEV))
        # the feature tiles of the state (its ReLU mask words behind them are bit patterns, not floats)
        out[skip] = (HF.render_bwd_rays(st, grads), st.feat[:, :8 * 1024])
        done()
    assert torch.isnan(out[True][1]).any(), "the skipping forward stored every tile: nothing was tested"
    assert not torch.isnan(out[False][1]).any()
    assert torch.isfinite(out[True][0]).all() and float(out[True][0].abs().max()) > 0
    assert bits_equal(out[True][0], out[False][0])


# ---- refusals ----------------------------------------------------------------------
def test_ineligible_configurations_are_refused(hn):
    s = rc.scene(hn, dev=DEV)
    freeze(s)
    rays = rc.ray_batch(hn, B).to(DEV).requires_grad_(True)
    with pytest.raises(ValueError, match="not the fused HashNeRF configuration"):
        hn.render_rays(rays, ray_grad="fused", **dict(rc.render_kw(s, 128, True), N_samples=32))
    with pytest.raises(ValueError, match="not the fused HashNeRF configuration"):
        hn.render_rays(rays[:, :8], ray_grad="fused", **rc.render_kw(s, 128, True))     # no view directions
    # 64 importance samples where the cell index does not fit a bin: the float-atomic schedule
    fine = hn.HashEmbedder(rc.box(1.5), log2_hashmap_size=14, finest_resolution=8192).to(DEV)
    s.nq = hn.NetworkQuery(fine, hn.SHEncoder())
    with pytest.raises(ValueError, match="binned"):
        hn.render_rays(rays, ray_grad="fused", **rc.render_kw(s, 64, True))
    # the default is unchanged: such rays take the unfused composition
    ret = hn.render_rays(rays, **rc.render_kw(s, 64, True))
    ret["rgb_map"].sum().backward()
    done()
    assert rays.grad is not None and torch.isfinite(rays.grad).all()
