"""Gradients with respect to rays on the device: hn_encode_bwd_input, hn_sh_bwd
and hn_composite_bwd_inputs against autograd of the fp32 oracle on the CPU,
then the standalone-op composition end to end (pose, ray origins and
directions).  Every comparison is norm-relative over all entries; each prints
the device-against-oracle error next to the oracle's own fp32-against-fp64
error on the same inputs before it asserts.

Targets: 1e-5 for the encode and SH input gradients (fp32
arithmetic in autograd's order), 1e-4 for the composite's, 5e-4 end to end
(hn_mlp_bwd's dx runs on the 2-part bf16 split)."""
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gpu_support import DEV, SMALL_BOX, SMALL_FINEST, SMALL_T, bits_equal, blender_nets, done, hf, rel_close, rel_err
from input_grad_cases import input_grad_points, sh_dirs

pytestmark = pytest.mark.gpu

TOL_ENC = TOL_SH = 1e-5
TOL_COMP = 1e-4
TOL_E2E = 5e-4
# hn_encode_bwd's table gradient sums the same values by float atomics in an
# order that differs from launch to launch: DESIGN §1's bar for it
TOL_ATOMIC_ORDER = 1e-5
N_ENC = 4099          # no multiple of the 4 points of a wave, nor of 256 threads


def report(what, got, want32, want64):
    """Print and return the device's error against the fp32 oracle; beside it the
    fp32 oracle's own error against the float64 one."""
    err, floor = rel_err(got, want32), rel_err(want32, want64)
    print(f"[input-grad] {what}: device vs fp32 oracle {err:.3e}, fp32 vs fp64 oracle {floor:.3e}")
    return err


# ---- 1. hash encoding --------------------------------------------------------------
_ENC = {}


def enc_case(hn, oracle, n_levels):
    """Embedder of n_levels at T = 14 with a uniform table, 4,099 points inside
    the box, outside it and on its faces, a random dfeat; the features and d x
    of the fp32 and the float64 oracle.  Built once per level count."""
    if n_levels in _ENC:
        return _ENC[n_levels]
    torch.manual_seed(20 + n_levels)
    emb = hn.HashEmbedder(SMALL_BOX, n_levels=n_levels, log2_hashmap_size=SMALL_T,
                          finest_resolution=SMALL_FINEST).to(DEV)
    with torch.no_grad():
        emb.table.uniform_(-0.5, 0.5)
    x = input_grad_points(N_ENC)
    dfeat = torch.randn(N_ENC, 2 * n_levels, generator=torch.Generator().manual_seed(21))
    res = oracle.level_resolutions(n_levels, 16, SMALL_FINEST)
    feats, want = [], []
    for dt in (torch.float32, torch.float64):
        xr = x.clone().to(dt).requires_grad_(True)
        feat, _ = oracle.hash_encode(xr, emb.table.detach().cpu().to(dt), SMALL_BOX[0].to(dt), SMALL_BOX[1].to(dt),
                                     res, SMALL_T)
        feats.append(feat.detach())
        want.append(torch.autograd.grad(feat, xr, dfeat.to(dt))[0])
    c = _ENC[n_levels] = SimpleNamespace(emb=emb, x=x.to(DEV), dfeat=dfeat.to(DEV), dx32=want[0], dx64=want[1],
                                         feat32=feats[0])
    return c


def enc_grads(c, x_grad, table_grad):
    """One forward and backward of the embedder -> (feat, x.grad, table.grad)."""
    x = c.x.clone().requires_grad_(x_grad)
    c.emb.table.requires_grad_(table_grad)
    c.emb.table.grad = None
    try:
        feat, _ = c.emb(x)
        feat.backward(c.dfeat)
        done()
        return feat.detach(), x.grad, c.emb.table.grad
    finally:
        c.emb.table.requires_grad_(True)
        c.emb.table.grad = None


@pytest.mark.parametrize("n_levels", [16, 5])
def test_encode_dx_matches_oracle_autograd(hn, oracle, n_levels):
    c = enc_case(hn, oracle, n_levels)
    feat, dx, dtable = enc_grads(c, True, False)
    assert bits_equal(feat.cpu(), c.feat32), "features not bit-exact: the two sides may have picked other cells"
    assert dtable is None, "a frozen table got a gradient: hn_encode_bwd ran"
    assert torch.isfinite(dx).all()
    err = report(f"encode dx, L = {n_levels}", dx, c.dx32, c.dx64)
    assert err <= TOL_ENC, f"encode dx (L = {n_levels}): relative error {err:.3e}"


@pytest.mark.parametrize("n_levels", [16, 5])
def test_encode_dx_is_bitwise_repeatable(hn, oracle, n_levels):
    c = enc_case(hn, oracle, n_levels)
    a, b = enc_grads(c, True, False)[1], enc_grads(c, True, False)[1]
    assert bits_equal(a, b)


def test_encode_both_gradients_match_the_separate_ones(hn, oracle):
    c = enc_case(hn, oracle, 16)
    _, dx_only, none = enc_grads(c, True, False)
    _, no_dx, dtable_only = enc_grads(c, False, True)
    _, dx, dtable = enc_grads(c, True, True)
    assert none is None and no_dx is None
    assert bits_equal(dx, dx_only)
    assert float(dtable.abs().max()) > 0
    rel_close(dtable, dtable_only.cpu().numpy(), TOL_ATOMIC_ORDER, "table gradient beside dx")


def test_encode_no_points_is_a_noop(hn, oracle):
    c = enc_case(hn, oracle, 16)
    L = hn._lib
    dx = torch.full((4, 3), 7.0, device=DEV)
    assert L.lib().hn_encode_bwd_input(c.emb.grid(), L.ptr(c.x), 0, L.ptr(c.emb.table), L.ptr(c.dfeat), L.ptr(dx),
                                       L.stream(dx.device)) == 0
    done()
    assert bool((dx == 7.0).all())
    x = torch.zeros((0, 3), device=DEV, requires_grad=True)
    feat, _ = c.emb(x)
    feat.sum().backward()
    done()
    assert x.grad.shape == (0, 3)
    c.emb.table.grad = None


# ---- 2. spherical harmonics --------------------------------------------------------
def test_sh_ddirs_matches_oracle_autograd(hn, oracle):
    d = sh_dirs(1000)
    go = torch.randn(1000, 16, generator=torch.Generator().manual_seed(22))
    want = []
    for dt in (torch.float32, torch.float64):
        dr = d.clone().to(dt).requires_grad_(True)
        want.append(torch.autograd.grad(oracle.sh_encode(dr), dr, go.to(dt))[0])
    dd = d.to(DEV).requires_grad_(True)
    hn.SHEncoder()(dd).backward(go.to(DEV))
    done()
    assert torch.isfinite(dd.grad).all()
    err = report("SH d dirs", dd.grad, *want)
    assert err <= TOL_SH, f"SH d dirs: relative error {err:.3e}"


# ---- 3. raw2outputs ----------------------------------------------------------------
def comp_inputs(S, noise, dead_ray=None):
    """37 rays of S samples: raw ~ N(0, 1) (about half the sigmas under the
    ReLU), increasing z in [2, 6], un-normalised directions, upstream gradients
    of rgb, acc, depth, entropy and weights."""
    g = torch.Generator().manual_seed(30 + S)
    B = 37
    raw = torch.randn(B, S, 4, generator=g)
    z, _ = torch.sort(2.0 + 4.0 * torch.rand(B, S, generator=g), -1)
    rays_d = torch.randn(B, 3, generator=g) * 1.5
    nz = torch.randn(B, S, generator=g) * 0.5 if noise else None
    up = dict(rgb=torch.randn(B, 3, generator=g), acc=torch.randn(B, generator=g), depth=torch.randn(B, generator=g),
              ent=torch.randn(B, generator=g), weights=torch.randn(B, S, generator=g))
    if dead_ray is not None:
        raw[dead_ray, :, 3] = -raw[dead_ray, :, 3].abs()
        raw[dead_ray, ::7, 3] = 0.0
    return raw, z, rays_d, nz, up


def comp_oracle(oracle, raw, z, rays_d, nz, up, white, dt, keys):
    raw, z, rays_d = (t.clone().to(dt).requires_grad_(True) for t in (raw, z, rays_d))
    rgb, _, acc, weights, depth, ent = oracle.raw2outputs(raw, z, rays_d, None if nz is None else nz.to(dt), white)
    outs = dict(rgb=rgb, acc=acc, depth=depth, ent=ent, weights=weights)
    return torch.autograd.grad([outs[k] for k in keys], [raw, z, rays_d], [up[k].to(dt) for k in keys])


def comp_device(HF, raw, z, rays_d, nz, up, white, keys, ray_grad):
    raw = raw.to(DEV).requires_grad_(True)
    z, rays_d = (t.to(DEV).requires_grad_(ray_grad) for t in (z, rays_d))
    rgb, _, acc, weights, depth, ent = HF.CompositeFn.apply(raw, z, rays_d, None if nz is None else nz.to(DEV), white)
    outs = dict(rgb=rgb, acc=acc, depth=depth, ent=ent, weights=weights)
    got = torch.autograd.grad([outs[k] for k in keys], [raw, z, rays_d] if ray_grad else [raw],
                              [up[k].to(DEV) for k in keys])
    done()
    return got


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("S", [64, 192])
def test_composite_dz_and_drays_match_oracle_autograd(hn, oracle, S, white, noise):
    HF = hf()
    raw, z, rays_d, nz, up = comp_inputs(S, noise)
    keys = ("rgb", "acc", "depth", "ent", "weights")
    w32 = comp_oracle(oracle, raw, z, rays_d, nz, up, white, torch.float32, keys)
    w64 = comp_oracle(oracle, raw, z, rays_d, nz, up, white, torch.float64, keys)
    d_raw, d_z, d_rays = comp_device(HF, raw, z, rays_d, nz, up, white, keys, True)
    (d_raw_before,) = comp_device(HF, raw, z, rays_d, nz, up, white, keys, False)
    assert bits_equal(d_raw, d_raw_before), "d_raw changed beside the input gradients"
    tag = f"S = {S}, white = {white}, noise = {noise}"
    errs = [report(f"composite {n} ({tag})", a, b, c) for n, a, b, c in
            (("d_raw", d_raw, w32[0], w64[0]), ("d_z", d_z, w32[1], w64[1]), ("d_rays_d", d_rays, w32[2], w64[2]))]
    for n, e in zip(("d_raw", "d_z", "d_rays_d"), errs):
        assert e <= TOL_COMP, f"composite {n} ({tag}): relative error {e:.3e}"


@pytest.mark.parametrize("S", [64, 192])
def test_composite_ray_without_density_gets_finite_zeros(hn, oracle, S):
    """All sigma <= 0 on ray 5 (some exactly 0), no gradient on depth (0 / 0 there)."""
    HF = hf()
    raw, z, rays_d, nz, up = comp_inputs(S, False, dead_ray=5)
    keys = ("rgb", "acc", "ent", "weights")
    w32 = comp_oracle(oracle, raw, z, rays_d, nz, up, True, torch.float32, keys)
    d_raw, d_z, d_rays = comp_device(HF, raw, z, rays_d, nz, up, True, keys, True)
    for t in (d_raw, d_z, d_rays):
        assert torch.isfinite(t).all()
    assert bool((d_z[5] == 0).all()) and bool((d_rays[5] == 0).all())
    assert bool((w32[1][5] == 0).all()) and bool((w32[2][5] == 0).all())
    rel_close(d_z, w32[1].numpy(), TOL_COMP, "composite d_z, no depth gradient")
    rel_close(d_rays, w32[2].numpy(), TOL_COMP, "composite d_rays_d, no depth gradient")


# ---- 4. end to end -----------------------------------------------------------------
SPARSE_W = 1e-3


def render_module():
    return import_module("hashnerf_pytorch_amd.render")


def scene(hn):
    s = blender_nets(hn, SMALL_T, 3, box=SMALL_BOX, finest=SMALL_FINEST)
    s.nq = hn.NetworkQuery(s.emb, hn.SHEncoder())
    return s


def render_kw(s, ni, white):
    return dict(network_query_fn=s.nq, perturb=0., N_importance=ni, network_fine=s.mf, N_samples=64,
                network_fn=s.mc, white_bkgd=white, raw_noise_std=0.)


def record_fine_z(monkeypatch):
    """The z_vals of every raw2outputs call of render_rays' composition (the
    second one of a render_rays is the fine pass's sorted z)."""
    R = render_module()
    seen, inner = [], R.raw2outputs

    def recording(raw, z_vals, *a, **k):
        seen.append(z_vals.detach())
        return inner(raw, z_vals, *a, **k)
    monkeypatch.setattr(R, "raw2outputs", recording)
    return seen


def oracle_ray_grads(oracle, s, c2w, rays_of_pose, near, far, ni, white, target, z_fine, dt):
    """The oracle's training loss on the rays rays_of_pose(c2w) -> (o, d,
    viewdirs), its fine pass on the device's fine z (past sample_pdf's
    discontinuity); the gradients of the pose and of o and d."""
    c2w = c2w.detach().clone().to(dt).requires_grad_(True)
    o, d, vd = rays_of_pose(c2w)
    o.retain_grad()
    d.retain_grad()
    B = o.shape[0]
    rb = torch.cat([o, d, torch.full((B, 1), near, dtype=dt), torch.full((B, 1), far, dtype=dt), vd], -1)
    w = [{k: v.detach().cpu().to(dt) for k, v in zip(oracle.MLP_KEYS, m.weights())} for m in (s.mc, s.mf)]
    ret = oracle.render_rays(rb, w[0], w[1], s.emb.table.detach().cpu().to(dt), SMALL_BOX[0].to(dt),
                             SMALL_BOX[1].to(dt), oracle.level_resolutions(16, 16, SMALL_FINEST), SMALL_T,
                             N_importance=ni, u=torch.linspace(0., 1., ni).to(dt).expand(B, ni), white_bkgd=white,
                             z_fine=z_fine.cpu().to(dt))
    oracle.training_loss(ret, target.to(dt), SPARSE_W).backward()
    return c2w.grad, o.grad, d.grad


def test_pose_gradient_blender_rays(hn, oracle, monkeypatch):
    """32 rays of a 400 x 400 blender camera, 64 + 128, white background: the
    pose is a leaf, the rays come from it through get_rays."""
    s = scene(hn)
    _, K = hn.rays.blender_intrinsics(400, 400)
    pose = hn.pose_spherical(30.0, -30.0, 4.0)[:3, :4]
    sel = torch.randperm(400 * 400, generator=torch.Generator().manual_seed(40))[:32]
    target = torch.rand(32, 3, generator=torch.Generator().manual_seed(41))

    def rays_of(get_rays):
        def f(c2w):
            o, d = get_rays(400, 400, K, c2w)
            o, d = o.reshape(-1, 3)[sel.to(o.device)], d.reshape(-1, 3)[sel.to(o.device)]
            return o, d, d / torch.norm(d, dim=-1, keepdim=True)
        return f
    seen = record_fine_z(monkeypatch)
    c2w = pose.to(DEV).requires_grad_(True)
    o, d, _ = rays_of(hn.get_rays)(c2w)
    o.retain_grad()
    d.retain_grad()
    rgb, _, _, ex = hn.render(400, 400, K, rays=(o, d), use_viewdirs=True, ndc=False, near=2., far=6.,
                              **render_kw(s, 128, True))
    loss, _ = hn.training_loss(rgb, ex, target.to(DEV), SPARSE_W)
    loss.backward()
    done()
    assert len(seen) == 2 and seen[1].shape == (32, 192)
    want = [oracle_ray_grads(oracle, s, pose, rays_of(oracle.get_rays), 2., 6., 128, True, target, seen[1], dt)
            for dt in (torch.float32, torch.float64)]
    names = ("c2w", "rays_o", "rays_d")
    errs = [report(f"blender 64 + 128: {n}", g, a, b) for n, g, a, b in zip(names, (c2w.grad, o.grad, d.grad), *want)]
    for n, g, e in zip(names, (c2w.grad, o.grad, d.grad), errs):
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, n
        assert e <= TOL_E2E, f"blender 64 + 128: d loss / d {n}: relative error {e:.3e}"


def test_pose_gradient_ndc_image(hn, oracle, monkeypatch):
    """render(H, W, K, c2w=pose) of an 11 x 14 forward-facing camera through NDC
    rays, 64 + 64: the pose's gradient through get_rays, get_ndc_rays and the
    view directions."""
    s = scene(hn)
    H, W, focal = 11, 14, 12.0
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    pose = torch.tensor([[0.98, 0.05, -0.19, 0.3], [-0.04, 0.99, 0.06, -0.2], [0.19, -0.05, 0.98, 0.4]])
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(42))
    get_ndc = hn.rays.get_ndc_rays       # torch glue, pinned to the reference by test_rays_golden

    def rays_of(c2w):
        o, d = oracle.get_rays(H, W, K, c2w)
        vd = (d / torch.norm(d, dim=-1, keepdim=True)).reshape(-1, 3)
        o, d = get_ndc(H, W, K[0][0], 1., o, d)
        return o.reshape(-1, 3), d.reshape(-1, 3), vd
    seen = record_fine_z(monkeypatch)
    c2w = pose.to(DEV).requires_grad_(True)
    rgb, _, _, ex = hn.render(H, W, K, c2w=c2w, use_viewdirs=True, ndc=True, near=0., far=1.,
                              **render_kw(s, 64, False))
    loss, _ = hn.training_loss(rgb, ex, target.to(DEV), SPARSE_W)
    loss.backward()
    done()
    assert len(seen) == 2 and seen[1].shape == (H * W, 128)
    want = [oracle_ray_grads(oracle, s, pose, rays_of, 0., 1., 64, False, target.reshape(-1, 3), seen[1], dt)
            for dt in (torch.float32, torch.float64)]
    err = report("NDC 64 + 64: c2w", c2w.grad, want[0][0], want[1][0])
    assert torch.isfinite(c2w.grad).all() and float(c2w.grad.abs().max()) > 0
    assert err <= TOL_E2E, f"NDC 64 + 64: d loss / d c2w: relative error {err:.3e}"


def small_ray_batch(hn, B=32):
    _, K = hn.rays.blender_intrinsics(400, 400)
    o, d = hn.get_rays(400, 400, K, hn.pose_spherical(30.0, -30.0, 4.0)[:3, :4].to(DEV))
    sel = torch.randperm(400 * 400, generator=torch.Generator().manual_seed(43))[:B].to(DEV)
    o, d = o.reshape(-1, 3)[sel], d.reshape(-1, 3)[sel]
    return torch.cat([o, d, torch.full((B, 1), 2., device=DEV), torch.full((B, 1), 6., device=DEV),
                      d / d.norm(dim=-1, keepdim=True)], -1).contiguous()


def test_render_rays_gives_a_ray_gradient(hn):
    s = scene(hn)
    rays = small_ray_batch(hn).requires_grad_(True)
    ret = hn.render_rays(rays, **render_kw(s, 128, True))
    (ret["rgb_map"].square().mean() + ret["rgb0"].square().mean()).backward()
    done()
    assert rays.grad is not None and rays.grad.shape == rays.shape
    assert torch.isfinite(rays.grad).all() and float(rays.grad[:, :6].abs().max()) > 0


def test_render_rays_without_ray_grad_is_the_fused_path(hn):
    """No grad on the rays: bitwise the fused kernels' outputs, as before."""
    HF, R = hf(), render_module()
    s = scene(hn)
    rays = small_ray_batch(hn)
    ret = hn.render_rays(rays, retraw=True, **render_kw(s, 128, True))
    cfg = HF.make_render_cfg(s.emb.grid(), True, False, False, n_importance=128)
    u = torch.linspace(0., 1., 128, device=DEV).expand(32, 128)
    direct = HF.render_rays_fused(cfg, rays, R._linspace_cached(64, rays.device), None, u, None, None, s.emb.table,
                                  s.mc.weights(), s.mf.weights())
    done()
    names = ("rgb_map", "depth_map", "acc_map", "sparsity_loss", "rgb0", "depth0", "acc0", "sparsity_loss0", "z_std",
             "raw")
    assert set(ret) == set(names)
    for n, t in zip(names, direct):
        assert bits_equal(ret[n], t), n


def test_whole_image_kernels_refuse_pose_gradients(hn):
    """The whole-image kernels form no gradient: poses that require grad are
    refused under grad mode, before any launch, and rendered under no_grad."""
    HF = hf()
    s = scene(hn)
    _, K = hn.rays.blender_intrinsics(8, 8)
    poses = hn.pose_spherical(30.0, -30.0, 4.0)[None, :3, :4].to(DEV).requires_grad_(True)
    cfg = HF.make_render_cfg(s.emb.grid(), True, False, False, n_importance=128)
    args = (cfg, 8, 8, K, poses, 2., 6., s.emb.table.detach(), [w.detach() for w in s.mc.weights() + s.mf.weights()])
    for fn in (HF.render_image, HF.render_views):
        with pytest.raises(ValueError, match="no gradient"):
            fn(*args)
    with torch.no_grad():
        rgb, _, _ = HF.render_views(*args)
    done()
    assert rgb.shape == (1, 8, 8, 3) and not rgb.requires_grad and torch.isfinite(rgb).all()


# ---- 5. parameters still learn -----------------------------------------------------
def test_parameter_gradients_unchanged_by_ray_grad(hn):
    """The standalone-op composition with the table and the weights requiring
    grad: their gradients with grad on the rays too are those without (the
    same kernels on the same upstream values; only float atomics reorder)."""
    R = render_module()
    s = scene(hn)
    params = [s.emb.table] + list(s.mc.weights()) + list(s.mf.weights())
    target = torch.rand(32, 3, generator=torch.Generator().manual_seed(44)).to(DEV)
    got = []
    for ray_grad in (False, True):
        rays = small_ray_batch(hn).requires_grad_(ray_grad)
        for p in params:
            p.grad = None
        ret = R._render_rays_unfused(rays, s.mc, s.nq, 64, False, False, 0., 128, s.mf, True, 0., False)
        loss, _ = hn.training_loss(ret["rgb_map"], ret, target, SPARSE_W)
        loss.backward()
        done()
        assert (rays.grad is not None) == ray_grad
        got.append([p.grad.clone() for p in params])
    for i, (a, b) in enumerate(zip(*got)):
        assert float(a.abs().max()) > 0
        rel_close(b, a.cpu().numpy(), TOL_ATOMIC_ORDER, f"parameter {i} (0 = table) with ray grad on")
