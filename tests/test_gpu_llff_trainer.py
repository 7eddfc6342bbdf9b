"""Trainer on the LLFF configuration: bounds and the NDC step come from the
data and create_nerf's kwargs, the explicit and autograd modes get final NDC
rays from the samplers, and every fusion holds as for blender.

The LLFF configuration: default_args(dataset_type="llff", N_importance=64,
raw_noise_std=1., white_bkgd=False, no_batching=False, precrop_iters=0) on
SyntheticLLFF.  Sizes: T = 14, N_rand 64, SyntheticLLFF(20, 20, 4) (a pool of
1,600 rays); the oracle step draws 32 rays, as test_gpu_dp.py's."""
from importlib import import_module

import numpy as np
import pytest
import torch

from gpu_support import bits_equal, done
from pool_order_key import pool_key, pool_perm

pytestmark = pytest.mark.gpu
DEV = "cuda"
_DATA = {}


def llff_data():
    if "d" not in _DATA:
        from hashnerf_pytorch_amd.train import SyntheticLLFF
        _DATA["d"] = SyntheticLLFF(20, 20, 4, DEV, seed=0)
    return _DATA["d"]


def llff_trainer(mode="explicit", seed=3, pool_order=0, **over):
    from hashnerf_pytorch_amd.train import Trainer, default_args
    kw = dict(dataset_type="llff", N_importance=64, raw_noise_std=1., white_bkgd=False, no_batching=False,
              precrop_iters=0, N_rand=64, log2_hashmap_size=14, sparse_loss_weight=1e-3, tv_loss_weight=1e-4,
              tv_until=10)
    kw.update(over)
    tr = Trainer(default_args(**kw), llff_data(), DEV, seed=seed, mode=mode, pool_order=pool_order)
    assert tr.ndc == (20, 20, llff_data().K[0][0]) and (tr.near, tr.far) == (0., 1.)
    assert "ndc" not in tr.kw_train                            # create_nerf leaves render()'s default: NDC on
    return tr


def weights(tr):
    return tr.kw_train["network_fn"].weights() + tr.kw_train["network_fine"].weights()


# ---- (a) the sampler's NDC step against render()'s own -----------------------------------
def test_sampler_ndc_step_is_renders(hn):
    """Step 1's batch of the LLFF trainer, rendered by render_rays, against
    render(H, W, K, rays=<the world rays of the same pool positions>,
    ndc=True, near=0., far=1., ...) from the same generator state (so both
    draw the trainer's t_rand and u, then the same noise): rgb_map and rgb0
    bitwise."""
    R = import_module("hashnerf_pytorch_amd.render")
    d = llff_data()
    tr, tw = llff_trainer(), llff_trainer()
    tw.ndc = None                                              # the same pool positions as world rays
    torch.cuda.manual_seed(41)
    batch = tr.draw_batch(1)
    world = tw.draw_batch(1)
    rays, wr = batch["rays"], world["rays"]
    assert rays.shape == (64, 11) and bits_equal(rays[:, 6:11], wr[:, 6:11])
    assert bits_equal(batch["target"], world["target"]) and not bits_equal(rays[:, 0:6], wr[:, 0:6])
    kw = {k: v for k, v in tr.kw_train.items() if k not in ("use_viewdirs", "embed_fn")}
    assert kw["raw_noise_std"] == 1. and kw["perturb"] > 0. and kw["N_importance"] == 64
    with torch.no_grad():
        torch.cuda.manual_seed(41)
        t_rand, u = torch.rand((64, 64), device=DEV), torch.rand((64, 64), device=DEV)
        assert torch.equal(t_rand, batch["t_rand"]) and torch.equal(u, batch["u"])
        torch.cuda.manual_seed(41)
        a = R.render_rays(rays, retraw=True, **kw)
        torch.cuda.manual_seed(41)
        rgb, depth, acc, ex = R.render(d.H, d.W, d.K, rays=(wr[:, 0:3], wr[:, 3:6]), ndc=True, near=0., far=1.,
                                       retraw=True, **tr.kw_train)
    print("max |rgb - rgb'|", float((a["rgb_map"] - rgb).abs().max()), "max |rgb0 - rgb0'|",
          float((a["rgb0"] - ex["rgb0"]).abs().max()))
    assert bool(torch.isfinite(rgb).all()) and float(rgb.abs().max()) > 0.
    assert bits_equal(a["rgb_map"], rgb), "rgb_map"
    assert bits_equal(a["rgb0"], ex["rgb0"]), "rgb0"
    done()


# ---- (b) explicit against autograd -------------------------------------------------------
def test_explicit_matches_autograd_llff(hn):
    """The two modes over 4 steps of the LLFF configuration, the tolerances of
    test_trainer_explicit_matches_autograd_64 (loss relative 1e-6, the MSE
    equal) at every step; step 1's gradients as there."""
    res = {}
    for mode in ("explicit", "autograd"):
        tr = llff_trainer(mode, seed=0)
        tr.fuse_table_step = False           # keep the table gradient to compare
        torch.manual_seed(123)
        out = []
        for k in range(4):
            loss, mse = tr.step()
            out.append((float(loss.detach()), float(mse)))
            if k == 0:
                g = (tr.embed_fn.table.grad.clone(), [p.grad.clone() for p in weights(tr)])
        res[mode] = (out, g)
        if mode == "explicit":
            assert tr._cfg.n_importance == 64 and tr.use_batching
    for k, ((le, me), (la, ma)) in enumerate(zip(res["explicit"][0], res["autograd"][0])):
        print(f"step {k + 1}: loss explicit {le!r} autograd {la!r} rel {abs(le - la) / abs(la):.3e}; mse {me!r} {ma!r}")
    te, we = res["explicit"][1]
    ta, wa = res["autograd"][1]
    print("table gradient rel", float((te - ta).norm() / ta.norm()))
    for k, ((le, me), (la, ma)) in enumerate(zip(res["explicit"][0], res["autograd"][0])):
        assert abs(le - la) <= 1e-6 * abs(la), k
        if k == 0:
            assert me == ma
    assert float((te - ta).norm() / ta.norm()) < 1e-5
    for x, y in zip(we, wa):
        torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-8)
    done()


# ---- (c) the fusions, per-image draws ----------------------------------------------------
_TRAJ = {}


def trajectory(off=None):
    """6 self-driven steps of the LLFF configuration with no_batching=True,
    every fusion on or one turned off."""
    if off in _TRAJ:
        return _TRAJ[off]
    tr = llff_trainer(no_batching=True, tv_until=4)
    if off is not None:
        assert getattr(tr, off) is True
        setattr(tr, off, False)
    torch.manual_seed(11)
    losses = [float(tr.step()[0]) for _ in range(6)]
    done()
    fuses = tr._fuses_next_batch()
    assert tr.draw_batch()["rays"][:, 6:8].tolist() == [[0., 1.]] * 64
    _TRAJ[off] = (losses, tr.embed_fn.table.detach().clone(), [p.detach().clone() for p in weights(tr)], fuses)
    return _TRAJ[off]


@pytest.mark.parametrize("off", ["fuse_table_step", "fuse_loss", "fuse_mlp_step", "fuse_next_batch", "fuse_prepass"])
def test_fusions_same_trajectory_llff(hn, off):
    """As test_trainer_fusions_same_trajectory_64: the table and the ten
    weights torch.equal after 6 steps; the next batch is drawn inside the
    backward for an LLFF run exactly as for blender."""
    a, b = trajectory(), trajectory(off)
    assert a[3] is True
    assert b[3] is (off not in ("fuse_next_batch", "fuse_table_step"))
    np.testing.assert_allclose(b[0], a[0], rtol=1e-6)
    assert torch.equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)
    assert len(set(a[0])) == 6


# ---- (d) pool_order ----------------------------------------------------------------------
def test_pool_order_llff(hn):
    """pool_order=1 against 0 over 4 steps: each batch is the other's rows in
    ascending (key, position), the key that of the NDC row (near 0, far 1) in
    the embedder's box -- bbox_for_llff's --, and the losses agree to
    test_trainer_pool_order's 1e-6.  As there, without jitter, raw noise or
    TV: those are drawn per row, so a reordered batch would meet other random
    numbers and no two losses could be compared."""
    d = llff_data()
    make = lambda order: llff_trainer(pool_order=order, perturb=0., raw_noise_std=0., tv_loss_weight=0.)
    tr0, tr1 = make(0), make(1)
    g = tr1.embed_fn.grid()
    box = (list(g.box_min), list(g.box_max))
    want = hn.bbox_for_llff(d.poses, [d.H, d.W, d.focal])
    assert box[0] == [float(v) for v in want[0]] and box[1] == [float(v) for v in want[1]]
    for i in range(1, 5):
        b0, b1 = tr0.draw_batch(i), tr1.draw_batch(i)
        keys, _ = pool_key(b0["rays"].cpu().numpy(), box[0], box[1], 0., 1.)
        perm = pool_perm(keys)
        assert sorted(perm.tolist()) == list(range(64)) and not np.array_equal(perm, np.arange(64))
        pt = torch.from_numpy(perm).to(DEV)
        assert bits_equal(b1["rays"], b0["rays"][pt]) and bits_equal(b1["target"], b0["target"][pt])
        l0, l1 = float(tr0.step(i, b0)[0]), float(tr1.step(i, b1)[0])
        print(f"step {i}: loss pool_order=0 {l0!r}  pool_order=1 {l1!r}  rel {abs(l1 - l0) / abs(l0):.3e}")
        assert np.isfinite(l0) and abs(l1 - l0) <= 1e-6 * abs(l0), i
    done()


# ---- (e) one step against the oracle -----------------------------------------------------
def test_one_step_gradient_vs_oracle_llff(hn, oracle):
    """test_gpu_dp.test_trainer_one_rank_gradient_vs_oracle on the LLFF
    configuration: the explicit step's loss and table / weight gradients
    against the oracle's autograd on the trainer's own batch (NDC rays, near 0,
    far 1, raw noise, black background), fine pass on the device's fine z.
    Its bar: 5e-4 relative."""
    from hashnerf_pytorch_amd import functional as HF
    O = oracle
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))
    tr = llff_trainer(N_rand=32, seed=0, tv_until=10 ** 6)
    tr.fuse_table_step = False
    e = tr.embed_fn
    with torch.no_grad():    # a trained-like table, as there
        e.table.uniform_(-0.5, 0.5, generator=torch.Generator(device=DEV).manual_seed(2))
    tab0 = e.table.detach().cpu().clone()
    nets = (tr.kw_train["network_fn"], tr.kw_train["network_fine"])
    w0 = [[p.detach().cpu().clone() for p in n.weights()] for n in nets]
    batch = tr.draw_batch(1)
    assert bool((batch["rays"][:, 6] == 0.).all()) and bool((batch["rays"][:, 7] == 1.).all())
    torch.cuda.manual_seed(99)               # the step's two randn draws, coarse then fine
    HF.DEBUG_KEEP = True
    try:
        lo, _ = tr._fused_forward_backward(1, batch)
    finally:
        HF.DEBUG_KEEP = False
    torch.cuda.manual_seed(99)
    noise_c = (torch.randn((32, 64), device=DEV) * 1.).cpu()
    noise_f = (torch.randn((32, 128), device=DEV) * 1.).cpu()
    z_fine = HF.LAST["z_fine"].cpu()
    assert z_fine.shape == (32, 128)
    g_table = e.table.grad.detach().cpu().clone()
    g_mlp = [p.grad.detach().cpu().clone() for p in weights(tr)]
    box = tuple(torch.as_tensor(v, dtype=torch.float32).cpu() for v in tr.data.bounding_box)
    tab = tab0.clone().requires_grad_(True)
    wc = {k: v.clone().requires_grad_(True) for k, v in zip(O.MLP_KEYS, w0[0])}
    wf = {k: v.clone().requires_grad_(True) for k, v in zip(O.MLP_KEYS, w0[1])}
    T = int(e.log2_hashmap_size)
    ret = O.render_rays(batch["rays"].cpu(), wc, wf, tab, box[0], box[1], O.level_resolutions(16, 16, 512), T,
                        N_importance=64, t_rand=batch["t_rand"].cpu(), u=batch["u"].cpu(), noise_c=noise_c,
                        noise_f=noise_f, white_bkgd=False, z_fine=z_fine)
    cubes, mv = batch["tv"]
    tv = sum(O.total_variation_loss(tab[l], l, mv[l].cpu(), T) for l in range(16))
    loss = O.training_loss(ret, batch["target"].cpu(), 1e-3) + 1e-4 * tv
    loss.backward()
    errs = [rel(g_table, tab.grad)] + [rel(a, r) for a, r in zip(
        g_mlp, [wc[k].grad for k in O.MLP_KEYS] + [wf[k].grad for k in O.MLP_KEYS])]
    loss = loss.detach()
    el = abs(float(lo) - float(loss)) / abs(float(loss))
    print("loss", float(lo), float(loss), f"rel {el:.3e}", "gradients rel", " ".join(f"{x:.2e}" for x in errs))
    assert el <= 5e-4, f"loss: relative {el:.3e}"
    assert errs[0] <= 5e-4, f"table gradient: relative {errs[0]:.3e}"
    for k, err in enumerate(errs[1:]):
        assert err <= 5e-4, f"MLP gradient {k}: relative {err:.3e}"
    done()


# ---- (f) bounds from the data ------------------------------------------------------------
class _Captured(Exception):
    pass


@pytest.mark.parametrize("bounds", [(0.1, 10.), None])
def test_bounds_come_from_the_data(hn, monkeypatch, bounds):
    """A data object with near = 0.1, far = 10. (the scannet config's) and
    ndc off: every mode's rays carry them -- the explicit and autograd modes'
    from the sampler, the eager mode's as render() packs them; a
    SyntheticBlender, which names none, still gets (2., 6.)."""
    from hashnerf_pytorch_amd.train import SyntheticBlender, Trainer, default_args
    R = import_module("hashnerf_pytorch_amd.render")
    data = SyntheticBlender(20, 20, 3, DEV, seed=0)
    if bounds:
        data.near, data.far = bounds
    want = list(bounds or (2., 6.))
    seen = {}

    def capture(rays_, *a, **kw):
        seen["rays"] = rays_
        raise _Captured

    for mode in ("explicit", "autograd", "eager"):
        for no_batching in ((True,) if mode == "eager" else (True, False)):
            tr = Trainer(default_args(N_rand=37, log2_hashmap_size=12, precrop_iters=0, no_batching=no_batching), data,
                         DEV, seed=1, mode=mode)
            assert tr.ndc is None and tr.kw_train["ndc"] is False
            if mode == "explicit":
                rays = tr.draw_batch(1)["rays"]
            elif mode == "autograd":
                rays = tr._draw_rays(1)[0]
            else:
                monkeypatch.setattr(R, "render_ray_batch", capture)
                with pytest.raises(_Captured):
                    tr.step()
                monkeypatch.undo()
                rays = seen["rays"]
            assert rays.shape == (37, 11)
            assert torch.equal(rays[:, 6:8], torch.tensor([want], dtype=torch.float32, device=DEV).expand(37, 2)), \
                (mode, no_batching)
            # world rays: the origin is the camera's
            assert bool((rays[:, 0:3].norm(dim=-1) - 4.0).abs().max() < 1e-4)
