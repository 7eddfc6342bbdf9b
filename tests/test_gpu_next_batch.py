"""hn_render_bwd_args.next_batch: the next step's Morton draw and uniform
draws made by extra workgroups of the binned backward's lists and placement
launches.  The same device functions run on the same seeds as in
hn_sample_batch_morton, and the backward's own workgroups are untouched, so
everything is compared bitwise: the drawn values against the stand-alone
sampler, the step's results against the step without a job, and a Trainer's
trajectory with Trainer.fuse_next_batch on against off.

Shapes (T=14): a 37x29 image with the window (3, 5, 20, 13) -- not a power of
two, a partially filled Morton tile -- and an 8x8 image uncropped; 1, 5, 37,
256 rays where the window holds them and the whole window once; rendering
batches of 1, 5, 37, 256 rays (one lists workgroup at 256, with and without
the stamp workgroup); no uniform draws and two (tiles with a tail)."""
import ctypes as C

import pytest
import torch

from gpu_support import bits_equal, forward_kind as forward, kind_scene as scene, loss_of, step_coeffs, ws_offsets

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BS = (1, 5, 37, 256)
# name -> (H, W, crop (y0, x0, h, w)), the job's n_rays
WINDOWS = {"crop20x13": ((37, 29, (3, 5, 20, 13)), (1, 5, 37, 256, 20 * 13)),
           "full8x8": ((8, 8, (0, 0, 8, 8)), (1, 5, 37, 8 * 8))}
_IMAGES = {}


def camera(hn, name):
    """Image, pose and intrinsics of a window's camera (built once, left unchanged)."""
    if name not in _IMAGES:
        H, W, crop = WINDOWS[name][0]
        g = torch.Generator().manual_seed(3 + H)
        _, K = hn.rays.blender_intrinsics(H, W)
        _IMAGES[name] = (torch.rand((H, W, 3), generator=g).to(DEV), hn.pose_spherical(40.0, -25.0, 4.0).to(DEV), K,
                         crop)
    return _IMAGES[name]


def make_job(HF, cam, n, n_uni, seed=0x1234567):
    """The job and, from the same generator state, nothing launched yet."""
    image, c2w, K, crop = cam
    torch.cuda.manual_seed(77)
    nb = HF.next_batch(image, c2w, n, K, 2., 6., crop, seed, uniforms=[(n, 64), (n, 128)][:n_uni] or None)
    for t in nb.out:
        t.fill_(float("nan"))
    return nb


def stand_alone(HF, cam, n, n_uni, seed=0x1234567):
    image, c2w, K, crop = cam
    torch.cuda.manual_seed(77)
    return HF.sample_rays(image, c2w, n, K, 2., 6., crop, seed, order=1, uniforms=[(n, 64), (n, 128)][:n_uni] or None)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("window", sorted(WINDOWS))
def test_job_draws_stand_alone_values_bitwise(hn, window, B):
    """One forward + render_bwd with a job; the job's rays / target / t_rand /
    u are torch.equal to hn_sample_batch_morton's for the same arguments, and
    the default generator ends where the stand-alone call leaves it.  Both
    forms of the lists launch: after the pre-pass, and as the backward's first
    kernel (prepass_done, one more workgroup ahead of the lists')."""
    from hashnerf_pytorch_amd import functional as HF
    s = scene(hn, B, "rand")
    cfg = HF.make_render_cfg(s.emb.grid(), True, False, True, scatter="binned")
    cam = camera(hn, window)
    for n in WINDOWS[window][1]:
        for n_uni in (0, 2):
            ref = stand_alone(HF, cam, n, n_uni)
            off_ref = torch.cuda.default_generators[0].get_offset()
            for fused in (False, True):
                out, st = forward(HF, s, cfg, fused, skip_dead=True)
                nb = make_job(HF, cam, n, n_uni)
                assert torch.cuda.default_generators[0].get_offset() == off_ref
                HF.render_bwd(st, {}, torch.empty_like(s.table), HF.zeros_like_all(s.ws), overwrite=True,
                              overwrite_mlp=True, loss=loss_of(s, out, torch.empty(4, device=DEV)),
                              prepass_done=fused, next_batch=nb)
                assert len(nb.out) == len(ref) == 2 + n_uni
                for k, (a, b) in enumerate(zip(nb.out, ref)):
                    assert a.shape == b.shape and a.data_ptr() != b.data_ptr()
                    assert torch.equal(a, b), (n, n_uni, fused, k)
    assert not torch.isnan(ref[0]).any()


def run_step(hn, HF, B, bin_cap, job):
    """One training step's backward (fused loss, table step, MLP steps, repack)
    on clones of the scene's parameters; everything it leaves behind."""
    s = scene(hn, B, "rand")
    cfg = HF.make_render_cfg(s.emb.grid(), True, False, True, scatter="binned")
    cfg.bin_cap = bin_cap
    g = torch.Generator().manual_seed(9)
    ws = [w.clone() for w in s.ws]
    table = s.table.clone()
    m = (torch.rand(table.shape, generator=g) - 0.5).to(DEV) * 1e-3
    v = torch.rand(table.shape, generator=g).to(DEV) * 1e-6
    wm = [(torch.rand(w.shape, generator=g) - 0.5).to(DEV) * 1e-3 for w in ws]
    wv = [torch.rand(w.shape, generator=g).to(DEV) * 1e-6 for w in ws]
    out, st = HF.render_fwd(cfg, s.rays, s.t_vals, s.t_rand, s.u, None, None, table, ws, True,
                            skip_dead_color=True, loss=dict(target=s.target, world=1, sparse_w=1e-3))
    lo = torch.empty(4, device=DEV)
    dws = HF.zeros_like_all(ws)
    nb = make_job(HF, camera(hn, "crop20x13"), 37, 2) if job else None
    HF.render_bwd(st, {}, None, dws, overwrite_mlp=True, loss=loss_of(s, out, lo),
                  table_step=(table, m, v, step_coeffs()), prepass_done=True,
                  mlp_step=[(p, a, b, step_coeffs()) for p, a, b in zip(ws, wm, wv)], repack=True, next_batch=nb)
    torch.cuda.synchronize()
    packed = st.wsb[:ws_offsets(B).slab].view(torch.float32).clone()
    return dict(lo=lo, table=table, m=m, v=v, packed=packed, ws=ws, wm=wm, wv=wv, dws=dws), nb


@pytest.mark.parametrize("bin_cap", [0, 64])
@pytest.mark.parametrize("B", [37, 256])
def test_step_with_job_bitwise(hn, B, bin_cap):
    """The same step with and without a job: loss, table, m, v, the ten
    weights (and their moments and gradients) and their packed copies are
    torch.equal.  bin_cap = 64 makes records spill, so the placement
    workgroups really place beside the emit workgroups: one 64-sample unit
    makes up to 64 x 16 levels x 4 corner rows = 4,096 records for the 32 bins
    of T = 14, twice what 32 regions of 64 hold."""
    from hashnerf_pytorch_amd import functional as HF
    (a, _), (b, nb) = run_step(hn, HF, B, bin_cap, False), run_step(hn, HF, B, bin_cap, True)
    for k in ("lo", "table", "m", "v", "packed"):
        assert bits_equal(a[k], b[k]), k
    for k in ("ws", "wm", "wv", "dws"):
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert bits_equal(x, y), (k, i)
    assert not bits_equal(a["table"], scene(hn, B, "rand").table)       # the step stepped
    for x, y in zip(nb.out, stand_alone(HF, camera(hn, "crop20x13"), 37, 2)):
        assert torch.equal(x, y)


def trajectory(hn, monkeypatch, fuse, explicit_at=()):
    from hashnerf_pytorch_amd import functional as HF
    from hashnerf_pytorch_amd.train import SyntheticBlender, Trainer, default_args
    data = SyntheticBlender(48, 48, 3, DEV, seed=0)
    args = default_args(N_rand=256, log2_hashmap_size=13, tv_loss_weight=1e-4, tv_until=5, precrop_iters=3,
                        sparse_loss_weight=1e-3)
    tr = Trainer(args, data, DEV, seed=5)
    assert tr.fuse_next_batch is True                     # the default
    tr.fuse_next_batch = fuse
    calls = dict(jobs=0, samplers=0)
    real_bwd, real_sample = HF.render_bwd, HF.sample_rays

    def bwd(*a, **kw):
        calls["jobs"] += kw.get("next_batch") is not None
        return real_bwd(*a, **kw)

    def sample(*a, **kw):
        calls["samplers"] += 1
        return real_sample(*a, **kw)

    monkeypatch.setattr(HF, "render_bwd", bwd)
    monkeypatch.setattr(HF, "sample_rays", sample)
    torch.manual_seed(17)
    losses = []
    for k in range(1, 9):
        if k in explicit_at:
            b = tr.draw_batch(k)
            losses.append(float(tr.step(k, b)[0]))
        else:
            losses.append(float(tr.step()[0]))
    monkeypatch.setattr(HF, "render_bwd", real_bwd)
    monkeypatch.setattr(HF, "sample_rays", real_sample)
    torch.cuda.synchronize()
    HF.L.check_device_faults()
    table = tr.embed_fn.table
    ost = tr.optimizer.state
    return dict(losses=losses, table=table.detach().clone(), m=ost[table]["exp_avg"].clone(),
                v=ost[table]["exp_avg_sq"].clone(), ws=[p.detach().clone() for p in tr._ws],
                wm=[ost[p]["exp_avg"].clone() for p in tr._ws], calls=calls, tr=tr)


def test_trainer_trajectory_bitwise(hn, monkeypatch):
    """8 self-driven steps (precrop through step 2, TV through step 5: both
    windows change inside the run) with fuse_next_batch on against off, and
    with explicit steps mixed in (b = draw_batch(i); step(i, b)): every
    step's loss and the final table / m / v / weights are torch.equal."""
    off = trajectory(hn, monkeypatch, False)
    on = trajectory(hn, monkeypatch, True)
    mixed = trajectory(hn, monkeypatch, True, explicit_at=(4, 7))
    assert off["calls"] == dict(jobs=0, samplers=8)
    assert on["calls"] == dict(jobs=8, samplers=1)        # only the first batch has no step before it
    # an explicit step takes the pending batch and draws none; the step after it samples again
    assert mixed["calls"] == dict(jobs=6, samplers=3)
    for r in (on, mixed):
        assert r["losses"] == off["losses"]
        for k in ("table", "m", "v"):
            assert torch.equal(r[k], off[k]), k
        for k in ("ws", "wm"):
            for x, y in zip(r[k], off[k]):
                assert torch.equal(x, y), k
    # the batch of step 9 is pending: handed out for 9, refused for any other step
    tr = on["tr"]
    with pytest.raises(RuntimeError, match="step 9"):
        tr.draw_batch(12)
    assert tr.draw_batch()["rays"].shape == (256, 11)


@pytest.mark.parametrize("case", ["atomic", "n_rays"])
def test_refused_job_queues_nothing(hn, case):
    """A job with the float-atomic schedule, and a job with more rays than
    its window: hn_render_bwd returns HN_E_SHAPE before any launch -- the
    job's outputs, the gradients and the loss are untouched and no device
    fault bit is set."""
    from hashnerf_pytorch_amd import functional as HF
    B = 37
    s = scene(hn, B, "rand")
    cfg = HF.make_render_cfg(s.emb.grid(), True, False, True, scatter="atomic" if case == "atomic" else "binned")
    assert hn._lib.lib().hn_render_scatter_mode(cfg, B) == (1 if case == "atomic" else 2)
    cam = camera(hn, "crop20x13")
    out, st = forward(HF, s, cfg, False, skip_dead=False)
    nb = make_job(HF, cam, 20 * 13 + 1 if case == "n_rays" else 37, 2)
    d_table = torch.full_like(s.table, 7.0)
    dws = HF.zeros_like_all(s.ws)
    lo = torch.full((4,), -1.0, device=DEV)
    with pytest.raises(RuntimeError, match=r"status 2"):
        HF.render_bwd(st, {}, d_table, dws, overwrite=True, overwrite_mlp=True, loss=loss_of(s, out, lo),
                      next_batch=nb)
    torch.cuda.synchronize()
    for t in nb.out:
        assert bool(torch.isnan(t).all())
    assert bool((d_table == 7.0).all()) and bool((lo == -1.0).all())
    assert all(int(torch.count_nonzero(g)) == 0 for g in dws)
    w = C.c_int32(-1)
    assert hn._lib.lib().hn_device_faults(C.byref(w), 0) == 0 and w.value == 0
