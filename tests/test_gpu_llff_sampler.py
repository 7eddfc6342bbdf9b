"""The samplers' NDC step (hn_ray_ndc; functional.sample_rays / next_batch /
sample_pool with ndc=(H, W, focal)): every draw hands out render()'s final NDC
ray in the launch that forms the world ray.

Yardstick: the same call without ndc, then rays.get_ndc_rays(H, W, K[0][0],
1., o, d) on the device (pinned by tests/golden/ndc.npz, which the reference
made).  Columns 0:6 are compared with it bitwise; near, far, the view
direction and the target with the world call's, bitwise.

Shapes: 3 images of 11 x 14 (not square, no power of two), a pool of 462 rays;
the full window and the crop (2, 3, 7, 9) of 63 pixels; 1, 37 and every pixel
of the window (154 / 63: the draw is without replacement, so the crop's
largest draw is its 63 pixels).  Poses and K: SyntheticLLFF(11, 14, 3), whose
rays all have d_z < 0 (test_llff_sampler_cpu.py asserts it on the CPU)."""
import numpy as np
import pytest
import torch

from gpu_support import bits_equal, forward_kind as forward, kind_scene as scene, loss_of, step_coeffs, ws_offsets
from pool_order_key import pool_key, pool_perm

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
H, W, N_IMG = 11, 14, 3
WINDOWS = {"full": ((0, 0, H, W), (1, 37, H * W)), "crop": ((2, 3, 7, 9), (1, 37, 7 * 9))}
SEED = 0x1234567
_DATA = {}


def llff(hn):
    """SyntheticLLFF(11, 14, 3) on the device (built once, left unchanged)."""
    if "d" not in _DATA:
        from hashnerf_pytorch_amd.train import SyntheticLLFF
        d = SyntheticLLFF(H, W, N_IMG, DEV, seed=0)
        d.ids = torch.as_tensor(d.i_train).to(DEV, torch.int32)
        d.ndc = (H, W, d.K[0][0])
        d.box = tuple([float(v) for v in b] for b in d.bounding_box)
        _DATA["d"] = d
    return _DATA["d"]


def yardstick(hn, d, world):
    """render()'s NDC step on a world batch: [n, 6] (o, d)."""
    o, dd = hn.get_ndc_rays(H, W, d.K[0][0], 1., world[:, 0:3], world[:, 3:6])
    return torch.cat([o, dd], -1)


def check_against_world(hn, d, got, world):
    (r, t), (rw, tw) = got[:2], world[:2]
    assert r.shape == rw.shape == (rw.shape[0], 11)
    assert bool((rw[:, 5] < 0).all())                                  # the input: every ray looks down -z
    assert bits_equal(r[:, 0:6], yardstick(hn, d, rw)), "o, d: get_ndc_rays of the world ray"
    assert bool(torch.isfinite(r).all())
    assert bits_equal(r[:, 6:11], rw[:, 6:11]), "near, far, view direction: the world ray's"
    assert bits_equal(t, tw), "target"
    assert not bits_equal(r[:, 0:6], rw[:, 0:6])


# ---- 1. per-image draws ------------------------------------------------------------------
@pytest.mark.parametrize("window", sorted(WINDOWS))
@pytest.mark.parametrize("order", [0, 1, "1+uniforms"])
def test_per_image_draws(hn, order, window):
    from hashnerf_pytorch_amd import functional as HF
    d = llff(hn)
    crop, ns = WINDOWS[window]
    gen = torch.cuda.default_generators[0]
    for img in (0, 2):
        for n in ns:
            uni = [(n, 64), (n, 64)] if order == "1+uniforms" else None
            kw = dict(order=0 if order == 0 else 1, uniforms=uni)
            draw = lambda **k: HF.sample_rays(d.images[img], d.poses[img], n, d.K, 0., 1., crop, SEED + n, **kw, **k)
            torch.cuda.manual_seed(77)
            world = draw()
            off = gen.get_offset()
            torch.cuda.manual_seed(77)
            got = draw(ndc=d.ndc)
            assert len(got) == len(world) == (4 if uni else 2)
            check_against_world(hn, d, got, world)
            assert bool((got[0][:, 6] == 0.).all()) and bool((got[0][:, 7] == 1.).all())
            if uni:
                assert gen.get_offset() == off
                torch.cuda.manual_seed(77)
                a, b = torch.rand((n, 64), device=DEV), torch.rand((n, 64), device=DEV)
                assert gen.get_offset() == off
                assert torch.equal(got[2], a) and torch.equal(got[3], b)


def test_orders_draw_the_same_set(hn):
    """order=1 lists order=0's NDC rays in Morton order of their pixels: the same rows."""
    from hashnerf_pytorch_amd import functional as HF
    d = llff(hn)
    a = HF.sample_rays(d.images[1], d.poses[1], 37, d.K, 0., 1., (0, 0, H, W), SEED, order=0, ndc=d.ndc)[0]
    b = HF.sample_rays(d.images[1], d.poses[1], 37, d.K, 0., 1., (0, 0, H, W), SEED, order=1, ndc=d.ndc)[0]
    rows = lambda r: sorted(map(bytes, r.cpu().numpy()))
    assert rows(a) == rows(b) and not torch.equal(a, b)


def test_no_draws_through_the_batch_entry_point(hn):
    """sample_rays(order=1) without uniforms calls hn_sample_batch_morton_ndc
    with no draws; its rays and target are hn_sample_rays_morton's (world) and
    hn_sample_rays_morton_ndc's (ndc) for the same sampler, bitwise.  A 16 x 16
    image, a 12 x 9 window inside it, 37 rays."""
    from hashnerf_pytorch_amd import functional as HF
    L = hn._lib
    g = torch.Generator().manual_seed(3)
    image = torch.rand((16, 16, 3), generator=g).to(DEV)
    c2w = torch.tensor([[1., 0., 0., 0.1], [0., 1., 0., -0.2], [0., 0., 1., 0.3]], device=DEV)
    K = [[20., 0., 8.], [0., 20., 8.], [0., 0., 1.]]
    crop, n = (2, 5, 12, 9), 37
    s = L.HnRaySampler()
    s.H, s.W = 16, 16
    s.crop_y0, s.crop_x0, s.crop_h, s.crop_w = crop
    s.fx, s.fy, s.cx, s.cy, s.near, s.far, s.seed = 20., 20., 8., 8., 0., 1., SEED
    nb = L.lib().hn_sample_rays_morton_workspace_bytes(s)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    nd = HF._ray_ndc("test", (16, 16, 20.))
    direct = []
    for ndc in (None, nd):
        rays, target = torch.full((n, 11), float("nan"), device=DEV), torch.full((n, 3), float("nan"), device=DEV)
        if ndc is None:
            st = L.lib().hn_sample_rays_morton(s, L.ptr(image), L.ptr(c2w), n, L.ptr(rays), L.ptr(target), L.ptr(ws), nb,
                                               L.stream(DEV))
        else:
            st = L.lib().hn_sample_rays_morton_ndc(s, L.ptr(image), L.ptr(c2w), n, L.ptr(rays), L.ptr(target),
                                                   L.ptr(ws), nb, ndc, L.stream(DEV))
        assert st == 0
        assert bool(torch.isfinite(rays).all()) and bool(torch.isfinite(target).all())
        direct.append((rays, target))
    assert not torch.equal(direct[0][0], direct[1][0])
    for ndc, (rays, target) in zip((None, (16, 16, 20.)), direct):
        got = HF.sample_rays(image, c2w, n, K, 0., 1., crop, SEED, order=1, ndc=ndc)
        assert len(got) == 2
        assert torch.equal(got[0], rays) and torch.equal(got[1], target), ndc


# ---- 2. pool draws -----------------------------------------------------------------------
def pool_draw(HF, d, start, n, **kw):
    return HF.sample_pool(d.images, d.poses, d.ids, d.K, 0., 1., 11, start, n, **kw)


@pytest.mark.parametrize("start,n", [(0, 1), (0, 37), (425, 37), (0, 462)])
def test_pool_draw(hn, start, n):
    """(425, 37) ends exactly at the pool's end: an epoch's short last batch."""
    from hashnerf_pytorch_amd import functional as HF
    d = llff(hn)
    gen = torch.cuda.default_generators[0]
    world = pool_draw(HF, d, start, n)
    check_against_world(hn, d, pool_draw(HF, d, start, n, ndc=d.ndc), world)
    torch.cuda.manual_seed(5)
    a = torch.rand((n, 64), device=DEV)
    off = gen.get_offset()
    torch.cuda.manual_seed(5)
    got = pool_draw(HF, d, start, n, ndc=d.ndc, uniforms=[(n, 64)])
    check_against_world(hn, d, got, world)
    assert torch.equal(got[2], a) and gen.get_offset() == off


@pytest.mark.parametrize("n", [37, 462])
def test_pool_draw_ordered(hn, n):
    """order=1 keys the FINAL ray: the rows are order 0's NDC rows under the
    lexsort of pool_order_key.py's keys of those rows (near 0, far 1, the LLFF
    box), the keys included; an implementation that keys the world ray first
    gives another key sequence on this input."""
    from hashnerf_pytorch_amd import functional as HF
    d = llff(hn)
    r0, t0 = pool_draw(HF, d, 0, n, ndc=d.ndc)
    w0, _ = pool_draw(HF, d, 0, n)
    r1, t1, k1 = pool_draw(HF, d, 0, n, ndc=d.ndc, order=1, box=d.box, return_keys=True)
    assert r1.shape == (n, 11) and t1.shape == (n, 3) and k1.shape == (n,)
    keys, _ = pool_key(r0.cpu().numpy(), d.box[0], d.box[1], 0., 1.)
    perm = pool_perm(keys)
    pt = torch.from_numpy(perm).to(DEV)
    # a permutation of order 0's rows, all 14 floats of a row bitwise
    assert sorted(perm.tolist()) == list(range(n))
    assert bits_equal(r1, r0[pt]) and bits_equal(t1, t0[pt])
    got = k1.cpu().numpy().astype(np.uint32)
    assert bool((np.diff(got.astype(np.int64)) >= 0).all()), "keys non-decreasing"
    # every key is the restatement's on the NDC row it stands beside
    np.testing.assert_array_equal(got, pool_key(r1.cpu().numpy(), d.box[0], d.box[1], 0., 1.)[0])
    np.testing.assert_array_equal(got, keys[perm])
    # rows with equal keys keep order 0's order
    tie = got[1:] == got[:-1]
    assert bool((perm[1:][tie] > perm[:-1][tie]).all())
    # keyed before the NDC step, the sequence would be another one
    kw, _ = pool_key(w0.cpu().numpy(), d.box[0], d.box[1], 0., 1.)
    assert not np.array_equal(kw[perm], got)
    if n > 1:
        assert not np.array_equal(pool_perm(kw), perm)
    # uniforms in the same launch, keys left out
    torch.cuda.manual_seed(5)
    a = torch.rand((n, 64), device=DEV)
    torch.cuda.manual_seed(5)
    out = pool_draw(HF, d, 0, n, ndc=d.ndc, order=1, box=d.box, uniforms=[(n, 64)])
    assert len(out) == 3 and bits_equal(out[0], r1) and bits_equal(out[1], t1) and torch.equal(out[2], a)


# ---- 3. the next-batch job ---------------------------------------------------------------
BS = (1, 5, 37, 256)


def make_job(HF, d, window, n, n_uni, ndc=True):
    torch.cuda.manual_seed(77)
    nb = HF.next_batch(d.images[1], d.poses[1], n, d.K, 0., 1., WINDOWS[window][0], SEED,
                       uniforms=[(n, 64), (n, 128)][:n_uni] or None, ndc=d.ndc if ndc else None)
    for t in nb.out:
        t.fill_(float("nan"))
    return nb


def stand_alone(HF, d, window, n, n_uni):
    torch.cuda.manual_seed(77)
    return HF.sample_rays(d.images[1], d.poses[1], n, d.K, 0., 1., WINDOWS[window][0], SEED, order=1,
                          uniforms=[(n, 64), (n, 128)][:n_uni] or None, ndc=d.ndc)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("window", sorted(WINDOWS))
def test_job_draws_stand_alone_values_bitwise(hn, window, B):
    """test_gpu_next_batch.py's check with an NDC job: the rays, target and
    uniforms a backward's job fills are the stand-alone NDC call's, bitwise,
    after the pre-pass and as the backward's first kernel (prepass_done)."""
    from hashnerf_pytorch_amd import functional as HF
    d = llff(hn)
    s = scene(hn, B, "rand")
    cfg = HF.make_render_cfg(s.emb.grid(), True, False, True, scatter="binned")
    for n in WINDOWS[window][1]:
        for n_uni in (0, 2):
            ref = stand_alone(HF, d, window, n, n_uni)
            off_ref = torch.cuda.default_generators[0].get_offset()
            for fused in (False, True):
                out, st = forward(HF, s, cfg, fused, skip_dead=True)
                nb = make_job(HF, d, window, n, n_uni)
                assert torch.cuda.default_generators[0].get_offset() == off_ref
                HF.render_bwd(st, {}, torch.empty_like(s.table), HF.zeros_like_all(s.ws), overwrite=True,
                              overwrite_mlp=True, loss=loss_of(s, out, torch.empty(4, device=DEV)),
                              prepass_done=fused, next_batch=nb)
                assert len(nb.out) == len(ref) == 2 + n_uni
                for k, (a, b) in enumerate(zip(nb.out, ref)):
                    assert a.shape == b.shape and a.data_ptr() != b.data_ptr()
                    assert torch.equal(a, b), (n, n_uni, fused, k)
    assert not torch.isnan(ref[0]).any()
    world = HF.sample_rays(d.images[1], d.poses[1], n, d.K, 0., 1., WINDOWS[window][0], SEED, order=1)
    check_against_world(hn, d, ref, world)


def run_step(hn, HF, B, bin_cap, job):
    """test_gpu_next_batch.run_step: one training step's backward on clones of
    the scene's parameters.  job: None, "world" or "ndc"."""
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
    nb = make_job(HF, llff(hn), "crop", 37, 2, ndc=job == "ndc") if job else None
    HF.render_bwd(st, {}, None, dws, overwrite_mlp=True, loss=loss_of(s, out, lo),
                  table_step=(table, m, v, step_coeffs()), prepass_done=True,
                  mlp_step=[(p, a, b, step_coeffs()) for p, a, b in zip(ws, wm, wv)], repack=True, next_batch=nb)
    torch.cuda.synchronize()
    packed = st.wsb[:ws_offsets(B).slab].view(torch.float32).clone()
    return dict(lo=lo, table=table, m=m, v=v, packed=packed, ws=ws, wm=wm, wv=wv, dws=dws), nb


@pytest.mark.parametrize("bin_cap", [0, 64])
@pytest.mark.parametrize("B", [37, 256])
def test_step_with_job_bitwise(hn, B, bin_cap):
    """The step's own results -- loss, table, moments, the ten weights, their
    packed copies -- are bitwise the same without a job, with a world job and
    with an NDC job (bin_cap = 64: records spill, so placement workgroups
    place beside the emit workgroups)."""
    from hashnerf_pytorch_amd import functional as HF
    (a, _), (w, _), (b, nb) = (run_step(hn, HF, B, bin_cap, j) for j in (None, "world", "ndc"))
    for other in (w, b):
        for k in ("lo", "table", "m", "v", "packed"):
            assert bits_equal(a[k], other[k]), k
        for k in ("ws", "wm", "wv", "dws"):
            for i, (x, y) in enumerate(zip(a[k], other[k])):
                assert bits_equal(x, y), (k, i)
    assert not bits_equal(a["table"], scene(hn, B, "rand").table)       # the step stepped
    for x, y in zip(nb.out, stand_alone(HF, llff(hn), "crop", 37, 2)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("bad", [0.0, float("nan"), float("inf")])
def test_refused_scalars_queue_nothing(hn, bad):
    """A zero or non-finite sx: HN_E_SHAPE from every entry point before any
    launch -- the outputs a refused job or draw would fill stay untouched."""
    import ctypes as C
    from hashnerf_pytorch_amd import functional as HF
    L = hn._lib
    d = llff(hn)
    nd = L.HnRayNdc()
    nd.sx, nd.sy = bad, -1.6
    s = scene(hn, 37, "rand")
    cfg = HF.make_render_cfg(s.emb.grid(), True, False, True, scatter="binned")
    out, st = forward(HF, s, cfg, False, skip_dead=False)
    nb = make_job(HF, d, "crop", 37, 2)
    nb.ndc = nd
    d_table = torch.full_like(s.table, 7.0)
    lo = torch.full((4,), -1.0, device=DEV)
    with pytest.raises(RuntimeError, match=r"status 2"):
        HF.render_bwd(st, {}, d_table, HF.zeros_like_all(s.ws), overwrite=True, overwrite_mlp=True,
                      loss=loss_of(s, out, lo), next_batch=nb)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in nb.out)
    assert bool((d_table == 7.0).all()) and bool((lo == -1.0).all())
    rays, target = torch.full((37, 11), 3.0, device=DEV), torch.full((37, 3), 3.0, device=DEV)
    p = L.HnRayPool()
    p.n_images, p.H, p.W, p.pose_stride = N_IMG, H, W, 16
    p.fx = p.fy = 11.2
    p.cx, p.cy, p.near, p.far = 7., 5.5, 0., 1.
    assert L.lib().hn_sample_pool_ndc(p, L.ptr(d.images), L.ptr(d.poses), L.ptr(d.ids), 0, 37, L.ptr(rays),
                                      L.ptr(target), nd, None) == 2
    torch.cuda.synchronize()
    assert bool((rays == 3.0).all()) and bool((target == 3.0).all())
    w = C.c_int32(-1)
    assert L.lib().hn_device_faults(C.byref(w), 0) == 0 and w.value == 0
