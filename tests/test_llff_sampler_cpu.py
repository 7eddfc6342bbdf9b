"""CPU side of the samplers' NDC step: the two scalars, the refusals made
before any library call, the declared and bound symbols, SyntheticLLFF's
invariants, and the conditions test_gpu_llff_sampler.py puts on its input
(every world ray has d_z < 0, every NDC ray is finite, keying the NDC rays
differs from keying the world rays)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
from pool_order_key import pool_key, pool_perm

H, W, N_IMG = 11, 14, 3
NEW = ("hn_sample_rays_ndc", "hn_sample_rays_morton_ndc", "hn_sample_batch_morton_ndc", "hn_sample_pool_ndc",
       "hn_sample_pool_ordered_ndc", "hn_render_bwd_ndc")


@pytest.mark.parametrize("hwf", [(11, 14, 11.5), (378, 504, 407.5652), (20, 20, 16.0), (400, 400, 555.5555155968841),
                                 (7, 1008, 3.1)])
def test_scalars_are_render_views_formula(hn, hwf):
    """sx, sy as float32 are what functional._render_views writes into
    hn_view_args.ndc_sx / ndc_sy: -1. / (W / (2. * focal)), -1. / (H / (2. * focal))
    in float64, rounded once by the struct."""
    HF = hn.functional
    Hh, Ww, focal = hwf
    va = hn._lib.HnViewArgs()
    va.ndc_sx, va.ndc_sy = -1. / (Ww / (2. * focal)), -1. / (Hh / (2. * focal))
    nd = HF._ray_ndc("test", hwf)
    bits = lambda x: np.float32(x).view(np.uint32)
    assert bits(nd.sx) == bits(va.ndc_sx) and bits(nd.sy) == bits(va.ndc_sy)
    assert HF.ndc_scalars(*hwf) == (-1. / (Ww / (2. * focal)), -1. / (Hh / (2. * focal)))
    # a numpy K entry (what a data object holds) gives the same scalars
    nd2 = HF._ray_ndc("test", (Hh, Ww, np.float64(focal)))
    assert bits(nd2.sx) == bits(nd.sx) and bits(nd2.sy) == bits(nd.sy)
    assert HF._ray_ndc("test", None) is None


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} after an argument that must be refused first")


@pytest.fixture
def no_library(hn, monkeypatch):
    """Any use of the HIP library fails the test: the refusals come first."""
    monkeypatch.setattr(hn._lib, "lib", lambda: NoLibrary())
    monkeypatch.setattr(hn._lib, "require_device", lambda *a: (_ for _ in ()).throw(
        AssertionError("device check before the refusal")))


@pytest.mark.parametrize("ndc", [(11, 14), (11, 14, 11.5, 1.), 11.5, "abc", [[11, 14, 11.5]]])
def test_refuses_ndc_that_is_no_triple(hn, no_library, ndc):
    HF = hn.functional
    img, pose = torch.zeros(H, W, 3), torch.eye(4)
    K = [[11.5, 0, 7.], [0, 11.5, 5.5], [0, 0, 1]]
    ids = torch.zeros(1, dtype=torch.int32)
    for order in (0, 1):
        with pytest.raises(ValueError, match="ndc"):
            HF.sample_rays(img, pose, 4, K, 0., 1., (0, 0, H, W), 1, order=order, ndc=ndc)
        with pytest.raises(ValueError, match="ndc"):
            HF.sample_pool(img[None], pose[None], ids, K, 0., 1., 1, 0, 4, order=order, box=([-1] * 3, [1] * 3),
                           ndc=ndc)
    with pytest.raises(ValueError, match="ndc"):
        HF.next_batch(img, pose, 4, K, 0., 1., (0, 0, H, W), 1, ndc=ndc)


@pytest.mark.parametrize("focal", [0., -11.5, float("nan"), float("inf")])
def test_refuses_focal_that_is_not_positive(hn, no_library, focal):
    HF = hn.functional
    img, pose = torch.zeros(H, W, 3), torch.eye(4)
    K = [[11.5, 0, 7.], [0, 11.5, 5.5], [0, 0, 1]]
    ids = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="focal"):
        HF.sample_rays(img, pose, 4, K, 0., 1., (0, 0, H, W), 1, ndc=(H, W, focal))
    with pytest.raises(ValueError, match="focal"):
        HF.next_batch(img, pose, 4, K, 0., 1., (0, 0, H, W), 1, ndc=(H, W, focal))
    with pytest.raises(ValueError, match="focal"):
        HF.sample_pool(img[None], pose[None], ids, K, 0., 1., 1, 0, 4, ndc=(H, W, focal))


def test_refuses_ordered_pool_batch_past_the_maximum(hn, no_library):
    HF = hn.functional
    img, pose = torch.zeros(1, H, W, 3), torch.eye(4)[None]
    K = [[11.5, 0, 7.], [0, 11.5, 5.5], [0, 0, 1]]
    with pytest.raises(ValueError, match=str(HF.POOL_ORDER_MAX)):
        HF.sample_pool(img, pose, torch.zeros(1, dtype=torch.int32), K, 0., 1., 1, 0, HF.POOL_ORDER_MAX + 1, order=1,
                       box=([-1] * 3, [1] * 3), ndc=(H, W, 11.5))
    with pytest.raises(ValueError, match="order"):
        HF.sample_rays(img[0], pose[0], 4, K, 0., 1., (0, 0, H, W), 1, order=2, ndc=(H, W, 11.5))


def test_symbols_declared_and_bound(hn):
    L = hn._lib
    src = open(os.path.join(ROOT, "include", "hashnerf_amd.h")).read()
    lib = L.lib()
    for name in NEW:
        assert re.search(r"^int32_t\s+%s\s*\(" % name, src, re.M), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
        sig = L.SIGNATURES[name][1]
        assert sig[-2] is C.POINTER(L.HnRayNdc) and sig[:-2] == L.SIGNATURES[name[:-4]][1][:-1]
        assert name in src[:src.index("#define HN_ABI_VERSION")], "listed in the ABI comment"
    assert re.search(r"typedef struct hn_ray_ndc \{\s*float sx, sy;\s*\} hn_ray_ndc;", src)
    assert C.sizeof(L.HnRayNdc) == 8 and L.HnRayNdc.sy.offset == 4
    assert [f[0] for f in L.HnNextBatch._fields_][-1] == "n_draws"        # hn_next_batch keeps its layout


def test_validation_without_gpu(hn):
    """NULL is the old call (same codes); a zero or non-finite scalar is
    HN_E_SHAPE, behind the call's other checks and before any launch (the
    device pointers are never dereferenced)."""
    L = hn._lib
    lib = L.lib()
    x = C.c_void_p(16)
    p = L.HnRayPool()
    p.n_images, p.H, p.W, p.pose_stride = N_IMG, H, W, 16
    s = L.HnRaySampler()
    s.H, s.W, s.crop_h, s.crop_w = H, W, H, W
    box = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)
    good, nd = L.HnRayNdc(), L.HnRayNdc()
    good.sx, good.sy = -1.6, -2.0
    ws = lib.hn_sample_rays_morton_workspace_bytes(s)
    assert ws > 0
    for sx, sy in ((0., -2.), (-1.6, 0.), (float("nan"), -2.), (-1.6, float("inf")), (float("-inf"), -2.)):
        nd.sx, nd.sy = sx, sy
        assert lib.hn_sample_rays_ndc(s, x, x, 8, x, x, nd, None) == 2
        assert lib.hn_sample_rays_morton_ndc(s, x, x, 8, x, x, x, ws, nd, None) == 2
        assert lib.hn_sample_batch_morton_ndc(s, x, x, 8, x, x, x, ws, 1, None, 0, nd, None) == 2
        assert lib.hn_sample_pool_ndc(p, x, x, x, 0, 8, x, x, nd, None) == 2
        assert lib.hn_sample_pool_ordered_ndc(p, x, x, x, 0, 8, box[0], box[1], x, x, None, 1, None, 0, nd,
                                              None) == 2
        # an empty draw is a no-op whatever else it names, as without
        assert lib.hn_sample_pool_ndc(p, None, None, None, 0, 0, None, None, nd, None) == 0
        assert lib.hn_sample_rays_ndc(s, None, None, 0, None, None, nd, None) == 0
    # the other checks come first, with their codes, for NULL and a good hn_ray_ndc alike
    for n in (None, good):
        assert lib.hn_sample_pool_ndc(p, None, None, None, 0, 8, None, None, n, None) == 1
        assert lib.hn_sample_pool_ndc(p, x, x, x, 460, 8, x, x, n, None) == 2           # past the pool's 462
        assert lib.hn_sample_rays_ndc(s, x, x, H * W + 1, x, x, n, None) == 2            # more rays than pixels
        assert lib.hn_sample_rays_morton_ndc(s, x, x, 8, x, x, x, ws - 1, n, None) == 3
        assert lib.hn_sample_pool_ordered_ndc(p, x, x, x, 0, 8, None, box[1], x, x, None, 1, None, 0, n, None) == 1
    nd.sx, nd.sy = 0., 0.
    assert lib.hn_sample_rays_morton_ndc(s, x, x, 8, x, x, x, ws - 1, nd, None) == 3     # workspace before ndc


def llff_cpu(hn):
    from hashnerf_pytorch_amd.train import SyntheticLLFF
    return SyntheticLLFF(H, W, N_IMG, "cpu", seed=0)


def pool_rows(hn, d):
    """The pool's rays in (image, row, column) order as hn_sample_pool forms
    them (get_rays_np in float64, rounded once), and their NDC rows."""
    rows = []
    for c in d.poses.numpy().astype(np.float64):
        o, dd = hn.get_rays_np(d.H, d.W, d.K, c[:3, :4])
        rows.append(np.concatenate([o, dd], -1).reshape(-1, 6).astype(np.float32))
    world = torch.from_numpy(np.concatenate(rows, 0))
    o, dd = hn.get_ndc_rays(d.H, d.W, d.K[0][0], 1., world[:, 0:3], world[:, 3:6])
    return world, torch.cat([o, dd], -1)


@pytest.mark.parametrize("hw_n", [(11, 14, 3), (20, 20, 4), (48, 64, 20)])
def test_synthetic_llff_invariants(hn, hw_n):
    from hashnerf_pytorch_amd.train import SyntheticBlender, SyntheticLLFF, default_args
    Hh, Ww, n = hw_n
    d = SyntheticLLFF(Hh, Ww, n, "cpu", seed=0, n_test=2)
    assert (d.near, d.far) == (0., 1.) and d.focal == d.K[0][0] == d.K[1][1]
    assert d.images.shape == (n, Hh, Ww, 3) and d.poses.shape == (n, 4, 4) and len(d.i_train) == n
    assert d.test_poses.shape == (2, 4, 4) and d.test_images is None
    lo, hi = hn.bbox_for_llff(d.poses, [Hh, Ww, d.focal])
    assert torch.equal(d.bounding_box[0], lo) and torch.equal(d.bounding_box[1], hi)
    for fld in vars(SyntheticBlender(4, 4, 2, "cpu")):
        assert hasattr(d, fld), fld
    for c in list(d.poses) + list(d.test_poses):
        o, dd = hn.get_rays(Hh, Ww, d.K, c[:3, :4])
        assert bool((dd[..., 2] < 0).all())                                  # strictly forward-facing
        no, nd = hn.get_ndc_rays(Hh, Ww, d.K[0][0], 1., o, dd)
        assert bool(torch.isfinite(no).all()) and bool(torch.isfinite(nd).all())
        # the NDC rays stay in the box between near 0 and far 1
        for t in (0., 1.):
            pts = no + t * nd
            assert bool((pts >= lo - 1e-4).all()) and bool((pts <= hi + 1e-4).all())
    a = default_args(dataset_type="llff", N_importance=64, raw_noise_std=1., white_bkgd=False, no_batching=False,
                     precrop_iters=0)
    assert a.dataset_type == "llff" and not a.no_ndc


def test_synthetic_llff_procedural_scene_is_visible(hn):
    """The shifted chair lies beyond z = -1 and inside every camera's view:
    the rendered images are not empty, and black where no ray meets it."""
    from hashnerf_pytorch_amd.train import LLFF_SCENE_SHIFT, SyntheticLLFF
    assert LLFF_SCENE_SHIFT[2] + 1.1 < -1.                 # the chair's extent is within 1.1 of its centre
    d = SyntheticLLFF(12, 16, 2, "cpu", seed=0, scene="procedural", n_test=1)
    assert d.images.shape == (2, 12, 16, 3) and d.test_images.shape == (1, 12, 16, 3)
    assert float(d.images.max()) > 0.3 and float(d.images.min()) < 1e-6
    assert float(d.images[:, 0].abs().max()) < 1e-6        # the top row looks past it: black background


def test_gpu_input_conditions(hn):
    """What test_gpu_llff_sampler.py assumes of SyntheticLLFF(11, 14, 3): d_z < 0
    for all 462 world rays, finite NDC rays, and NDC keys (near 0, far 1, the
    LLFF box) that differ from the world rays' keys in value and in order."""
    d = llff_cpu(hn)
    world, ndc = pool_rows(hn, d)
    assert world.shape == (462, 6)
    assert bool((world[:, 5] < 0).all()) and bool(torch.isfinite(ndc).all())
    box = tuple([float(v) for v in b] for b in d.bounding_box)
    kn, clamped = pool_key(ndc.numpy(), box[0], box[1], 0., 1.)
    kw, _ = pool_key(world.numpy(), box[0], box[1], 0., 1.)
    assert not clamped.any()                               # mid-depth NDC points lie inside bbox_for_llff's box
    assert not np.array_equal(kn, kw)
    assert not np.array_equal(pool_perm(kn), pool_perm(kw))
    assert len(np.unique(kn)) > 400


def test_golden_llff_pose_is_forward_facing(hn):
    """The reference-made LLFF fixture's pose satisfies the same condition."""
    g = golden("render_views_llff")
    o, dd = hn.get_rays(int(g["H"]), int(g["W"]), g["K"], torch.from_numpy(g["c2w"]))
    assert bool((dd[..., 2] < 0).all())


def test_render_ray_batch_does_no_ndc_step(hn):
    """render_ray_batch hands the packed rays to render_rays as they are, ndc
    on or off: the explicit and autograd trainers' rays must be final."""
    from importlib import import_module
    R = import_module("hashnerf_pytorch_amd.render")       # (the package's `render` is the function)
    calls = []

    def fake(rays, **kw):
        calls.append((rays, kw))
        return {"rgb_map": rays[:, :3], "depth_map": rays[:, 0], "acc_map": rays[:, 0]}

    orig = R.render_rays
    try:
        R.render_rays = fake
        rays = torch.arange(22.).reshape(2, 11)
        R.render_ray_batch(rays, (2,), ndc=True, near=0., far=1., use_viewdirs=True, perturb=1.)
    finally:
        R.render_rays = orig
    assert len(calls) == 1 and torch.equal(calls[0][0], rays) and calls[0][1] == {"perturb": 1.}
