"""N_importance = 64 (the LLFF configurations' sample counts) without a device:
the reference-made fixtures pinned against the oracle, rays.bbox_for_llff bit
for bit against bbox.get_bbox3d_for_llff, and what the C ABI and the Python
dispatch accept and refuse for a 64 + 64 configuration."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, pcg_table
from gpu_support import MLP_KW, golden_ni64

NAMES = ["render_ni64_white_perturb", "render_ni64_black_det"]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_render_rays_step_ni64(oracle, name):
    """tests/test_oracle_golden.py::test_render_rays_step's assertions on the
    64 + 64 fixtures: pins the fixtures (and the oracle's N_importance)."""
    g = golden_ni64(name)
    assert g["u"].shape == (64, 64) and g["raw"].shape == (64, 128, 4) and g["table_grad"].shape == (16, 1 << 14, 2)
    tab = t(pcg_table(g["table_seed"], g["log2T"])).requires_grad_(True)
    res = oracle.level_resolutions(16, 16, int(g["finest"]))
    rays_o, rays_d = t(g["rays_o"]), t(g["rays_d"])
    viewdirs = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
    B = rays_o.shape[0]
    rb = torch.cat([rays_o, rays_d, 2. * torch.ones(B, 1), 6. * torch.ones(B, 1), viewdirs], -1)
    wc = {k: t(g["wc:" + k]).clone().requires_grad_(True) for k in oracle.MLP_KEYS}
    wf = {k: t(g["wf:" + k]).clone().requires_grad_(True) for k in oracle.MLP_KEYS}
    t_rand = t(g["t_rand"]) if float(g["perturb"]) > 0 else None
    ret = oracle.render_rays(rb, wc, wf, tab, t(g["box_min"]), t(g["box_max"]), res, int(g["log2T"]),
                             N_importance=64, t_rand=t_rand, u=t(g["u"]), white_bkgd=bool(g["white"]))
    for k, gk in (("rgb_map", "rgb"), ("depth_map", "depth"), ("acc_map", "acc"), ("rgb0", "rgb0"),
                  ("depth0", "depth0"), ("acc0", "acc0"), ("sparsity_loss", "sparsity_loss"),
                  ("sparsity_loss0", "sparsity_loss0"), ("z_std", "z_std"), ("raw", "raw")):
        np.testing.assert_allclose(ret[k].detach().numpy(), g[gk], rtol=1e-5, atol=1e-6, err_msg=k)
    loss = oracle.training_loss(ret, t(g["target"]), float(g["sparse_w"]))
    np.testing.assert_allclose(loss.item(), g["loss"], rtol=1e-6)
    loss.backward()
    np.testing.assert_allclose(tab.grad.numpy(), g["table_grad"], rtol=1e-4, atol=1e-8)
    for tag, w in (("c", wc), ("f", wf)):
        for k in oracle.MLP_KEYS:
            np.testing.assert_allclose(w[k].grad.numpy(), g[f"g{tag}:{k}"], rtol=1e-4, atol=1e-7)


def test_committed_fixtures_under_the_size_limit():
    for n in NAMES:
        for f in (n + ".npz", n + ".tg_hi.npz"):
            assert os.path.getsize(os.path.join(GOLDEN, f)) <= 1 << 20, f


def test_bbox_for_llff_bitexact_vs_reference(hn):
    """rays.bbox_for_llff against bbox.get_bbox3d_for_llff's (min, max)."""
    g = golden("bbox_llff")
    hwf = (int(g["H"]), int(g["W"]), float(g["focal"]))
    for poses in (g["poses"], torch.from_numpy(g["poses"])):
        lo, hi = hn.bbox_for_llff(poses, hwf, near=float(g["near"]), far=float(g["far"]))
        np.testing.assert_array_equal(lo.numpy(), g["box_min"])
        np.testing.assert_array_equal(hi.numpy(), g["box_max"])
    assert hn.rays.bbox_for_llff is hn.bbox_for_llff and hn.bbox_for_blender is hn.rays.bbox_for_blender
    lo, hi = hn.bbox_for_llff(g["poses"], hwf)                 # the defaults are near 0, far 1
    np.testing.assert_array_equal(lo.numpy(), g["box_min"])
    # NDC: the corner rays reach past [-1, 1] in x and y (shifted cameras), and z runs from -1 (near) to 1 (far)
    assert -2. < lo[0] < -1. and 1. < hi[0] < 2. and abs(float(lo[2]) + 1.0001) < 1e-6
    assert abs(float(hi[2]) - 1.0001) < 1e-3


def _cfg(L, ni, T=19, scatter=0):
    cfg = L.HnRenderCfg()
    cfg.grid = L.make_grid(16, 2, T, [-1.5] * 3, [1.5] * 3, [[0.1] * 3] * 16)
    cfg.n_samples, cfg.n_importance, cfg.white_bkgd, cfg.scatter = 64, ni, 1, scatter
    return cfg


def _image_args(L):
    """Valid-looking arguments; the pointers are never dereferenced."""
    a = L.HnImageArgs()
    a.n_views, a.H, a.W, a.pose_stride = 2, 6, 5, 16
    a.fx = a.fy = 10.
    a.cx, a.cy, a.near, a.far = 2.5, 3., 2., 6.
    a.poses = a.t_vals = a.u = a.table = a.rgb = a.depth = a.acc = 4096
    for m in (a.coarse, a.fine):
        m.sigma0 = m.sigma1 = m.color0 = m.color1 = m.color2 = 4096
    return a


def test_c_abi_accepts_64_without_gpu(hn):
    """hn_render_cfg.n_importance = 64 through the host-only entry points
    (T = 19, 4096 rays): a workspace no larger than the 128 cfg's, the binned
    schedule, no whole-image kernel, and no third sample count."""
    L = hn._lib
    lib = L.lib()
    SHAPE = 2
    c64, c128, n = _cfg(L, 64), _cfg(L, 128), 4096
    b64, b128 = lib.hn_render_workspace_bytes(c64, n), lib.hn_render_workspace_bytes(c128, n)
    assert 0 < b64 <= b128
    assert lib.hn_render_scatter_mode(c64, n) == 2
    # accepted: the bins' geometry is reported (0 bins for a refused cfg), and an empty batch is HN_OK
    s64, s128 = C.c_int32(0), C.c_int32(0)
    assert lib.hn_render_bins(c64, n, C.byref(s64)) == lib.hn_render_bins(c128, n, C.byref(s128)) > 0
    assert s64.value == s128.value > 0
    empty = L.HnRenderFwdArgs()
    assert lib.hn_render_fwd(c64, empty, None, 0, None) == 0
    assert lib.hn_render_bwd(c64, L.HnRenderBwdArgs(), None, 0, None) == 0
    assert lib.hn_render_scatter_mode(_cfg(L, 64, scatter=1), n) == 1     # still reports what a cfg would get
    assert lib.hn_render_scatter_mode(_cfg(L, 64, T=23), n) == 1
    assert lib.hn_render_image_workspace_bytes(c64) == 0
    assert lib.hn_render_image_workspace_bytes(c128) > 0
    ws = C.c_void_p(4096)
    nb = lib.hn_render_image_workspace_bytes(c128)
    assert lib.hn_render_image(c64, _image_args(L), ws, nb, None) == SHAPE
    assert lib.hn_render_image_variant(c64, _image_args(L), 1, ws, nb, None) == SHAPE
    # any other count is still refused, by every entry point that takes a cfg
    c96 = _cfg(L, 96)
    assert lib.hn_render_image(c96, _image_args(L), ws, nb, None) == SHAPE
    fa = L.HnRenderFwdArgs()
    fa.n_rays = n
    assert lib.hn_render_fwd(c96, fa, ws, 1 << 40, None) == SHAPE
    ba = L.HnRenderBwdArgs()
    ba.n_rays = n
    assert lib.hn_render_bwd(c96, ba, ws, 1 << 40, None) == SHAPE
    assert lib.hn_abi_version() == 14


def test_training_on_the_atomic_schedule_is_refused_before_any_launch(hn):
    """A 64 cfg whose backward would be the float-atomic schedule: hn_render_fwd
    with feat != NULL and hn_render_bwd return HN_E_SHAPE (host checks only: no
    device is needed to see them)."""
    L = hn._lib
    lib = L.lib()
    cfg, n, x = _cfg(L, 64, scatter=1), 512, 4096
    nb = lib.hn_render_workspace_bytes(cfg, n)
    fa = L.HnRenderFwdArgs()
    fa.n_rays = n
    for k in ("rays", "t_vals", "u", "table", "rgb", "depth", "acc", "sparsity", "rgb0", "depth0", "acc0",
              "sparsity0", "z_std", "z_coarse", "z_fine", "raw_c", "raw_f", "fine_src", "feat"):
        setattr(fa, k, x)
    for m in (fa.coarse, fa.fine):
        m.sigma0 = m.sigma1 = m.color0 = m.color1 = m.color2 = x
    assert lib.hn_render_fwd(cfg, fa, C.c_void_p(x), nb, None) == 2
    ba = L.HnRenderBwdArgs()
    ba.n_rays = n
    for k in ("rays", "table", "z_coarse", "z_fine", "raw_c", "raw_f", "fine_src", "feat", "d_table"):
        setattr(ba, k, x)
    for m in (ba.coarse, ba.fine, ba.d_coarse, ba.d_fine):
        m.sigma0 = m.sigma1 = m.color0 = m.color1 = m.color2 = x
    assert lib.hn_render_bwd(cfg, ba, C.c_void_p(x), nb, None) == 2


def _nets(hn):
    box = (torch.tensor([-1.5, -1.5, -1.]), torch.tensor([1.5, 1.5, 1.]))
    emb = hn.HashEmbedder(box, log2_hashmap_size=14, finest_resolution=512)
    return hn.NetworkQuery(emb, hn.SHEncoder()), hn.NeRFSmall(**MLP_KW), hn.NeRFSmall(**MLP_KW)


def test_fusable_at_64_and_image_kernel_is_not(hn):
    from hashnerf_pytorch_amd.render import _fusable, _image_ineligible
    nq, mc, mf = _nets(hn)
    rays = torch.empty(1, 11)
    assert _fusable(rays, mc, nq, 64, 64, mf)
    assert _fusable(rays, mc, nq, 64, 128, mf)
    assert not _fusable(rays, mc, nq, 64, 96, mf)
    assert not _fusable(rays, mc, nq, 32, 64, mf)
    kw = dict(network_fn=mc, network_query_fn=nq, N_samples=64, network_fine=mf, perturb=0., raw_noise_std=0.,
              ndc=False, use_viewdirs=True)
    assert _image_ineligible(dict(kw, N_importance=128)) is None
    why = _image_ineligible(dict(kw, N_importance=64))
    assert why is not None and "N_importance" in why
    K = [[10., 0., 2.5], [0., 10., 3.], [0., 0., 1.]]
    with pytest.raises(ValueError, match="N_importance"):
        hn.render_image(6, 5, K, torch.eye(4)[:3], **dict(kw, N_importance=64))


def test_make_render_cfg_carries_the_count(hn):
    from hashnerf_pytorch_amd import functional as HF
    nq, _, _ = _nets(hn)
    cfg = HF.make_render_cfg(nq.embed_fn.grid(), True, False, True, n_importance=64)
    assert (cfg.n_samples, cfg.n_importance) == (64, 64)
    assert HF._fine_counts(cfg) == (64, 128)
    assert HF._fine_counts(HF.make_render_cfg(nq.embed_fn.grid(), True, False, True)) == (128, 192)
