"""The fused ray gradient's chain rule, pinned on the CPU in float64 before any
kernel: tests/ray_grad_model.py (sums of per-sample dx, z dx and dsh, the
composite's d |d|, J_sh) against autograd of oracle.render_rays with the ray
batch as a leaf.  Plus the C ABI of hn_render_bwd_rays and its workspace
query: declared, bound with matching argument counts, every argument checked
before any launch, and render_rays' refusal of an unknown ray_grad."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from gpu_support import rel_err
from ray_grad_model import ray_grad_model

HEADER = os.path.join(ROOT, "include", "hashnerf_amd.h")
T = 12
BOX = (torch.tensor([-1.5, -1.5, -1.5], dtype=torch.float64), torch.tensor([1.5, 1.5, 1.5], dtype=torch.float64))


def five_rays():
    """Four rays from a camera at distance 4 through the +-1.5 box between
    near 2 and far 6 (their far samples lie behind it), and one that points
    away from it: every sample outside, clamped onto the surface.  Directions
    are not unit length; the view directions are."""
    g = torch.Generator().manual_seed(60)
    o = torch.tensor([0.3, -0.2, 4.0], dtype=torch.float64).expand(5, 3).clone()
    d = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64) + 0.25 * (torch.rand(5, 3, generator=g,
                                                                                 dtype=torch.float64) - 0.5)
    d[4] = torch.tensor([0.9, 0.4, 0.3], dtype=torch.float64)
    d = d * torch.tensor([1.0, 1.3, 0.8, 1.1, 1.2], dtype=torch.float64)[:, None]
    vd = d / torch.norm(d, dim=-1, keepdim=True)
    return torch.cat([o, d, torch.full((5, 1), 2.0, dtype=torch.float64), torch.full((5, 1), 6.0, dtype=torch.float64),
                      vd], -1)


@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("ni", [128, 64])
def test_model_is_autograd_of_the_oracle(oracle, ni, white):
    g = torch.Generator().manual_seed(61 + ni)
    res = oracle.level_resolutions(16, 16, 64)
    tables = torch.rand(16, 2 ** T, 2, generator=g, dtype=torch.float64) - 0.5
    wc, wf = ({k: v.double() for k, v in oracle.init_nerf_small(g).items()} for _ in range(2))
    rays = five_rays()
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * torch.linspace(2., 6., 64, dtype=torch.float64)[None, :, None]
    outside = ((pts < BOX[0]) | (pts > BOX[1])).any(-1)
    assert bool(outside[4].all()) and bool(outside[:4].any()) and not bool(outside[:4].all())
    u = torch.rand(5, ni, generator=g, dtype=torch.float64)
    noise_c = 0.3 * torch.randn(5, 64, generator=g, dtype=torch.float64)
    noise_f = 0.3 * torch.randn(5, 64 + ni, generator=g, dtype=torch.float64)
    target = torch.rand(5, 3, generator=g, dtype=torch.float64)
    ga, gd = (torch.randn(5, generator=g, dtype=torch.float64) for _ in range(2))

    def loss_of(ret):    # every output that has an upstream gradient in hn_render_bwd_args
        return oracle.training_loss(ret, target, 1e-3) + (ga * (ret["acc_map"] + 0.5 * ret["acc0"])).sum() + \
            (gd * (ret["depth_map"] - ret["depth0"])).sum()
    leaf = rays.clone().requires_grad_(True)
    ret = oracle.render_rays(leaf, wc, wf, tables, BOX[0], BOX[1], res, T, N_importance=ni, u=u, noise_c=noise_c,
                             noise_f=noise_f, white_bkgd=white)
    # depth = num / acc is defined
    assert float(ret["acc_map"].detach().min()) > 0 and float(ret["acc0"].detach().min()) > 0
    (want,) = torch.autograd.grad(loss_of(ret), leaf)
    got = ray_grad_model(oracle, rays, wc, wf, tables, BOX[0], BOX[1], res, T, ni, u, white, loss_of, noise_c, noise_f)
    assert float(want[:, 0:6].abs().min()) > 0 and float(want[:, 8:11].abs().min()) > 0
    for name, cols in (("d o", slice(0, 3)), ("d d", slice(3, 6)), ("d viewdir", slice(8, 11))):
        err = rel_err(got[:, cols], want[:, cols])
        print(f"[ray-grad model] ni = {ni}, white = {white}: {name} {err:.3e}")
        assert err <= 1e-11, (name, err)
    assert bool((got[:, 6:8] == 0).all())
    # and on a given fine z (the route the device tests take): the same gradient
    got_z = ray_grad_model(oracle, rays, wc, wf, tables, BOX[0], BOX[1], res, T, ni, u, white, loss_of, noise_c,
                           noise_f, z_fine=ret["z_vals"].detach())
    assert rel_err(got_z, got) <= 1e-13


def test_header_declares_and_lib_binds_the_ray_gradient(hn):
    src = open(HEADER).read()
    lib = hn._lib.lib()
    for res, name in (("int32_t", "hn_render_bwd_rays"), ("size_t", "hn_render_bwd_rays_workspace_bytes")):
        m = re.search(r"^" + res + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", src, re.M)
        assert m, f"{name} not declared in the header"
        assert name in hn._lib.SIGNATURES, name
        assert len(hn._lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
        assert hasattr(lib, name), name
    assert lib.hn_abi_version() == 14       # additive: the ABI number stays


def test_ray_gradient_argument_validation_without_gpu(hn):
    L = hn._lib
    lib = L.lib()
    HF = hn.functional
    box = (torch.tensor([-1.5, -1.5, -1.5]), torch.tensor([1.5, 1.5, 1.5]))
    emb = hn.HashEmbedder(box, log2_hashmap_size=14, finest_resolution=64)
    x = C.c_void_p(16)   # never dereferenced: validation happens before any launch
    for ni in (128, 64):
        cfg = HF.make_render_cfg(emb.grid(), True, False, False, n_importance=ni)
        # packed nets 2 x 30208 | d raw n x 256 x 4 | marks n | partials n x 8 x 22, floats
        for n in (0, 1, 37):
            assert lib.hn_render_bwd_rays_workspace_bytes(cfg, n) == 4 * (2 * 30208 + n * (1024 + 1 + 176)), (ni, n)
        assert lib.hn_render_bwd_rays_workspace_bytes(cfg, -1) == 0
        # additive: the render workspace is what it was
        assert lib.hn_render_workspace_bytes(cfg, 64) == 186440376
        need = lib.hn_render_bwd_rays_workspace_bytes(cfg, 37)
        a = L.HnRenderBwdArgs()
        a.n_rays = 0
        assert lib.hn_render_bwd_rays(cfg, a, None, 0, None, None) == 0         # no rays: nothing to do
        assert lib.hn_render_bwd_rays(cfg, None, x, need, x, None) == 1         # no args
        a.n_rays = -1
        assert lib.hn_render_bwd_rays(cfg, a, x, need, x, None) == 2
        a.n_rays = 37
        assert lib.hn_render_bwd_rays(cfg, a, x, need, x, None) == 1            # nothing given
        for k in ("rays", "table", "z_coarse", "z_fine", "raw_c", "raw_f", "fine_src"):
            setattr(a, k, 16)
        for m in (a.coarse, a.fine):
            for k in ("sigma0", "sigma1", "color0", "color1", "color2"):
                setattr(m, k, 16)
        assert lib.hn_render_bwd_rays(cfg, a, x, need, x, None) == 1            # no saved state (feat)
        a.feat = 16
        assert lib.hn_render_bwd_rays(cfg, a, x, need, None, None) == 1         # no d_rays
        assert lib.hn_render_bwd_rays(cfg, a, None, need, x, None) == 1         # no scratch
        assert lib.hn_render_bwd_rays(cfg, a, x, need - 4, x, None) == 3        # scratch too small
        a.prepass_done = 1
        assert lib.hn_render_bwd_rays(cfg, a, x, need, x, None) == 2            # the g_* arrays are the upstream
        a.prepass_done = 0
        a.fine.color2 = None
        assert lib.hn_render_bwd_rays(cfg, a, x, need, x, None) == 1            # a net's tensor missing
    cfg = HF.make_render_cfg(emb.grid(), True, False, False, n_importance=128)
    cfg.n_importance = 96
    assert lib.hn_render_bwd_rays_workspace_bytes(cfg, 37) == 0
    a = L.HnRenderBwdArgs()
    a.n_rays = 0
    assert lib.hn_render_bwd_rays(cfg, a, x, 1 << 30, x, None) == 2             # a bad n_importance, before n_rays == 0
    assert lib.hn_render_bwd_rays(None, a, x, 1 << 30, x, None) == 1


def test_render_rays_refuses_an_unknown_ray_grad(hn):
    with pytest.raises(ValueError, match="ray_grad"):
        hn.render_rays(torch.zeros(4, 11), None, None, 64, ray_grad="unfused")
