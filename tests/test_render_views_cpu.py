"""hn_render_views without a device: the two symbols and hn_view_args' layout
against the compiled header, every host check of the entry point (none of its
pointers is dereferenced before a launch), the workspace size, and what
render._views_ineligible accepts and names beside render._image_ineligible."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import GOLDEN, ROOT, golden
from gpu_support import MLP_KW

HEADER = os.path.join(ROOT, "include", "hashnerf_amd.h")
OK, NULL, SHAPE, WORKSPACE = 0, 1, 2, 3
X = 4096   # a pointer that is never dereferenced


def _cfg(L, ni, T=19):
    cfg = L.HnRenderCfg()
    cfg.grid = L.make_grid(16, 2, T, [-1.5] * 3, [1.5] * 3, [[0.1] * 3] * 16)
    cfg.n_samples, cfg.n_importance, cfg.white_bkgd = 64, ni, 1
    return cfg


def _view_args(L, **over):
    """Valid-looking arguments; fields of the image member by their names."""
    va = L.HnViewArgs()
    a = va.image
    a.n_views, a.H, a.W, a.pose_stride = 2, 6, 5, 16
    a.fx = a.fy = 10.
    a.cx, a.cy, a.near, a.far = 2.5, 3., 0., 1.
    a.poses = a.t_vals = a.u = a.table = a.rgb = a.depth = a.acc = X
    for m in (a.coarse, a.fine):
        m.sigma0 = m.sigma1 = m.color0 = m.color1 = m.color2 = X
    va.ndc, va.ndc_sx, va.ndc_sy = 1, -4., -10. / 3.
    for k, v in over.items():
        setattr(va if k in ("ndc", "ndc_sx", "ndc_sy", "variant") else a, k, v)
    return va


def test_symbols_declared_exported_and_bound(hn):
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:int32_t|size_t)\s+(hn_\w+)\s*\(", src, re.M))
    lib = hn._lib.lib()
    for n in ("hn_render_views", "hn_render_views_workspace_bytes"):
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in hn._lib.SIGNATURES, n
    assert lib.hn_abi_version() == hn._lib.ABI_VERSION == 14
    from hashnerf_pytorch_amd.render import render_views
    assert hn.render_views is render_views and "render_views" in hn.__all__


def test_view_args_layout_matches_compiled_header(hn, tmp_path):
    """Every field offset of hn_view_args and of its hn_image_args member as
    gcc lays out the header (test_capi's method)."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    L = hn._lib
    structs = {"hn_view_args": L.HnViewArgs, "hn_image_args": L.HnImageArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hashnerf_amd.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for f in cls._fields_:
            lines.append(f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out if l.strip()}
    for cname, cls in structs.items():
        assert got[(cname, "sizeof")] == C.sizeof(cls), cname
        for f in cls._fields_:
            assert got[(cname, f[0])] == getattr(cls, f[0]).offset, (cname, f[0])
    assert L.HnViewArgs.image.offset == 0
    assert [f[0] for f in L.HnViewArgs._fields_] == ["image", "ndc", "ndc_sx", "ndc_sy", "variant"]


def test_workspace_bytes(hn):
    L = hn._lib
    lib = L.lib()
    c64, c128 = _cfg(L, 64), _cfg(L, 128)
    n = lib.hn_render_views_workspace_bytes(c64)
    assert n == lib.hn_render_views_workspace_bytes(c128) == lib.hn_render_image_workspace_bytes(c128) > 0
    assert lib.hn_render_views_workspace_bytes(_cfg(L, 64, T=12)) == n    # the fixed grid's, whatever the table
    assert lib.hn_render_views_workspace_bytes(_cfg(L, 96)) == 0
    assert lib.hn_render_views_workspace_bytes(None) == 0


def test_validation_without_gpu(hn):
    L = hn._lib
    lib = L.lib()
    c64, c128 = _cfg(L, 64), _cfg(L, 128)
    nb = lib.hn_render_views_workspace_bytes(c64)
    ws = C.c_void_p(X)

    def call(cfg, va, w=ws, n=nb):
        return lib.hn_render_views(cfg, va, w, n, None)

    assert call(None, _view_args(L)) == NULL
    assert call(c64, None) == NULL
    assert call(_cfg(L, 96), _view_args(L)) == SHAPE
    # 64 and 128 pass every check up to the first NULL pointer, with and without ndc
    for cfg in (c64, c128):
        for ndc in (0, 1):
            for k in ("poses", "t_vals", "u", "table", "rgb", "depth", "acc"):
                assert call(cfg, _view_args(L, ndc=ndc, **{k: None})) == NULL, (cfg.n_importance, ndc, k)
            va = _view_args(L, ndc=ndc)
            va.image.fine.color1 = None
            assert call(cfg, va) == NULL
            assert call(cfg, _view_args(L, ndc=ndc), w=None) == NULL           # no workspace
            assert call(cfg, _view_args(L, ndc=ndc), n=nb - 1) == WORKSPACE    # one byte short
            assert call(cfg, _view_args(L, ndc=ndc, n_views=0), w=None, n=0) == OK   # nothing to render: no launch
    perturbed = _cfg(L, 64)
    perturbed.perturb = 1
    assert call(perturbed, _view_args(L)) == SHAPE
    assert call(c64, _view_args(L, ndc=2)) == SHAPE
    assert call(c64, _view_args(L, ndc=-1)) == SHAPE
    assert call(c64, _view_args(L, variant=4)) == SHAPE      # an undocumented bit
    assert call(c64, _view_args(L, variant=-1)) == SHAPE
    for variant in (1, 2, 3):                                # the documented ones reach the pointer checks
        assert call(c64, _view_args(L, variant=variant, rgb=None)) == NULL
    for bad in (dict(H=0), dict(W=-3), dict(pose_stride=9), dict(n_views=-1)):
        assert call(c64, _view_args(L, **bad)) == SHAPE, bad
    # every one of these is refused ahead of the NULL pointers and the workspace
    assert call(c64, _view_args(L, ndc=2, rgb=None), n=0) == SHAPE
    # more than 2^31 - 1 pixels per view
    assert call(c64, _view_args(L, H=1 << 16, W=1 << 16)) == SHAPE
    # the earlier entry points keep their own refusal on the same host path
    assert lib.hn_render_image(c64, _view_args(L).image, ws, nb, None) == SHAPE
    assert lib.hn_render_image(c128, _view_args(L, rgb=None).image, ws, nb, None) == NULL
    assert lib.hn_render_image(c128, _view_args(L).image, ws, nb - 1, None) == WORKSPACE


def test_llff_fixture_pinned_against_the_oracle(oracle):
    """render_views_llff.npz: render_image.npz's keys, far under the size
    limit, a composite that is exercised, and the oracle on its inputs within
    the GPU test's comparison of the reference's outputs (the generator's own
    checks, so a regenerated file cannot drift past them unseen)."""
    import sys
    sys.path.insert(0, GOLDEN)
    try:
        import make_golden_views as MV
    finally:
        sys.path.remove(GOLDEN)
    g = golden("render_views_llff")
    assert sorted(g) == sorted(golden("render_image"))
    assert os.path.getsize(os.path.join(GOLDEN, "render_views_llff.npz")) <= 1 << 17
    assert (int(g["H"]), int(g["W"]), int(g["log2T"])) == (11, 14, 12) and g["acc"].shape == (11, 14)
    assert ((g["acc"] > 0.05) & (g["acc"] < 0.95)).any()
    rgb, acc = MV.oracle_views(g)
    assert MV.mostly_close_frac(rgb, g["rgb"].reshape(-1, 3)) >= 0.6
    assert MV.mostly_close_frac(acc, g["acc"].reshape(-1)) >= 0.6


def _nets(hn):
    box = (torch.tensor([-1.5, -1.5, -1.]), torch.tensor([1.5, 1.5, 1.]))
    emb = hn.HashEmbedder(box, log2_hashmap_size=14, finest_resolution=512)
    return hn.NetworkQuery(emb, hn.SHEncoder()), hn.NeRFSmall(**MLP_KW), hn.NeRFSmall(**MLP_KW)


def test_views_eligibility(hn):
    from hashnerf_pytorch_amd.render import _image_ineligible, _views_ineligible
    nq, mc, mf = _nets(hn)
    kw = dict(network_fn=mc, network_query_fn=nq, N_samples=64, network_fine=mf, perturb=0., raw_noise_std=0.,
              use_viewdirs=True)
    for ni in (64, 128):
        for ndc in (True, False):
            assert _views_ineligible(dict(kw, N_importance=ni, ndc=ndc)) is None, (ni, ndc)
        assert _views_ineligible(dict(kw, N_importance=ni)) is None      # render()'s default ndc=True
    llff = dict(kw, N_importance=64, ndc=True)
    for bad, why in ((dict(perturb=1.), "perturb"), (dict(raw_noise_std=1.), "raw_noise_std"),
                     (dict(use_viewdirs=False), "view directions"), (dict(c2w_staticcam=torch.eye(4)), "staticcam"),
                     (dict(retraw=True), "retraw"), (dict(N_importance=96), "not the fused"),
                     (dict(N_samples=32), "not the fused"), (dict(network_fine=None), "not the fused")):
        got = _views_ineligible(dict(llff, **bad))
        assert got is not None and why in got, (bad, got)
    # render_image's own contract is untouched
    assert "N_importance" in _image_ineligible(dict(kw, N_importance=64, ndc=False))
    assert "ndc rays" == _image_ineligible(dict(kw, N_importance=128, ndc=True))
    assert _image_ineligible(dict(kw, N_importance=128, ndc=False)) is None
    K = [[10., 0., 2.5], [0., 10., 3.], [0., 0., 1.]]
    with pytest.raises(ValueError, match="perturb"):
        hn.render_views(6, 5, K, torch.eye(4)[:3], **dict(llff, perturb=1.))


def test_functional_render_views_refuses_cpu_tensors(hn):
    HF = hn.functional
    nq, mc, mf = _nets(hn)
    ws = mc.weights() + mf.weights()
    K = [[10., 0., 2.5], [0., 10., 3.], [0., 0., 1.]]
    poses = torch.eye(4)[None, :3]
    for ni, ndc in ((64, True), (128, False)):
        cfg = HF.make_render_cfg(nq.embed_fn.grid(), False, False, False, n_importance=ni)
        with pytest.raises(RuntimeError, match="ROCm"):
            HF.render_views(cfg, 6, 5, K, poses, 0., 1., nq.embed_fn.table, ws, ndc=ndc)
    with pytest.raises(RuntimeError, match="ROCm"):
        HF.render_image(HF.make_render_cfg(nq.embed_fn.grid(), False, False, False), 6, 5, K, poses, 2., 6.,
                        nq.embed_fn.table, ws)
    with pytest.raises(RuntimeError, match="ROCm"):
        hn.render_views(6, 5, K, poses[0], network_fn=mc, network_query_fn=nq, N_samples=64, network_fine=mf,
                        N_importance=64, use_viewdirs=True)
