"""hn_render_image without a device: the exports, the ctypes mirror of
hn_image_args against the compiled header, argument validation (every check
returns before any launch), the workspace size, and the refusal of CPU
tensors."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hashnerf_amd.h")


def _cfg(L, levels=16):
    cfg = L.HnRenderCfg()
    cfg.grid = L.make_grid(levels, 2, 14, [-1.5] * 3, [1.5] * 3, [[0.1] * 3] * levels)
    cfg.n_samples, cfg.n_importance, cfg.white_bkgd = 64, 128, 1
    return cfg


def _args(L, n_views=2, H=6, W=5, pose_stride=16):
    """Valid-looking arguments; the pointers are never dereferenced."""
    x = 4096
    a = L.HnImageArgs()
    a.n_views, a.H, a.W, a.pose_stride = n_views, H, W, pose_stride
    a.fx = a.fy = 10.
    a.cx, a.cy, a.near, a.far = 2.5, 3., 2., 6.
    a.poses = a.t_vals = a.u = a.table = a.rgb = a.depth = a.acc = x
    for m in (a.coarse, a.fine):
        m.sigma0 = m.sigma1 = m.color0 = m.color1 = m.color2 = x
    return a


def test_symbols_exported_and_declared(hn):
    src = open(HEADER).read()
    L = hn._lib
    for name in ("hn_render_image", "hn_render_image_workspace_bytes", "hn_render_image_variant"):
        assert re.search(r"^\s*(?:int32_t|size_t)\s+" + name + r"\s*\(", src, re.M), name
        assert hasattr(L.lib(), name), name
        assert name in L.SIGNATURES, name
    assert L.lib().hn_abi_version() == 14          # additive: the version stays


def test_image_args_layout_matches_compiled_header(hn, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls = hn._lib.HnImageArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hashnerf_amd.h"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(hn_image_args));']
    for f in cls._fields_:
        lines.append(f'printf("{f[0]} %zu\\n", offsetof(hn_image_args, {f[0]}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[0]: int(l.split()[1]) for l in out if l.strip()}
    assert got["sizeof"] == C.sizeof(cls)
    for f in cls._fields_:
        assert got[f[0]] == getattr(cls, f[0]).offset, f[0]
    # and the header's struct has no field the mirror lacks
    body = re.search(r"typedef struct hn_image_args \{(.*?)\} hn_image_args;", open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"[\s*,](\w+)\s*(?=,|$)", decl.strip())]
    assert names == [f[0] for f in cls._fields_]


def test_validation_without_gpu(hn):
    L = hn._lib
    lib = L.lib()
    cfg = _cfg(L)
    nbytes = lib.hn_render_image_workspace_bytes(cfg)
    ws = C.c_void_p(4096)
    call = lambda cfg, a, ws=ws, n=nbytes: lib.hn_render_image(cfg, a, ws, n, None)
    NULL, SHAPE, WORKSPACE = 1, 2, 3
    assert call(None, _args(L)) == NULL
    assert call(cfg, None) == NULL
    a = _args(L)
    a.poses = None
    assert call(cfg, a) == NULL
    a = _args(L)
    a.rgb = None
    assert call(cfg, a) == NULL
    assert call(cfg, _args(L), ws=None) == NULL
    assert call(cfg, _args(L, H=0)) == SHAPE
    assert call(cfg, _args(L, W=-3)) == SHAPE
    assert call(cfg, _args(L, n_views=-1)) == SHAPE
    assert call(cfg, _args(L, pose_stride=13)) == SHAPE
    jitter = _cfg(L)
    jitter.perturb = 1
    assert call(jitter, _args(L)) == SHAPE
    assert call(_cfg(L, levels=8), _args(L)) == SHAPE      # check_cfg's own refusals come first
    assert call(cfg, _args(L), n=nbytes - 1) == WORKSPACE
    assert call(cfg, _args(L, n_views=0)) == 0
    assert call(cfg, _args(L, n_views=0), ws=None, n=0) == 0   # nothing to render: nothing else is looked at
    # more ray groups than the kernel's 32-bit index
    assert call(cfg, _args(L, n_views=40, H=1 << 14, W=1 << 14)) == SHAPE
    # the measured alternatives take the same checks, and only the documented bits
    assert lib.hn_render_image_variant(cfg, _args(L, n_views=0), 3, None, 0, None) == 0
    assert lib.hn_render_image_variant(cfg, _args(L), 4, ws, nbytes, None) == SHAPE
    assert lib.hn_render_image_variant(cfg, _args(L, pose_stride=13), 1, ws, nbytes, None) == SHAPE


def test_workspace_depends_on_cfg_only(hn):
    L = hn._lib
    lib = L.lib()
    n = lib.hn_render_image_workspace_bytes(_cfg(L))
    # both nets' packed weights and one 8 KiB slot per wave of the fixed grid
    assert n >= 2 * L.MLP_PACKED_FLOATS * 4 + 4096 * 8192
    white = _cfg(L)
    white.white_bkgd, white.lindisp = 0, 1
    assert lib.hn_render_image_workspace_bytes(white) == n
    # the size a 1 x 1 and an 8-view 800 x 800 call need is this one number: both pass the size check
    ws = C.c_void_p(4096)
    for a in (_args(L, n_views=1, H=1, W=1), _args(L, n_views=8, H=800, W=800)):
        a.poses = None          # stops at the NULL check, before the workspace check
        assert lib.hn_render_image(_cfg(L), a, ws, n, None) == 1
        a = _args(L, a.n_views, a.H, a.W)
        assert lib.hn_render_image(_cfg(L), a, ws, n - 1, None) == 3


def test_render_image_refuses_cpu_tensors(hn):
    from hashnerf_pytorch_amd import functional as HF
    L = hn._lib
    poses = torch.eye(4)[None, :3]
    table = torch.zeros(16, 1 << 14, 2)
    ws = [torch.zeros(64, 32), torch.zeros(16, 64), torch.zeros(64, 31), torch.zeros(64, 64), torch.zeros(3, 64)] * 2
    K = [[10., 0., 2.5], [0., 10., 3.], [0., 0., 1.]]
    with pytest.raises(RuntimeError, match="ROCm"):
        HF.render_image(_cfg(L), 6, 5, K, poses, 2., 6., table, ws)


def test_render_image_names_why_a_configuration_is_not_eligible(hn):
    K = [[10., 0., 2.5], [0., 10., 3.], [0., 0., 1.]]
    with pytest.raises(ValueError, match="not eligible"):
        hn.render_image(6, 5, K, torch.eye(4)[:3], ndc=False, use_viewdirs=True)   # no fused networks
