"""The closed forms behind the input-gradient kernels, pinned on the CPU in
float64 against autograd of the oracle: hn_encode_bwd_input's d feat / d x
(the cell from the clamped point, the weights from the unclamped one) and
hn_sh_bwd's derivatives of the 16 SH polynomials.  Plus the C ABI of the three
new entry points: declared, bound with matching argument counts, arguments
checked before any launch."""
import os
import re

import torch

from conftest import ROOT
from gpu_support import SMALL_BOX, SMALL_FINEST, SMALL_T, rel_err
from input_grad_cases import input_grad_points, sh_dirs

HEADER = os.path.join(ROOT, "include", "hashnerf_amd.h")

NEW = ("hn_encode_bwd_input", "hn_sh_bwd", "hn_composite_bwd_inputs")


def encode_dx_closed_form(oracle, x, tables, box_min, box_max, resolutions, log2T, dfeat):
    """What hn_encode_bwd_input computes: per level sum_f dfeat_f * d f / d w_a /
    (vmax_a - vmin_a), summed over the levels; d f / d w the nested-lerp
    derivatives of the 8 corner values (corner c = 4 i + 2 j + k)."""
    xc = torch.clamp(x, min=box_min, max=box_max)
    dx = torch.zeros_like(x)
    for lvl, res in enumerate(resolutions):
        gs = (box_max - box_min) / res
        idx = torch.floor((xc - box_min) / gs).int()              # the cell: clamped point
        vmin = idx * gs + box_min
        vmax = vmin + gs
        w = (x - vmin) / (vmax - vmin)                            # the weights: unclamped point
        e = tables[lvl][oracle.spatial_hash(idx.unsqueeze(1) + oracle.CORNERS.unsqueeze(0), log2T)]   # [n, 8, 2]
        wx, wy, wz = w[:, 0:1], w[:, 1:2], w[:, 2:3]
        c00, c01 = e[:, 0] * (1 - wx) + e[:, 4] * wx, e[:, 1] * (1 - wx) + e[:, 5] * wx
        c10, c11 = e[:, 2] * (1 - wx) + e[:, 6] * wx, e[:, 3] * (1 - wx) + e[:, 7] * wx
        c0, c1 = c00 * (1 - wy) + c10 * wy, c01 * (1 - wy) + c11 * wy
        g = dfeat[:, 2 * lvl:2 * lvl + 2]
        g0, g1 = g * (1 - wz), g * wz
        dwz = g * (c1 - c0)
        dwy = g0 * (c10 - c00) + g1 * (c11 - c01)
        dwx = (g0 * (1 - wy)) * (e[:, 4] - e[:, 0]) + (g1 * (1 - wy)) * (e[:, 5] - e[:, 1]) + \
              (g0 * wy) * (e[:, 6] - e[:, 2]) + (g1 * wy) * (e[:, 7] - e[:, 3])
        dx = dx + torch.stack([dwx.sum(-1), dwy.sum(-1), dwz.sum(-1)], -1) / (vmax - vmin)
    return dx


def sh_ddirs_closed_form(oracle, d, go):
    """What hn_sh_bwd computes: d sh16 / d (x, y, z) contracted with go [n, 16]."""
    x, y, z = d.unbind(-1)
    C1, C2, C3 = oracle.SH_C1, oracle.SH_C2, oracle.SH_C3
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    g = [None] * 4 + [C2[i] * go[:, 4 + i] for i in range(5)] + [C3[i] * go[:, 9 + i] for i in range(7)]
    dx = -C1 * go[:, 3] + g[4] * y - 2 * g[6] * x + g[7] * z + 2 * g[8] * x + 6 * g[9] * xy + g[10] * yz \
        - 2 * g[11] * xy - 6 * g[12] * xz + g[13] * (4 * zz - 3 * xx - yy) + 2 * g[14] * xz + 3 * g[15] * (xx - yy)
    dy = -C1 * go[:, 1] + g[4] * x + g[5] * z - 2 * g[6] * y - 2 * g[8] * y + 3 * g[9] * (xx - yy) + g[10] * xz \
        + g[11] * (4 * zz - xx - 3 * yy) - 6 * g[12] * yz - 2 * g[13] * xy - 2 * g[14] * yz - 6 * g[15] * xy
    dz = C1 * go[:, 2] + g[5] * y + 4 * g[6] * z + g[7] * x + g[10] * xy + 8 * g[11] * yz \
        + g[12] * (6 * zz - 3 * xx - 3 * yy) + 8 * g[13] * xz + g[14] * (xx - yy)
    return torch.stack([dx, dy, dz], -1)


def test_encode_dx_closed_form_is_autograd_of_the_oracle(oracle):
    g = torch.Generator().manual_seed(3)
    box_min, box_max = (b.double() for b in SMALL_BOX)
    for n_levels in (16, 5):
        res = oracle.level_resolutions(n_levels, 16, SMALL_FINEST)
        tables = (torch.rand(n_levels, 2 ** SMALL_T, 2, generator=g, dtype=torch.float64) - 0.5)
        x = input_grad_points(500).double().requires_grad_(True)
        xd = x.detach()
        outside = ((xd < box_min) | (xd > box_max)).any(-1)
        on_face = ((xd == box_min) | (xd == box_max)).any(-1)
        assert outside.sum() >= 50 and on_face.sum() >= 96
        for a in range(3):      # outside on each side, on each face
            assert (xd[:, a] < box_min[a]).any() and (xd[:, a] > box_max[a]).any()
            assert (xd[:, a] == box_min[a]).any() and (xd[:, a] == box_max[a]).any()
        dfeat = torch.randn(500, 2 * n_levels, generator=g, dtype=torch.float64)
        feat, _ = oracle.hash_encode(x, tables, box_min, box_max, res, SMALL_T)
        (want,) = torch.autograd.grad(feat, x, dfeat)
        got = encode_dx_closed_form(oracle, xd, tables, box_min, box_max, res, SMALL_T, dfeat)
        assert rel_err(got, want) <= 1e-13, (n_levels, rel_err(got, want))
        # the trap: weights of the clamped point give another gradient outside the box
        xc = torch.clamp(xd, min=box_min, max=box_max)
        bad = encode_dx_closed_form(oracle, xc, tables, box_min, box_max, res, SMALL_T, dfeat)
        assert rel_err(bad[outside], want[outside]) > 1e-3


def test_sh_ddirs_closed_form_is_autograd_of_the_oracle(oracle):
    g = torch.Generator().manual_seed(4)
    d = sh_dirs(1000).double().requires_grad_(True)
    go = torch.randn(1000, 16, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(oracle.sh_encode(d), d, go)
    got = sh_ddirs_closed_form(oracle, d.detach(), go)
    assert rel_err(got, want) <= 1e-13, rel_err(got, want)


def test_header_declares_and_lib_binds_the_input_gradients(hn):
    src = open(HEADER).read()
    lib = hn._lib.lib()
    for name in NEW:
        m = re.search(r"^int32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", src, re.M)
        assert m, f"{name} not declared in the header"
        assert name in hn._lib.SIGNATURES, name
        assert len(hn._lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
        assert hasattr(lib, name), name
    assert lib.hn_abi_version() == 14       # additive: the ABI number stays


def test_input_gradient_argument_validation_without_gpu(hn):
    L = hn._lib
    lib = L.lib()
    g = L.make_grid(16, 2, 14, [-1] * 3, [1] * 3, [[0.1] * 3] * 16)
    x = 16      # never dereferenced: validation happens before any launch
    assert lib.hn_encode_bwd_input(g, None, 0, None, None, None, None) == 0     # n == 0 is a no-op
    assert lib.hn_encode_bwd_input(g, x, 8, x, x, None, None) == 1
    assert lib.hn_encode_bwd_input(g, x, 8, None, x, x, None) == 1
    assert lib.hn_encode_bwd_input(g, x, -1, x, x, x, None) == 2
    g.n_features = 4
    assert lib.hn_encode_bwd_input(g, x, 8, x, x, x, None) == 2                 # check_grid
    assert lib.hn_sh_bwd(None, None, 0, None, None) == 0
    assert lib.hn_sh_bwd(x, None, 8, x, None) == 1
    assert lib.hn_composite_bwd_inputs(None, None, None, None, 0, 64, 1, None, None, None, None, None, None, None,
                                       None) == 0
    assert lib.hn_composite_bwd_inputs(x, x, x, None, 4, 300, 1, None, None, None, None, None, x, x, None) == 2
    assert lib.hn_composite_bwd_inputs(None, x, x, None, 4, 64, 1, None, None, None, None, None, x, x, None) == 1
    assert lib.hn_composite_bwd_inputs(x, x, x, None, 4, 64, 1, None, None, None, None, None, None, None,
                                       None) == 0                                # neither output asked for

