"""The resident form's colour-net fragments (hn_render_fwd_form 2): its
workgroups read color_net.0's geo half and color_net.2 from their LDS image
beside the sigma nets (color_net.1 stays loaded at use), with the rows the
packing leaves zero (sigma_net.1 rows 16-31, color_net.2 rows 3-31) not held at
all: a lane of those rows takes zero bits.  So (1) the packed buffer must hold
zero bits there, whatever the weights, and (2) with density everywhere -- every
tile of every ray runs the colour net -- form 2 equals form 1 bit for bit.

Shapes: T=14, finest 64; B in {1, 16, 17}: one ray, exactly one workgroup, one
+ one ray."""
import numpy as np
import pytest
import torch

import test_gpu_fwd_resident as R
from gpu_support import OUT_KEYS, SMALL_T as T, backward_after_loss_forward as backward, bits_equal, small_scene

DEV = torch.device("cuda:0")
NAMES = ("F0", "F1", "F2G", "F2S", "F3", "F4")
GROUPS = dict(F0=12, F1=12, F2G=6, F2S=6, F3=24, F4=12)       # OB x groups per output block
REG_OFF = dict(zip(NAMES, np.cumsum([0] + [GROUPS[r] * 256 for r in NAMES])[:-1]))
FWD_FLOATS = 18432
DRAWS = [("target", "rand", 3), ("t_rand", "rand", 64), (("u", 128), "rand", 128), (("u", 64), "rand", 64)]


def res_at(hn, fine):
    """hn_render_fwd_res_map's second array as [group][lane] per forward region."""
    at = np.full(FWD_FLOATS // 4, -7, np.int32)
    assert hn._lib.lib().hn_render_fwd_res_map(fine, None, 0, at.ctypes.data, at.size) > 0
    return {r: at[REG_OFF[r] // 4:REG_OFF[r] // 4 + GROUPS[r] * 64].reshape(GROUPS[r], 64) for r in NAMES}


def density_everywhere(emb, ws, hn):
    """The coarsest level's first feature +0.5 at every vertex (a point's
    trilinear weights sum to 1, inside the box and out), and both nets' raw sigma
    relu of it alone, as in test_gpu_fwd_resident.scene: 0.5 at every sample."""
    i = torch.arange(17)
    v = torch.stack(torch.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3)
    emb.table[0, hn.embedding.hash(v, T).to(DEV), 0] = 0.5
    for s0, s1 in ((ws[0], ws[1]), (ws[5], ws[6])):
        s0[0].zero_()
        s0[0, 0] = 1.0
        s1[0].zero_()
        s1[0, 0] = 1.0


def scene(hn, B, colour="init"):
    """colour: the colour nets' weights as initialised, plain randn (their third
    bf16 part matters), or randn rounded to bf16 (parts 1 and 2 are zero)."""
    def edit(emb, nets, ws):
        density_everywhere(emb, ws, hn)
        if colour != "init":
            g = torch.Generator().manual_seed(77)
            for j in (2, 3, 4, 7, 8, 9):
                w = torch.randn(ws[j].shape, generator=g)
                ws[j].copy_((w.bfloat16().float() if colour == "bf16" else w).to(DEV))
    return small_scene(hn, ("colour", B, colour), B, 400 + B, DRAWS, edit)


def packed_nets(hn, ws):
    """Both nets packed by a one-ray forward: [2][MLP_PACKED_FLOATS] int32 bits from the workspace."""
    from hashnerf_pytorch_amd import functional as HF
    s = scene(hn, 1)
    v = dict(loss=False, ni=128, skip=True, noise=False, white=True)
    wsb = torch.zeros(hn._lib.lib().hn_render_workspace_bytes(R.make_cfg(HF, s, v), 1), dtype=torch.uint8, device=DEV)
    R.forward(HF, s, v, "resident", keep_feat=False, ws=ws, wsb=wsb)
    torch.cuda.synchronize()
    n = hn._lib.MLP_PACKED_FLOATS
    return wsb[:2 * n * 4].view(torch.int32).view(2, n).cpu().numpy()


def check_compare(hn, s, v, B):
    """Form 1 against form 2, everything test_gpu_fwd_resident compares, and
    every tile of either pass with a positive raw sigma: none skips the colour net."""
    from hashnerf_pytorch_amd import functional as HF
    res = []
    for form in ("ring", "resident"):
        out, st = R.forward(HF, s, v, form)
        torch.cuda.synchronize()
        marks = grads = None
        if v["loss"]:
            marks = R.workspace_marks(HF, st, B, v)
            grads = backward(HF, s, out, st)
            torch.cuda.synchronize()
        res.append((out, st, marks, grads))
    (oa, sa, ma, ga), (ob, sb, mb, gb) = res
    for raw in (oa["raw_c"], oa["raw_f"], ob["raw_c"], ob["raw_f"]):
        assert bool((raw[..., 3].reshape(B, -1, 32) > 0).any(-1).all()), "a tile without density"
    for k in OUT_KEYS:
        assert bits_equal(oa[k], ob[k]), k
    assert torch.count_nonzero(oa["raw_f"][..., :3]) > 0 and torch.count_nonzero(oa["raw_c"][..., :3]) > 0
    assert bits_equal(sa.fine_src, sb.fine_src), "fine_src"
    (fa, stored), (fb, _) = R.stored_tiles(sa, oa, v), R.stored_tiles(sb, ob, v)
    assert bool(stored[:, :2 + (64 + v["ni"]) // 32].all())
    assert torch.equal(fa, fb), "feature cache and masks"
    assert torch.count_nonzero(fa[:, :8192]) > 0 and torch.count_nonzero(fa[:, 8192:]) > 0
    if v["loss"]:
        for name, x, y in zip(("d raw", "marks", "stamp"), ma, mb):
            assert bits_equal(x, y), name
        assert torch.count_nonzero(ma[0]) > 0 and torch.count_nonzero(ma[2]) > 0
        names = ("loss", "d_table") + tuple(f"NeRFSmall gradient {j}" for j in range(10))
        for name, x, y in zip(names, ga, gb):
            assert bits_equal(x, y), name
        assert torch.count_nonzero(ga[1]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("special", [False, True], ids=["normal", "special"])
def test_dropped_lanes_are_zero_bits_in_the_packed_nets(hn, special):
    """Two random nets packed; every packed float of a lane the map drops from a
    held group is all-zero bits, and each held region has nonzero kept words.
    special: -0.0, denormals and 1e30 among the kept rows' weights."""
    ws = R.make_nets(hn, seed=11)
    if special:
        # (sigma_net.1's geo rows and color_net.2 of both nets: the density row stays as drawn, so the packing
        # forward's sampling sees ordinary weights)
        vals = torch.tensor([-0.0, 1e-40, -1e-42, 1e30, -1e30], device=DEV)
        for w in (ws[1][1:], ws[4], ws[6][1:], ws[9]):
            flat = w.reshape(-1)
            idx = torch.arange(0, flat.numel(), 7, device=DEV)
            flat[idx] = vals[torch.arange(idx.numel(), device=DEV) % vals.numel()]
            assert flat.data_ptr() == w.data_ptr()
        for w in (ws[1], ws[4]):
            assert bool((w == 0).any()) and bool((w.abs() > 1e29).any()) and bool(((w != 0) & (w.abs() < 1e-38)).any())
    P = packed_nets(hn, ws)
    dropped_lanes = {"F1": 32, "F4": 58}
    for fine in (0, 1):
        at = res_at(hn, fine)
        for r in NAMES:
            held = (at[r] >= 0).any(1)                                   # groups with a kept lane
            if not held.any():
                continue
            words = P[fine, REG_OFF[r]:REG_OFF[r] + GROUPS[r] * 256].reshape(GROUPS[r], 64, 4)
            dropped = held[:, None] & (at[r] < 0)
            assert np.all(dropped.sum(1)[held] == dropped_lanes.get(r, 0)), r
            assert not words[dropped].any(), (fine, r)
            assert words[at[r] >= 0].any(), (fine, r)


@pytest.mark.gpu
@pytest.mark.parametrize("loss", [False, True], ids=["fwd", "loss"])
@pytest.mark.parametrize("ni", [128, 64])
@pytest.mark.parametrize("B", [1, 16, 17])
def test_every_tile_takes_the_colour_path_bitwise(hn, B, ni, loss):
    check_compare(hn, scene(hn, B), dict(loss=loss, ni=ni, skip=True, noise=False, white=True), B)


@pytest.mark.gpu
@pytest.mark.parametrize("colour", ["randn", "bf16"])
def test_part_split_of_color_net_1(hn, colour):
    """B = 17 with colour weights whose third bf16 part matters (plain randn:
    all three parts of every colour chunk are nonzero, those read from LDS and
    those loaded at use), and with colour weights rounded to bf16 (parts 1 and
    2 are zero)."""
    B = 17
    s = scene(hn, B, colour)
    P = packed_nets(hn, s.ws)
    for fine in (0, 1):
        f3 = P[fine, REG_OFF["F3"]:REG_OFF["F4"]].reshape(8, 3, 256)    # [chunk][part][word]
        assert f3[:, 0].any()
        if colour == "randn":
            assert f3[:, 1].any() and f3[:, 2].any()
        else:
            assert not f3[:, 1:].any()
    for loss in (False, True):
        check_compare(hn, s, dict(loss=loss, ni=128, skip=True, noise=False, white=True), B)
