"""hn_render_fwd_res_map without a device: what a workgroup of the resident
forward holds of a packed net in LDS, and where (the map at kResRegs, hn_mlp.h;
the host entry calls the functions the kernel copies and reads through),
against a plain restatement of the rule.

A packed net's forward regions are OB x groups x 256 floats, a group 64 lanes of
4 floats, a split region's chunk 3 groups (parts 0-2); lane = 32 h + output row.
Held per net: sigma_net.0 (F0) whole, sigma_net.1 (F1) rows 0-15, color_net.0's
geo half (F2G) whole, color_net.2 (F4) rows 0-2.  The packing leaves the other
rows of F1 and F4 zero, and the kernel takes zero bits for them.  color_net.1
(F3) is not held: holding parts 0 and 1 of the fine net's measured no faster."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hashnerf_amd.h")
E_SHAPE = 2
NAMES = ("F0", "F1", "F2G", "F2S", "F3", "F4")
KS = dict(F0=16, F1=32, F2G=8, F2S=8, F3=32, F4=32)      # f32 k-steps
OB = dict(F0=2, F1=1, F2G=2, F2S=2, F3=2, F4=1)          # 32-row output blocks
NS = 3                                                   # parts of a chunk
GPO = {r: NS * KS[r] // 8 for r in NAMES}                # groups per output block
REG_OFF = dict(zip(NAMES, np.cumsum([0] + [OB[r] * GPO[r] * 256 for r in NAMES])[:-1]))
FWD_FLOATS = sum(OB[r] * GPO[r] * 256 for r in NAMES)    # 18432: the forward regions of a packed net
KEEP = dict(F0=32, F1=16, F2G=32, F4=3)                  # rows kept of each 32-lane half
NET_BYTES = 12288 + 6144 + 6144 + 1152                   # F0 | F1 rows 0-15 | F2G | F4 rows 0-2
# the kernel's other LDS in its loss-mode resident instantiation: 16 waves x 1472 floats, 96 floats of grid
# sizes, 1024 key bytes
OTHER_LDS = 16 * 1472 * 4 + 96 * 4 + 1024
LDS_LIMIT = 163840


def parts_held(fine, r):
    return {"F0": NS, "F1": NS, "F2G": NS, "F4": NS, "F3": 0, "F2S": 0}[r]


def res_map(hn, fine):
    f = hn._lib.lib().hn_render_fwd_res_map
    n = f(fine, None, 0, None, 0)
    assert n > 0
    src = np.full(n, -7, np.int32)
    at = np.full(FWD_FLOATS // 4, -7, np.int32)
    assert f(fine, src.ctypes.data, n, at.ctypes.data, at.size) == n
    return n, src, at


def test_export_and_signature(hn):
    text = open(HEADER).read()
    assert re.search(r"^int32_t hn_render_fwd_res_map\(", text, re.M)
    assert "hn_render_fwd_res_map" in text[:text.index("#define HN_ABI_VERSION")], "listed in the ABI comment"
    L = hn._lib
    res, args = L.SIGNATURES["hn_render_fwd_res_map"]
    assert res is C.c_int32 and len(args) == 5
    assert L.lib().hn_abi_version() == L.ABI_VERSION == 14
    assert L.MLP_PACKED_FLOATS == 30208 and FWD_FLOATS == 18432


def test_validation(hn):
    f = hn._lib.lib().hn_render_fwd_res_map
    n = f(0, None, 0, None, 0)
    src, at = np.zeros(n, np.int32), np.zeros(FWD_FLOATS // 4, np.int32)
    for fine in (-1, 2):
        assert f(fine, src.ctypes.data, n, at.ctypes.data, at.size) == -E_SHAPE
    assert f(0, src.ctypes.data, n - 1, None, 0) == -E_SHAPE
    assert f(0, None, 0, at.ctypes.data, at.size - 1) == -E_SHAPE
    assert f(0, src.ctypes.data, n, None, 0) == n == f(0, None, 0, at.ctypes.data, at.size)


def test_image_size_is_the_budget(hn):
    nc, nf = res_map(hn, 0)[0], res_map(hn, 1)[0]
    assert 4 * nc == 4 * nf == NET_BYTES == 25728
    assert 4 * (nc + nf) == 51456
    assert OTHER_LDS + 4 * (nc + nf) == 147072 <= LDS_LIMIT


@pytest.mark.parametrize("fine", [0, 1])
def test_src_is_injective_and_within_the_forward_regions(hn, fine):
    n, src, _ = res_map(hn, fine)
    assert src.min() >= 0 and src.max() < FWD_FLOATS
    assert np.unique(src).size == n


@pytest.mark.parametrize("fine", [0, 1])
def test_every_lane_of_every_group(hn, fine):
    """Kept lanes: 4 consecutive image floats at a 16-byte aligned offset whose
    src are the lane's 4 packed floats, each run of kept lanes at consecutive
    addresses, and together they are the whole image.  Everything else: -1; a
    group has zero lanes only in F1 (rows >= 16) and F4 (rows >= 3)."""
    n, src, at = res_map(hn, fine)
    covered = np.zeros(n, bool)
    lanes = np.arange(64)
    for r in NAMES:
        first = None
        for ob in range(OB[r]):
            for g in range(GPO[r]):
                base = REG_OFF[r] + (ob * GPO[r] + g) * 256
                a = at[base // 4:base // 4 + 64]
                held = g % NS < parts_held(fine, r)
                kept = held & ((lanes & 31) < KEEP.get(r, 32))
                assert np.array_equal(a >= 0, kept), (r, ob, g)
                assert np.all(a[~kept] == -1)
                if not held:
                    continue
                ak = a[kept]
                assert np.all(ak % 4 == 0) and np.all(ak + 3 < n)
                for d in range(4):
                    assert np.array_equal(src[ak + d], base + 4 * lanes[kept] + d), (r, ob, g, d)
                    assert not covered[ak + d].any()
                    covered[ak + d] = True
                # 16 B per lane at consecutive addresses within each 16-lane group
                both = kept[:-1] & kept[1:] & (lanes[:-1] // 16 == lanes[1:] // 16)
                assert np.all(a[1:][both] == a[:-1][both] + 4), (r, ob, g)
                first = int(ak.min()) if first is None else min(first, int(ak.min()))
        if parts_held(fine, r):
            assert first % 4 == 0, r      # the region starts 16-byte aligned
    assert covered.all()


def test_zero_lanes_are_the_two_named_sets(hn):
    for fine in (0, 1):
        _, _, at = res_map(hn, fine)
        for r in NAMES:
            if not parts_held(fine, r):
                continue
            a = at[REG_OFF[r] // 4:REG_OFF[r] // 4 + OB[r] * GPO[r] * 64].reshape(-1, NS, 64)
            a = a[:, :parts_held(fine, r)]                 # the held groups
            zero = (a < 0).reshape(-1, 64)
            want = (np.arange(64) & 31) >= {"F1": 16, "F4": 3}.get(r, 32)
            assert np.all(zero == want), r


def test_color_net_1_is_loaded_at_use_in_both_nets(hn):
    _, srcc, atc = res_map(hn, 0)
    _, srcf, atf = res_map(hn, 1)
    for at in (atc, atf):
        assert np.all(at[REG_OFF["F3"] // 4:REG_OFF["F4"] // 4] == -1)    # every part of color_net.1
        assert np.all(at[REG_OFF["F2S"] // 4:REG_OFF["F3"] // 4] == -1)   # the SH half: once per ray, at use
    # the two nets' images are laid out alike
    assert np.array_equal(srcf, srcc) and np.array_equal(atf, atc)
