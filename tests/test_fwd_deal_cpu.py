"""hn_render_fwd_deal without a device: which rays the workgroups of the
resident forward take (fwd_res_deal, hn_render_fwd.h; the host entry calls the
function the kernel calls), against a plain restatement of the rule.

Workgroup b of nb = ceil(n_rays / 16) runs on XCD b % 8 and takes four runs of
4 consecutive rays.  Where nb is a multiple of 32 (and at most 2048: the keys
of an XCD's runs are one LDS byte each, 1024 of them) the batch is cut into
segments of 64 rays, XCD x owns the segments = x (mod 8), sorts their runs
stably by descending key and deals them in rounds over its nb / 8 workgroups,
even rounds forward, odd rounds backward.  Every other grid: one run from each
quarter of the XCD's band (nb % 8 == 0) or of the batch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hashnerf_amd.h")
OK, E_NULL, E_SHAPE = 0, 1, 2
SEG_RUNS = 16     # 64 rays
MAX_RUNS = 1024   # per XCD


def deal(hn, n_rays, nb, keys):
    out = np.full(4 * nb, -1, np.int32)
    k = None if keys is None else np.ascontiguousarray(keys, np.uint8)
    st = hn._lib.lib().hn_render_fwd_deal(n_rays, nb, None if k is None else k.ctypes.data, out.ctypes.data)
    assert st == OK
    return out.reshape(nb, 4)


def band_map(nb):
    """The map before the deal, and of every grid it does not apply to."""
    b, s = np.meshgrid(np.arange(nb), np.arange(4), indexing="ij")
    run = (b % 8) * (nb // 8 * 4) + s * (nb // 8) + b // 8 if nb % 8 == 0 else s * nb + b
    return 4 * run


def rule_applies(nb):
    return nb % 32 == 0 and nb // 2 <= MAX_RUNS


def expected(n_rays, nb, keys):
    if not rule_applies(nb):
        return band_map(nb)
    keys = np.zeros(4 * nb, np.int64) if keys is None else np.asarray(keys, np.int64).copy()
    keys[4 * np.arange(4 * nb) >= n_rays] = 0
    nw, nr = nb // 8, nb // 2
    out = np.empty((nb, 4), np.int64)
    for x in range(8):
        j = np.arange(nr)
        runs = (j // SEG_RUNS * 8 + x) * SEG_RUNS + j % SEG_RUNS      # the XCD's runs in batch order
        order = sorted(range(nr), key=lambda i: -keys[runs[i]])      # (sorted is stable)
        for s in range(4):
            rnd = order[s * nw:(s + 1) * nw]
            if s % 2:
                rnd = rnd[::-1]
            for w in range(nw):
                out[8 * w + x, s] = 4 * runs[rnd[w]]
    return out


def key_sets(n_rays, nb, seed):
    rng = np.random.default_rng(seed)
    half = np.where(np.arange(4 * nb) < 2 * nb, 4, 0)
    return {"equal": None, "zeros": np.zeros(4 * nb, np.uint8), "fours": np.full(4 * nb, 4, np.uint8),
            "random": rng.integers(0, 5, 4 * nb), "halves": half}


def check(hn, n_rays, seed=0):
    nb = (n_rays + 15) // 16
    for name, keys in key_sets(n_rays, nb, seed).items():
        got = deal(hn, n_rays, nb, keys)
        # every run below 16 nb once: every ray below n_rays exactly once, none at or past 16 nb
        assert np.array_equal(np.sort(got.ravel()), 4 * np.arange(4 * nb)), (n_rays, name)
        assert np.array_equal(got, expected(n_rays, nb, keys)), (n_rays, name)
    return nb


def test_export_and_signature(hn):
    src = open(HEADER).read()
    assert re.search(r"^int32_t hn_render_fwd_deal\(", src, re.M)
    assert "hn_render_fwd_deal" in src[:src.index("#define HN_ABI_VERSION")], "listed in the ABI comment"
    L = hn._lib
    assert hasattr(L.lib(), "hn_render_fwd_deal")
    res, args = L.SIGNATURES["hn_render_fwd_deal"]
    assert res is C.c_int32 and len(args) == 4
    assert L.lib().hn_abi_version() == L.ABI_VERSION == 14


def test_validation(hn):
    f = hn._lib.lib().hn_render_fwd_deal
    out = np.zeros(8, np.int32)
    keys = np.zeros(8, np.uint8)
    assert f(20, 2, keys.ctypes.data, None) == E_NULL
    assert f(33, 2, keys.ctypes.data, out.ctypes.data) == E_SHAPE     # rays past the grid
    assert f(-1, 2, keys.ctypes.data, out.ctypes.data) == E_SHAPE
    assert f(0, 0, keys.ctypes.data, out.ctypes.data) == E_SHAPE
    keys[3] = 5
    assert f(20, 2, keys.ctypes.data, out.ctypes.data) == E_SHAPE     # a key above 4
    keys[3] = 4
    assert f(20, 2, keys.ctypes.data, out.ctypes.data) == OK
    assert f(0, 2, None, out.ctypes.data) == OK


@pytest.mark.parametrize("lo", range(1, 701, 100))
def test_small_batches(hn, lo):
    """Every n_rays in 1..700 with the grid the launch uses.  nb = 32 (497..512
    rays) is the only one of these grids the rule applies to; all the others
    keep the earlier map."""
    for n_rays in range(lo, lo + 100):
        nb = check(hn, n_rays, seed=n_rays)
        assert rule_applies(nb) == (nb == 32)


@pytest.mark.parametrize("n_rays", [1024, 4096, 4090, 8192, 32768])
def test_full_batches(hn, n_rays):
    nb = check(hn, n_rays, seed=n_rays)
    assert rule_applies(nb)


@pytest.mark.parametrize("nb", [1, 7, 8, 24, 63, 72, 257, 2080, 4096])
def test_other_grids_keep_the_earlier_map(hn, nb):
    """No multiple of 32, or more than 1024 runs per XCD: the earlier map,
    whatever the keys."""
    assert not rule_applies(nb)
    keys = np.random.default_rng(nb).integers(0, 5, 4 * nb)
    for k in (None, keys):
        assert np.array_equal(deal(hn, 16 * nb, nb, k), band_map(nb))


def test_equal_keys_is_segment_interleave_and_snake(hn):
    """With all keys equal the sort keeps the batch's order: XCD x's workgroup
    w takes, in round s, run s nw + (w or nw - 1 - w) of its segments' runs."""
    nb, nw = 256, 32
    got = deal(hn, 4096, nb, None)
    assert np.array_equal(got, deal(hn, 4096, nb, np.full(4 * nb, 3)))
    for b in range(nb):
        for s in range(4):
            x, w = b % 8, b // 8
            j = s * nw + (nw - 1 - w if s % 2 else w)
            assert got[b, s] == 4 * ((j // 16 * 8 + x) * 16 + j % 16)


def test_halves_are_balanced(hn):
    """What the deal is for: with the batch's first half heavy (key 4) and its
    second half empty (key 0), 4,096 rays, every workgroup's key sum is within
    one run (4) of the mean.  (The band map gives whole XCDs 16 and others 0.)"""
    nb = 256
    keys = np.where(np.arange(4 * nb) < 2 * nb, 4, 0)
    got = deal(hn, 4096, nb, keys)
    sums = keys[got // 4].sum(1)
    assert np.all(np.abs(sums - sums.mean()) <= 4), (sums.min(), sums.max(), sums.mean())
    old = keys[band_map(nb) // 4].sum(1)
    assert old.max() == 16 and old.min() == 0
