"""hn_sample_pool_ordered without a device: the export and its ctypes
signature, the argument checks (all made before any launch) and the numpy
restatement of the key (pool_order_key.py) that the GPU tests compare the
kernel against, pinned on the pool fixture."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT, golden
from pool_order_key import pool_key, pool_perm

HEADER = os.path.join(ROOT, "include", "hashnerf_amd.h")
OK, E_NULL, E_SHAPE = 0, 1, 2


def test_export_and_signature(hn):
    src = open(HEADER).read()
    assert re.search(r"^int32_t hn_sample_pool_ordered\(", src, re.M)
    assert re.search(r"^#define HN_POOL_ORDER_MAX 8192$", src, re.M)
    L = hn._lib
    assert hasattr(L.lib(), "hn_sample_pool_ordered")
    res, args = L.SIGNATURES["hn_sample_pool_ordered"]
    assert res is C.c_int32 and len(args) == 15
    assert L.POOL_ORDER_MAX == hn.functional.POOL_ORDER_MAX == 8192
    assert L.lib().hn_abi_version() == L.ABI_VERSION == 14


def test_validation_without_device(hn):
    L = hn._lib
    f = L.lib().hn_sample_pool_ordered
    p = L.HnRayPool()
    p.n_images, p.H, p.W, p.pose_stride = 3, 64, 64, 16           # 12,288 positions
    p.near, p.far = 2., 6.
    x = C.c_void_p(16)   # never dereferenced: validation happens before any launch
    lo, hi = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)
    assert f(p, None, None, None, 0, 0, None, None, None, None, None, 0, None, 0, None) == OK
    assert f(p, x, x, x, 0, 0, lo, hi, x, x, x, 0, None, 0, None) == OK
    assert f(None, x, x, x, 0, 8, lo, hi, x, x, x, 0, None, 0, None) == E_NULL
    assert f(p, x, x, x, 0, 8, lo, hi, None, None, None, 0, None, 0, None) == E_NULL     # no outputs
    assert f(p, x, x, x, 0, 8, lo, hi, x, None, None, 0, None, 0, None) == E_NULL
    assert f(p, None, x, x, 0, 8, lo, hi, x, x, None, 0, None, 0, None) == E_NULL
    assert f(p, x, x, x, 0, 8, None, None, x, x, None, 0, None, 0, None) == E_NULL       # no box
    assert f(p, x, x, x, 0, 8, lo, None, x, x, None, 0, None, 0, None) == E_NULL
    assert f(p, x, x, x, 0, 8193, lo, hi, x, x, None, 0, None, 0, None) == E_SHAPE       # > HN_POOL_ORDER_MAX
    assert f(p, x, x, x, 12281, 8, lo, hi, x, x, None, 0, None, 0, None) == E_SHAPE      # past the pool
    assert f(p, x, x, x, -1, 8, lo, hi, x, x, None, 0, None, 0, None) == E_SHAPE
    assert f(p, x, x, x, 0, -8, lo, hi, x, x, None, 0, None, 0, None) == E_SHAPE
    flat = (C.c_float * 3)(1, -1, 1)                                                     # max == min on y
    assert f(p, x, x, x, 0, 8, (C.c_float * 3)(-1, -1, -1), flat, x, x, None, 0, None, 0, None) == E_SHAPE
    assert f(p, x, x, x, 0, 8, hi, lo, x, x, None, 0, None, 0, None) == E_SHAPE          # reversed
    inf = (C.c_float * 3)(1, 1, float("inf"))
    assert f(p, x, x, x, 0, 8, lo, inf, x, x, None, 0, None, 0, None) == E_SHAPE
    nan = (C.c_float * 3)(float("nan"), -1, -1)
    assert f(p, x, x, x, 0, 8, nan, hi, x, x, None, 0, None, 0, None) == E_SHAPE
    # the draws: make_uni's checks, as hn_uniform_philox reports them
    d = (L.HnUniformDraw * 5)()
    assert L.lib().hn_uniform_philox(1, d, 5, None) == E_SHAPE                           # n_draws = 5
    assert f(p, x, x, x, 0, 8, lo, hi, x, x, None, 1, d, 5, None) == E_SHAPE
    assert f(p, x, x, x, 0, 8, lo, hi, x, x, None, 1, None, 1, None) == E_NULL
    d[0].numel, d[0].threads, d[0].offset = 8, 256, 2                                    # offset not a multiple of 4
    assert f(p, x, x, x, 0, 8, lo, hi, x, x, None, 1, d, 1, None) == E_SHAPE
    d[0].offset, d[0].out = 4, None
    assert f(p, x, x, x, 0, 8, lo, hi, x, x, None, 1, d, 1, None) == E_NULL              # no output
    p.pose_stride = 9
    assert f(p, x, x, x, 0, 8, lo, hi, x, x, None, 0, None, 0, None) == E_SHAPE          # hn_sample_pool's own


def _fixture_rays():
    r = golden("pool_rays")["rays_rgb"]                    # [1440, (ro, rd, rgb), 3]
    return np.concatenate([r[:, 0], r[:, 1]], -1)


def test_numpy_key_on_the_fixture():
    """The fixture exercises ties, clamping and a near-injective key: the
    counts below were computed from it and pin the helper."""
    rays = _fixture_rays()
    assert rays.shape == (1440, 6) and rays.dtype == np.float32
    k10, c10 = pool_key(rays, [-1.] * 3, [1.] * 3, 2., 6.)
    assert k10.dtype == np.uint32 and int(k10.max()) < 2 ** 30
    assert len(np.unique(k10)) == 1338
    assert int(c10.sum()) == 460                           # 31.9 % of the rays clamp on some axis
    assert round(100. * c10.mean(), 1) == 31.9
    k15, _ = pool_key(rays, [-1.5] * 3, [1.5] * 3, 2., 6.)
    assert len(np.unique(k15)) == 1438


def test_numpy_key_bits_and_order():
    """Hand-made rays: axis a's cell c lands on bits 3k + a, NaN -> cell 0,
    the box's far face -> cell 1023, and equal keys keep their positions."""
    rays = np.zeros((6, 6), dtype=np.float32)              # d = 0: the point is o
    rays[0, :3] = (-1., -1., -1.)                          # cell (0, 0, 0)
    rays[1, :3] = (1., -1., -1.)                           # x = 1023
    rays[2, :3] = (-1., 5., -1.)                           # y clamps to 1023
    rays[3, :3] = (-1., -1., np.nan)                       # NaN -> 0
    rays[4, :3] = (-1. + 2. * 5 / 1024, -1., -1. + 2. * 2 / 1024)   # x = 5 (0b101), z = 2
    rays[5, :3] = (-1., -1., -1.)
    k, c = pool_key(rays, [-1.] * 3, [1.] * 3)
    x1023 = sum(1 << (3 * b) for b in range(10))
    assert list(k) == [0, x1023, x1023 << 1, 0, (1 << 0) | (1 << 6) | (1 << (3 + 2)), 0]
    assert list(c) == [False, False, True, True, False, False]
    assert list(pool_perm(k)) == [0, 3, 5, 4, 1, 2]
