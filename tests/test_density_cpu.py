"""Density queries without a GPU: the C ABI's argument checks (no launch is
made), the lattice's coordinate rule, density_grid's cell-centre lattice and
the occupancy words' layout."""
import ctypes as C

import numpy as np
import pytest
import torch

X = C.c_void_p(16)   # never dereferenced: every check runs before any launch


def _field(L, levels=16):
    g = L.make_grid(levels, 2, 12, [-1] * 3, [1] * 3, [[0.1] * 3] * levels)
    w = L.HnMlp()
    for k in ("sigma0", "sigma1", "color0", "color1", "color2"):
        setattr(w, k, 16)
    return g, w


def _lattice(L, dims):
    lat = L.HnLattice()
    for a in range(3):
        lat.lo[a], lat.step[a], lat.dims[a] = -1.0, 0.1, dims[a]
    return lat


def test_lattice_struct_size(hn):
    assert C.sizeof(hn._lib.HnLattice) == 40


def test_points_argument_checks(hn):
    L = hn._lib
    lib = L.lib()
    g, w = _field(L)
    ws = lib.hn_mlp_workspace_bytes()
    ok = dict(g=g, w=w, table=X, x=X, n=33, thr=0.0, sigma=X, occ=X, ws=X, nbytes=ws)

    def call(**kw):
        a = {**ok, **kw}
        return lib.hn_density_points(a["g"], a["w"], a["table"], a["x"], a["n"], a["thr"], a["sigma"], a["occ"],
                                     a["ws"], a["nbytes"], None)

    assert call(g=None) == 1
    assert call(w=None) == 1
    w1 = L.HnMlp()
    w1.sigma0 = w1.sigma1 = w1.color0 = w1.color1 = 16                       # one tensor of the net missing
    assert call(w=w1) == 1
    assert call(table=None) == 1
    assert call(x=None) == 1
    assert call(sigma=None, occ=None) == 1                                   # both outputs NULL
    assert call(ws=None) == 1
    assert call(g=_field(L, 15)[0]) == 2                                     # a 15-level grid
    g4 = _field(L)[0]
    g4.n_features = 4
    assert call(g=g4) == 2                                                   # check_grid's own refusals
    assert call(n=-1) == 2
    assert call(n=L.DENSITY_MAX_POINTS + 1) == 2
    assert call(nbytes=ws - 4) == 3                                          # a short workspace
    assert call(n=0) == 0                                                    # nothing to do
    assert call(n=0, x=None, ws=None, nbytes=0) == 0
    assert lib.hn_status_string(call(nbytes=0)).decode() == "workspace too small"


def test_lattice_argument_checks(hn):
    L = hn._lib
    lib = L.lib()
    g, w = _field(L)
    ws = lib.hn_mlp_workspace_bytes()
    ok = dict(g=g, w=w, table=X, lat=_lattice(L, (5, 3, 2)), thr=0.0, sigma=X, occ=X, ws=X, nbytes=ws)

    def call(**kw):
        a = {**ok, **kw}
        return lib.hn_density_lattice(a["g"], a["w"], a["table"], a["lat"], a["thr"], a["sigma"], a["occ"], a["ws"],
                                      a["nbytes"], None)

    assert call(g=None) == 1
    assert call(w=None) == 1
    assert call(table=None) == 1
    assert call(lat=None) == 1
    assert call(sigma=None, occ=None) == 1
    assert call(ws=None) == 1
    assert call(g=_field(L, 15)[0]) == 2
    for dims in ((0, 3, 2), (5, -1, 2), (5, 3, 0)):                          # a zero or negative dim
        assert call(lat=_lattice(L, dims)) == 2, dims
    # the product past 2^31 tiles of 32 points (2^36): just past after two factors; and, with two
    # factors that reach the bound exactly, third factors whose product would wrap int64 to a
    # value inside the bound (2^64 + 2^36, 0 mod 2^64, -2^36 mod 2^64)
    assert (1 << 18) * (1 << 18) == L.DENSITY_MAX_POINTS
    assert call(lat=_lattice(L, (1 << 18, (1 << 18) + 1, 1))) == 2
    assert call(lat=_lattice(L, ((1 << 31) - 1,) * 3)) == 2
    for nz in ((1 << 28) + 1, 1 << 28, (1 << 31) - 1, 2):
        assert call(lat=_lattice(L, (1 << 18, 1 << 18, nz))) == 2, nz
        assert call(lat=_lattice(L, (nz, 1 << 18, 1 << 18))) == 2, nz
    # the bound itself is accepted: the call goes on to the workspace check (and launches nothing)
    assert call(lat=_lattice(L, (1 << 18, 1 << 18, 1)), nbytes=ws - 4) == 3
    assert call(nbytes=ws - 4) == 3


@pytest.mark.parametrize("dims", [(5, 3, 2), (33, 2, 3)])
def test_lattice_coords_rule(hn, dims):
    """lattice_coords is lo + arange * step in float32, bit for bit, laid out [nz, ny, nx, 3]."""
    HF = hn.functional
    lo, step = (-1.7, 0.31, 2.05), (0.113, 0.977, -0.25)
    c = HF.lattice_coords(lo, step, dims)
    nx, ny, nz = dims
    assert c.shape == (nz, ny, nx, 3) and c.dtype == torch.float32
    ax = [torch.tensor(lo[a], dtype=torch.float32) + torch.arange(n, dtype=torch.float32) *
          torch.tensor(step[a], dtype=torch.float32) for a, n in enumerate(dims)]
    for iz in range(nz):
        for iy in range(ny):
            for ix in range(nx):
                want = torch.stack([ax[0][ix], ax[1][iy], ax[2][iz]])
                assert torch.equal(c[iz, iy, ix].view(torch.int32), want.view(torch.int32)), (ix, iy, iz)
    # the same rule in numpy float32: one multiply, one add
    q = np.arange(nx, dtype=np.float32) * np.float32(step[0]) + np.float32(lo[0])
    assert np.array_equal(c[0, 0, :, 0].numpy().view(np.int32), q.view(np.int32))
    with pytest.raises(ValueError, match="dims"):
        HF.lattice_coords(lo, step, (4, 0, 2))


def test_cell_centre_lattice(hn):
    """density_grid's default lattice: step = (bmax - bmin) / n and lo = bmin + 0.5 * step in float32."""
    from importlib import import_module
    R = import_module("hashnerf_pytorch_amd.render")   # (hn.render is the function)
    bmin, bmax = torch.tensor([-4.0249, -4.0249, -3.3366]), torch.tensor([4.0249, 4.0249, 3.2414])
    for res, dims in ((16, (16, 16, 16)), ((7, 33, 2), (7, 33, 2))):
        lo, step, d = R.cell_centre_lattice(res, bmin, bmax)
        assert d == dims
        n = np.array(dims, dtype=np.float32)
        want_step = (bmax.numpy() - bmin.numpy()) / n
        want_lo = bmin.numpy() + np.float32(0.5) * want_step
        assert want_step.dtype == np.float32 and want_lo.dtype == np.float32
        assert np.array_equal(step.numpy().view(np.int32), want_step.view(np.int32))
        assert np.array_equal(lo.numpy().view(np.int32), want_lo.view(np.int32))
        # the first and the last point sit half a cell inside the box
        c = hn.functional.lattice_coords(lo, step, d)
        np.testing.assert_allclose(c[0, 0, 0].numpy() - bmin.numpy(), 0.5 * want_step, rtol=1e-5)
        np.testing.assert_allclose(bmax.numpy() - c[-1, -1, -1].numpy(), 0.5 * want_step, rtol=1e-4)
    with pytest.raises(ValueError, match="resolution"):
        R.cell_centre_lattice((4, 4), bmin, bmax)


def test_unpack_occupancy_round_trip(hn):
    dims = (7, 5, 3)                                                         # 105 points: 3 full words + 9 bits
    rng = np.random.default_rng(5)
    occ = rng.random(dims[::-1]) < 0.4
    flat = occ.reshape(-1)
    padded = np.zeros(((flat.size + 31) // 32) * 32, dtype=bool)
    padded[:flat.size] = flat
    words = np.packbits(padded, bitorder="little").view(np.uint32)
    wt = torch.from_numpy(words.view(np.int32).copy())
    back = hn.unpack_occupancy(wt, dims)
    assert back.dtype == torch.bool and back.shape == (3, 5, 7)
    assert np.array_equal(back.numpy(), occ)
    for q in (0, 31, 32, 104):                                               # bit q & 31 of word q >> 5
        assert bool((int(words[q >> 5]) >> (q & 31)) & 1) == bool(flat[q])
    with pytest.raises(ValueError, match="words"):
        hn.unpack_occupancy(wt[:-1], dims)


def test_oracle_fp32_against_fp64_on_the_gpu_tests_points(oracle):
    """What test_gpu_density.test_points_against_oracle rests on: on the point pool's points inside the
    box or on its faces the oracle's fp32 sigma is within rtol = atol = 1e-5 of its fp64 sigma (a table and
    a net of the GPU test's distributions: uniform +-0.5 at T = 12, nn.Linear's init), so the fp32 oracle
    can be the reference there; on the points scaled past the box it is not -- the trilinear weights of the
    unclamped point reach the hundreds -- so no fp32 evaluation can meet that tolerance on them."""
    from gpu_support import BLENDER_BOX
    from input_grad_cases import input_grad_points
    gen = torch.Generator().manual_seed(3)
    table = torch.rand(16, 2 ** 12, 2, generator=gen) - 0.5
    w = oracle.init_nerf_small(gen)
    x = input_grad_points(32 * 64 + 5, BLENDER_BOX)
    lo, hi = BLENDER_BOX
    res = oracle.level_resolutions(16, 16, 512)

    def sigma(dt):
        f, _ = oracle.hash_encode(x.to(dt), table.to(dt), lo.to(dt), hi.to(dt), [r.to(dt) for r in res], 12)
        inp = torch.cat([f, torch.zeros(x.shape[0], 16, dtype=dt)], -1)
        return oracle.nerf_small(inp, {k: v.to(dt) for k, v in w.items()})[:, 3]

    s32, s64 = sigma(torch.float32).double(), sigma(torch.float64)
    excess = (s32 - s64).abs() - (1e-5 + 1e-5 * s64.abs())
    outside = ((x < lo) | (x > hi)).any(-1)
    print(f"fp32 vs fp64 oracle: inside/on faces max |diff| {float((s32 - s64).abs()[~outside].max()):.3e}, "
          f"outside max relative {float(((s32 - s64).abs() / s64.abs())[outside].max()):.3e}")
    assert int((~outside).sum()) > 1500 and float(excess[~outside].max()) < 0.0
    assert float(excess[outside].max()) > 0.0 and float(s64[outside].abs().max()) > 1e3


def test_module_api_refuses_other_fields_and_cpu_tensors(hn):
    box = (torch.tensor([-1., -1, -1]), torch.tensor([1., 1, 1]))
    kw = dict(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64, input_ch=32,
              input_ch_views=16)
    net = hn.NeRFSmall(**kw)
    emb5 = hn.HashEmbedder(box, n_levels=5, log2_hashmap_size=10)
    with pytest.raises(ValueError, match="5 levels"):
        hn.density_grid(4, net, hn.NetworkQuery(emb5, hn.SHEncoder()))
    emb = hn.HashEmbedder(box, log2_hashmap_size=10)
    with pytest.raises(ValueError, match="NetworkQuery"):
        hn.query_density(torch.zeros(4, 3), net, lambda *a: None)
    with pytest.raises(ValueError, match="NeRFSmall"):
        hn.query_density(torch.zeros(4, 3), torch.nn.Linear(3, 4), hn.NetworkQuery(emb, hn.SHEncoder()))
    with pytest.raises(RuntimeError, match="ROCm"):                          # CPU tensors raise as elsewhere
        hn.density_grid(4, net, hn.NetworkQuery(emb, hn.SHEncoder()))
    with pytest.raises(RuntimeError, match="ROCm"):
        hn.query_density(torch.zeros(4, 3), net, hn.NetworkQuery(emb, hn.SHEncoder()))
