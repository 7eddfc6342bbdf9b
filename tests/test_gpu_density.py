"""Density queries on the GPU: the density kernel's sigma against the module
composition (bitwise) and the oracle, the lattice against explicit points
(bitwise), the occupancy words, output bounds, repeatability and the module API.
The field is gpu_support.blender_nets at T = 12: every call here is a few
thousand tiles at most."""
from importlib import import_module

import numpy as np
import pytest
import torch

from gpu_support import BLENDER_BOX, DEV, bits_equal, blender_nets, close, hf
from input_grad_cases import input_grad_points, sh_dirs

pytestmark = pytest.mark.gpu

N_POOL = 32 * 64 + 5
LATTICES = [(5, 3, 2), (33, 2, 3), (64, 64, 64)]   # under one tile | tiles wrap rows, partial last tile | 8,192 tiles


@pytest.fixture(scope="module")
def field(hn):
    """One field, the point pool (input_grad_points over the blender box: inside,
    scaled past it, on its faces) and the module composition's sigma on the
    pool, computed once and left unchanged."""
    s = blender_nets(hn, T=12, seed=3)
    s.nq = hn.NetworkQuery(s.emb, hn.SHEncoder())
    s.grid, s.table, s.ws = s.emb.grid(), s.emb.table.detach(), [w.detach() for w in s.mc.weights()]
    s.pool_cpu = input_grad_points(N_POOL, BLENDER_BOX)
    s.pool = s.pool_cpu.to(DEV)
    lo, hi = BLENDER_BOX
    s.outside = ((s.pool_cpu < lo) | (s.pool_cpu > hi)).any(-1)
    s.on_face = ((s.pool_cpu == lo) | (s.pool_cpu == hi)).any(-1) & ~s.outside
    s.inside = ~s.outside & ~s.on_face
    assert int(s.outside.sum()) > 100 and int(s.on_face.sum()) == 96 and int(s.inside.sum()) > 1000
    with torch.no_grad():
        feat, _ = s.emb(s.pool)
        sh = hn.SHEncoder()(sh_dirs(N_POOL).to(DEV))
        s.ref = s.mc(torch.cat([feat, sh], -1))[:, 3].contiguous()
    return s


def _subset(s, n):
    """Indices of n pool points that mix the three kinds (n = 1: a face point)."""
    if n == N_POOL:
        return torch.arange(N_POOL)
    kinds = [torch.nonzero(m).reshape(-1) for m in (s.on_face, s.outside, s.inside)]
    idx = torch.stack([k[:(n + 2) // 3] for k in kinds], 1).reshape(-1)[:n]   # face, outside, inside, face, ...
    assert idx.numel() == n
    return idx


def _lattice(dims):
    """A lattice whose first and last x planes and last y and z planes lie outside the blender box."""
    lo = (-4.6, -3.9, -3.0)
    span = (9.2, 8.1, 7.0)
    return lo, tuple(sp / (n - 1) for sp, n in zip(span, dims)), dims


def _pack(mask):
    """bool [n] (CPU) -> the int32 occupancy words: bit q & 31 of word q >> 5."""
    m = np.zeros(((mask.numel() + 31) // 32) * 32, dtype=bool)
    m[:mask.numel()] = mask.numpy()
    return torch.from_numpy(np.packbits(m, bitorder="little").view(np.int32).copy())


@pytest.mark.parametrize("n", [1, 33, N_POOL])
def test_points_bitwise_module_composition(hn, field, n):
    """query_density == NeRFSmall(cat[HashEmbedder(p), SH(d)])[:, 3], bit for bit: the same R_F0 / R_F1
    products in the same order on bit-exact features."""
    s = field
    idx = _subset(s, n)
    if n > 1:
        assert s.outside[idx].any() and s.on_face[idx].any() and s.inside[idx].any()
    got = hn.query_density(s.pool[idx.to(DEV)], s.mc, s.nq)
    assert got.shape == (n,) and not got.requires_grad
    assert bits_equal(got, s.ref[idx.to(DEV)].contiguous())
    if n == 33:   # [..., 3] -> [...]; the composition run on these 33 points alone gives the same bits
        p = s.pool[idx.to(DEV)]
        assert bits_equal(hn.query_density(p.reshape(3, 11, 3), s.mc, s.nq), got.reshape(3, 11))
        with torch.no_grad():
            feat, _ = s.emb(p)
            alone = s.mc(torch.cat([feat, hn.SHEncoder()(sh_dirs(33, seed=2).to(DEV))], -1))[:, 3].contiguous()
        assert bits_equal(got, alone)


def test_points_against_oracle(hn, field, oracle):
    """oracle.hash_encode + oracle.nerf_small column 3 within rtol = atol = 1e-5 (test_nerf_small_fwd_bwd's
    tolerance for this net), on the pool's points inside the box and on its faces.  On those the oracle's own
    fp32-against-fp64 difference stays inside the tolerance, so the fp32 oracle is the reference.  The points
    scaled past the box are left to the bitwise test: there the trilinear weights (from the unclamped point,
    as the reference forms them) reach the hundreds on the fine levels, sigma reaches 1e5 and the oracle's
    fp32 and fp64 values leave the tolerance by orders of magnitude -- no evaluation in fp32 can meet 1e-5
    there.  Both are asserted without a GPU, on a table and net of the same distributions:
    test_density_cpu.test_oracle_fp32_against_fp64_on_the_gpu_tests_points."""
    s = field
    keep = ~s.outside
    x = s.pool_cpu[keep]
    feat, _ = oracle.hash_encode(x, s.table.cpu(), BLENDER_BOX[0], BLENDER_BOX[1], oracle.level_resolutions(16, 16, 512),
                                 12)
    w = {k: v.cpu() for k, v in zip(oracle.MLP_KEYS, s.ws)}
    ref = oracle.nerf_small(torch.cat([feat, torch.zeros(x.shape[0], 16)], -1), w)[:, 3]
    got = hn.query_density(s.pool[keep.to(DEV)], s.mc, s.nq)
    err = (got.cpu() - ref).abs()
    print(f"sigma vs oracle on {x.shape[0]} points: max |diff| {float(err.max()):.3e}, "
          f"max |ref| {float(ref.abs().max()):.3e}")
    close(got, ref.numpy(), rtol=1e-5, atol=1e-5, msg="sigma")


@pytest.mark.parametrize("dims", LATTICES)
def test_lattice_bitwise_points(hn, field, dims):
    """density_lattice == density_points on lattice_coords(...): the kernel's own coordinates are the host rule's."""
    s, HF = field, hf()
    lo, step, dims = _lattice(dims)
    pts = HF.lattice_coords(lo, step, dims)
    box_lo, box_hi = BLENDER_BOX
    out = ((pts < box_lo) | (pts > box_hi)).any(-1)
    assert out.any() and not out.all()
    want = HF.density_points(s.grid, s.table, s.ws, pts.reshape(-1, 3).to(DEV))
    got = HF.density_lattice(s.grid, s.table, s.ws, lo, step, dims)
    assert got.shape == dims[::-1]
    assert bits_equal(got.reshape(-1), want)


@pytest.mark.parametrize("threshold", [0.0, 0.02])
def test_occupancy_words(hn, field, threshold):
    s, HF = field, hf()
    lo, step, dims = _lattice((33, 2, 3))
    n = 33 * 2 * 3
    sigma, occ = HF.density_lattice(s.grid, s.table, s.ws, lo, step, dims, threshold=threshold)
    assert occ.dtype == torch.int32 and occ.shape == ((n + 31) // 32,)
    mask = (sigma.reshape(-1) > threshold).cpu()
    assert 0 < int(mask.sum()) < n
    assert torch.equal(occ.cpu(), _pack(mask))
    assert (int(occ[-1]) & 0xffffffff) >> (n & 31) == 0                       # the last word's tail bits
    assert torch.equal(HF.unpack_occupancy(occ, dims).cpu().reshape(-1), mask)
    # each output alone is the same bits
    only_occ = HF.density_lattice(s.grid, s.table, s.ws, lo, step, dims, threshold=threshold, want_sigma=False)
    assert torch.equal(only_occ, occ)
    assert bits_equal(HF.density_lattice(s.grid, s.table, s.ws, lo, step, dims), sigma)
    # points: several whole words, then a partial one
    ps, pocc = HF.density_points(s.grid, s.table, s.ws, s.pool, threshold=threshold)
    assert bits_equal(ps, s.ref)
    assert torch.equal(pocc.cpu(), _pack((ps > threshold).cpu()))
    assert torch.equal(HF.density_points(s.grid, s.table, s.ws, s.pool, threshold=threshold, want_sigma=False), pocc)
    sg, inside = hn.query_density(s.pool, s.mc, s.nq, threshold=threshold)
    assert inside.dtype == torch.bool and torch.equal(inside, ps > threshold) and bits_equal(sg, ps)


def test_outputs_stay_in_bounds(hn, field):
    """64 sentinel elements on each side of both outputs stay intact (a 198-point lattice: 7 words, the last
    partial; 33 points: 2 words)."""
    s, HF = field, hf()
    lo, step, dims = _lattice((33, 2, 3))
    SF, SI = 12345.0, 0x5a5a5a5a

    def guarded(n):
        w = (n + 31) // 32
        return (torch.full((n + 128,), SF, device=DEV), torch.full((w + 128,), SI, dtype=torch.int32, device=DEV), w)

    def intact(fb, ib, n, w):
        return bool((fb[:64] == SF).all() and (fb[64 + n:] == SF).all() and (ib[:64] == SI).all() and
                    (ib[64 + w:] == SI).all())

    n = 33 * 2 * 3
    fb, ib, w = guarded(n)
    HF.density_lattice(s.grid, s.table, s.ws, lo, step, dims, threshold=0.0, out=(fb[64:64 + n], ib[64:64 + w]))
    sigma, occ = HF.density_lattice(s.grid, s.table, s.ws, lo, step, dims, threshold=0.0)
    assert intact(fb, ib, n, w)
    assert bits_equal(fb[64:64 + n], sigma.reshape(-1)) and torch.equal(ib[64:64 + w], occ)
    n = 33
    fb, ib, w = guarded(n)
    p = s.pool[_subset(s, n).to(DEV)]
    HF.density_points(s.grid, s.table, s.ws, p, threshold=0.0, out=(fb[64:64 + n], ib[64:64 + w]))
    sigma, occ = HF.density_points(s.grid, s.table, s.ws, p, threshold=0.0)
    assert intact(fb, ib, n, w)
    assert bits_equal(fb[64:64 + n], sigma) and torch.equal(ib[64:64 + w], occ)


def test_repeatable(hn, field):
    s, HF = field, hf()
    lo, step, dims = _lattice((64, 64, 64))
    a = HF.density_lattice(s.grid, s.table, s.ws, lo, step, dims, threshold=0.0)
    b = HF.density_lattice(s.grid, s.table, s.ws, lo, step, dims, threshold=0.0)
    assert bits_equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_module_api(hn, field):
    s, HF = field, hf()
    R = import_module("hashnerf_pytorch_amd.render")
    sigma = hn.density_grid(16, s.mc, s.nq)
    assert sigma.shape == (16, 16, 16) and sigma.dtype == torch.float32 and not sigma.requires_grad
    lo, step, dims = R.cell_centre_lattice(16, *s.emb.box())
    assert dims == (16, 16, 16)
    assert bits_equal(sigma, HF.density_lattice(s.grid, s.table, s.ws, lo, step, dims))
    # cell centres lie inside the box: there the lattice is the composition's sigma too
    assert bits_equal(sigma.reshape(-1), hn.query_density(HF.lattice_coords(lo, step, dims).to(DEV), s.mc,
                                                          s.nq).reshape(-1))
    # (nx, ny, nz), caller's bounds, occupancy alone
    bounds = (torch.tensor([-1.0, -2.0, -0.5]), torch.tensor([1.0, 2.0, 1.5]))
    sg, words = hn.density_grid((9, 4, 5), s.mc, s.nq, bounds=bounds, threshold=0.01)
    assert sg.shape == (5, 4, 9) and words.shape == ((180 + 31) // 32,)
    assert torch.equal(hn.unpack_occupancy(words, (9, 4, 5)), sg > 0.01)
    assert torch.equal(hn.density_grid((9, 4, 5), s.mc, s.nq, bounds=bounds, threshold=0.01, want_sigma=False), words)
    # no points: empty answers, with and without a threshold
    none = s.pool[:0].reshape(0, 4, 3)
    assert hn.query_density(none, s.mc, s.nq).shape == (0, 4)
    sg, inside = hn.query_density(none, s.mc, s.nq, threshold=0.0)
    assert sg.shape == (0, 4) and inside.shape == (0, 4) and inside.dtype == torch.bool
    emb5 = hn.HashEmbedder(BLENDER_BOX, n_levels=5, log2_hashmap_size=12).to(DEV)
    with pytest.raises(ValueError, match="5 levels"):
        hn.density_grid(16, s.mc, hn.NetworkQuery(emb5, hn.SHEncoder()))
    with pytest.raises(ValueError, match="5 levels"):
        hn.query_density(s.pool[:4], s.mc, hn.NetworkQuery(emb5, hn.SHEncoder()))
