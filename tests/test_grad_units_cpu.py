"""tests/grad_units.py on the CPU, before any kernel is judged with it:

* touched_entries against autograd: the fp32 oracle's table gradient is zero
  everywhere outside it, on the +-1.5 box and on the +-1.0 box where most
  samples clamp onto the surface;
* planted defects: each is put into the fp32 oracle's own gradients, sized from
  the measured norms so that the whole-tensor 5e-4 of the existing comparisons
  still passes (asserted), and must fail the per-unit check by name;
* input selection: for every case of tests/test_gpu_grad_units.py the fp32
  oracle's error against the float64 one is at most a quarter of the bar in
  every unit (both on the fp32 oracle's fine z), so the inputs keep away from
  the decision flips that make that error swing with the ray seed."""
import pytest
import torch

import grad_units as gu
import ray_grad_cases as rc
from gpu_support import SMALL_FINEST, SMALL_T, rel_err

_SCENES, _ORACLE = {}, {}


def scene_of(hn, half):
    if half not in _SCENES:
        _SCENES[half] = rc.scene(hn, half)
    return _SCENES[half]


def oracle_of(hn, oracle, key, dt=torch.float32):
    """(inputs, draws, (ret, d table, ten weight gradients)) of a case, computed once and left unchanged; the
    float64 run takes the fp32 run's fine z."""
    if (key, dt) not in _ORACLE:
        inp = gu.INPUTS[key]
        d = gu.draws(inp)
        z = None if dt == torch.float32 else oracle_of(hn, oracle, key)[2][0]["z_vals"].detach()
        _ORACLE[key, dt] = (inp, d, gu.small_scene_grads(oracle, scene_of(hn, inp.half), inp, d, dt, z))
    return _ORACLE[key, dt]


def all_points(d, ret):
    return torch.cat([gu.sample_points(d.rays, ret["z_vals0"]), gu.sample_points(d.rays, ret["z_vals"])], 1)


# ---- touched_entries -------------------------------------------------------------
@pytest.mark.parametrize("key", [(128, True), "perturb", "box1"])
def test_touched_entries_cover_the_oracles_gradient(hn, oracle, key):
    inp, d, (ret, d_table, _) = oracle_of(hn, oracle, key)
    res = oracle.level_resolutions(16, 16, SMALL_FINEST)
    pts = all_points(d, ret)
    if inp.half == 1.0:
        assert float((pts.abs() > 1.0).any(-1).float().mean()) > 0.5, "most samples clamp"
    touched = gu.touched_entries(pts, rc.box(inp.half), res, SMALL_T)
    assert 0 < int(touched.sum()) < touched.numel()
    assert torch.isfinite(d_table).all()
    gu.check_support(inp.name, d_table, touched)
    # and no wider than it has to be: the gradient's support lies within the entries of the samples with density,
    # and fills them but for the corners whose trilinear weight is exactly zero (a coordinate on a cell face)
    live = torch.cat([ret["raw0"][..., 3] + (0 if d.noise_c is None else d.noise_c),
                      ret["raw"][..., 3] + (0 if d.noise_f is None else d.noise_f)], 1).detach() > 0
    assert 0 < int(live.sum()) < live.numel()
    support = gu.touched_entries(pts[live], rc.box(inp.half), res, SMALL_T)
    nonzero = (d_table != 0).any(-1)
    assert not bool((nonzero & ~support).any())
    assert int((support & ~nonzero).sum()) <= 0.01 * int(support.sum())


def test_check_support_sees_one_entry(hn, oracle):
    """One nonzero written into an entry no sample touches: far below any norm-relative bound."""
    inp, d, (ret, d_table, dws) = oracle_of(hn, oracle, (128, True))
    touched = gu.touched_entries(all_points(d, ret), rc.box(inp.half), oracle.level_resolutions(16, 16, SMALL_FINEST),
                                 SMALL_T)
    lvl, row = (~touched).nonzero()[1234].tolist()
    bad = d_table.clone()
    bad[lvl, row, 1] = 1e-12
    assert rel_err(bad, d_table) <= gu.BAR
    gu.check_all("planted", (bad, dws), (d_table, dws), None)           # its bin's norm does not see it either
    with pytest.raises(AssertionError, match=rf"\[\[{lvl}, {row}\]\]"):
        gu.check_support("planted", bad, touched)
    nan = d_table.clone()
    nan[lvl, row, 0] = float("nan")
    with pytest.raises(AssertionError, match="not exactly 0.0"):
        gu.check_support("planted", nan, touched)


def test_zero_reference_unit_must_be_exactly_zero():
    want = torch.zeros(64, 31)
    want[:, :16] = 1.0
    got = want.clone()
    gu.check_units("zero block", gu.weight_units(got), gu.weight_units(want), None)
    got[5, 20] = 1e-30
    with pytest.raises(AssertionError, match="columns 16-30: inf"):
        gu.check_units("zero block", gu.weight_units(got), gu.weight_units(want), None)
    got[5, 20] = float("nan")
    with pytest.raises(AssertionError, match="row 5: nan"):
        gu.check_units("zero block", gu.weight_units(got), gu.weight_units(want), None)


# ---- planted defects ---------------------------------------------------------------
def scaled(a, index, share, stated):
    """a with a[index] scaled by 1 + f: f as stated, or the largest that leaves the whole-tensor error
    (f * share, share = ||a[index]|| / ||a||) at 0.9 of the bar."""
    f = min(stated, 0.9 * gu.BAR / share)
    assert f > 1.2 * gu.BAR, "the unit carries too much of the tensor for any norm to tell the two checks apart"
    out = a.clone()
    out[index] *= 1 + f
    return out


def planted(hn, oracle):
    """name -> (which tensor: 0 the table, 1 + i a weight gradient; the tensor with the defect; the unit that
    must be named)."""
    inp, d, (ret, d_table, dws) = oracle_of(hn, oracle, (128, True))
    share = lambda a, index: float(a[index].norm() / a.norm())
    out = {}
    out["level 0 scaled by 1.004"] = (0, scaled(d_table, 0, share(d_table, 0), 0.004), "level 0:")
    half = slice(0, 1 << (SMALL_T - 1))
    out["one bin of level 1 scaled by 1.01"] = (0, scaled(d_table, (1, half), share(d_table, (1, half)), 0.01),
                                                "level 1 bin 0 ")
    # a quarter of a row's value moved to the next row, for five rows of level 15's bin 1: the rows whose size
    # puts the moved norm midway (geometrically) between the bar of the bin and the bar of the whole table
    lo = 1 << (SMALL_T - 1)
    bin_ = d_table[15, lo:]
    m = gu.BAR * float((bin_.norm() * d_table.norm()).sqrt())
    size = bin_[:-1].norm(dim=-1)
    order = (size - m / (0.25 * 10 ** 0.5)).abs().argsort().tolist()
    rows = []
    for r in order:
        if all(abs(r - q) > 1 for q in rows):
            rows.append(r)
        if len(rows) == 5:
            break
    moved = d_table.clone()
    for r in rows:
        moved[15, lo + r] -= 0.25 * d_table[15, lo + r]
        moved[15, lo + r + 1] += 0.25 * d_table[15, lo + r]
    out["a quarter of five rows moved to the next row in level 15's bin 1"] = (0, moved, "level 15 bin 1 ")
    # rows 16-31 of one 32-sample tile's share missing from fine color_net.1.weight, for a single ray
    i = gu.WEIGHT_NAMES.index("fine.color_net.1.weight")
    share16 = tile_shares(oracle, scene_of(hn, inp.half), inp, d, ret, dws[i])
    whole = share16.flatten(2).norm(dim=-1) / dws[i].norm()
    per_row = (share16.norm(dim=-1) / dws[i][16:32].norm(dim=-1)).amax(-1)
    per_row[whole > 0.8 * gu.BAR] = 0
    ray, tile = divmod(int(per_row.argmax()), per_row.shape[1])
    lane = dws[i].clone()
    lane[16:32] -= share16[ray, tile]
    out[f"ray {ray}'s tile {tile}: rows 16-31 missing from fine color_net.1.weight"] = (1 + i, lane, "row ")
    j = gu.WEIGHT_NAMES.index("coarse.sigma_net.0.weight")
    cols = (slice(None), slice(16, 32))
    if share(dws[j], cols) > share(dws[j], (slice(None), slice(0, 16))):
        cols = (slice(None), slice(0, 16))
    out["one 16-column block of sigma_net.0.weight scaled by 1.01"] = (
        1 + j, scaled(dws[j], cols, share(dws[j], cols), 0.01), f"columns {cols[1].start}-{cols[1].stop - 1}:")
    return (d_table, dws), out


def tile_shares(oracle, s, inp, d, ret, full):
    """Rows 16-31 of every (ray, 32-sample fine tile)'s share of d loss / d fine color_net.1.weight: [B, tiles,
    16, 64].  d loss / d raw once; a tile's share is the gradient of sum(raw . d raw) over its samples."""
    w = rc.oracle_weights(oracle, s, torch.float32)[1]
    w["color_net.1.weight"].requires_grad_(True)
    z = ret["z_vals"].detach()
    raw = oracle.run_network(gu.sample_points(d.rays, z), d.rays[:, -3:], w, s.emb.table.detach(), *rc.box(inp.half),
                             oracle.level_resolutions(16, 16, SMALL_FINEST), SMALL_T)
    leaf = raw.detach().requires_grad_(True)
    rgb, _, _, _, _, sp = oracle.raw2outputs(leaf, z, d.rays[:, 3:6], d.noise_f, inp.white)
    (torch.mean((rgb - d.target) ** 2) + rc.SPARSE_W * sp.sum()).backward()
    tiles = raw.shape[1] // 32
    per_tile = (raw * leaf.grad).reshape(gu.B, tiles, -1).sum(-1)
    out = torch.stack([torch.autograd.grad(per_tile[r, t], w["color_net.1.weight"], retain_graph=True)[0][16:32]
                       for r in range(gu.B) for t in range(tiles)]).reshape(gu.B, tiles, 16, 64)
    assert rel_err(out.sum((0, 1)), full[16:32]) <= 1e-5, "the tiles' shares sum to the gradient"
    return out


DEFECTS = 5


@pytest.mark.parametrize("which", range(DEFECTS))
def test_planted_defect_passes_the_whole_tensor_check_and_fails_the_units(hn, oracle, which):
    (d_table, dws), defects = planted(hn, oracle) if "planted" not in _ORACLE else _ORACLE["planted"]
    _ORACLE["planted"] = ((d_table, dws), defects)
    assert len(defects) == DEFECTS
    name, (tensor, bad, unit) = list(defects.items())[which]
    clean = [d_table] + dws
    got = list(clean)
    got[tensor] = bad
    whole = rel_err(bad, clean[tensor])
    print(f"[grad-units] planted: {name}: whole tensor {whole:.3e}")
    assert 0 < whole <= gu.BAR, "the defect must pass today's whole-tensor check"
    tensor_name = "table" if tensor == 0 else gu.WEIGHT_NAMES[tensor - 1]
    with pytest.raises(AssertionError, match=f"planted: {tensor_name}: .*{unit}"):
        gu.check_all("planted", (got[0], got[1:]), (d_table, dws), None)
    gu.check_all("clean", (d_table, dws), (d_table, dws), None)


# ---- input selection ---------------------------------------------------------------
@pytest.mark.parametrize("key", gu.FLOORED, ids=str)
def test_case_inputs_keep_every_unit_floor_within_a_quarter_of_the_bar(hn, oracle, key):
    inp, _, (_, t32, w32) = oracle_of(hn, oracle, key)
    _, _, (_, t64, w64) = oracle_of(hn, oracle, key, torch.float64)
    assert all(float(x.abs().max()) > 0 for x in [t32] + w32)
    floors = gu.check_all(f"floor of {inp.name}, seed {inp.seed}", (t32, w32), (t64, w64), None, bar=gu.FLOOR,
                          versus="fp32 vs fp64 oracle")
    assert max(v[1] for v in floors.values()) <= gu.FLOOR


def test_box1_inputs_are_finite(hn, oracle):
    """The +-1.0 box: no floor criterion (float64 picks other surface cells); the fp32 oracle is finite and
    every tensor has a gradient.  Its support is test_touched_entries_cover_the_oracles_gradient's."""
    _, _, (ret, t32, w32) = oracle_of(hn, oracle, "box1")
    assert all(torch.isfinite(x).all() and float(x.abs().max()) > 0 for x in [t32] + w32)
    assert all(torch.isfinite(ret[k]).all() for k in ("rgb_map", "rgb0", "sparsity_loss", "sparsity_loss0"))
