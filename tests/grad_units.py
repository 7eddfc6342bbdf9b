"""Judging the fused backward's gradients unit by unit: the table gradient per
level and per bin of the binned scatter, each NeRFSmall weight gradient per row
and per block of 16 columns, and the table entries no sample touches.  One norm
over a whole tensor cannot see one unit that is wrong: on the small scene level
0 carries 8.5 % of the table gradient's norm, so 0.6 % there stays under 5e-4
of the whole.

The reference of every unit is the fp32 oracle on the device's own fine z (the
device's encoding is bit-exact with it: both pick the same cells); the fp32
oracle's own error against the float64 one is printed beside it as the floor.
Entry by entry float64 is no reference: a ReLU pre-activation, a raw sigma or a
cell coordinate within rounding of its threshold flips a decision between the
two precisions.  The inputs below were picked on the CPU so that no unit's
floor exceeds a quarter of the bar (tests/test_grad_units_cpu.py asserts it).

A plain module: the cases, their inputs (made on the CPU: the same values on
every machine), the oracle's gradients and the comparisons."""
from types import SimpleNamespace

import numpy as np
import torch

import ray_grad_cases as rc
from gpu_support import SMALL_FINEST, SMALL_T

BAR = 5e-4                  # the project's end-to-end bound (DESIGN, "Full fused step vs oracle on the device's z")
FLOOR = BAR / 4             # what the fp32 oracle's own error against float64 may reach in any unit of a case
B = 37                      # no multiple of 4 or 16
SMALL_BINS_PER_LEVEL = 2    # HF.render_bins at T = 14: 32 bins of 2^13 rows (the GPU tests assert it)
WEIGHT_NAMES = tuple(f"{net}.{k}" for net in ("coarse", "fine")
                     for k in ("sigma_net.0.weight", "sigma_net.1.weight", "color_net.0.weight",
                               "color_net.1.weight", "color_net.2.weight"))


# ---- the cases' inputs -----------------------------------------------------------
# Ray seeds (ray_grad_cases.ray_batch), chosen by the reference alone: the first of 43, 44, 45 whose worst unit
# of the fp32 oracle against the float64 one is within FLOOR = 1.25e-4 with both on the fp32 oracle's fine z (on
# the CPU, tests/test_grad_units_cpu.py), and within the bar itself with both on the device's fine z (which
# equals the oracle's bitwise in about two samples of three; tests/test_gpu_grad_units.py asserts it).  Measured
# worst unit (table, weights) per candidate on the oracle's z | on the device's z, the chosen one last:
#   det 64 + 128 white    43: 7.9e-5, 7.5e-5 | 7.4e-4, 5.8e-3; 44: 9.8e-5, 8.7e-5 | 1.6e-4, 1.7e-4
#   det 64 + 128 black    43: 5.7e-5, 1.9e-4; 44: 7.1e-5, 7.7e-5 | 1.1e-4, 1.1e-4
#   det 64 + 64  white    43: 2.7e-4, 4.3e-4; 44: 5.4e-5, 5.2e-5 | 5.4e-5, 5.2e-5
#   det 64 + 64  black    43: 2.1e-4, 2.9e-4; 44: 3.6e-5, 8.3e-5 | 3.6e-5, 8.4e-5
#   perturbed 64 + 128    43: 1.5e-4, 2.3e-4; 44: 1.3e-4, 1.1e-4; 45: 9.1e-5, 8.8e-5 | 9.1e-5, 8.8e-5
#   raw noise 64 + 128    43: 6.7e-5, 7.2e-5 | 6.9e-5, 7.7e-5
# (Seed 43 of 64 + 128 white: on the device's z one row of the fine sigma_net.0.weight differs by 5.8e-3 between
# the two oracles, a ReLU pre-activation within rounding of zero; seeds 45 and 46 of the deterministic cases reach
# 1e-3 to 3e-2 in a weight row on either z.)
# The +-1.0 box has no such criterion (most records land on surface cells, where the precisions pick other
# cells): its oracle must be finite with its support within touched_entries of its samples with density.
def _inputs(name, half, ni, white, seed, perturb=False, noise=False):
    return SimpleNamespace(name=name, half=half, ni=ni, white=white, seed=seed, perturb=perturb, noise=noise)


INPUTS = {
    (128, True): _inputs("64 + 128, white", 1.5, 128, True, 44),
    (128, False): _inputs("64 + 128, black", 1.5, 128, False, 44),
    (64, True): _inputs("64 + 64, white", 1.5, 64, True, 44),
    (64, False): _inputs("64 + 64, black", 1.5, 64, False, 44),
    "perturb": _inputs("64 + 128, white, perturbed", 1.5, 128, True, 45, perturb=True),
    "noise": _inputs("64 + 128, white, raw noise", 1.5, 128, True, 43, noise=True),
    "box1": _inputs("64 + 128, white, box +-1", 1.0, 128, True, 51),
}
FLOORED = [k for k in INPUTS if k != "box1"]


def draws(inp):
    """The case's rays [B, 11], target and random draws, on the CPU from the case's seed.  Deterministic draws:
    t_rand None, u the linspace."""
    import hn_loader
    d = SimpleNamespace(rays=rc.ray_batch(hn_loader.load(), B, inp.seed), t_rand=None, noise_c=None, noise_f=None)
    g = torch.Generator().manual_seed(1000 + inp.seed)
    d.target = torch.rand(B, 3, generator=g)
    d.u = torch.linspace(0., 1., inp.ni).expand(B, inp.ni).contiguous()
    if inp.perturb:
        d.t_rand, d.u = torch.rand(B, 64, generator=g), torch.rand(B, inp.ni, generator=g)
    if inp.noise:
        d.noise_c, d.noise_f = 0.3 * torch.randn(B, 64, generator=g), 0.3 * torch.randn(B, 64 + inp.ni, generator=g)
    return d


# ---- the oracle's gradients --------------------------------------------------------
def oracle_grads(oracle, table, weights, box, finest, T, rays, dt, ni, white, loss, z_fine=None, t_rand=None, u=None,
                 noise_c=None, noise_f=None):
    """Autograd of loss(ret) through oracle.render_rays in dtype dt -> (ret, d table, the ten weight gradients).
    weights: the ten NeRFSmall tensors, coarse then fine."""
    c = lambda t: None if t is None else t.detach().cpu().to(dt)
    tab = c(table).requires_grad_(True)
    w = [{k: c(v).requires_grad_(True) for k, v in zip(oracle.MLP_KEYS, ws)} for ws in (weights[:5], weights[5:])]
    ret = oracle.render_rays(c(rays), w[0], w[1], tab, c(box[0]), c(box[1]), oracle.level_resolutions(16, 16, finest),
                             T, N_importance=ni, t_rand=c(t_rand), u=c(u), noise_c=c(noise_c), noise_f=c(noise_f),
                             white_bkgd=white, z_fine=c(z_fine))
    loss(ret, dt).backward()
    return ret, tab.grad, [m[k].grad for m in w for k in oracle.MLP_KEYS]


def small_scene_grads(oracle, s, inp, d, dt, z_fine=None):
    """oracle_grads of a small-scene case (s: ray_grad_cases.scene) under the training loss."""
    def loss(ret, dt):
        return oracle.training_loss(ret, d.target.to(dt), rc.SPARSE_W)
    return oracle_grads(oracle, s.emb.table, list(s.mc.weights()) + list(s.mf.weights()), rc.box(inp.half),
                        SMALL_FINEST, SMALL_T, d.rays, dt, inp.ni, inp.white, loss, z_fine, d.t_rand, d.u, d.noise_c,
                        d.noise_f)


def sample_points(rays, z):
    """o + d z in fp32, as oracle.render_rays forms them: [B, n, 3]."""
    rays, z = rays.detach().cpu().float(), z.detach().cpu().float()
    return rays[..., None, 0:3] + rays[..., None, 3:6] * z[..., :, None]


# ---- units -------------------------------------------------------------------------
def _f64(a):
    return np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, np.float64)


def table_units(d_table, n_bins_per_level):
    """[L, 2^T, 2] -> [(name, values)]: every level, and every bin of the binned scatter (n_bins_per_level
    consecutive row ranges of a level; 0: levels only)."""
    t = _f64(d_table)
    units = [(f"level {l}", t[l].reshape(-1)) for l in range(t.shape[0])]
    if n_bins_per_level:
        rows = t.shape[1] // n_bins_per_level
        assert rows * n_bins_per_level == t.shape[1]
        units += [(f"level {l} bin {b} (bin {l * n_bins_per_level + b}, rows {b * rows}-{(b + 1) * rows - 1})",
                   t[l, b * rows:(b + 1) * rows].reshape(-1))
                  for l in range(t.shape[0]) for b in range(n_bins_per_level)]
    return units


def weight_units(dw):
    """[rows, cols] -> [(name, values)]: every row, and every block of 16 columns (the last one ragged where
    cols is no multiple of 16: 31 = 16 + 15)."""
    w = _f64(dw)
    units = [(f"row {r}", w[r]) for r in range(w.shape[0])]
    units += [(f"columns {c}-{min(c + 16, w.shape[1]) - 1}", w[:, c:c + 16].reshape(-1))
              for c in range(0, w.shape[1], 16)]
    return units


def unit_errors(got, want):
    """||got - want|| / ||want|| of every unit; a unit whose reference is all zero must be exactly zero
    (0 where it is, inf where it is not)."""
    assert [n for n, _ in got] == [n for n, _ in want]
    out = np.empty(len(got))
    for i, ((_, g), (_, w)) in enumerate(zip(got, want)):
        den = np.linalg.norm(w)
        if den > 0:
            out[i] = np.linalg.norm(g - w) / den
        else:
            out[i] = 0.0 if not np.any(g != 0) else np.inf     # (a NaN counts as nonzero)
    return out


def check_units(what, got, want32, want64, bar=BAR, versus="device vs fp32 oracle"):
    """Every unit of got within bar of want32 (unit lists of table_units / weight_units of one tensor).  Prints
    the worst unit's error beside the fp32 oracle's own error against want64 in that unit and in its worst unit
    (want64 None: not printed), and names the failing units.  -> (worst unit's name, its error, its floor, the
    largest floor)."""
    err = unit_errors(got, want32)
    floor = unit_errors(want32, want64) if want64 is not None else np.full(len(err), np.nan)
    worst = int(np.argmax(np.nan_to_num(err, nan=np.inf)))
    name = got[worst][0]
    beside = "" if want64 is None else f", fp32 vs fp64 oracle {floor[worst]:.3e} (its worst unit {floor.max():.3e})"
    print(f"[grad-units] {what}: worst unit {name}: {versus} {err[worst]:.3e}{beside}")
    bad = sorted((i for i in range(len(err)) if not err[i] <= bar), key=lambda i: -np.nan_to_num(err[i], nan=np.inf))
    assert not bad, (f"{what}: {len(bad)} of {len(err)} units over {bar:g}, worst first: "
                     + "; ".join(f"{got[i][0]}: {err[i]:.3e}" for i in bad[:8]))
    return name, float(err[worst]), float(floor[worst]), float(floor.max())


def check_all(case, got, want32, want64, n_bins_per_level=SMALL_BINS_PER_LEVEL, bar=BAR, **kw):
    """check_units of the table gradient and of the ten weight gradients; got / want: (d table, [ten])."""
    none = (None, [None] * 10)
    w64 = none if want64 is None else want64
    u = lambda f, t, *a: None if t is None else f(t, *a)
    res = {"table": check_units(f"{case}: table", *(u(table_units, x[0], n_bins_per_level)
                                                    for x in (got, want32, w64)), bar, **kw)}
    for i, name in enumerate(WEIGHT_NAMES):
        res[name] = check_units(f"{case}: {name}", *(u(weight_units, x[1][i]) for x in (got, want32, w64)), bar, **kw)
    return res


# ---- support -----------------------------------------------------------------------
def touched_entries(points, box, resolutions, T):
    """The (level, row) pairs that any corner of any point hashes to, as a bool [L, 2^T]: oracle.hash_encode's
    clamp, floor and hash restated in fp32 (hash_encoding.py:59-82)."""
    from oracle.hashnerf_oracle import CORNERS, spatial_hash
    lo, hi = (b.detach().cpu().float() for b in box)
    x = points.detach().cpu().float().reshape(-1, 3)
    x = torch.max(torch.min(x, hi), lo)
    out = torch.zeros((len(resolutions), 1 << T), dtype=torch.bool)
    for lvl, res in enumerate(resolutions):
        gs = (hi - lo) / res
        idx = torch.floor((x - lo) / gs).int()
        h = spatial_hash(idx.unsqueeze(1) + CORNERS.unsqueeze(0), T)
        out[lvl, h.reshape(-1)] = True
    return out


def check_support(what, d_table, touched):
    """Every table entry outside touched is exactly zero (a NaN is not)."""
    zero = (d_table.detach().cpu() == 0).all(-1)
    bad = (~zero & ~touched).nonzero()
    assert bad.shape[0] == 0, (f"{what}: {bad.shape[0]} table rows no sample touches are not exactly 0.0, first "
                               f"(level, row) {bad[:4].tolist()}")
