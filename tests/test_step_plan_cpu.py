"""Trainer._plan without a GPU: the one place that decides which launches an
explicit-mode step makes.  Every expected StepPlan is written out as
literals, one row per single change from the defaults."""
import types

import pytest
import torch

from test_next_batch_cpu import bare_trainer

T, F = True, False
#          binned skip_dead fuse_loss fold_pre table_own mlp_slab defer prefetch next_in_bwd
DEFAULT = (T,     T,        T,        T,       T,        T,       F,    F,       T)
SEGMENTED = types.SimpleNamespace(seg_bins=[(0, 4), (4, 8)])      # what _plan reads of a ShardedTableStep
WHOLE = types.SimpleNamespace(seg_bins=None)
CPU = torch.device("cpu")

ROWS = [
    # the ten flags
    (dict(fuse_table_step=False), {}, (T, T, T, T, F, F, F, F, F)),
    (dict(skip_dead_rows=False), {}, DEFAULT),                    # the owner pass's row mask: no launch differs
    (dict(dp_sharded=False), {}, DEFAULT),                        # read at setup, through _xchg (below)
    (dict(dp_chunks=4), {}, DEFAULT),
    (dict(prefetch=True), {}, (T, T, T, T, T, T, F, T, F)),
    (dict(fuse_next_batch=False), {}, (T, T, T, T, T, T, F, F, F)),
    (dict(fuse_mlp_step=False), {}, (T, T, T, T, T, F, F, F, T)),
    (dict(fuse_loss=False), {}, (T, T, F, F, T, T, F, F, T)),
    (dict(fuse_prepass=False), {}, (T, T, T, F, T, T, F, F, T)),
    (dict(dense_bwd=True), {}, (T, F, T, T, T, T, F, F, T)),
    # the trainer's setting
    (dict(world=2), {}, (T, T, T, F, F, F, F, F, F)),
    (dict(world=2, _xchg=WHOLE), {}, (T, T, T, F, F, F, F, F, F)),
    (dict(world=2, _xchg=SEGMENTED), {}, (T, T, T, F, F, F, T, F, F)),
    (dict(scatter="atomic"), {}, (F, F, T, F, F, F, F, F, F)),
    (dict(mode="autograd"), {}, (T, T, T, T, T, T, F, F, F)),
    (dict(use_batching=True), {}, (T, T, T, T, T, T, F, F, F)),
    (dict(ray_order=0), {}, (T, T, T, T, T, T, F, F, F)),
    (dict(kw_train=dict(perturb=0.0)), {}, (T, T, T, T, T, T, F, F, F)),
    (dict(device=CPU), {}, (T, T, T, T, T, T, F, F, F)),
    (dict(device=CPU, prefetch=True), {}, (T, T, T, T, T, T, F, F, F)),
    # the step's call
    ({}, dict(batch_given=True), DEFAULT),
    (dict(prefetch=True), dict(batch_given=True), (T, T, T, T, T, T, F, F, F)),
    ({}, dict(self_driven=False), (T, T, T, T, T, T, F, F, F)),
]


def test_default_plan(hn):
    """One GPU, binned schedule, a self-driven step: every fusion on, the
    owner pass inside the backward, no side-stream prefetch."""
    from hashnerf_pytorch_amd.train import StepPlan
    p = bare_trainer(hn)._plan(self_driven=True)
    assert isinstance(p, StepPlan) and p._fields == ("binned", "skip_dead_color", "fuse_loss", "fold_prepass",
                                                     "table_in_owner", "mlp_in_slab", "owner_defer", "prefetch",
                                                     "next_in_bwd")
    assert p.binned and p.skip_dead_color and p.fuse_loss and p.fold_prepass and p.table_in_owner
    assert p.mlp_in_slab and p.next_in_bwd and not p.owner_defer and not p.prefetch
    assert tuple(p) == DEFAULT and all(type(x) is bool for x in p)
    assert tuple(bare_trainer(hn)._plan()) == (T, T, T, T, T, T, F, F, F)     # the arguments' defaults


@pytest.mark.parametrize("over,call,want", ROWS, ids=[",".join([*o, *c]) + f"#{k}" for k, (o, c, _) in enumerate(ROWS)])
def test_plan_single_changes(hn, over, call, want):
    tr = bare_trainer(hn, **over)
    p = tr._plan(**{"self_driven": True, **call})
    assert tuple(p) == want and all(type(x) is bool for x in p)
    if "self_driven" not in call:
        assert tr._fuses_next_batch() is want[8]             # the self-driven plan's answer


def test_plan_follows_flags_between_steps(hn):
    """The plan is formed from the flags as they stand at each call."""
    tr = bare_trainer(hn)
    assert tuple(tr._plan(self_driven=True)) == DEFAULT
    tr.fuse_loss = False
    assert tuple(tr._plan(self_driven=True)) == (T, T, F, F, T, T, F, F, T)
    tr.fuse_loss = True
    assert tuple(tr._plan(self_driven=True)) == DEFAULT


def test_dense_bwd_cannot_go_stale(hn):
    """Trainer.dense_bwd set before setup reaches the cfg; set after setup it
    changes the cfg and the plan (it was silently ignored).  A Trainer on the
    CPU device constructs and sets up: nothing there needs a GPU."""
    from hashnerf_pytorch_amd.train import SyntheticBlender, Trainer, default_args
    data = SyntheticBlender(16, 16, 2, "cpu")
    tr = Trainer(default_args(N_rand=64, log2_hashmap_size=12), data, "cpu")
    assert tr._cfg is None and tr.dense_bwd is False and tr._live is False and tr._livem is False
    tr.dense_bwd = True
    assert tr.dense_bwd is True
    tr._fused_setup()
    assert tr._cfg.dense_bwd == 1 and tr.dense_bwd is True
    assert tr._binned and hn._lib.lib().hn_render_scatter_mode(tr._cfg, 64) == 2
    assert tr._plan().skip_dead_color is False
    tr.dense_bwd = False
    assert tr._cfg.dense_bwd == 0 and tr.dense_bwd is False
    assert tr._plan().skip_dead_color is True
    tr._cfg.dense_bwd = 1                                       # the cfg's field is the flag
    assert tr.dense_bwd is True and tr._plan().skip_dead_color is False
    tr.dense_bwd = False
    tr._drop_setup()
    assert tr._cfg is None and tr._xchg is None and tr.dense_bwd is False
    tr._fused_setup()
    assert tr._cfg.dense_bwd == 0
