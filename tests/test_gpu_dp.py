"""Data-parallel training step on the device (BASELINE configs[3]).

* Two ranks (child processes, gloo, both on the one GPU) each run the HIP
  explicit-mode Trainer on their half of a global batch and SUM-all-reduce
  (Trainer.allreduce_grads).  The reduced table and NeRFSmall gradients must
  equal the one-rank gradients of the whole batch (relative 1e-5: the two
  ranks' binned table sums are each rounded once, the one-rank sum once; the
  MLP weight-gradient slabs are summed in another order).  The exchange is
  the one of run_nerf.py:640-642 (backward -> [all-reduce] -> step) under the
  per-rank loss rule of train.dp_loss (MSE / world, entropy sums unscaled, TV
  on rank 0 only).
* The one-rank gradient itself is checked against the CPU oracle on a 32-ray
  batch (the oracle's fine pass on the device's importance samples, as
  test_gpu_parity.test_fused_step_vs_oracle_on_device_z), TV included.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _trainer(hn, n_rand, HW=64, **over):
    from hashnerf_pytorch_amd.train import SyntheticBlender, Trainer, default_args
    spec_args = dict(N_rand=n_rand, log2_hashmap_size=14, tv_loss_weight=1e-4, tv_until=10 ** 6,
                     sparse_loss_weight=1e-3)
    spec_args.update(over)
    data = SyntheticBlender(HW, HW, 4, DEV, seed=0)
    tr = Trainer(default_args(**spec_args), data, DEV, seed=0)
    tr.fuse_table_step = False
    return tr, spec_args


def _grads(tr):
    ws = tr.kw_train["network_fn"].weights() + tr.kw_train["network_fine"].weights()
    return tr.embed_fn.table.grad.detach().cpu().clone(), [p.grad.detach().cpu().clone() for p in ws]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _launch(args, world=2, timeout=150):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dp_worker.py")] + args,
                                      env=env, cwd=ROOT))
    codes = []
    for p in procs:
        try:
            codes.append(p.wait(timeout=timeout))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    assert codes == [0] * world, codes


def test_dp_sharded_table_step_equals_allreduce(hn, tmp_path):
    """Two ranks, 8 training steps each (RAdam updates from step 6; TV on
    through step 4): the sharded exchange (reduce-scatter -> RAdam on the
    rank's shard -> all-gather, train.ShardedTableStep) leaves the table, its
    gathered RAdam moments and the MLP weights bitwise equal to the all-reduce
    + full RAdam path (two-rank sums are order-free; the per-element update is
    the same kernel).  The collectives run RCCL's calls (reduce_scatter_tensor
    into the shard, in-place all_gather_into_tensor into the parameter
    buffer), emulated on gloo into the same out-tensors (train.Collectives).
    The first sharded run exchanges in 4 bin-aligned segments (deferred
    owner pass per segment), the resumed one in a single exchange.
    The second sharded run resumes after 7 steps: the moments are gathered
    into the optimizer, the exchange is rebuilt from them, and the run ends
    bitwise where the uninterrupted all-reduce run does (the moments must
    carry over: from zero, step 8's update would differ)."""
    res = {}
    for name, args in (("sharded", ["1", "8"]), ("allreduce", ["0", "8"]), ("resumed", ["1", "8", "7"])):
        out = str(tmp_path / f"train_{name}.pt")
        _launch(["train", out] + args)
        res[name] = torch.load(out, weights_only=True)
    b = res["allreduce"]
    for name in ("sharded", "resumed"):
        a = res[name]
        assert a["step"] == b["step"] == 8
        for k in ("table", "m", "v"):
            assert torch.equal(a[k], b[k]), (name, k)
        assert torch.count_nonzero(a["m"]) > 0
        for x, y in zip(a["mlp"], b["mlp"]):
            assert torch.equal(x, y), name


def test_dp_empty_rank_batch(hn, tmp_path):
    """use_batching with a pool of 133 rays, N_rand 66, two ranks: every
    second step's global batch is the epoch's last position alone, so rank 0
    draws no rays; it joins the sharded exchange with its TV gradient alone
    instead of failing inside the owner pass while rank 1 waits in the
    reduce-scatter.  Six steps (three empty-rank steps)."""
    out = str(tmp_path / "pool.pt")
    _launch(["train_pool", out, "6", "-"])
    got = torch.load(out, weights_only=True)
    assert got["step"] == 6 and got["finite"]


def test_dp_device_collectives_production_calls(hn, tmp_path):
    """The sharded exchange on device tensors through the production calls
    (reduce_scatter_tensor with async_op, all_gather_into_tensor) on gloo,
    against the emulation the GPU tests use by default: the same table after
    six steps, incl. the empty-rank steps above with the TV term on the empty
    rank (round 6: its TV gradient goes through the binned records and the
    exact owner pass, hn_render_bwd with n_rays = 0, instead of the
    float-atomic hn_tv_bwd whose sums made the two runs' tables differ,
    r05a-d).  First a probe of the two
    calls on small device tensors: where this gloo build does not give their
    defined results for device tensors the comparison is skipped with the
    probe's numbers -- the production calls are then pinned by the CPU gloo
    test (tests/test_dp_gloo.py) and run on RCCL only."""
    pp = str(tmp_path / "probe.pt")
    _launch(["probe", pp])
    pr = torch.load(pp, weights_only=True)
    if not (torch.equal(pr["rs"], pr["rs_want"]) and torch.equal(pr["ag"], pr["ag_want"])):
        pytest.skip(f"gloo device-tensor collectives differ from their definition: reduce_scatter_tensor "
                    f"{pr['rs'].tolist()} (want {pr['rs_want'].tolist()}), all_gather_into_tensor "
                    f"{pr['ag'].tolist()} (want {pr['ag_want'].tolist()})")
    res = {}
    for em in ("1", "0"):
        out = str(tmp_path / f"pool_{em}.pt")
        _launch(["train_pool", out, "6", em, "1"])
        res[em] = torch.load(out, weights_only=True)
    assert torch.equal(res["0"]["table"], res["1"]["table"])


@pytest.mark.parametrize("B,T,HW,i", [(512, 14, 64, 1), (16384, 19, 200, 501)],
                         ids=["small", "config4_rank_shape"])
def test_dp_two_ranks_equal_global_batch(hn, tmp_path, B, T, HW, i):
    """Two ranks on halves of a global batch: the SUM exchange of their
    gradients = the one-rank gradient of the whole batch (relative 1e-5).
    config4_rank_shape: BASELINE configs[3]'s per-rank shape (T=19, finest
    512, 8,192 rays per rank; configs/hotdog.txt) against the one-rank
    16,384-ray gradient, full image (i > precrop_iters), TV on rank 0."""
    tr, spec_args = _trainer(hn, B, log2_hashmap_size=T, HW=HW)
    batch = tr.draw_batch(i)
    assert batch["tv"] is not None and batch["rays"].shape[0] == B
    tr._fused_forward_backward(i, batch)
    torch.cuda.synchronize()
    g_table, g_mlp = _grads(tr)
    world = 2
    ranks = []
    for r in range(world):
        sl = slice(r * B // world, (r + 1) * B // world)
        d = {k: batch[k][sl].cpu() for k in ("rays", "target", "t_rand", "u")}
        if r == 0:                                    # TV counted once (train.dp_loss)
            d["tv_cubes"], d["tv_mv"] = list(batch["tv"][0]), batch["tv"][1].cpu()
        ranks.append(d)
    spec = dict(H=HW, W=HW, n_img=4, args=spec_args, i=i, ranks=ranks)
    bpath, opath = str(tmp_path / "batch.pt"), str(tmp_path / "dp_out.pt")
    torch.save(spec, bpath)
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dp_worker.py"), bpath, opath],
                                      env=env, cwd=ROOT))
    codes = []
    for p in procs:
        try:
            codes.append(p.wait(timeout=100))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    assert codes == [0] * world, codes
    got = torch.load(opath, weights_only=True)
    e = _rel(got["table"], g_table)
    assert e <= 1e-5, f"table gradient: relative {e:.3e}"
    for k, (a, b) in enumerate(zip(got["mlp"], g_mlp)):
        e = _rel(a, b)
        assert e <= 1e-5, f"MLP gradient {k}: relative {e:.3e}"


def test_trainer_one_rank_gradient_vs_oracle(hn, oracle):
    """The explicit trainer's launch sequence (sampler batch, fused render,
    TV, fused loss, binned backward + TV backward) on 32 rays against the
    oracle's autograd of run_nerf.py:612-636 with the same inputs.
    (The samples' own check leaves 3 % of the fine z out; test_gpu_sampling.py judges every importance sample.)"""
    from hashnerf_pytorch_amd import functional as HF
    O = oracle
    tr, _ = _trainer(hn, 32)
    e = tr.embed_fn
    # a trained-like table (the init's U(-1e-4, 1e-4) leaves every ray nearly
    # transparent, where the composite backward's terms cancel and both fp32
    # gradients carry large relative rounding errors)
    with torch.no_grad():
        e.table.uniform_(-0.5, 0.5, generator=torch.Generator(device=DEV).manual_seed(2))
    tab0 = e.table.detach().cpu().clone()
    nets = (tr.kw_train["network_fn"], tr.kw_train["network_fine"])
    w0 = [[p.detach().cpu().clone() for p in n.weights()] for n in nets]
    batch = tr.draw_batch(1)
    HF.DEBUG_KEEP = True
    try:
        tr._fused_forward_backward(1, batch)
    finally:
        HF.DEBUG_KEEP = False
    z_fine = HF.LAST["z_fine"].cpu()
    g_table, g_mlp = _grads(tr)
    box = tuple(torch.as_tensor(v, dtype=torch.float32).cpu() for v in tr.data.bounding_box)
    tab = tab0.clone().requires_grad_(True)
    wc = {k: v.clone().requires_grad_(True) for k, v in zip(O.MLP_KEYS, w0[0])}
    wf = {k: v.clone().requires_grad_(True) for k, v in zip(O.MLP_KEYS, w0[1])}
    T = int(e.log2_hashmap_size)
    ret = O.render_rays(batch["rays"].cpu(), wc, wf, tab, box[0], box[1], O.level_resolutions(16, 16, 512), T,
                        t_rand=batch["t_rand"].cpu(), u=batch["u"].cpu(), white_bkgd=True, z_fine=z_fine)
    same = np.isclose(z_fine.numpy(), ret["z_vals"].detach().numpy(), rtol=0, atol=1e-5)
    assert same.mean() > 0.97, f"only {same.mean():.4f} of fine samples agree"
    cubes, mv = batch["tv"]
    tv = sum(O.total_variation_loss(tab[l], l, mv[l].cpu(), T) for l in range(16))
    loss = O.training_loss(ret, batch["target"].cpu(), 1e-3) + 1e-4 * tv
    loss.backward()
    err = _rel(g_table, tab.grad)
    assert err <= 5e-4, f"table gradient: relative {err:.3e}"
    for k, (a, ref) in enumerate(zip(g_mlp, [wc[k].grad for k in O.MLP_KEYS] + [wf[k].grad for k in O.MLP_KEYS])):
        err = _rel(a, ref)
        assert err <= 5e-4, f"MLP gradient {k}: relative {err:.3e}"
