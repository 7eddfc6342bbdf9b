"""hn_sample_pool_ordered on the device (functional.sample_pool(order=1) and
Trainer(pool_order=1)): the batch is hn_sample_pool's, bitwise, in ascending
(key, position) with the key of pool_order_key.py; the uniforms made in the
same launch are torch.rand's."""
import numpy as np
import pytest
import torch

from conftest import golden
from pool_order_key import pool_key, pool_perm

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 11


@pytest.fixture(scope="module")
def pool(hn):
    """The fixture pool: 3 training images of 20 x 24, 1,440 rays."""
    g = golden("pool_rays")
    return dict(images=torch.from_numpy(g["images"]).to(DEV), poses=torch.from_numpy(g["poses"]).to(DEV),
                ids=torch.from_numpy(g["i_train"]).to(DEV, torch.int32), K=g["K"])


def _draw(hn, pl, start, n, **kw):
    return hn.functional.sample_pool(pl["images"], pl["poses"], pl["ids"], pl["K"], 2., 6., SEED, start, n, **kw)


def _check_ordered(hn, pl, start, n, box):
    """order=1 is order=0 under the lexsort permutation of the numpy keys,
    bitwise, keys included, and again on a second call."""
    r0, t0 = _draw(hn, pl, start, n)
    keys, _ = pool_key(r0.cpu().numpy(), box[0], box[1], 2., 6.)
    perm = pool_perm(keys)
    pt = torch.from_numpy(perm).to(DEV)
    r1, t1, k1 = _draw(hn, pl, start, n, order=1, box=box, return_keys=True)
    assert r1.shape == (n, 11) and t1.shape == (n, 3) and k1.shape == (n,) and k1.dtype == torch.int32
    assert torch.equal(r1, r0[pt]), "rays: hn_sample_pool's rows in (key, position) order"
    assert torch.equal(t1, t0[pt])
    np.testing.assert_array_equal(k1.cpu().numpy().astype(np.uint32), keys[perm])
    r2, t2, k2 = _draw(hn, pl, start, n, order=1, box=box, return_keys=True)
    assert torch.equal(r2, r1) and torch.equal(t2, t1) and torch.equal(k2, k1)
    return keys


@pytest.mark.parametrize("half_side", [1.0, 1.5])
@pytest.mark.parametrize("start,n", [(0, 1440), (700, 300), (0, 1), (1439, 1), (0, 64), (0, 65)])
def test_same_rays_in_key_order(hn, pool, half_side, start, n):
    box = ([-half_side] * 3, [half_side] * 3)
    keys = _check_ordered(hn, pool, start, n, box)
    if n == 1440:   # the whole pool: the counts test_pool_order_cpu pins for the fixture (ties, clamping)
        assert len(np.unique(keys)) == (1338 if half_side == 1.0 else 1438)


@pytest.mark.parametrize("start,n", [(4096, 8192), (0, 4097)])
def test_capacity(hn, start, n):
    """HN_POOL_ORDER_MAX rays (the whole LDS array, no padding), and one more
    than a power of two (padded to 8,192)."""
    from hashnerf_pytorch_amd.train import SyntheticBlender
    d = SyntheticBlender(64, 64, 3, DEV, seed=0)            # 12,288 pool rays
    pl = dict(images=d.images, poses=d.poses, ids=torch.as_tensor(d.i_train).to(DEV, torch.int32), K=d.K)
    box = tuple([float(v) for v in b] for b in d.bounding_box)
    _check_ordered(hn, pl, start, n, box)
    with pytest.raises(ValueError, match="8192"):
        _draw(hn, pl, 0, 8193, order=1, box=box)


def test_all_ties_keep_the_shuffle_order(hn, pool):
    box = ([10.] * 3, [11.] * 3)                            # every ray clamps to key 0
    r0, t0 = _draw(hn, pool, 0, 1440)
    r1, t1, k1 = _draw(hn, pool, 0, 1440, order=1, box=box, return_keys=True)
    assert int(k1.abs().max()) == 0
    assert torch.equal(r1, r0) and torch.equal(t1, t0)


@pytest.mark.parametrize("n", [300, 4097])
def test_uniforms_in_the_launch(hn, n):
    from hashnerf_pytorch_amd.train import SyntheticBlender
    d = SyntheticBlender(64, 64, 3, DEV, seed=0)
    pl = dict(images=d.images, poses=d.poses, ids=torch.as_tensor(d.i_train).to(DEV, torch.int32), K=d.K)
    box = tuple([float(v) for v in b] for b in d.bounding_box)
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    torch.cuda.manual_seed(77)
    a, b = torch.rand((n, 64), device=DEV), torch.rand((n, 128), device=DEV)
    off = gen.get_offset()
    torch.cuda.manual_seed(77)
    r1, t1, u1, u2, k1 = _draw(hn, pl, 100, n, order=1, box=box, uniforms=[(n, 64), (n, 128)], return_keys=True)
    assert gen.get_offset() == off
    assert torch.equal(u1, a) and torch.equal(u2, b)
    r0, t0, k0 = _draw(hn, pl, 100, n, order=1, box=box, return_keys=True)
    assert torch.equal(r1, r0) and torch.equal(t1, t0) and torch.equal(k1, k0)
    # order=0 takes the uniforms from torch_uniform's own launch: same values
    torch.cuda.manual_seed(77)
    out = _draw(hn, pl, 100, n, uniforms=[(n, 64), (n, 128)])
    assert len(out) == 4 and torch.equal(out[2], a) and torch.equal(out[3], b) and gen.get_offset() == off


def test_keys_null(hn, pool):
    box = ([-1.] * 3, [1.] * 3)
    out = _draw(hn, pool, 700, 300, order=1, box=box)
    assert len(out) == 2
    r1, t1, _ = _draw(hn, pool, 700, 300, order=1, box=box, return_keys=True)
    assert torch.equal(out[0], r1) and torch.equal(out[1], t1)
    with pytest.raises(ValueError, match="box"):
        _draw(hn, pool, 0, 8, order=1)


def test_trainer_pool_order(hn):
    from hashnerf_pytorch_amd.train import SyntheticBlender, Trainer, default_args

    def make(order, N_rand=300):
        data = SyntheticBlender(16, 16, 3, DEV, seed=0)     # pool of 768 rays
        args = default_args(N_rand=N_rand, log2_hashmap_size=12, no_batching=False, perturb=0., tv_loss_weight=0.)
        return Trainer(args, data, DEV, seed=3, pool_order=order)

    tr0, tr1 = make(0), make(1)
    g = tr1.embed_fn.grid()
    box = (list(g.box_min), list(g.box_max))
    sizes = [[], []]
    for _ in range(4):
        b0, b1 = tr0.draw_batch(), tr1.draw_batch()
        sizes[0].append(b0["rays"].shape[0])
        sizes[1].append(b1["rays"].shape[0])
        keys, _ = pool_key(b0["rays"].cpu().numpy(), box[0], box[1], 2., 6.)
        pt = torch.from_numpy(pool_perm(keys)).to(DEV)
        assert torch.equal(b1["rays"], b0["rays"][pt]) and torch.equal(b1["target"], b0["target"][pt])
        tr0.global_step += 1
        tr1.global_step += 1
    assert sizes[0] == sizes[1] == [300, 300, 168, 300]
    assert (tr0.epoch, tr0.i_batch) == (tr1.epoch, tr1.i_batch) == (1, 300)
    # the same rays meet the same weights; the loss is an fp64 sum in another order
    l0, l1 = float(tr0.step()[0]), float(tr1.step()[0])
    print(f"loss pool_order=0 {l0!r}  pool_order=1 {l1!r}  rel {abs(l1 - l0) / abs(l0):.3e}")
    assert np.isfinite(l0) and np.isfinite(l1)
    assert abs(l1 - l0) <= 1e-6 * abs(l0)
    with pytest.raises(ValueError, match="8192"):
        make(1, N_rand=8193)
