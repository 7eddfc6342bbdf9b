"""numpy restatement of hn_sample_pool_ordered's key and order (helper of
test_pool_order_cpu.py and test_gpu_pool_order.py; include/hashnerf_amd.h has
the definition).  Every operation is a float32 one, as the kernel's."""
import numpy as np

F = np.float32


def pool_key(rays, box_min, box_max, near=2., far=6.):
    """rays [n, >= 6] float32 (o = [:, 0:3], d = [:, 3:6]) -> (uint32 keys [n],
    bool [n]: the ray's mid-depth point was clamped on some axis)."""
    rays = np.asarray(rays, dtype=F)
    tm = F(0.5) * (F(near) + F(far))
    key = np.zeros(rays.shape[0], dtype=np.uint32)
    clamped = np.zeros(rays.shape[0], dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            lo, hi = F(box_min[a]), F(box_max[a])
            pt = rays[:, a] + rays[:, 3 + a] * tm
            u = (pt - lo) / (hi - lo)
            assert pt.dtype == F and u.dtype == F
            clamped |= ~((u >= 0) & (u <= 1))
            u = np.fmin(np.fmax(u, F(0)), F(1))          # fmax(NaN, 0) = 0
            c = np.minimum((u * F(1024)).astype(np.int32), 1023).astype(np.uint32)
            for k in range(10):
                key |= ((c >> np.uint32(k)) & np.uint32(1)) << np.uint32(3 * k + a)
    return key, clamped


def pool_perm(keys):
    """Ascending (key, position): ties keep the shuffle's order."""
    return np.lexsort((np.arange(len(keys)), keys))
