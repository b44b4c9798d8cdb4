"""k_pose_optimization on the directed inputs of poseopt_edge_cases.py against
the numpy restatement tests/poseopt_ref.py, every output bit for bit (NaN
positions comparing equal): through the single-frame call, and packed into
batches that share a camera and a level table, once with the edge records in
LDS and once, one keypoint slot of stride further, in the handle's device
scratch (the GLOBAL instantiation), with junk past every count that must stay.
test_poseopt_edge_cases.py shows on the CPU which paths these inputs reach."""
import functools

import numpy as np
import pytest

import poseopt_cases as pc
import poseopt_edge_cases as E
import test_gpu_poseopt as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.mark.parametrize("name", list(E.CASES))
def test_directed_single(gpu, name):
    c, r = E.run(name)
    n, pose, outlier, info = T._one_frame(gpu, c)
    T._assert_result(pose, outlier, info, r, name)
    assert n == r["n_inliers"]
    no_edge = c["point_index"] < 0
    assert (outlier[no_edge] == pc.SENTINEL).all()
    if r["n_edges"] < 0:
        assert (outlier == pc.SENTINEL).all() and pose.tobytes() == c["pose"][0].tobytes()


def batch_key(c):
    """What one batch call shares: the camera and the level table."""
    return (np.asarray(c.get("cam", pc.CAM), np.float32).tobytes(),
            np.asarray(c.get("levels", pc.INV_LEVEL_SIGMA2), np.float32).tobytes())


@functools.lru_cache(maxsize=None)
def groups():
    g = {}
    for name in E.CASES:
        g.setdefault(batch_key(E.run(name)[0]), []).append(name)
    return sorted(g.values())


def _group_ids():
    return ["+".join(names)[:60] for names in groups()]


@pytest.mark.parametrize("above", [0, 1], ids=["lds", "scratch"])
@pytest.mark.parametrize("names", groups(), ids=_group_ids())
def test_directed_batch(gpu, torch, names, above):
    """All cases of one camera and level table in one call; kp_stride at the
    LDS boundary, then one above it."""
    cr = [E.run(n) for n in names]
    c0 = cr[0][0]
    kp_stride = gpu.ORBmatcher.pose_optimization_lds_edges() + above
    assert max(len(c["keys"]) for c, _ in cr) < kp_stride
    run = T._pack_batch(gpu, torch, [c for c, _ in cr], kp_stride, "f3" if above else "mp",
                        levels=c0.get("levels"), cam=c0.get("cam"))
    d_pout, d_outl, d_info = run(gpu.ORBmatcher())
    torch.cuda.synchronize()
    T._check_batch(gpu, cr, kp_stride, d_pout, d_outl, d_info)
    outl = T._host(d_outl, np.uint8, (len(cr), kp_stride))
    for i, (c, _) in enumerate(cr):
        assert (outl[i, :len(c["keys"])][c["point_index"] < 0] == pc.SENTINEL).all(), names[i]
