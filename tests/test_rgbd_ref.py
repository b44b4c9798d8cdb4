"""Hand-computed answers for tests/rgbd_ref.py, the restatement the GPU RGB-D
kernels are compared against (src/Tracking.cc:229-230, src/Frame.cc:707-744,
src/Tracking.cc:969-1021, :1181-1197, :1263-1318)."""
import numpy as np
import pytest

import rgbd_ref
from rgbd_cases import BREAK_CASES, keypoints

f32 = np.float32


def _keys(xy):
    return keypoints(np.array(xy, f32))


# a 4 x 3 image (cols x rows); keypoints at fractional positions inside it
_XY = [(0.0, 0.0), (1.9, 0.5), (3.0, 2.0), (2.2, 1.7), (0.999, 2.999)]
_POS = [(0, 0), (0, 1), (2, 3), (1, 2), (2, 0)]  # (row, col) each truncates to


def test_conversion_condition_branches():
    assert not rgbd_ref.needs_conversion(1.0, np.float32)
    assert rgbd_ref.needs_conversion(f32(1.0) + f32(2e-5), np.float32)
    assert not rgbd_ref.needs_conversion(f32(1.0) + f32(5e-6), np.float32)
    assert rgbd_ref.needs_conversion(1.0, np.uint16)
    assert rgbd_ref.needs_conversion(1.0 / 5000.0, np.uint16)


@pytest.mark.parametrize("dtype,factor", [
    (np.float32, 1.0),            # bits pass through
    (np.float32, 1.0 + 2e-5),     # converted: the product is rounded to float
    (np.uint16, 1.0),             # converted because of the type
    (np.uint16, 1.0 / 5000.0),    # TUM: DepthMapFactor 5000
], ids=["f32_1", "f32_1p2e-5", "u16_1", "u16_5000"])
def test_stereo_from_rgbd_4x3(dtype, factor):
    if dtype == np.float32:
        img = np.array([[1.5, 0.0, 2.25, -3.0],
                        [0.75, 4.0, 8.0, 16.0],
                        [0.1, 0.2, 0.3, 32.0]], f32)
    else:
        img = np.array([[5000, 0, 65535, 1],
                        [2500, 10000, 20000, 40000],
                        [1, 2, 3, 15000]], np.uint16)
    keys = _keys(_XY)
    un = keys.copy()
    un["x"] += f32(0.25)
    bf = f32(40.0)
    ur, z = rgbd_ref.stereo_from_rgbd(keys, un, img, factor, bf)
    fac = f32(factor)
    for i, (r, c) in enumerate(_POS):
        src = img[r, c]
        if dtype == np.float32 and factor == 1.0:
            d = src
        else:
            d = f32(f32(src) * fac)
        if d > 0:
            assert z[i].tobytes() == f32(d).tobytes()
            assert ur[i].tobytes() == f32(un["x"][i] - f32(bf / d)).tobytes()
        else:
            assert z[i] == -1 and ur[i] == -1
    # spot values worked by hand
    if dtype == np.float32 and factor == 1.0:
        assert z.tolist() == [1.5, -1.0, 32.0, 8.0, f32(0.1)]
        assert ur[0] == f32(0.25) - f32(40.0) / f32(1.5)
        assert ur[2] == f32(3.25) - f32(1.25)
    if dtype == np.uint16 and factor == 1.0:
        assert z.tolist() == [5000.0, -1.0, 15000.0, 20000.0, 1.0]
    if dtype == np.uint16 and factor != 1.0:
        assert z[0] == f32(5000.0) * f32(1.0 / 5000.0) and z[4] == f32(1.0) * f32(1.0 / 5000.0)
    if dtype == np.float32 and factor != 1.0:
        assert z[0] == f32(1.5) * f32(1.0 + 2e-5) and z[0] != f32(1.5)


def test_stereo_from_rgbd_outside_is_minus_one():
    img = np.ones((3, 4), f32)
    keys = _keys([(4.0, 0.0), (0.0, 3.0), (-1.0, 0.0), (-0.5, -0.5), (np.nan, 0.0), (3e9, 1.0)])
    ur, z = rgbd_ref.stereo_from_rgbd(keys, keys, img, 1.0, 40.0)
    # (-0.5, -0.5) truncates to (0, 0): inside
    assert z.tolist() == [-1, -1, -1, 1, -1, -1]
    assert ur[3] == f32(-0.5) - f32(40.0)


def test_unproject_identity_and_general():
    keys = _keys([(10.0, 20.0), (30.5, 7.25), (1.0, 1.0)])
    depth = np.array([2.0, -1.0, 4.0], f32)
    eye = np.eye(3, dtype=f32).reshape(9)
    x, v = rgbd_ref.unproject_stereo(keys, depth, eye, np.zeros(3, f32), 2.0, 4.0, 6.0, 8.0)
    assert v.tolist() == [1, 0, 1]
    # x = (10 - 6) * 2 * 0.5 = 4, y = (20 - 8) * 2 * 0.25 = 6
    assert x[0].tolist() == [4.0, 6.0, 2.0] and x[1].tolist() == [0, 0, 0]
    assert x[2].tolist() == [-10.0, -7.0, 4.0]
    # Rcw = rotation by 90 degrees about z: Rwc = Rcw^T
    rcw = np.array([0, -1, 0, 1, 0, 0, 0, 0, 1], f32)
    ow = np.array([1, 2, 3], f32)
    x, v = rgbd_ref.unproject_stereo(keys, depth, rcw, ow, 2.0, 4.0, 6.0, 8.0)
    # X = rcw[0]*4 + rcw[3]*6 + rcw[6]*2 + 1 = 7;  Y = rcw[1]*4 + rcw[4]*6 + rcw[7]*2 + 2 = -2
    assert x[0].tolist() == [7.0, -2.0, 5.0]


@pytest.mark.parametrize("name", sorted(BREAK_CASES))
def test_break_rule(name):
    depth, th, n_sorted, n_visit = BREAK_CASES[name]()
    mp_state = np.zeros(len(depth), np.uint8)
    order, create = rgbd_ref.close_points(depth, mp_state, th)
    assert len(order) == n_sorted, name
    assert len(create) == n_visit, name
    assert create.all()
    z = depth[order]
    assert (np.diff(z) >= 0).all()


def test_ties_inf_and_states():
    depth = np.array([3.0, 1.0, 3.0, np.inf, 0.0, -2.0, np.nan, 1.0], f32)
    mp_state = np.array([2, 0, 1, 2, 0, 0, 0, 2], np.uint8)
    order, create = rgbd_ref.close_points(depth, mp_state, 2.0)
    assert order.tolist() == [1, 7, 0, 2, 3]     # ties by index, +inf last
    assert create.tolist() == [1, 0, 0, 1, 0]    # fewer than 100 points: all visited
    outlier = np.array([0, 0, 0, 0, 0, 0, 0, 1], np.uint8)
    # close: z in (0, 2): indices 1 (no point), 7 (point, outlier)
    assert rgbd_ref.close_counts(depth, mp_state, outlier, 2.0) == (0, 2)
    assert rgbd_ref.close_counts(depth, mp_state, outlier, 3.5) == (2, 2)
    # z == th is not close
    assert rgbd_ref.close_counts(depth, mp_state, outlier, 3.0) == (0, 2)
