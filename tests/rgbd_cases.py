"""Inputs shared by the CPU and GPU RGB-D tests (test infrastructure): the
break-rule frames with their hand-computed answers, and keypoint records."""
import numpy as np

f32 = np.float32

KEYPOINT_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
     ("octave", "<i4"), ("class_id", "<i4")])


def keypoints(xy):
    k = np.zeros(len(xy), KEYPOINT_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["size"], k["class_id"] = 31.0, -1
    return k


def _frame(c, size, th=f32(5.0), seed=0):
    """`size` positive depths, c of them <= th (so size - c beyond it), shuffled,
    with a few non-positive slots mixed in.  The loop processes every close
    point, goes on to 100 points if there are fewer, and stops one past the
    first position that is beyond th with more than 100 processed: n_visit =
    min(size, max(c, 100) + 1)."""
    rng = np.random.default_rng(1000 * c + size + seed)
    near = rng.uniform(0.5, 5.0, c).astype(f32)
    far = rng.uniform(5.5, 40.0, size - c).astype(f32)
    z = np.concatenate([near, far, np.array([0.0, -1.0, np.nan], f32)])
    rng.shuffle(z)
    return z, th, size, min(size, max(c, 100) + 1)


def _all_far_40():
    z, th, n, _ = _frame(0, 40)
    return z, th, 40, 40


def _z_equals_th():
    # 150 points at exactly th, then 10 beyond: z == th never breaks, so the
    # loop stops one past the first point beyond th
    z = np.concatenate([np.full(150, 5.0, f32), np.linspace(6, 7, 10).astype(f32)])
    return z, f32(5.0), 160, 151


def _equal_depths():
    # 120 equal far depths: the break comes after position 100 (nPoints = 101)
    return np.full(120, 9.0, f32), f32(5.0), 120, 101


def _with_inf():
    z = np.concatenate([np.linspace(1, 4, 30).astype(f32), np.array([np.inf], f32)])
    return z, f32(5.0), 31, 31


BREAK_CASES = {"all_far_40": _all_far_40, "z_equals_th": _z_equals_th,
               "equal_depths": _equal_depths, "with_inf": _with_inf}
for _c in (0, 99, 100, 101, 150):
    for _extra in (0, 1, 5):
        if _c + _extra > 0:
            BREAK_CASES[f"c{_c}_n{_c + _extra}"] = (
                lambda c=_c, e=_extra: _frame(c, c + e))
