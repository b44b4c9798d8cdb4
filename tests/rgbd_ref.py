"""Restatement in numpy float32 of the reference's RGB-D passages (test
infrastructure; the parity target of depth_kernels.hip):

  stereo_from_rgbd   Tracking::GrabImageRGBD's conversion (src/Tracking.cc:229-230)
                     + Frame::ComputeStereoFromRGBD (src/Frame.cc:707-728)
  unproject_stereo   Frame::UnprojectStereo (src/Frame.cc:730-744) per keypoint
  close_points       the vDepthIdx loops of Tracking::UpdateLastFrame
                     (src/Tracking.cc:969-1021) and CreateNewKeyFrame (:1263-1318)
  close_counts       Tracking::NeedNewKeyFrame's counts (:1181-1197)

The loops are kept as the reference writes them (no closed forms).  Three
points the reference leaves to OpenCV are pinned here, none of them against a
real OpenCV build: convertTo is cvtScale_<T, float, float>, (float)src * scale
with the scale narrowed to float; Mat::at<float>(float, float) truncates its
arguments toward zero; mRwc * x3Dc sums float products left to right.
"""
import math

import numpy as np

f32 = np.float32
DEPTH_U16, DEPTH_F32 = 0, 1


def needs_conversion(depth_map_factor, depth_dtype):
    """(fabs(mDepthMapFactor-1.0f)>1e-5) || imDepth.type()!=CV_32F (src/Tracking.cc:229):
    a float subtraction, its magnitude compared with the double 1e-5."""
    diff = f32(f32(depth_map_factor) - f32(1.0))
    return math.fabs(float(diff)) > 1e-5 or np.dtype(depth_dtype) != np.dtype(np.float32)


def _trunc(v):
    """float -> int as the arguments of Mat::at<float>(int, int) convert; None
    where the conversion is undefined (NaN, beyond int)."""
    v = float(v)
    if v != v or abs(v) >= 2147483648.0:
        return None
    return int(v)  # toward zero


@np.errstate(all="ignore")
def stereo_from_rgbd(keys, keys_un, depth, depth_map_factor, bf):
    """(mvuRight, mvDepth).  `depth` is the image as GrabImageRGBD receives it
    (uint16 or float32, any row pitch); depth_map_factor is mDepthMapFactor as
    Tracking holds it (already inverted, src/Tracking.cc:143-147)."""
    n = len(keys)
    rows, cols = depth.shape
    factor = f32(depth_map_factor)
    convert = needs_conversion(depth_map_factor, depth.dtype)
    u_right = np.full(n, -1, f32)   # :709
    z_out = np.full(n, -1, f32)     # :710
    for i in range(n):              # :712
        v = keys["y"][i]            # :717
        u = keys["x"][i]            # :718
        row, col = _trunc(v), _trunc(u)
        if row is None or col is None or not (0 <= row < rows and 0 <= col < cols):
            continue                # undefined in the reference; -1 / -1 here
        src = depth[row, col]       # :720, converted on the fly
        d = f32(f32(src) * factor) if convert else f32(src)
        if d > 0:                   # :722
            z_out[i] = d
            u_right[i] = f32(keys_un["x"][i] - f32(f32(bf) / d))  # :725
    return u_right, z_out


@np.errstate(all="ignore")
def unproject_stereo(keys_un, depth, rcw, ow, fx, fy, cx, cy):
    """(x3D (n, 3), valid (n,)): UnprojectStereo(i) for every i; an empty Mat is
    valid = 0 with a zero row."""
    n = len(keys_un)
    rcw = np.asarray(rcw, f32).reshape(9)
    ow = np.asarray(ow, f32).reshape(3)
    invfx = f32(f32(1.0) / f32(fx))   # src/Frame.cc:115
    invfy = f32(f32(1.0) / f32(fy))
    cx, cy = f32(cx), f32(cy)
    x3d = np.zeros((n, 3), f32)
    valid = np.zeros(n, np.uint8)
    for i in range(n):
        z = f32(depth[i])              # :732
        if z > 0:                      # :733
            u = keys_un["x"][i]
            v = keys_un["y"][i]
            x = f32(f32(f32(u - cx) * z) * invfx)   # :737
            y = f32(f32(f32(v - cy) * z) * invfy)   # :738
            for r in range(3):         # mRwc = mRcw.t(): row r of Rwc is column r of Rcw
                s = f32(f32(rcw[r] * x) + f32(rcw[3 + r] * y))
                s = f32(s + f32(rcw[6 + r] * z))
                x3d[i, r] = f32(s + ow[r])          # :740
            valid[i] = 1
    return x3d, valid


def close_points(depth, mp_state, th_depth):
    """(order, create): the keypoint index at every position of the sorted
    vDepthIdx, and bCreateNew at each position the loop processes before its
    break (len(create) = n_visit).  mp_state: 0 NULL, 1 Observations() < 1,
    2 observed."""
    th = f32(th_depth)
    v_depth_idx = []                       # :971
    for i in range(len(depth)):            # :973
        z = f32(depth[i])
        if z > 0:                          # :976
            v_depth_idx.append((z, i))
    if not v_depth_idx:                    # :982
        return np.zeros(0, np.int32), np.zeros(0, np.uint8)
    v_depth_idx = sorted(v_depth_idx)      # :985 (pairs: z, then index)
    create = []
    n_points = 0                           # :989
    for j in range(len(v_depth_idx)):      # :990
        i = v_depth_idx[j][1]
        create_new = False
        if mp_state[i] == 0:               # :997
            create_new = True
        elif mp_state[i] == 1:             # :999
            create_new = True
        if create_new:
            n_points += 1                  # :1012
        else:
            n_points += 1                  # :1016
        create.append(1 if create_new else 0)
        if v_depth_idx[j][0] > th and n_points > 100:   # :1019
            break
    return (np.array([i for _, i in v_depth_idx], np.int32), np.array(create, np.uint8))


def close_counts(depth, mp_state, outlier, th_depth):
    """(nTrackedClose, nNonTrackedClose) of NeedNewKeyFrame (:1181-1197)."""
    th = f32(th_depth)
    tracked = non_tracked = 0
    for i in range(len(depth)):
        z = f32(depth[i])
        if z > 0 and z < th:                       # :1187
            if mp_state[i] != 0 and not outlier[i]:  # :1189
                tracked += 1
            else:
                non_tracked += 1
    return tracked, non_tracked
