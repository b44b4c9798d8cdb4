"""Independent pure-Python / numpy restatements used to cross-check the C++ oracle
on small inputs (test infrastructure only).

They follow the reference text directly, written a second time and differently
(numpy where the rule is arithmetic, plain lists where it is control flow), so a
transcription slip in oracle/orb_oracle.cpp shows up as a disagreement.
"""
from __future__ import annotations

import math

import numpy as np

CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3),
          (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def f32(x):
    return np.float32(x)


# ------------------------------------------------------------------ FAST (A.1)
def fast(img: np.ndarray, t: int):
    """cv::FAST(img, kps, t, nonmax=True) from its mathematical definition:
    corner iff 9 contiguous circle pixels are all < v-t or all > v+t; score =
    max(t, best dark arc, best bright arc) - 1; NMS vs 8-neighbours with
    non-corners (and everything outside rows/cols 3..n-4) at 0."""
    t = min(max(t, 0), 255)
    h, w = img.shape
    I = img.astype(np.int32)
    score = np.zeros((h, w), np.int32)
    corner = np.zeros((h, w), bool)
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            v = I[y, x]
            ring = [I[y + dy, x + dx] for dx, dy in CIRCLE]
            dark = [v - r for r in ring]  # > t for dark pixels
            best_d = max(min(dark[(k + j) % 16] for j in range(9)) for k in range(16))
            best_b = max(min(-dark[(k + j) % 16] for j in range(9)) for k in range(16))
            if best_d > t or best_b > t:
                corner[y, x] = True
                score[y, x] = max(t, best_d, best_b) - 1
    out = []
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            if not corner[y, x]:
                continue
            s = score[y, x]
            if all(s > score[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                   if dy or dx):
                out.append((x, y, s))
    return out


# --------------------------------------------------------- resize INTER_LINEAR (A.2)
def resize_linear(src: np.ndarray, dw: int, dh: int) -> np.ndarray:
    sh, sw = src.shape
    scale_x = 1.0 / (dw / sw)
    scale_y = 1.0 / (dh / sh)

    def coeffs(n_dst, n_src, scale, clamp):
        idx = np.zeros(n_dst, np.int64)
        w0 = np.zeros(n_dst, np.int64)
        w1 = np.zeros(n_dst, np.int64)
        edge = np.zeros(n_dst, bool)
        for d in range(n_dst):
            f = f32((d + 0.5) * scale - 0.5)
            s = int(math.floor(f))
            f = f32(f - f32(s))
            if clamp:
                if s < 0:
                    f, s = f32(0), 0
                if s + 1 >= n_src:
                    edge[d] = True
                    if s >= n_src - 1:
                        f, s = f32(0), n_src - 1
            idx[d] = s
            w0[d] = int(np.rint(f32(f32(1) - f) * f32(2048)))
            w1[d] = int(np.rint(f * f32(2048)))
        return idx, w0, w1, edge

    xi, a0, a1, xedge = coeffs(dw, sw, scale_x, True)
    yi, b0, b1, _ = coeffs(dh, sh, scale_y, False)
    first_edge = int(np.argmax(xedge)) if xedge.any() else dw
    S = src.astype(np.int64)
    x1 = np.minimum(xi + 1, sw - 1)
    H = S[:, xi] * a0 + S[:, x1] * a1
    H[:, first_edge:] = S[:, xi[first_edge:]] * 2048
    r0 = np.clip(yi, 0, sh - 1)
    r1 = np.clip(yi + 1, 0, sh - 1)
    D = (H[r0] * b0[:, None] + H[r1] * b1[:, None] + (1 << 21)) >> 22
    return np.clip(D, 0, 255).astype(np.uint8)


# ------------------------------------------------------ GaussianBlur 7x7 (A.3)
def gaussian_kernel_int():
    """getGaussianKernel(7, 2, CV_32F) then cvRound(k * 256)."""
    x = np.arange(7) - 3.0
    k = np.array([f32(math.exp(-0.5 / (2.0 * 2.0) * v * v)) for v in x], np.float32)
    s = 0.0
    for v in k:
        s += float(v)
    k = np.array([f32(float(v) * (1.0 / s)) for v in k], np.float32)
    return [int(np.rint(f32(v) * f32(256))) for v in k]


def blur7(src: np.ndarray) -> np.ndarray:
    k = np.array(gaussian_kernel_int(), np.int64)
    p = np.pad(src.astype(np.int64), 3, mode="reflect")  # numpy 'reflect' == BORDER_REFLECT_101
    h, w = src.shape
    rows = sum(k[i] * p[:, i:i + w] for i in range(7))
    cols = sum(k[j] * rows[j:j + h, :] for j in range(7))
    return np.clip((cols + (1 << 15)) >> 16, 0, 255).astype(np.uint8)


# ----------------------------------------------------------- fastAtan2 (A.4)
def fast_atan2(y, x):
    y, x = f32(y), f32(x)
    r2d = f32(180.0 / math.pi)
    p1, p3 = f32(0.9997878412794807) * r2d, f32(-0.3258083974640975) * r2d
    p5, p7 = f32(0.1555786518463281) * r2d, f32(-0.04432655554792128) * r2d
    ax, ay = abs(x), abs(y)
    eps = f32(2.220446049250313e-16)
    if ax >= ay:
        c = f32(ay / f32(ax + eps))
        c2 = f32(c * c)
        a = f32(f32(f32(f32(f32(f32(f32(p7 * c2) + p5) * c2) + p3) * c2) + p1) * c)
    else:
        c = f32(ax / f32(ay + eps))
        c2 = f32(c * c)
        a = f32(f32(90) - f32(f32(f32(f32(f32(f32(f32(p7 * c2) + p5) * c2) + p3) * c2) + p1) * c))
    if x < 0:
        a = f32(f32(180) - a)
    if y < 0:
        a = f32(f32(360) - a)
    return a


# ------------------------------------------------- DistributeOctTree (a5)
class _Node:
    __slots__ = ("keys", "ul", "ur", "bl", "br", "nomore", "seq")

    def __init__(self, ul, ur, bl, br, seq):
        self.keys, self.ul, self.ur, self.bl, self.br = [], ul, ur, bl, br
        self.nomore, self.seq = False, seq


def distribute(keys, minX, maxX, minY, maxY, N):
    """keys: list of (x, y, response) relative to the border origin.
    Python list as the std::list (index 0 = front); node creation sequence as
    the pointer tie-break."""
    nIni = int(math.floor(float(f32(f32(maxX - minX) / f32(maxY - minY))) + 0.5))  # roundf
    hX = f32(f32(maxX - minX) / f32(nIni))
    seq = [0]

    def new(ul, ur, bl, br):
        n = _Node(ul, ur, bl, br, seq[0])
        seq[0] += 1
        return n

    lst = []
    ini = []
    for i in range(nIni):
        ulx, urx = int(f32(hX * f32(i))), int(f32(hX * f32(i + 1)))
        n = new((ulx, 0), (urx, 0), (ulx, maxY - minY), (urx, maxY - minY))
        lst.append(n)
        ini.append(n)
    for k in keys:
        ini[int(f32(f32(k[0]) / hX))].keys.append(k)
    lst = [n for n in lst if n.keys]
    for n in lst:
        n.nomore = len(n.keys) == 1

    def divide(p):
        hx = int(math.ceil(float(f32(p.ur[0] - p.ul[0]) / f32(2))))
        hy = int(math.ceil(float(f32(p.br[1] - p.ul[1]) / f32(2))))
        c1 = new(p.ul, (p.ul[0] + hx, p.ul[1]), (p.ul[0], p.ul[1] + hy), (p.ul[0] + hx, p.ul[1] + hy))
        c2 = new(c1.ur, p.ur, c1.br, (p.ur[0], p.ul[1] + hy))
        c3 = new(c1.bl, c1.br, p.bl, (c1.br[0], p.bl[1]))
        c4 = new(c3.ur, c2.br, c3.br, p.br)
        for k in p.keys:
            if k[0] < c1.ur[0]:
                (c1 if k[1] < c1.br[1] else c3).keys.append(k)
            elif k[1] < c1.br[1]:
                c2.keys.append(k)
            else:
                c4.keys.append(k)
        out = []
        for c in (c1, c2, c3, c4):
            c.nomore = len(c.keys) == 1
            if c.keys:
                out.append(c)
        return out

    # creation numbers only matter among pushed nodes: renumber at push time
    counter = [nIni]

    def push_children(children, sized):
        nonlocal lst
        for c in children:
            c.seq = counter[0]
            counter[0] += 1
            lst.insert(0, c)
            if len(c.keys) > 1:
                sized.append(c)

    finish = False
    sized = []
    while not finish:
        prev = len(lst)
        sized = []
        n_expand = 0
        i = 0
        while i < len(lst):
            nd = lst[i]
            if nd.nomore:
                i += 1
                continue
            before = len(sized)
            kids = divide(nd)
            lst.pop(i)
            push_children(kids, sized)
            n_expand += len(sized) - before
            i += len(kids)  # skip the children now in front of the cursor
        if len(lst) >= N or len(lst) == prev:
            finish = True
        elif len(lst) + n_expand * 3 > N:
            while not finish:
                prev = len(lst)
                cand = sorted(sized, key=lambda n: (len(n.keys), n.seq))
                sized = []
                for nd in reversed(cand):
                    kids = divide(nd)
                    lst.remove(nd)
                    push_children(kids, sized)
                    if len(lst) >= N:
                        break
                if len(lst) >= N or len(lst) == prev:
                    finish = True
    result = []
    for nd in lst:
        best = nd.keys[0]
        for k in nd.keys[1:]:
            if k[2] > best[2]:
                best = k
        result.append(best)
    return result


# ------------------------------------------------- grid + GetFeaturesInArea
def grid_cells(keys, width, height):
    invW = f32(f32(64) / f32(width))
    invH = f32(f32(48) / f32(height))
    cells = {}
    for i, k in enumerate(keys):
        vx, vy = f32(f32(k["x"]) * invW), f32(f32(k["y"]) * invH)
        px = int(math.floor(float(vx) + 0.5)) if vx >= 0 else -int(math.floor(-float(vx) + 0.5))
        py = int(math.floor(float(vy) + 0.5)) if vy >= 0 else -int(math.floor(-float(vy) + 0.5))
        if 0 <= px < 64 and 0 <= py < 48:
            cells.setdefault((px, py), []).append(i)
    return cells, invW, invH


def features_in_area(keys, cells, invW, invH, x, y, r, minL, maxL, closed=False):
    """`closed` switches the window's strict `<` to the wrong neighbour `<=`
    (sensitivity tests only)."""
    x, y, r = f32(x), f32(y), f32(r)
    x0 = max(0, int(math.floor(float(f32(f32(x - r) * invW)))))
    if x0 >= 64:
        return []
    x1 = min(63, int(math.ceil(float(f32(f32(x + r) * invW)))))
    if x1 < 0:
        return []
    y0 = max(0, int(math.floor(float(f32(f32(y - r) * invH)))))
    if y0 >= 48:
        return []
    y1 = min(47, int(math.ceil(float(f32(f32(y + r) * invH)))))
    if y1 < 0:
        return []
    check = minL > 0 or maxL >= 0
    out = []
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            for i in cells.get((ix, iy), []):
                k = keys[i]
                if check and (k["octave"] < minL or (maxL >= 0 and k["octave"] > maxL)):
                    continue
                dx, dy = abs(f32(k["x"] - x)), abs(f32(k["y"] - y))
                if (dx <= r and dy <= r) if closed else (dx < r and dy < r):
                    out.append(i)
    return out


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def search_by_projection_local(keys, desc, scale, width, height, mps, mp_desc, th, nnratio,
                               locked=None):
    cells, invW, invH = grid_cells(keys, width, height)
    lock = np.zeros(len(keys), bool) if locked is None else locked.astype(bool).copy()
    km = np.full(len(keys), -1, np.int32)
    n = 0
    for m, mp in enumerate(mps):
        if not mp["in_view"] or mp["bad"]:
            continue
        lvl = int(mp["level"])
        r = f32(2.5) if float(mp["view_cos"]) > 0.998 else f32(4.0)  # float vs double literal
        if f32(th) != f32(1.0):
            r = f32(r * f32(th))
        rs = f32(r * f32(scale[lvl]))
        idxs = features_in_area(keys, cells, invW, invH, mp["proj_x"], mp["proj_y"], rs, lvl - 1, lvl)
        best, bl, best2, bl2, bi = 256, -1, 256, -1, -1
        for i in idxs:
            if lock[i]:
                continue
            d = hamming(mp_desc[m], desc[i])
            if d < best:
                best2, bl2 = best, bl
                best, bl, bi = d, int(keys[i]["octave"]), i
            elif d < best2:
                best2, bl2 = d, int(keys[i]["octave"])
        if best <= 100:
            if bl == bl2 and f32(best) > f32(f32(nnratio) * f32(best2)):
                continue
            km[bi] = m
            if mp["has_obs"]:
                lock[bi] = True
            n += 1
    return n, km


def frustum(mps, rcw, tcw, ow, cam, width, height, cos_limit, log_scale, n_levels):
    """Vectorised numpy restatement of Frame::isInFrustum + MapPoint::PredictScale
    (src/Frame.cc:303-366, src/MapPoint.cc:435-450) with the oracle's pinned
    arithmetic: float32 Pc / projection, float64 norm and dot.  log via numpy
    float64 (the oracle pins fdlibm's scheme; both agree after rounding to float)."""
    f32 = np.float32
    fx, fy, cx, cy, bf, _ = (f32(c) for c in cam)
    R = np.asarray(rcw, f32).reshape(3, 3)
    t = np.asarray(tcw, f32)
    P = mps["pos"].astype(f32)
    pc = [((R[i, 0] * P[:, 0] + R[i, 1] * P[:, 1]) + R[i, 2] * P[:, 2]) + t[i] for i in range(3)]
    X, Y, Z = pc
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invz = f32(1.0) / Z
        u = fx * X * invz + cx
        v = fy * Y * invz + cy
        O = P - np.asarray(ow, f32)
        dist = np.sqrt(((O[:, 0].astype(np.float64) ** 2) + O[:, 1].astype(np.float64) ** 2)
                       + O[:, 2].astype(np.float64) ** 2).astype(f32)
        N = mps["normal"].astype(np.float64)
        dot = ((O[:, 0] * N[:, 0]) + O[:, 1] * N[:, 1]) + O[:, 2] * N[:, 2]
        view_cos = (dot / dist.astype(np.float64)).astype(f32)
        maxd = f32(1.2) * mps["max_distance"]
        mind = f32(0.8) * mps["min_distance"]
        ok = (mps["seen"] == 0) & (mps["bad"] == 0) & ~(Z < 0)
        ok &= ~((u < 0) | (u > f32(width)) | (v < 0) | (v > f32(height)))
        ok &= ~((dist < mind) | (dist > maxd))
        ok &= ~(view_cos < f32(cos_limit))
        ratio = mps["max_distance"] / dist
        lr = np.log(ratio.astype(np.float64)).astype(f32)
        q = np.ceil(lr / f32(log_scale))
        level = np.where(q < 0, 0, np.where(q >= n_levels, n_levels - 1,
                                            np.nan_to_num(q).astype(np.int64)))
    return ok, u, v, u - bf * invz, view_cos, level


def _rot_bin(a1, a2):
    # ORBmatcher's histogram bin with factor 1/HISTO_LENGTH (src/ORBmatcher.cc:516-524)
    rot = f32(f32(a1) - f32(a2))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    v = f32(rot * f32(f32(1.0) / f32(30)))
    b = int(math.floor(float(v) + 0.5))
    return 0 if b == 30 else b


def _three_maxima(counts, ge=False):
    """ComputeThreeMaxima (src/ORBmatcher.cc:1761-1807).  `ge` switches the scan's
    strict `s > max` to the wrong neighbour `s >= max` (sensitivity tests only)."""
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    over = (lambda s, m: s >= m) if ge else (lambda s, m: s > m)
    for i, s in enumerate(counts):
        if over(s, m1):
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
        elif over(s, m2):
            m3, m2, i3, i2 = m2, s, i2, i
        elif over(s, m3):
            m3, i3 = s, i
    if m2 < f32(0.1) * f32(m1):
        i2 = i3 = -1
    elif m3 < f32(0.1) * f32(m1):
        i3 = -1
    return i1, i2, i3


def search_for_initialization(keys1, desc1, keys2, desc2, width, height, prev, window,
                              nnratio, check_ori, rules=(), trace=None):
    """Independent restatement of ORBmatcher::SearchForInitialization
    (src/ORBmatcher.cc:429-577) in plain Python.

    `rules` names wrong neighbours of the reference's rules (sensitivity tests
    only): mdist_lt (skip on vMatchedDistance < d), th_lt (best < 50), ratio_le
    (best <= second * nnratio), window_le (|dx| <= r), tie_last (the last
    minimum in scan order), no_stolen_vote (a stolen query's histogram entry
    goes with its match), no_level_f1 / no_level_f2 (the level filter dropped).
    `trace`, a list, receives one dict per level-0 query in processing order:
    i1, cand [(i2, distance) in scan order], mdist (vMatchedDistance of each
    candidate when the query is processed), b1, b2, bi, accept, stole (the
    previous owner or -1)."""
    cells, invW, invH = grid_cells(keys2, width, height)
    prev = np.array(prev, np.float32).reshape(len(keys1), 2).copy()
    m12 = np.full(len(keys1), -1, np.int32)
    mdist = [1 << 31] * len(keys2)
    m21 = [-1] * len(keys2)
    hist = [[] for _ in range(30)]
    n = 0
    lvl2 = (-1, -1) if "no_level_f2" in rules else (0, 0)
    for i1 in range(len(keys1)):
        if keys1[i1]["octave"] > 0 and "no_level_f1" not in rules:
            continue
        idx = features_in_area(keys2, cells, invW, invH, prev[i1, 0], prev[i1, 1], window,
                               lvl2[0], lvl2[1], closed="window_le" in rules)
        t = dict(i1=i1, cand=[], mdist=[], b1=1 << 31, b2=1 << 31, bi=-1, accept=False, stole=-1)
        if trace is not None:
            trace.append(t)
        if not idx:
            continue
        b1, b2, bi = 1 << 31, 1 << 31, -1
        for i2 in idx:
            d = hamming(desc1[i1], desc2[i2])
            t["cand"].append((i2, d))
            t["mdist"].append(mdist[i2])
            if (mdist[i2] < d) if "mdist_lt" in rules else (mdist[i2] <= d):
                continue
            if d < b1 or ("tie_last" in rules and d == b1):
                b2, b1, bi = b1, d, i2
            elif d < b2:
                b2 = d
        t.update(b1=b1, b2=b2, bi=bi)
        low = b1 < 50 if "th_lt" in rules else b1 <= 50
        lim = f32(f32(b2) * f32(nnratio))
        if low and (f32(b1) <= lim if "ratio_le" in rules else f32(b1) < lim):
            if m21[bi] >= 0:
                t["stole"] = m21[bi]
                m12[m21[bi]] = -1
                n -= 1
                if "no_stolen_vote" in rules:
                    for h in hist:
                        if m21[bi] in h:
                            h.remove(m21[bi])
            m12[i1], m21[bi], mdist[bi] = bi, i1, b1
            t["accept"] = True
            n += 1
            if check_ori:
                hist[_rot_bin(keys1[i1]["angle"], keys2[bi]["angle"])].append(i1)
    if check_ori:
        keep = _three_maxima([len(h) for h in hist])
        for b in range(30):
            if b in keep:
                continue
            for i1 in hist[b]:
                if m12[i1] >= 0:
                    m12[i1] = -1
                    n -= 1
    for i1 in range(len(keys1)):
        if m12[i1] >= 0:
            prev[i1] = (keys2[m12[i1]]["x"], keys2[m12[i1]]["y"])
    return n, m12, prev


def distinctive_descriptor(desc, rules=()):
    """MapPoint::ComputeDistinctiveDescriptors' BestIdx (src/MapPoint.cc:285-318).
    `rules` (sensitivity tests only): median_upper (index n / 2 for
    (n - 1) / 2), best_le (the last row with the smallest median)."""
    n = len(desc)
    if n == 0:
        return -1
    bits = np.unpackbits(desc, axis=1).astype(np.int32)
    D = (bits[:, None, :] != bits[None, :, :]).sum(-1)
    k = n // 2 if "median_upper" in rules else int(0.5 * (n - 1))
    best, bi = 1 << 31, 0
    for i in range(n):
        med = int(np.sort(D[i])[k])
        if med <= best if "best_le" in rules else med < best:
            best, bi = med, i
    return bi


# ------------------------------------------- §8(f) ORBmatcher variants (scalar)
def _xf(R, t, P):
    R = np.asarray(R, np.float32).reshape(3, 3)
    return [f32(f32(f32(R[r, 0] * f32(P[0])) + f32(R[r, 1] * f32(P[1]))) + f32(R[r, 2] * f32(P[2])))
            + f32(t[r]) for r in range(3)]


def _norm(a):
    return f32(math.sqrt(sum(float(x) * float(x) for x in a)))


def _dotd(a, b):
    return sum(float(x) * float(y) for x, y in zip(a, b))


def _level(maxd, dist, log_scale, n_levels):
    ratio = f32(f32(maxd) / f32(dist))
    q = np.ceil(f32(f32(math.log(float(ratio))) / f32(log_scale)))
    return 0 if q < 0 else (n_levels - 1 if q >= n_levels else int(q))


def _sim3_pose(S):
    S = np.asarray(S, np.float32).reshape(3, 4)
    scw = f32(math.sqrt(sum(float(S[0, k]) ** 2 for k in range(3))))
    inv = 1.0 / float(scw)
    R = np.array([[f32(float(S[r, c]) * inv) for c in range(3)] for r in range(3)], np.float32)
    t = np.array([f32(float(S[r, 3]) * inv) for r in range(3)], np.float32)
    ow = np.array([-(f32(f32(R[0, i] * t[0]) + f32(R[1, i] * t[1])) + f32(R[2, i] * t[2]))
                   for i in range(3)], np.float32)
    return R, t, ow


# Rule switches (sensitivity tests only).  Every restatement below takes
# `rules`, a collection of names of WRONG neighbours of a reference rule; the
# default, no names, is the reference.
#   th_strict  the distance threshold's <= becomes < (or < becomes <=)
#   tie_flip   first minimum becomes last minimum on ties (or last becomes first)
#   top4       a point whose TOPK nearest candidates are all locked gets no match
#   stereo_flip  u_right >= 0 becomes > 0 (or > 0 becomes >= 0)
#   bounds_flip  half-open image bounds become closed (or closed become half-open)
#   hist_ge    ComputeThreeMaxima scans with s >= max
#   no_claims  claims inside a vocabulary node are ignored
TOPK = 4  # matcher_common.h TOPK: candidates the device keeps per point


def _in_kf(x, y, w, h, closed=False):
    if closed:
        return 0 <= x <= w and 0 <= y <= h
    return 0 <= x < w and 0 <= y < h


def _out_frame(u, v, w, h, half_open=False):
    if half_open:
        return u < 0 or u >= w or v < 0 or v >= h
    return u < 0 or u > w or v < 0 or v > h


def _best(keys, desc, cells, invW, invH, dq, u, v, r, lo, hi, skip=None, gate=None,
          check_levels=False, init=256, rules=()):
    """GetFeaturesInArea + first-minimum scan; the level filter is either the
    function's (check_levels) or the loop's (kpLevel < lo || > hi)."""
    idx = features_in_area(keys, cells, invW, invH, u, v, r, lo if check_levels else -1,
                           hi if check_levels else -1)
    bd, bi = init, -1
    cands = []
    for j in idx:
        o = int(keys[j]["octave"])
        if not check_levels and (o < lo or o > hi):
            continue
        if gate is not None and not gate(j):
            continue
        d = hamming(dq, desc[j])
        cands.append((d, len(cands), j))
        if skip is not None and skip(j):
            continue
        if d < bd or ("tie_flip" in rules and d == bd and bi >= 0):
            bd, bi = d, j
    if "top4" in rules and skip is not None and len(cands) > TOPK and \
            all(skip(j) for _, _, j in sorted(cands)[:TOPK]):
        return init, -1
    return bd, bi


def search_by_projection_sim3(keys, desc, scale, width, height, S, cam, mps, mp_desc, th,
                              kp_matched, log_scale, n_levels=8, rules=()):
    fx, fy, cx, cy = (f32(c) for c in cam[:4])
    cells, invW, invH = grid_cells(keys, width, height)
    R, t, ow = _sim3_pose(S)
    km = np.array(kp_matched, np.int32).copy()
    n = 0
    for i, mp in enumerate(mps):
        if mp["bad"] or mp["seen"]:
            continue
        Pc = _xf(R, t, mp["pos"])
        if Pc[2] < 0:
            continue
        invz = f32(f32(1) / Pc[2])
        u = f32(f32(fx * f32(Pc[0] * invz)) + cx)
        v = f32(f32(fy * f32(Pc[1] * invz)) + cy)
        if not _in_kf(u, v, width, height, "bounds_flip" in rules):
            continue
        PO = [f32(f32(mp["pos"][k]) - ow[k]) for k in range(3)]
        dist = _norm(PO)
        if dist < f32(f32(0.8) * mp["min_distance"]) or dist > f32(f32(1.2) * mp["max_distance"]):
            continue
        if _dotd(PO, mp["normal"]) < 0.5 * float(dist):
            continue
        lvl = _level(mp["max_distance"], dist, log_scale, n_levels)
        bd, bi = _best(keys, desc, cells, invW, invH, mp_desc[i], u, v,
                       f32(f32(th) * f32(scale[lvl])), lvl - 1, lvl, skip=lambda j: km[j] >= 0,
                       rules=rules)
        if bd < 50 or (bd == 50 and "th_strict" not in rules):
            km[bi] = i
            n += 1
    return n, km


def fuse(keys, desc, scale, inv_sigma2, width, height, u_right, R, t, ow, cam, mps, mp_desc, th,
         log_scale, n_levels=8, rules=()):
    fx, fy, cx, cy, bf = (f32(c) for c in cam[:5])
    cells, invW, invH = grid_cells(keys, width, height)
    best = np.full(len(mps), -1, np.int32)
    n = 0
    for i, mp in enumerate(mps):
        if mp["bad"] or mp["seen"]:
            continue
        Pc = _xf(R, t, mp["pos"])
        if Pc[2] < 0:
            continue
        invz = f32(f32(1) / Pc[2])
        u = f32(f32(fx * f32(Pc[0] * invz)) + cx)
        v = f32(f32(fy * f32(Pc[1] * invz)) + cy)
        if not _in_kf(u, v, width, height, "bounds_flip" in rules):
            continue
        ur = f32(u - f32(bf * invz))
        PO = [f32(f32(mp["pos"][k]) - f32(ow[k])) for k in range(3)]
        dist = _norm(PO)
        if dist < f32(f32(0.8) * mp["min_distance"]) or dist > f32(f32(1.2) * mp["max_distance"]):
            continue
        if _dotd(PO, mp["normal"]) < 0.5 * float(dist):
            continue
        lvl = _level(mp["max_distance"], dist, log_scale, n_levels)

        def gate(j):
            k = keys[j]
            ex, ey = f32(u - f32(k["x"])), f32(v - f32(k["y"]))
            e2 = f32(f32(ex * ex) + f32(ey * ey))
            if u_right[j] > 0 or (u_right[j] == 0 and "stereo_flip" not in rules):
                er = f32(ur - f32(u_right[j]))
                return float(f32(f32(e2 + f32(er * er)) * f32(inv_sigma2[k["octave"]]))) <= 7.8
            return float(f32(e2 * f32(inv_sigma2[k["octave"]]))) <= 5.99

        bd, bi = _best(keys, desc, cells, invW, invH, mp_desc[i], u, v,
                       f32(f32(th) * f32(scale[lvl])), lvl - 1, lvl, gate=gate, rules=rules)
        if bd < 50 or (bd == 50 and "th_strict" not in rules):
            best[i] = bi
            n += 1
    return n, best


def search_by_sim3(kf1, kf2, cam, s12, R12, t12, th, log_scale, n_levels=8, rules=()):
    fx, fy, cx, cy = (f32(c) for c in cam[:4])
    R12 = np.asarray(R12, np.float32).reshape(3, 3)
    sR12 = np.array([[f32(float(s12) * float(R12[r, c])) for c in range(3)] for r in range(3)])
    sR21 = np.array([[f32((1.0 / float(s12)) * float(R12[c, r])) for c in range(3)]
                     for r in range(3)])
    t21 = np.array([-(f32(f32(sR21[r, 0] * f32(t12[0])) + f32(sR21[r, 1] * f32(t12[1])))
                      + f32(sR21[r, 2] * f32(t12[2]))) for r in range(3)], np.float32)

    def direction(A, B, sR, tt):
        cells, invW, invH = grid_cells(B["keys"], B["width"], B["height"])
        out = np.full(len(A["keys"]), -1, np.int32)
        for i, mp in enumerate(A["mps"]):
            if not A["valid"][i] or A["already"][i] or mp["bad"]:
                continue
            Pb = _xf(sR, tt, _xf(A["Rw"], A["tw"], mp["pos"]))
            if Pb[2] < 0:
                continue
            invz = f32(1.0 / float(Pb[2]))
            u = f32(f32(fx * f32(Pb[0] * invz)) + cx)
            v = f32(f32(fy * f32(Pb[1] * invz)) + cy)
            if not _in_kf(u, v, B["width"], B["height"], "bounds_flip" in rules):
                continue
            dist = _norm(Pb)
            if dist < f32(f32(0.8) * mp["min_distance"]) or dist > f32(f32(1.2) * mp["max_distance"]):
                continue
            lvl = _level(mp["max_distance"], dist, log_scale, n_levels)
            bd, bi = _best(B["keys"], B["desc"], cells, invW, invH, A["mp_desc"][i], u, v,
                           f32(f32(th) * f32(B["scale"][lvl])), lvl - 1, lvl, init=1 << 31,
                           rules=rules)
            if bd < 100 or (bd == 100 and "th_strict" not in rules):
                out[i] = bi
        return out

    m1 = direction(kf1, kf2, sR21, t21)
    m2 = direction(kf2, kf1, sR12, np.asarray(t12, np.float32))
    m12 = np.array([j if j >= 0 and m2[j] == i else -1 for i, j in enumerate(m1)], np.int32)
    return int((m12 >= 0).sum()), m12


def search_by_bow_kf(d1, a1, mp1, bad1, fv1, d2, a2, mp2, bad2, fv2, nnratio, check_ori,
                     rules=()):
    m12 = np.full(len(d1), -1, np.int32)
    matched2 = np.zeros(len(d2), bool)
    hist = [[] for _ in range(30)]
    nodes2 = {int(fv2[0][k]): fv2[2][fv2[1][k]:fv2[1][k + 1]] for k in range(len(fv2[0]))}
    for k in range(len(fv1[0])):
        f2 = nodes2.get(int(fv1[0][k]))
        if f2 is None:
            continue
        for i1 in fv1[2][fv1[1][k]:fv1[1][k + 1]]:
            if mp1[i1] < 0 or bad1[i1]:
                continue
            b1, b2, bi = 256, 256, -1
            for i2 in f2:
                if (matched2[i2] and "no_claims" not in rules) or mp2[i2] < 0 or bad2[i2]:
                    continue
                d = hamming(d1[i1], d2[i2])
                if d < b1:
                    b2, b1, bi = b1, d, i2
                elif "tie_flip" in rules and d == b1:
                    b2, bi = d, i2
                elif d < b2:
                    b2 = d
            if (b1 < 50 or (b1 == 50 and "th_strict" in rules)) and \
                    f32(b1) < f32(f32(nnratio) * f32(b2)):
                m12[i1] = mp2[bi]
                matched2[bi] = True
                if check_ori:
                    hist[_rot_bin(a1[i1], a2[bi])].append(i1)
    if check_ori:
        keep = _three_maxima([len(h) for h in hist], "hist_ge" in rules)
        for b in range(30):
            if b not in keep:
                for i1 in hist[b]:
                    m12[i1] = -1
    return int((m12 >= 0).sum()), m12


def search_by_projection_reloc(keys, desc, scale, width, height, R, t, ow, cam, mps, mp_desc,
                               kf_angle, th, orb_dist, check_ori, kp_locked, log_scale,
                               n_levels=8, rules=()):
    fx, fy, cx, cy = (f32(c) for c in cam[:4])
    cells, invW, invH = grid_cells(keys, width, height)
    lock = np.asarray(kp_locked, bool).copy()
    km = np.full(len(keys), -1, np.int32)
    hist = [[] for _ in range(30)]
    for i, mp in enumerate(mps):
        if mp["bad"] or mp["seen"]:
            continue
        Pc = _xf(R, t, mp["pos"])
        invz = f32(1.0 / float(Pc[2]))
        u = f32(f32(f32(fx * Pc[0]) * invz) + cx)
        v = f32(f32(f32(fy * Pc[1]) * invz) + cy)
        if _out_frame(u, v, width, height, "bounds_flip" in rules):
            continue
        PO = [f32(f32(mp["pos"][k]) - f32(ow[k])) for k in range(3)]
        dist = _norm(PO)
        if dist < f32(f32(0.8) * mp["min_distance"]) or dist > f32(f32(1.2) * mp["max_distance"]):
            continue
        lvl = _level(mp["max_distance"], dist, log_scale, n_levels)
        bd, bi = _best(keys, desc, cells, invW, invH, mp_desc[i], u, v,
                       f32(f32(th) * f32(scale[lvl])), lvl - 1, lvl + 1, skip=lambda j: lock[j],
                       check_levels=True, rules=rules)
        if bd < orb_dist or (bd == orb_dist and "th_strict" not in rules):
            lock[bi] = True
            km[bi] = i
            if check_ori:
                hist[_rot_bin(kf_angle[i], keys[bi]["angle"])].append(bi)
    if check_ori:
        keep = _three_maxima([len(h) for h in hist], "hist_ge" in rules)
        for b in range(30):
            if b not in keep:
                for j in hist[b]:
                    km[j] = -2
    return int((km >= 0).sum()), km


def search_for_triangulation(kf1, kf2, level_sigma2, F12, cam, Cw, R2w, t2w, fv1, fv2,
                             only_stereo, check_ori, rules=()):
    fx, fy, cx, cy = (f32(c) for c in cam[:4])
    stereo = (lambda ur: ur > 0) if "stereo_flip" in rules else (lambda ur: ur >= 0)
    F = np.asarray(F12, np.float32).reshape(3, 3)
    C2 = _xf(R2w, t2w, Cw)
    invz = f32(f32(1) / C2[2])
    ex = f32(f32(f32(fx * C2[0]) * invz) + cx)
    ey = f32(f32(f32(fy * C2[1]) * invz) + cy)
    k1s, k2s = kf1["keys"], kf2["keys"]
    m12 = np.full(len(k1s), -1, np.int32)
    hist = [[] for _ in range(30)]
    nodes2 = {int(fv2[0][k]): fv2[2][fv2[1][k]:fv2[1][k + 1]] for k in range(len(fv2[0]))}
    for k in range(len(fv1[0])):
        f2 = nodes2.get(int(fv1[0][k]))
        if f2 is None:
            continue
        for i1 in fv1[2][fv1[1][k]:fv1[1][k + 1]]:
            if kf1["has_mp"][i1]:
                continue
            st1 = stereo(kf1["u_right"][i1])
            if only_stereo and not st1:
                continue
            kp1 = k1s[i1]
            a = f32(f32(f32(kp1["x"] * F[0, 0]) + f32(kp1["y"] * F[1, 0])) + F[2, 0])
            b = f32(f32(f32(kp1["x"] * F[0, 1]) + f32(kp1["y"] * F[1, 1])) + F[2, 1])
            c = f32(f32(f32(kp1["x"] * F[0, 2]) + f32(kp1["y"] * F[1, 2])) + F[2, 2])
            bd, bi = 50, -1
            for i2 in f2:
                if kf2["has_mp"][i2]:
                    continue
                st2 = stereo(kf2["u_right"][i2])
                if only_stereo and not st2:
                    continue
                d = hamming(kf1["desc"][i1], kf2["desc"][i2])
                if d > 50 or d > bd:
                    continue
                if d == 50 and "th_strict" in rules:
                    continue
                if d == bd and bi >= 0 and "tie_flip" in rules:
                    continue
                kp2 = k2s[i2]
                if not st1 and not st2:
                    dx, dy = f32(ex - kp2["x"]), f32(ey - kp2["y"])
                    if f32(f32(dx * dx) + f32(dy * dy)) < f32(100 * kf2["scale"][kp2["octave"]]):
                        continue
                num = f32(f32(f32(a * kp2["x"]) + f32(b * kp2["y"])) + c)
                den = f32(f32(a * a) + f32(b * b))
                if den == 0:
                    continue
                if float(f32(f32(num * num) / den)) < 3.84 * float(level_sigma2[kp2["octave"]]):
                    bd, bi = d, i2
            if bi >= 0:
                m12[i1] = bi
                if check_ori:
                    hist[_rot_bin(kp1["angle"], k2s[bi]["angle"])].append(i1)
    if check_ori:
        keep = _three_maxima([len(h) for h in hist], "hist_ge" in rules)
        for bb in range(30):
            if bb not in keep:
                for i1 in hist[bb]:
                    m12[i1] = -1
    return int((m12 >= 0).sum()), m12


def search_by_projection_frame(keys, desc, scale, width, height, last, last_desc, cam, tlc_z, th,
                               mono, check_ori, kp_locked=None, u_right=None, rules=()):
    """SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1460-1619).
    `last` rows carry xc, yc, invzc (x3Dc and 1/z), last_octave, last_angle, valid
    (pMP && !outlier), has_obs (Observations() > 0 of the point written into the
    current frame) and mp_id.  A keypoint may be written several times (points
    without observations do not lock it); every write is one nmatches++ and one
    histogram entry, and every entry of a rejected bin is one nmatches--.
    Returns (nmatches, kp_match): id written last, -1 untouched, -2 reset."""
    fx, fy, cx, cy, bf, mb = (f32(c) for c in cam)
    cells, invW, invH = grid_cells(keys, width, height)
    lock = np.zeros(len(keys), bool) if kp_locked is None else np.asarray(kp_locked, bool).copy()
    entry = lock.copy()
    held = [None] * len(keys)  # None untouched, id, or "null" after the filter
    fwd = f32(tlc_z) > mb and not mono
    bwd = -f32(tlc_z) > mb and not mono
    hist = [[] for _ in range(30)]
    n = 0
    for i, L in enumerate(last):
        if not L["valid"]:
            continue
        invzc = f32(L["invzc"])
        if invzc < 0:
            continue
        u = f32(f32(f32(fx * f32(L["xc"])) * invzc) + cx)
        v = f32(f32(f32(fy * f32(L["yc"])) * invzc) + cy)
        if _out_frame(u, v, width, height, "bounds_flip" in rules):
            continue
        o = int(L["last_octave"])
        r = f32(f32(th) * f32(scale[o]))
        if fwd:
            idx = features_in_area(keys, cells, invW, invH, u, v, r, o, -1)
        elif bwd:
            idx = features_in_area(keys, cells, invW, invH, u, v, r, 0, o)
        else:
            idx = features_in_area(keys, cells, invW, invH, u, v, r, o - 1, o + 1)
        bd, bi = 256, -1
        cands = []  # what a TOPK candidate list would hold: entry locks filtered out
        for j in idx:
            if entry[j]:
                continue
            if u_right is not None and (u_right[j] > 0 or
                                        (u_right[j] == 0 and "stereo_flip" in rules)):
                er = abs(f32(f32(u - f32(bf * invzc)) - f32(u_right[j])))
                if er > r:
                    continue
            d = hamming(last_desc[i], desc[j])
            cands.append((d, len(cands), j))
            if lock[j]:
                continue
            if d < bd or ("tie_flip" in rules and d == bd and bi >= 0):
                bd, bi = d, j
        if "top4" in rules and len(cands) > TOPK and all(lock[j] for _, _, j in
                                                          sorted(cands)[:TOPK]):
            continue
        if bd < 100 or (bd == 100 and "th_strict" not in rules):
            held[bi] = int(L["mp_id"])
            lock[bi] = bool(L["has_obs"])
            n += 1
            if check_ori:
                hist[_rot_bin(L["last_angle"], keys[bi]["angle"])].append(bi)
    if check_ori:
        keep = _three_maxima([len(h) for h in hist], "hist_ge" in rules)
        for b in range(30):
            if b not in keep:
                for j in hist[b]:
                    held[j] = "null"
                    n -= 1
    km = np.array([-1 if h is None else (-2 if h == "null" else h) for h in held], np.int32)
    return n, km.reshape(len(keys))


def search_by_bow(kf_desc, kf_angle, kf_mp, kf_bad, kf_fv, f_desc, f_angle, f_fv, nnratio,
                  check_ori, rules=()):
    """SearchByBoW(pKF, F, vpMapPointMatches) (src/ORBmatcher.cc:164-306): TH_LOW is
    `<=` here (`<` between KeyFrames), a Frame feature with a match is skipped by
    later KeyFrame features, the first minimum wins.  Returns (nmatches, f_match)."""
    fm = np.full(len(f_desc), -1, np.int32)
    taken = np.zeros(len(f_desc), bool)
    hist = [[] for _ in range(30)]
    n = 0
    nodes_f = {int(f_fv[0][k]): f_fv[2][f_fv[1][k]:f_fv[1][k + 1]] for k in range(len(f_fv[0]))}
    for k in range(len(kf_fv[0])):
        ff = nodes_f.get(int(kf_fv[0][k]))
        if ff is None:
            continue
        for ik in kf_fv[2][kf_fv[1][k]:kf_fv[1][k + 1]]:
            if kf_mp[ik] < 0 or (kf_bad is not None and kf_bad[ik]):
                continue
            b1, b2, bi = 256, 256, -1
            for jf in ff:
                if taken[jf] and "no_claims" not in rules:
                    continue
                d = hamming(kf_desc[ik], f_desc[jf])
                if d < b1:
                    b2, b1, bi = b1, d, jf
                elif "tie_flip" in rules and d == b1:
                    b2, bi = d, jf
                elif d < b2:
                    b2 = d
            if (b1 < 50 or (b1 == 50 and "th_strict" not in rules)) and \
                    f32(b1) < f32(f32(nnratio) * f32(b2)):
                fm[bi] = kf_mp[ik]
                taken[bi] = True
                n += 1
                if check_ori:
                    hist[_rot_bin(kf_angle[ik], f_angle[bi])].append(bi)
    if check_ori:
        keep = _three_maxima([len(h) for h in hist], "hist_ge" in rules)
        for b in range(30):
            if b not in keep:
                for j in hist[b]:
                    fm[j] = -1
                    n -= 1
    return n, fm


_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def vocab_transform(voc, desc, levelsup, scoring, weighting):
    """DBoW2 TemplatedVocabulary::transform (TemplatedVocabulary.h:1128-1283),
    written from the text a second time: children lists rebuilt from the
    parent table in file order, descent by a first-index argmin (strict '<'),
    BowVector / FeatureVector as dicts sorted at the end."""
    parent = np.asarray(voc["parent"])
    n_nodes = len(parent)
    children = [[] for _ in range(n_nodes)]
    for i in range(1, n_nodes):
        children[int(parent[i])].append(i)
    words = {}
    for i in range(1, n_nodes):
        if voc["leaf"][i]:
            words[i] = len(words)
    nd = np.asarray(voc["desc"], np.uint8)
    L = int(voc["L"])
    nid_level = L - levelsup
    bow, fv = {}, {}
    fword, fnode = [], []
    tf = weighting in (0, 1)
    if not words:
        return [], [], [], [0], [], [], []
    for i, f in enumerate(np.asarray(desc, np.uint8).reshape(-1, 32)):
        node, level, nid = 0, 0, 0
        nid_set = nid_level <= 0
        while True:
            level += 1
            ch = children[node]
            d = _POP8[np.bitwise_xor(nd[ch], f)].sum(axis=1)
            node = ch[int(np.argmin(d))]  # first minimum
            if level == nid_level:
                nid, nid_set = node, True
            if not children[node]:
                break
        if not nid_set:
            nid = node
        w = float(voc["weight"][node])
        wid = words.get(node, 0)
        fword.append(wid if w > 0 else 0xFFFFFFFF)
        fnode.append(nid)
        if w > 0:
            if tf:
                bow[wid] = bow[wid] + w if wid in bow else w
            elif wid not in bow:
                bow[wid] = w
            fv.setdefault(nid, []).append(i)
    keys = sorted(bow)
    vals = [bow[k] for k in keys]
    must = scoring != 5
    if tf and vals and not must:
        vals = [v / float(len(vals)) for v in vals]
    if must:
        norm = 0.0
        if scoring == 1:
            for v in vals:
                norm += v * v
            norm = math.sqrt(norm)
        else:
            for v in vals:
                norm += abs(v)
        if norm > 0.0:
            vals = [v / norm for v in vals]
    nodes = sorted(fv)
    offs = [0]
    feats = []
    for k in nodes:
        feats.extend(fv[k])
        offs.append(len(feats))
    return keys, vals, nodes, offs, feats, fword, fnode


def undistort_points(xy, K, dist):
    """cvUndistortPoints (OpenCV, as Frame::UndistortKeyPoints calls it with
    P = mK, src/Frame.cc:468), restated a second time with Python floats
    (IEEE doubles, no fused multiply-add): widen, 5 fixed-point iterations,
    map through RR = K, narrow to float32."""
    K = [float(np.float32(v)) for v in np.asarray(K, np.float32).reshape(9)]
    k = [float(np.float32(v)) for v in np.asarray(dist, np.float32).reshape(-1)]
    k = k + [0.0] * (12 - len(k))
    fx, fy, cx, cy = K[0], K[4], K[2], K[5]
    ifx, ify = 1.0 / fx, 1.0 / fy
    out = np.zeros((len(xy), 2), np.float32)
    for i, (u, v) in enumerate(np.asarray(xy, np.float32).reshape(-1, 2)):
        x = (float(u) - cx) * ifx
        y = (float(v) - cy) * ify
        x0, y0 = x, y
        for _ in range(5):
            r2 = x * x + y * y
            icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / \
                (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
            dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
            x = (x0 - dx) * icdist
            y = (y0 - dy) * icdist
        xx = K[0] * x + K[1] * y + K[2]
        yy = K[3] * x + K[4] * y + K[5]
        ww = 1.0 / (K[6] * x + K[7] * y + K[8])
        out[i] = (np.float32(xx * ww), np.float32(yy * ww))
    return out


# ------------------------------------------- Frame::ComputeStereoMatches (a11)
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _roundf(x, even=False):
    """roundf on a float32: half away from zero (np.rint, half to even, is the
    wrong neighbour `round_even`)."""
    x = np.float32(x)
    if even:
        return np.float32(np.rint(x))
    return np.float32(math.copysign(math.floor(abs(float(x)) + 0.5), float(x)))


def stereo_match(lkeys, ldesc, scale, rkeys, rdesc, lpyr, rpyr, inv_scale, bf, fx, width, height,
                 rules=(), trace=None):
    """Frame::ComputeStereoMatches, src/Frame.cc:516-704, restated: (u_right,
    depth, sad).  sad = the best SAD of every match accepted at :676-686,
    whether or not the median prune of :690-703 then resets it, -1 elsewhere.
    Float arithmetic is np.float32 wherever the reference computes in float.

    rules: the wrong neighbours of the reference's rules (test_stereo_edge_cases
    lists which input separates which).  trace: a dict that receives, per left
    keypoint and for the prune, what the census functions count."""
    F = np.float32
    rules = set(rules)
    N, NR = len(lkeys), len(rkeys)
    ur, dp, sad = np.full(N, -1, F), np.full(N, -1, F), np.full(N, -1, np.int32)
    scale, inv = np.asarray(scale, F), np.asarray(inv_scale, F)
    ldesc = np.asarray(ldesc, np.uint8).reshape(N, 32)
    rdesc = np.asarray(rdesc, np.uint8).reshape(NR, 32)
    nrows = lpyr[0].shape[0]
    even = "round_even" in rules
    # :531-544, vRowIndices
    rows = [[] for _ in range(nrows)]
    bands = []
    for iR in range(NR):
        y = F(rkeys["y"][iR])
        r = F(2.0) * scale[int(rkeys["octave"][iR])]
        if "band_round" in rules:
            lo, hi = int(_roundf(y - r)), int(_roundf(y + r))
        else:
            lo, hi = int(math.floor(y - r)), int(math.ceil(y + r))
        bands.append((lo, hi))
        for yi in range(lo, hi + 1):
            rows[yi].append(iR)
    mb = F(bf) / F(fx)
    minD, maxD = F(0), F(bf) / mb
    rx, roct = rkeys["x"].astype(F), rkeys["octave"].astype(np.int64)
    accepted = []
    kps = []
    for iL in range(N):
        t = dict(stage="none")
        kps.append(t)
        lvl = int(lkeys["octave"][iL])
        uL, vL = F(lkeys["x"][iL]), F(lkeys["y"][iL])
        row = int(_roundf(vL)) if "row_round" in rules else int(vL)   # float -> size_t
        cand = np.asarray(rows[row] if row < nrows else [], np.int64)
        t["row_len"] = len(cand)
        if len(cand) == 0:
            continue
        minU, maxU = uL - maxD, uL - minD
        if maxU < 0:
            continue
        dlim = 2 if "octave_pm2" in rules else 1
        octd = roct[cand] - lvl
        t["oct_delta"] = sorted(set(int(v) for v in octd))
        uR = rx[cand]
        lo_ok = (uR > minU) if "minu_strict" in rules else (uR >= minU)
        hi_ok = (uR < maxU) if "maxu_strict" in rules else (uR <= maxU)
        inoct = np.abs(octd) <= 1
        t["ur_eq_minu"] = int((inoct & (uR == minU)).sum())
        t["ur_eq_maxu"] = int((inoct & (uR == maxU)).sum())
        t["ur_below_minu"] = int((inoct & (uR == np.nextafter(minU, F(-np.inf)))).sum())
        t["ur_above_maxu"] = int((inoct & (uR == np.nextafter(maxU, F(np.inf)))).sum())
        ok = (np.abs(octd) <= dlim) & lo_ok & hi_ok
        c = cand[ok]
        t["n_pass"] = len(c)
        if len(c) == 0:
            continue
        d = _POP8[np.bitwise_xor(rdesc[c], ldesc[iL][None, :])].sum(axis=1)
        best = int(d.min())
        where = np.nonzero(d == best)[0]
        k = int(where[-1] if "tie_last" in rules else where[0])   # strict <: the first minimum
        t.update(best_dist=best, n_tied=len(where), best_pos=int(np.nonzero(ok)[0][k]),
                 best_idx=int(c[k]), best_oct_delta=int(roct[c[k]] - lvl))
        if not (best < 75 or ("hamming_le" in rules and best <= 75)) or best >= 100:
            continue
        t["stage"] = "descriptor"
        uR0 = rx[c[k]]
        sf = inv[lvl]
        suL, svL, suR0 = _roundf(uL * sf, even), _roundf(vL * sf, even), _roundf(uR0 * sf, even)
        half = lambda v: abs(float(v) - math.trunc(float(v))) == 0.5
        t["halves"] = int(half(uL * sf)) + int(half(vL * sf)) + int(half(uR0 * sf))
        IL, IR = lpyr[lvl], rpyr[lvl]
        cols = IR.shape[1]
        w, L = 5, 5
        iniu, endu = suR0 + F(L) - F(w), suR0 + F(L) + F(w) + F(1)
        t.update(level=lvl, endu=float(endu), cols=cols, sx=float(suR0))
        if iniu < 0 or (endu > cols if "endu_gt" in rules else endu >= cols):
            t["stage"] = "border"
            continue
        x0, y0, xr = int(suL) - w, int(svL) - w, int(suR0) - L - w
        assert x0 >= 0 and y0 >= 0 and xr >= 0, "outside the defined domain"
        assert y0 + 11 <= IL.shape[0] and x0 + 11 <= IL.shape[1] and xr + 21 <= cols
        pl = IL[y0:y0 + 11, x0:x0 + 11].astype(np.int64)
        pl = pl - pl[w, w]
        strip = IR[y0:y0 + 11, xr:xr + 21].astype(np.int64)
        dists = []
        for s in range(2 * L + 1):
            pr = strip[:, s:s + 11] - strip[w, s + w]
            dists.append(int(np.abs(pl - pr).sum()))
        t["sads"] = list(dists)
        if "sad_s16" in rules:   # the odd shifts ride in the high half of a packed word
            dists = [v - 65536 if (s & 1) and v >= 32768 else v for s, v in enumerate(dists)]
        best_sad, inc = 2147483647, 0
        for s, v in enumerate(dists):
            if F(v) < F(best_sad) or ("sad_first_vs_last" in rules and F(v) <= F(best_sad)):
                best_sad, inc = v, s - L
        t.update(best_sad=best_sad, inc=inc, sad_ties=sum(v == best_sad for v in dists))
        if inc in (-L, L):
            if "edge_inc_kept" not in rules:
                t["stage"] = "edge_inc"
                continue
            delta = F(0)
        else:
            d1, d2, d3 = F(dists[L + inc - 1]), F(dists[L + inc]), F(dists[L + inc + 1])
            with np.errstate(all="ignore"):
                delta = (d1 - d3) / (F(2.0) * (d1 + d3 - F(2.0) * d2))
        t["delta"] = float(delta)
        if delta < -1 or delta > 1:
            t["stage"] = "delta"
            continue
        best_ur = scale[lvl] * ((suR0 + F(inc)) + delta)
        disp = uL - best_ur
        t["disparity"] = float(disp)
        t["maxd"] = float(maxD)
        if not (disp >= minD and (disp < maxD or ("maxd_le" in rules and disp <= maxD))):
            t["stage"] = "disparity"
            continue
        if disp <= 0 and "no_zero_disp_branch" not in rules:
            disp = F(0.01)
            best_ur = F(np.float64(uL) - 0.01)
            t["zero_branch"] = True
        with np.errstate(all="ignore"):
            dp[iL] = F(bf) / disp
        ur[iL] = best_ur
        sad[iL] = best_sad
        accepted.append((best_sad, iL))
        t["stage"] = "accepted"
    prune = dict(V=len(accepted))
    if accepted:   # the reference indexes an empty vector otherwise (undefined)
        accepted.sort()
        V = len(accepted)
        median = F(accepted[(V - 1) // 2 if "median_lower" in rules else V // 2][0])
        th = F(1.5) * F(1.4) * median
        n_reset = 0
        for s, iL in reversed(accepted):
            if F(s) < th or ("prune_le" in rules and F(s) <= th):
                break
            ur[iL] = dp[iL] = F(-1)
            kps[iL]["stage"] = "pruned"
            n_reset += 1
        prune.update(median=float(median), th=float(th), reset=n_reset,
                     at_th=sum(float(s) == float(th) for s, _ in accepted))
    if trace is not None:
        trace.update(kp=kps, bands=bands, prune=prune, nrows=nrows)
    return ur, dp, sad
