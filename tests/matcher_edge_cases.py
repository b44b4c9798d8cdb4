"""Directed inputs for the ORBmatcher variant kernels (test infrastructure),
shared by the CPU tests (oracle against pyref, census, sensitivity) and the GPU
tests (kernels against the oracle).

The natural scenes of scenarios.py never reach most places where these kernels
branch: a vocabulary node with more than one 64-lane trip, a point whose TOPK
nearest candidates are all locked, a conflict and a slow lane in one 64-point
batch, equal distances in different trips, thresholds met exactly.  Every
generator here builds one such input and returns a `case`: a dict with
`family` (which variant it is for), the arguments of the call, and, where the
answer follows from the construction alone, `expect` (the output array).

Camera: fx = fy = 512, cx = 320, cy = 240, 640x480, identity pose and points
at depth 8, so a point meant for pixel (u, v) projects to exactly (u, v) in
float32 under every variant's arithmetic, and image bounds can be hit exactly.
Float equalities of the distance and chi-square gates are found by stepping
through neighbouring floats (np.nextafter) until pyref's pinned formula gives
the wanted side, and asserted here.

census_*: how often each target condition occurs in an input under the
reference's sequential order, written with pyref.grid_cells,
pyref.features_in_area and pyref.hamming only.
"""
import math

import numpy as np

import pyref

f32 = np.float32

TOPK = 4    # matcher_common.h TOPK: candidates kept per point by k_pp_match / k_frame_candidates
WAVE = 64   # wave width: points per speculative batch, lanes per vocabulary-node trip

W, H = 640, 480
FX = FY = 512.0
CX, CY = 320.0, 240.0
BF = 64.0
CAM = (FX, FY, CX, CY, BF, BF / FX)
Z = 8.0
N_LEVELS = 8
SCALE = np.ones(N_LEVELS, f32)
for _i in range(1, N_LEVELS):
    SCALE[_i] = f32(SCALE[_i - 1] * f32(1.2))
SIGMA2 = (SCALE * SCALE).astype(f32)
INV_SIGMA2 = (f32(1.0) / SIGMA2).astype(f32)
LS = f32(math.log(f32(1.2)))
EYE = np.eye(3, dtype=f32)
ZERO3 = np.zeros(3, f32)

KEYPOINT_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
     ("octave", "<i4"), ("class_id", "<i4")])
MAP_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"),
                            ("max_distance", "<f4"), ("bad", "u1"), ("seen", "u1"),
                            ("has_obs", "u1"), ("_pad", "u1")])
POSE_DTYPE = np.dtype([("rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("ow", "<f4", (3,))])
LAST_MP_DTYPE = np.dtype([("xc", "<f4"), ("yc", "<f4"), ("invzc", "<f4"), ("last_octave", "<i4"),
                          ("last_angle", "<f4"), ("valid", "u1"), ("has_obs", "u1"),
                          ("_pad", "u1", 2), ("mp_id", "<i4")])


def pose_record():
    rec = np.zeros(1, POSE_DTYPE)
    rec["rcw"] = EYE.reshape(1, 9)
    return rec


def scw(s=2.0):
    """Scw = [sR | st] with R = I, t = 0: normalised to the identity pose."""
    S = np.zeros((3, 4), f32)
    S[:, :3] = f32(s) * EYE
    return S


# ------------------------------------------------------------------ building blocks
def keypoints(x, y, octave=0, angle=0.0):
    k = np.zeros(len(x), KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"], k["angle"] = x, y, octave, angle
    k["size"] = 31.0 * SCALE[k["octave"]]
    k["response"], k["class_id"] = 50.0, -1
    return k


def flip_bits(desc, nbits, start=0):
    """`desc` with bits start..start+nbits-1 flipped: Hamming distance exactly nbits."""
    bits = np.unpackbits(np.asarray(desc, np.uint8).reshape(32))
    bits[start:start + nbits] ^= 1
    return np.packbits(bits)


def noisy(rng, base, p):
    bits = np.unpackbits(np.asarray(base, np.uint8), axis=-1)
    return np.packbits(bits ^ (rng.random(bits.shape) < p).astype(np.uint8), axis=-1)


def map_point(u, v, level=0, behind=False):
    """A MapPoint that the identity pose projects to exactly (u, v), with the
    scale-invariance range that predicts `level` and its normal along the
    viewing ray (cosine 1).  `behind`: mirrored through the centre, so Pc.z < 0
    and the projection is still (u, v)."""
    s = -1.0 if behind else 1.0
    pos = np.array([s * (u - CX) / FX * Z, s * (v - CY) / FY * Z, s * Z], f32)
    assert float(pos[0]) == s * (u - CX) / FX * Z and float(pos[1]) == s * (v - CY) / FY * Z
    mp = np.zeros(1, MAP_POINT_DTYPE)[0]
    dist = pyref._norm(pos)
    mp["pos"] = pos
    mp["normal"] = (pos.astype(np.float64) / float(dist)).astype(f32)
    mp["max_distance"] = f32(float(dist) * 1.2 ** level * 0.93)
    mp["min_distance"] = f32(mp["max_distance"] / f32(5.0))
    assert pyref._level(mp["max_distance"], dist, LS, N_LEVELS) == level
    return mp


class Scene:
    """Keypoints and MapPoints added one by one.  `lone` puts a point and its
    only candidate on a free site of a 40 px lattice (windows of radius up to
    12 px stay disjoint), with their descriptors a given distance apart."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.kx, self.ky, self.ko, self.ka, self.kd, self.kur = [], [], [], [], [], []
        self.mps, self.md, self.mang, self.tags = [], [], [], []
        self.pair = []   # per point: its intended keypoint (or -1)
        self.site = 0

    def kp(self, x, y, desc, octave=0, angle=0.0, u_right=-1.0):
        self.kx.append(x); self.ky.append(y); self.ko.append(octave); self.ka.append(angle)
        self.kd.append(np.asarray(desc, np.uint8)); self.kur.append(u_right)
        return len(self.kx) - 1

    def pt(self, mp, desc, kp=-1, angle=0.0, **tag):
        self.mps.append(mp); self.md.append(np.asarray(desc, np.uint8)); self.mang.append(angle)
        self.pair.append(kp); self.tags.append(tag)
        return len(self.mps) - 1

    def next_site(self):
        s = self.site
        self.site += 1
        assert s < 14 * 10
        return 40.0 + 40.0 * (s % 14), 40.0 + 40.0 * (s // 14)

    def lone(self, d=0, level=0, octave=None, at=None, kp_at=None, behind=False, angle=0.0,
             kp_angle=0.0, u_right=-1.0, edit=None, **tag):
        u, v = self.next_site() if at is None else at
        kx, ky = (u + 1.0, v) if kp_at is None else kp_at
        q = self.rng.integers(0, 256, 32, dtype=np.uint8)
        k = self.kp(kx, ky, flip_bits(q, d), level if octave is None else octave, kp_angle, u_right)
        mp = map_point(u, v, level, behind)
        if edit is not None:
            edit(mp)
        return self.pt(mp, q, k, angle, d=d, behind=behind, **tag)

    def frame(self):
        keys = keypoints(np.array(self.kx, f32), np.array(self.ky, f32), np.array(self.ko),
                         np.array(self.ka, f32))
        return keys, np.array(self.kd, np.uint8).reshape(-1, 32), np.array(self.kur, f32)

    def points(self):
        return (np.array(self.mps, MAP_POINT_DTYPE), np.array(self.md, np.uint8).reshape(-1, 32),
                np.array(self.mang, f32))


def _case(family, **kw):
    kw["family"] = family
    return kw


def reloc_case(keys, desc, mps, mp_desc, kf_angle, th=10.0, orb_dist=100, check_ori=False,
               locked=None, **extra):
    return _case("reloc", keys=keys, desc=desc, mps=mps, mp_desc=mp_desc, kf_angle=kf_angle,
                 th=th, orb_dist=orb_dist, check_ori=check_ori,
                 locked=np.zeros(len(keys), np.uint8) if locked is None else locked, **extra)


def sim3_case(keys, desc, mps, mp_desc, th=10.0, kp_matched=None, **extra):
    return _case("sim3", keys=keys, desc=desc, mps=mps, mp_desc=mp_desc, th=th,
                 kp_matched=np.full(len(keys), -1, np.int32) if kp_matched is None
                 else kp_matched, **extra)


def fuse_case(keys, desc, u_right, mps, mp_desc, th=3.0, **extra):
    return _case("fuse", keys=keys, desc=desc, u_right=u_right, mps=mps, mp_desc=mp_desc, th=th,
                 **extra)


def fuse_sim3_case(keys, desc, mps, mp_desc, th=4.0, **extra):
    return _case("fuse_sim3", keys=keys, desc=desc, mps=mps, mp_desc=mp_desc, th=th, **extra)


def frame_case(keys, desc, last, last_desc, th=10.0, tlc_z=0.0, mono=1, check_ori=False,
               locked=None, u_right=None, **extra):
    return _case("frame", keys=keys, desc=desc, last=last, last_desc=last_desc, th=th,
                 tlc_z=tlc_z, mono=mono, check_ori=check_ori,
                 locked=np.zeros(len(keys), np.uint8) if locked is None else locked,
                 u_right=u_right, **extra)


def last_points(u, v, octave, angle=0.0, has_obs=1, valid=1, behind=False):
    n = len(u)
    last = np.zeros(n, LAST_MP_DTYPE)
    last["xc"] = ((np.asarray(u, f32) - f32(CX)) / f32(FX) * f32(Z)).astype(f32)
    last["yc"] = ((np.asarray(v, f32) - f32(CY)) / f32(FY) * f32(Z)).astype(f32)
    last["invzc"] = np.where(behind, f32(-1.0 / Z), f32(1.0 / Z))
    last["last_octave"], last["last_angle"] = octave, angle
    last["valid"], last["has_obs"] = valid, has_obs
    last["mp_id"] = np.arange(n, dtype=np.int32) + 1000
    return last


# ------------------------------------------------------------------- A / C: crowded
CLUSTERS = ((120.0, 120.0), (320.0, 240.0), (500.0, 380.0))


def _crowd(seed, nkeys, n, bases=6, noise=0.02, side=60.0, clusters=CLUSTERS):
    """nkeys keypoints and n projections in 60x60 px clusters (quarter-pixel
    coordinates), descriptors = one of a few base descriptors with bit noise:
    windows hold tens of candidates at nearly equal distances."""
    rng = np.random.default_rng(seed)
    B = rng.integers(0, 256, (bases, 32), dtype=np.uint8)

    def place(m):
        c = np.array(clusters)[rng.integers(0, len(clusters), m)]
        xy = c + np.round(rng.uniform(-side / 2, side / 2, (m, 2)) * 4) / 4
        return xy[:, 0].astype(f32), xy[:, 1].astype(f32)

    kx, ky = place(nkeys)
    keys = keypoints(kx, ky, rng.integers(0, 3, nkeys), rng.choice([0.0, 30.0, 60.0, 200.0], nkeys))
    desc = noisy(rng, B[rng.integers(0, bases, nkeys)], noise)
    pu, pv = place(n)
    pdesc = noisy(rng, B[rng.integers(0, bases, n)], noise)
    return rng, keys, desc, pu, pv, pdesc


def _crowd_points(rng, pu, pv, level=1):
    mps = np.array([map_point(float(u), float(v), level) for u, v in zip(pu, pv)],
                   MAP_POINT_DTYPE).reshape(len(pu))
    mps["bad"] = rng.random(len(pu)) < 0.03
    mps["seen"] = rng.random(len(pu)) < 0.05
    return mps


def crowded_reloc(nkeys=600, n=400, seed=1, locked_frac=0.1, th=10.0, orb_dist=100,
                  check_ori=True, **crowd):
    """Census minimum: >= 10 slow points and >= 10 near-claims (at the default size)."""
    rng, keys, desc, pu, pv, pdesc = _crowd(seed, nkeys, n, **crowd)
    mps = _crowd_points(rng, pu, pv)
    lk = (rng.random(nkeys) < locked_frac).astype(np.uint8)
    ang = rng.choice([0.0, 30.0, 60.0, 90.0], n).astype(f32)
    win = [None if (m["bad"] or m["seen"]) else (float(u), float(v), f32(f32(th) * SCALE[1]), 0, 2)
           for m, u, v in zip(mps, pu, pv)]
    return reloc_case(keys, desc, mps, pdesc, ang, th, orb_dist, check_ori, lk, windows=win)


def crowded_sim3(nkeys=600, n=400, seed=2, matched_frac=0.1, th=10.0, **crowd):
    """Census minimum: >= 10 slow points and >= 10 near-claims (at the default size)."""
    rng, keys, desc, pu, pv, pdesc = _crowd(seed, nkeys, n, **crowd)
    mps = _crowd_points(rng, pu, pv)
    km = np.where(rng.random(nkeys) < matched_frac, rng.integers(0, max(n, 1), nkeys),
                  -1).astype(np.int32)
    win = [None if (m["bad"] or m["seen"]) else (float(u), float(v), f32(f32(th) * SCALE[1]), 0, 1)
           for m, u, v in zip(mps, pu, pv)]
    return sim3_case(keys, desc, mps, pdesc, th, km, windows=win)


def crowded_frame(nkeys=400, n=600, seed=3, locked_frac=0.1, th=10.0, check_ori=True,
                  obs_frac=0.5, stereo=False, tlc_z=0.0, **crowd):
    """has_obs half and half: points without observations share keypoints, a
    point with observations overwrites and locks.  Census minimum: >= 10 slow
    points, >= 10 near-claims, >= 10 keypoints written more than once and, with
    the rotation filter on, >= 10 keypoints that lose some but not all writers."""
    rng, keys, desc, pu, pv, pdesc = _crowd(seed, nkeys, n, **crowd)
    last = last_points(pu, pv, 1, rng.choice([0.0, 30.0, 60.0, 90.0], n),
                       rng.random(n) < obs_frac, rng.random(n) < 0.95)
    lk = (rng.random(nkeys) < locked_frac).astype(np.uint8)
    ur = None
    if stereo:  # u - bf / z = u - 8: within the radius for most, beyond it for some
        ur = np.where(rng.random(nkeys) < 0.6, keys["x"] - f32(8.0) + rng.choice(
            [0.0, 2.0, 11.5, 13.0], nkeys).astype(f32), -1).astype(f32)
    mono = 0 if stereo else 1
    fwd = tlc_z > CAM[5] and not mono
    bwd = -tlc_z > CAM[5] and not mono
    lo, hi = (1, -1) if fwd else ((0, 1) if bwd else (0, 2))
    win = [None if not L["valid"] else (float(u), float(v), f32(f32(th) * SCALE[1]), lo, hi)
           for L, u, v in zip(last, pu, pv)]
    return frame_case(keys, desc, last, pdesc, th, tlc_z, mono, check_ori, lk, ur, windows=win)


def crowded_fuse(nkeys=300, n=257, seed=8, sim3=False):
    """Fuse / FuseSim3 over crowded windows (no claims: every point independent);
    a third of the keypoints stereo with u_right near u - bf / z."""
    rng, keys, desc, _, _, _ = _crowd(seed, nkeys, n)
    src = rng.integers(0, nkeys, n)   # points within a pixel of a keypoint: inside the 5.99 gate
    step = np.array([-1.0, -0.5, 0.0, 0.5, 1.0], f32)
    pu, pv = keys["x"][src] + rng.choice(step, n), keys["y"][src] + rng.choice(step, n)
    pdesc = noisy(rng, desc[src], 0.02)
    mps = _crowd_points(rng, pu, pv)
    if sim3:
        return fuse_sim3_case(keys, desc, mps, pdesc, 4.0)
    ur = np.where(rng.random(nkeys) < 0.33, keys["x"] - f32(8.0) + rng.choice(
        [0.0, 1.0, 2.5], nkeys).astype(f32), -1).astype(f32)
    return fuse_case(keys, desc, ur, mps, pdesc, 3.0)


# ------------------------------------------------------------------- A / C: chain
def _chain(n_pts=130, n_keys=200):
    """n_pts points on one pixel with one descriptor, n_keys keypoints with the
    same descriptor inside their window: every distance ties, the scan order
    decides, and from the fifth point on the TOPK nearest are always locked."""
    rng = np.random.default_rng(7)
    D = rng.integers(0, 256, 32, dtype=np.uint8)
    ix = np.arange(n_keys)
    kx = (311.0 + (ix % 18)).astype(f32)   # |x - 320| <= 9 < 10
    ky = (232.0 + (ix // 18)).astype(f32)
    order = rng.permutation(n_keys)        # indices unrelated to the scan order
    keys = keypoints(kx[order], ky[order], 0, 0.0)
    desc = np.tile(D, (n_keys, 1))
    return keys, desc, np.tile(D, (n_pts, 1))


def chain_reloc(n_pts=130):
    """Census minimum: >= 100 slow points."""
    keys, desc, pd = _chain(n_pts)
    mps = np.array([map_point(320.0, 240.0, 0)] * n_pts, MAP_POINT_DTYPE)
    win = [(320.0, 240.0, f32(10.0), -1, 1)] * n_pts
    return reloc_case(keys, desc, mps, pd, np.zeros(n_pts, f32), windows=win)


def chain_sim3(n_pts=130):
    """Census minimum: >= 100 slow points."""
    keys, desc, pd = _chain(n_pts)
    mps = np.array([map_point(320.0, 240.0, 0)] * n_pts, MAP_POINT_DTYPE)
    win = [(320.0, 240.0, f32(10.0), -1, 0)] * n_pts
    return sim3_case(keys, desc, mps, pd, windows=win)


def chain_frame(n_pts=130):
    """Census minimum: >= 100 slow points (all points have observations)."""
    keys, desc, pd = _chain(n_pts)
    last = last_points(np.full(n_pts, 320.0), np.full(n_pts, 240.0), 0)
    win = [(320.0, 240.0, f32(10.0), -1, 1)] * n_pts
    return frame_case(keys, desc, last, pd, windows=win)


# ------------------------------------------------------------------- A / C: mixed
def _mixed(order):
    """Two groups far apart.  `c`: two points on one pixel with one descriptor
    and three keypoints there, so the second conflicts with the first inside a
    batch.  `s`: five such points over six keypoints, four at distance 0 and
    two further: the four claim in turn (each cutting the batch), the fifth
    finds its TOPK nearest locked and is slow.  order "cs": a conflict comes
    before the first slow lane of the batch; "sc": the slow lane comes first
    (and, after the cuts, at lane 0 of its batch)."""
    rng = np.random.default_rng(11)
    sc = Scene(11)
    groups = {}
    A = rng.integers(0, 256, 32, dtype=np.uint8)
    for dx, d in ((-2.0, 0), (0.0, 1), (3.0, 2)):
        sc.kp(100.0 + dx, 100.0, flip_bits(A, d))
    groups["c"] = [(100.0, 100.0, A)] * 2
    S = rng.integers(0, 256, 32, dtype=np.uint8)
    for dx, d in ((-4.0, 0), (-2.0, 0), (0.0, 0), (2.0, 0), (4.0, 3), (6.0, 5)):
        sc.kp(400.0 + dx, 300.0, flip_bits(S, d))
    groups["s"] = [(400.0, 300.0, S)] * 5
    pts = [p for g in order for p in groups[g]]
    keys, desc, _ = sc.frame()
    return keys, desc, pts


def mixed_reloc(order):
    keys, desc, pts = _mixed(order)
    mps = np.array([map_point(u, v, 0) for u, v, _ in pts], MAP_POINT_DTYPE)
    pd = np.array([d for _, _, d in pts], np.uint8)
    win = [(u, v, f32(10.0), -1, 1) for u, v, _ in pts]
    return reloc_case(keys, desc, mps, pd, np.zeros(len(pts), f32), windows=win)


def mixed_sim3(order):
    keys, desc, pts = _mixed(order)
    mps = np.array([map_point(u, v, 0) for u, v, _ in pts], MAP_POINT_DTYPE)
    pd = np.array([d for _, _, d in pts], np.uint8)
    win = [(u, v, f32(10.0), -1, 0) for u, v, _ in pts]
    return sim3_case(keys, desc, mps, pd, windows=win)


def mixed_frame(order):
    """"sc": the slow point ends up at lane 0 of its batch (inline rescan);
    "cs": at a later lane of the first batch it is seen in (batch cut)."""
    keys, desc, pts = _mixed(order)
    last = last_points([u for u, _, _ in pts], [v for _, v, _ in pts], 0)
    pd = np.array([d for _, _, d in pts], np.uint8)
    win = [(u, v, f32(10.0), -1, 1) for u, v, _ in pts]
    return frame_case(keys, desc, last, pd, windows=win)


def entry_slow(family):
    """A point whose TOPK nearest are locked on entry (no earlier point needed):
    slow at lane 1 of a batch with no conflict before it, then a conflict pair."""
    keys, desc, pts = _mixed("sc")
    pts = [pts[5], pts[0], pts[5], pts[6]]  # c, s, c, c
    mps = np.array([map_point(u, v, 0) for u, v, _ in pts], MAP_POINT_DTYPE)
    pd = np.array([d for _, _, d in pts], np.uint8)
    lk = np.zeros(len(keys), np.uint8)
    lk[3:7] = 1   # the four keypoints at distance 0 of group s
    if family == "reloc":
        win = [(u, v, f32(10.0), -1, 1) for u, v, _ in pts]
        return reloc_case(keys, desc, mps, pd, np.zeros(len(pts), f32), locked=lk, windows=win)
    win = [(u, v, f32(10.0), -1, 0) for u, v, _ in pts]
    return sim3_case(keys, desc, mps, pd, kp_matched=np.where(lk > 0, 77, -1).astype(np.int32),
                     windows=win)


# --------------------------------------------------------------- A / B: gates
def _search(x0, toward, want):
    """First float from x0 toward `toward` for which want(x) holds."""
    x = f32(x0)
    for _ in range(64):
        if want(x):
            return x
        x = np.nextafter(x, f32(toward))
    raise AssertionError("no float with the wanted property near %r" % x0)


def _dist_edits(mp0):
    """Edits of min_distance / max_distance that put dist exactly on the
    0.8f*min and 1.2f*max gates and one step to either side."""
    dist = pyref._norm(mp0["pos"])
    lo = lambda m: f32(f32(0.8) * f32(m))
    hi = lambda m: f32(f32(1.2) * f32(m))
    m_eq = _search(f32(float(dist) / 0.8 * (1 - 1e-6)), 1e9, lambda m: lo(m) >= dist)
    M_eq = _search(f32(float(dist) / 1.2 * (1 + 1e-6)), 0.0, lambda m: hi(m) <= dist)
    if lo(m_eq) != dist or hi(M_eq) != dist:
        return None
    m_rej = _search(m_eq, 1e9, lambda m: lo(m) > dist)
    m_in = np.nextafter(m_eq, f32(0))
    M_rej = _search(M_eq, 0.0, lambda m: hi(m) < dist)
    M_in = np.nextafter(M_eq, f32(1e9))
    assert lo(m_in) < dist and hi(M_in) > dist

    def set_min(v):
        return lambda mp: mp.__setitem__("min_distance", v)

    def set_max(v):  # the level is predicted from max_distance: ratio ~ 1/1.2 clamps to 0
        def e(mp):
            mp["max_distance"] = v
            mp["min_distance"] = f32(v / f32(8.0))
        return e

    return [("min_eq", set_min(m_eq), True), ("min_rej", set_min(m_rej), False),
            ("min_in", set_min(m_in), True), ("max_eq", set_max(M_eq), True),
            ("max_rej", set_max(M_rej), False), ("max_in", set_max(M_in), True)]


def gates_scene():
    """Lone-candidate windows, one per rule.  Tags say which gate a point sits
    on; gates_expect() turns them into the answer for each family."""
    sc = Scene(21)
    for d in (49, 50, 51, 63, 64, 65, 99, 100, 101):
        sc.lone(d=d)
    sc.lone(d=0, behind=True)                       # Pc.z < 0
    # image bounds: the candidate keypoint sits inside the grid next to the edge
    sc.lone(at=(0.0, 200.0), kp_at=(2.0, 200.0), edge="min")
    sc.lone(at=(200.0, 0.0), kp_at=(200.0, 2.0), edge="min")
    # (x < 635, y < 475); at level 7 its 6 px are inside Fuse's chi-square gate too
    sc.lone(at=(640.0, 200.0), kp_at=(634.0, 200.0), level=7, edge="max")
    sc.lone(at=(280.0, 480.0), kp_at=(280.0, 474.0), level=7, edge="max")
    # distance gates: for each, the next site whose dist has an exact partner
    # under 0.8f * min (1.2f * max)
    for k in range(6):
        edits = None
        while edits is None:
            site = sc.next_site()
            edits = _dist_edits(map_point(site[0], site[1], 0))
        name, edit, keep = edits[k]
        sc.lone(at=site, edit=edit, gate=name, keep=keep)
    # predicted level at both ends.  Below: the lower clamp (q < 0) cannot be
    # reached past the distance gate, which wants max_distance >= dist / 1.2 and
    # so q = ceil(log(ratio) / log 1.2) >= ceil(-1 +- rounding): this point, with
    # ratio 0.84, gives ceil(-0.96) = -0 and level 0 without clamping (asserted),
    # and max_eq above sits within rounding of -1 (-0.99999993 at its site: -0 too)
    def low(mp):
        dist = pyref._norm(mp["pos"])
        mp["max_distance"] = f32(float(dist) * 0.84)
        q = f32(f32(math.log(float(f32(mp["max_distance"] / dist)))) / LS)
        assert -1 < q < 0 and pyref._level(mp["max_distance"], dist, LS, N_LEVELS) == 0
    sc.lone(level=0, edit=low, clamp=0)

    def top(mp):   # above: q = 10 >= nLevels, clamped to 7
        mp["max_distance"] = f32(mp["max_distance"] * 1.2 ** 3)
        mp["min_distance"] = f32(mp["min_distance"] / 8)
        dist = pyref._norm(mp["pos"])
        assert np.ceil(f32(f32(math.log(float(f32(mp["max_distance"] / dist)))) / LS)) > 7
    sc.lone(level=7, octave=7, edit=top, clamp=7)
    # viewing cosine: normal along z only, dot = 8 * nz against 0.5 * dist
    for name, step, keep in (("cos_eq", None, True), ("cos_below", 0.0, False),
                             ("cos_above", 1.0, True)):
        def tilt(mp, step=step):
            nz = f32(pyref._norm(mp["pos"]) / f32(16.0))
            assert 8.0 * float(nz) == 0.5 * float(pyref._norm(mp["pos"]))
            mp["normal"] = (0.0, 0.0, nz if step is None else np.nextafter(nz, f32(step)))
        sc.lone(edit=tilt, cos=name, keep=keep)
    return sc


def gates_expect(sc, family, thr):
    """Index of the matched keypoint per point (-1 none), from the tags alone."""
    kf = family != "reloc"   # KeyFrame variants: depth test, half-open bounds, cosine test
    out = []
    for tag, k in zip(sc.tags, sc.pair):
        ok = tag["d"] <= thr and tag.get("keep", True) is not False
        if "cos" in tag and not kf:
            ok = tag["d"] <= thr
        if kf and (tag["behind"] or tag.get("edge") == "max"):
            ok = False
        out.append(k if ok else -1)
    return np.array(out, np.int32)


def _claim_expect(pairs, nkeys):
    km = np.full(nkeys, -1, np.int32)
    for i, k in enumerate(pairs):
        if k >= 0:
            km[k] = i
    return km


def gates_reloc(orb_dist):
    sc = gates_scene()
    keys, desc, _ = sc.frame()
    mps, md, ang = sc.points()
    exp = gates_expect(sc, "reloc", orb_dist)
    return reloc_case(keys, desc, mps, md, ang, 10.0, orb_dist, False,
                      expect=_claim_expect(exp, len(keys)), tags=sc.tags)


def gates_sim3():
    sc = gates_scene()
    keys, desc, _ = sc.frame()
    mps, md, _ = sc.points()
    exp = gates_expect(sc, "sim3", 50)
    return sim3_case(keys, desc, mps, md, 10.0, expect=_claim_expect(exp, len(keys)), tags=sc.tags)


def gates_fuse_sim3():
    sc = gates_scene()
    keys, desc, _ = sc.frame()
    mps, md, _ = sc.points()
    return fuse_sim3_case(keys, desc, mps, md, 10.0, expect=gates_expect(sc, "fuse_sim3", 50),
                          tags=sc.tags)


def _chi2_pair(limit, lo, hi):
    """Adjacent floats e_in < e_out in [lo, hi) with e*e on either side of
    `limit` under Fuse's arithmetic (float square, compared as double)."""
    e = _search(f32(math.sqrt(limit)) - f32(8e-6), hi, lambda x: float(f32(x * x)) > limit)
    e_in = np.nextafter(e, f32(lo))
    assert float(f32(e_in * e_in)) <= limit < float(f32(e * e))
    return e_in, e


def gates_fuse():
    """Fuse: the shared gates, then first-minimum ties across grid columns and
    rows, and the 5.99 / 7.8 chi-square gates on either side with u_right -1,
    exactly 0.0 (stereo here: >= 0) and positive."""
    sc = gates_scene()
    rng = sc.rng
    # ties: scan order is grid column, then row, then insertion; the later-added
    # keypoint in the lower column / row must win
    q = rng.integers(0, 256, 32, dtype=np.uint8)
    u, v = sc.next_site()
    sc.kp(u + 6.0, v, flip_bits(q, 4))           # next grid column (cell boundary at u + 5)
    k = sc.kp(u + 4.0, v, flip_bits(q, 4, 10))
    sc.pt(map_point(u + 5.0, v, 0), q, k, d=4, behind=False, tie="column")
    q = rng.integers(0, 256, 32, dtype=np.uint8)
    u, v = sc.next_site()
    sc.kp(u, v + 6.0, flip_bits(q, 4))           # same column, next row
    k = sc.kp(u, v + 4.0, flip_bits(q, 4, 10))
    sc.pt(map_point(u, v + 5.0, 0), q, k, d=4, behind=False, tie="row")
    # chi-square, mono (u_right -1): ex on either side of sqrt(5.99); u = 2.5 so
    # that u - kp.x is exact to the last bit of ex
    e_in, e_out = _chi2_pair(5.99, 2.0, 3.0)
    for e, keep, vv in ((e_in, True, 60.0), (e_out, False, 100.0)):
        assert f32(f32(2.5) - f32(f32(2.5) - e)) == e
        sc.lone(at=(2.5, vv), kp_at=(float(f32(2.5) - e), vv), chi="mono", keep=keep)
    # stereo: ur = u - bf / z = u - 8.  u = 8, u_right = 0.0 exactly: er = 0 and
    # ex * ex = 6.25 lies between 5.99 (mono gate) and 7.8 (stereo gate)
    sc.lone(at=(8.0, 140.0), kp_at=(5.5, 140.0), u_right=0.0, chi="zero", keep=True)
    sc.lone(at=(8.0, 180.0), kp_at=(5.5, 180.0), u_right=-1.0, chi="minus", keep=False)
    e_in, e_out = _chi2_pair(7.8, 2.0, 3.0)
    for e, keep, vv in ((e_in, True, 220.0), (e_out, False, 260.0)):
        ur = f32(f32(3.0) - e)
        assert ur > 0 and f32(f32(3.0) - ur) == e
        sc.lone(at=(11.0, vv), kp_at=(11.0, vv), u_right=float(ur), chi="stereo", keep=keep)
    keys, desc, ur = sc.frame()
    mps, md, _ = sc.points()
    return fuse_case(keys, desc, ur, mps, md, 10.0, expect=gates_expect(sc, "fuse", 50),
                     tags=sc.tags)


def gates_frame():
    """SearchByProjectionFrame: 100 / 101, invzc < 0, the four closed bounds,
    u_right exactly 0.0 (not stereo here: > 0) and er == radius (kept)."""
    sc = Scene(31)
    spec = []   # (u, v, kp index, expected)

    def lone(d, at=None, kp_at=None, u_right=-1.0, behind=False, keep=True, octave=0, kp_oct=0):
        u, v = sc.next_site() if at is None else at
        kx, ky = (u + 1.0, v) if kp_at is None else kp_at
        q = sc.rng.integers(0, 256, 32, dtype=np.uint8)
        k = sc.kp(kx, ky, flip_bits(q, d), kp_oct, 0.0, u_right)
        spec.append((u, v, q, behind, octave, k if keep else -1))

    lone(99); lone(100); lone(101, keep=False)
    lone(0, behind=True, keep=False)
    lone(0, at=(0.0, 200.0), kp_at=(3.0, 200.0))
    lone(0, at=(200.0, 0.0), kp_at=(200.0, 3.0))
    lone(0, at=(640.0, 200.0), kp_at=(634.0, 200.0))
    lone(0, at=(280.0, 480.0), kp_at=(280.0, 474.0))
    # ur = u - 8; radius 10: er == 10 kept, one step beyond rejected; u_right 0.0
    # exactly is "no stereo" here, so a far-off projection (er = 32) still matches
    u, v = sc.next_site()
    lone(0, at=(u, v), u_right=float(f32(u - 8.0 - 10.0)))
    u, v = sc.next_site()
    lone(0, at=(u, v), u_right=float(np.nextafter(f32(u - 8.0 - 10.0), f32(0))), keep=False)
    lone(0, at=(40.0, 440.0), u_right=0.0)
    # level ranges at the bottom and the top octave (mono: o-1..o+1)
    lone(0, octave=0, kp_oct=1)
    lone(0, octave=0, kp_oct=2, keep=False)
    lone(0, octave=7, kp_oct=6)
    lone(0, octave=7, kp_oct=5, keep=False)
    keys, desc, ur = sc.frame()
    last = last_points([s[0] for s in spec], [s[1] for s in spec], [s[4] for s in spec],
                       behind=np.array([s[3] for s in spec]))
    md = np.array([s[2] for s in spec], np.uint8)
    km = np.full(len(keys), -1, np.int32)
    for i, s in enumerate(spec):
        if s[5] >= 0:
            km[s[5]] = last["mp_id"][i]
    win = [(s[0], s[1], f32(f32(10.0) * SCALE[s[4]]), s[4] - 1, s[4] + 1) for s in spec]
    return frame_case(keys, desc, last, md, u_right=ur, expect=km, windows=win)


def levels_frame(direction, octave):
    """fwd (tlc_z > mb: octave >= o), bwd (octave 0..o) and mono (o-1..o+1) level
    ranges: one keypoint per octave around a point of `octave`.  The expected
    keypoint is the allowed octave farthest from `octave` (the upper one first)."""
    sc = Scene(41)
    q = sc.rng.integers(0, 256, 32, dtype=np.uint8)
    for o in range(N_LEVELS):    # distances fall with |o - octave|: the farthest allowed wins
        sc.kp(300.0 + o, 200.0, flip_bits(q, 30 - abs(o - octave) * 3 - (o > octave)), o)
    keys, desc, _ = sc.frame()
    last = last_points([303.0], [200.0], [octave])
    tlc = {"fwd": 1.0, "bwd": -1.0, "mono": 0.0}[direction]
    lo, hi = {"fwd": (octave, 7), "bwd": (0, octave), "mono": (octave - 1, octave + 1)}[direction]
    allowed = [o for o in range(N_LEVELS) if lo <= o <= hi]
    win = min(allowed, key=lambda o: 30 - abs(o - octave) * 3 - (o > octave))
    km = np.full(N_LEVELS, -1, np.int32)
    km[win] = 1000
    return frame_case(keys, desc, last, q.reshape(1, 32), th=10.0, tlc_z=tlc,
                      mono=1 if direction == "mono" else 0,
                      u_right=np.full(N_LEVELS, -1.0, f32), expect=km)


# ----------------------------------------------------------------- B: SearchBySim3
def by_sim3_case(n=257, seed=5, with_masks=True):
    """Two KeyFrames over the same crowded keypoints (KF2's shifted by a pixel),
    each keypoint with a MapPoint at its own pixel: windows hold many near-equal
    candidates, so many pairs agree in one direction only.  Census minimum
    (census_mutual): >= 10 one-way pairs, >= 20 mutual."""
    rng, keys, desc, _, _, _ = _crowd(seed, n, 1, bases=6, noise=0.03)
    keys["octave"] = rng.integers(0, 2, n)
    k2 = keys.copy()
    k2["x"] = (k2["x"] + np.round(rng.uniform(-1, 1, n) * 4) / 4).astype(f32)
    perm = rng.permutation(n)
    k2, d2 = k2[perm], noisy(rng, desc[perm], 0.01)
    out = []
    for kk, dd in ((keys, desc), (k2, d2)):
        mps = np.array([map_point(float(k["x"]), float(k["y"]), int(k["octave"]))
                        for k in kk], MAP_POINT_DTYPE)
        mps["bad"] = rng.random(n) < 0.03
        out.append(dict(keys=kk, desc=dd, scale=SCALE, width=W, height=H, Rw=EYE, tw=ZERO3,
                        mps=mps, mp_desc=noisy(rng, dd, 0.01),
                        valid=(rng.random(n) < (0.9 if with_masks else 2)).astype(np.uint8),
                        already=(rng.random(n) < (0.05 if with_masks else -1)).astype(np.uint8)))
    return _case("by_sim3", kf1=out[0], kf2=out[1], s12=1.0, R12=EYE, t12=ZERO3, th=7.5)


def by_sim3_thresholds():
    """Lone windows at distance 99, 100, 101 in both directions (bestDist starts
    at INT_MAX; accepted iff <= 100), a projection exactly on maxX (half-open:
    outside) and a first-minimum tie."""
    rng = np.random.default_rng(6)
    xs = np.array([100.0, 200.0, 300.0, 400.0, 630.0], f32)
    ds = (99, 100, 101, 0, 0)
    q = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    k1 = keypoints(xs, np.full(5, 100.0, f32))
    k2 = k1.copy()
    k2["x"][4] = 634.0
    # the last pair: KF1's point projects onto maxX exactly (half-open: outside),
    # KF2's onto its own keypoint, 4 px from KF1's
    mp1 = np.array([map_point(float(x), 100.0, 0) for x in (100.0, 200.0, 300.0, 400.0, 640.0)],
                   MAP_POINT_DTYPE)
    mp2 = np.array([map_point(float(x), 100.0, 0) for x in k2["x"]], MAP_POINT_DTYPE)
    d2 = np.array([flip_bits(q[i], ds[i]) for i in range(5)], np.uint8)
    # a tie: KF1's keypoint 5 sees two KF2 keypoints (5 and 6, one grid cell) with
    # its own descriptor; the first minimum is 5, and 5 sees KF1's 5 in turn
    t = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    k1 = np.concatenate([k1, keypoints(np.array([500.0], f32), np.array([100.0], f32))])
    k2 = np.concatenate([k2, keypoints(np.array([499.0, 501.0], f32), np.full(2, 100.0, f32))])
    mp1 = np.concatenate([mp1, np.array([map_point(500.0, 100.0, 0)], MAP_POINT_DTYPE)])
    mp2 = np.concatenate([mp2, np.array([map_point(499.0, 100.0, 0), map_point(501.0, 100.0, 0)],
                                        MAP_POINT_DTYPE)])
    q, d2 = np.concatenate([q, t]), np.concatenate([d2, t, t])
    kf = lambda keys, desc, mps: dict(keys=keys, desc=desc, scale=SCALE, width=W, height=H,
                                      Rw=EYE, tw=ZERO3, mps=mps, mp_desc=desc,
                                      valid=np.ones(len(keys), np.uint8),
                                      already=np.zeros(len(keys), np.uint8))
    # KF1 points carry q and look at KF2's descriptors d2; KF2 points carry d2
    # and look at KF1's descriptors q: the same distance both ways
    return _case("by_sim3", kf1=kf(k1, q, mp1), kf2=kf(k2, d2, mp2), s12=1.0, R12=EYE, t12=ZERO3,
                 th=7.5, expect=np.array([0, 1, -1, 3, -1, 5], np.int32))


# --------------------------------------------------------- D: vocabulary nodes
NODE_SIZES = (1, 63, 64, 65, 128, 129, 200)
TIE_POS = (0, 63, 64, 127)


def _tie_pairs(size):
    """Disjoint position pairs from TIE_POS: across trips where the node has two."""
    if size >= 129:
        return [(0, 127), (63, 64), (65, size - 1)]
    if size >= 128:
        return [(0, 127), (63, 64)]
    if size >= 65:
        return [(63, 64), (0, 1)]
    return [(0, size - 1)] if size >= 2 else []


def node_scene(sizes=NODE_SIZES, ties=False, extras=True, seed=50):
    """One vocabulary node per entry of `sizes`, present in both feature vectors,
    the second vector's node holding that many features.  Each first-vector
    feature ("probe") has descriptor q, its node's other-side features are 120
    bits from q except the planted ones:
      best     one feature at distance 10 in the node's LAST position
      d49/50/51 one feature at that distance (TH_LOW: <= 50 Frame, < 50 KeyFrames)
      ratio    30 against 40: d1 == nnratio * d2 at 0.75, rejected
      equal    d1 == d2 == 20, rejected by the ratio test
      claim    three probes with one q preferring one feature (5), then a second
               (30), then nothing: later ones must see the claims
      masked   a probe without MapPoint / with a bad one
    With ties=True (run with nnratio 1.25 so that d1 == d2 passes the ratio
    test) the probes are pairs of features at distance 20 at positions from
    {0, 63, 64, 127}: BoW keeps the first in position order, triangulation the
    last.  extras: ids only in one vector, below and above all shared ids.
    Returns dict(n1, n2, node1, node2, d1, d2, probes) with probes = list of
    (index1, kind, expected index2 per form)."""
    rng = np.random.default_rng(seed)
    ids = [10 + 7 * k for k in range(len(sizes))]
    node2, d2 = [], []
    node1, d1, probes = [], [], []
    mask1 = []
    for nid, size in zip(ids, sizes):
        base = len(node2)
        node2 += [nid] * size
        slots = [None] * size        # (q index, distance) planted per position
        free = list(range(size - 1, -1, -1))

        def probe(kind, plants, expect):
            i1 = len(node1)
            node1.append(nid)
            q = rng.integers(0, 256, 32, dtype=np.uint8)
            d1.append(q)
            for p, d in plants:
                assert slots[p] is None
                slots[p] = (q, d)
            probes.append((i1, kind, expect))
            mask1.append(kind == "masked")
            return q

        if ties:
            for a, b in _tie_pairs(size):
                probe("tie", [(a, 20), (b, 20)], dict(first=base + a, last=base + b))
        else:
            probe("best", [(free.pop(0), 10)], dict(any=base + size - 1))
            if size >= 12:
                for d in (49, 50, 51):
                    p = free.pop(0)
                    probe("d%d" % d, [(p, d)], dict(any=base + p, d=d))
                p, p2 = free.pop(0), free.pop()
                probe("ratio", [(p, 30), (p2, 40)], dict(none=True, tri=base + p))
                p, p2 = free.pop(0), free.pop()
                probe("equal", [(p, 20), (p2, 20)], dict(none=True, tri=base + max(p, p2)))
                pa, pb = free.pop(0), free.pop(0)
                q = probe("claim", [(pa, 5), (pb, 30)], dict(any=base + pa, tri=base + pa))
                for exp in (dict(any=base + pb, tri=base + pa), dict(none=True, tri=base + pa)):
                    probes.append((len(node1), "claim", exp))
                    node1.append(nid); d1.append(q); mask1.append(False)
                p = free.pop(0)
                probe("masked", [(p, 0)], dict(none=True, tri=base + p))
        for p in range(size):
            if slots[p] is None:
                d2.append(rng.integers(0, 256, 32, dtype=np.uint8))  # ~128 bits from any q
            else:
                q, d = slots[p]
                d2.append(flip_bits(q, d))
    d1a, d2a = np.array(d1, np.uint8).reshape(-1, 32), np.array(d2, np.uint8).reshape(-1, 32)
    if extras:
        lo1, hi1, lo2, hi2 = 5, 900, 2, 1000   # ids present in one vector only
        node1 = [lo1] + node1 + [hi1]
        node2 = [lo2] + node2 + [hi2]
        r = rng.integers(0, 256, (4, 32), dtype=np.uint8)
        d1a = np.concatenate([r[0:1], d1a, r[0:1]])   # equal descriptors across the two
        d2a = np.concatenate([r[0:1], d2a, r[0:1]])   # vectors, but never the same node
        probes = [(i + 1, k, {kk: (vv + 1 if kk in ("any", "tri", "first", "last") else vv)
                              for kk, vv in e.items()}) for i, k, e in probes]
        mask1 = [False] + mask1 + [False]
    return dict(node1=np.array(node1), node2=np.array(node2), d1=d1a, d2=d2a, probes=probes,
                mask1=np.array(mask1, bool))


def _fv(node_of):
    """DBoW2 FeatureVector as CSR (ids ascending, offsets, feature indices ascending)."""
    node_of = np.asarray(node_of, np.int64)
    order = np.argsort(node_of, kind="stable")
    ids, counts = np.unique(node_of, return_counts=True)
    return (ids.astype(np.uint32), np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
            order.astype(np.uint32))


def _node_check(ns):
    """Unplanted features are random: far (> 80 bits) from every probe of the node."""
    for nid in np.unique(ns["node1"]):
        a, b = ns["d1"][ns["node1"] == nid], ns["d2"][ns["node2"] == nid]
        if len(a) and len(b):
            D = np.unpackbits(a[:, None, :] ^ b[None, :, :], axis=2).sum(2)
            assert ((D <= 51) | (D > 80)).all()


def bow_case(form, sizes=NODE_SIZES, ties=False, extras=True, check_ori=False):
    """form "frame": SearchByBoW(pKF, F); "kf": SearchByBoW(pKF1, pKF2)."""
    ns = node_scene(sizes, ties, extras)
    _node_check(ns)
    n1, n2 = len(ns["d1"]), len(ns["d2"])
    mp1 = np.where(ns["mask1"], -1, np.arange(n1) + 5000).astype(np.int32)
    bad1 = np.zeros(n1, np.uint8)
    nnratio = 1.25 if ties else 0.75
    fv1, fv2 = _fv(ns["node1"]), _fv(ns["node2"])
    a1, a2 = np.zeros(n1, f32), np.zeros(n2, f32)
    thr = 50 if form == "frame" else 49
    pairs = []   # (index1, index2) accepted
    for i1, kind, e in ns["probes"]:
        if "none" in e or ("d" in e and e["d"] > thr):
            continue
        pairs.append((i1, e["first"] if "first" in e else e["any"]))
    if form == "frame":
        exp = np.full(n2, -1, np.int32)
        for i1, i2 in pairs:
            exp[i2] = mp1[i1]
        return _case("bow", kf_desc=ns["d1"], kf_angle=a1, kf_mp=mp1, kf_bad=bad1, kf_fv=fv1,
                     f_desc=ns["d2"], f_angle=a2, f_fv=fv2, nnratio=nnratio, check_ori=check_ori,
                     expect=exp, n_expect=len(pairs))
    mp2 = (np.arange(n2) + 10000).astype(np.int32)
    exp = np.full(n1, -1, np.int32)
    for i1, i2 in pairs:
        exp[i1] = mp2[i2]
    return _case("bow_kf", d1=ns["d1"], a1=a1, mp1=mp1, bad1=bad1, fv1=fv1, d2=ns["d2"], a2=a2,
                 mp2=mp2, bad2=np.zeros(n2, np.uint8), fv2=fv2, nnratio=nnratio,
                 check_ori=check_ori, expect=exp, n_expect=len(pairs))


# F12 of a camera pair whose epipolar line of (x, y) is  (1 - x/256) * y2 - y = 0:
# with every keypoint on the row y = 0 each pair passes with dsqr = 0, a KF2
# keypoint at height e has dsqr = e * e for x = 0, and x = 256 gives den == 0.
F12 = np.array([[0, -1.0 / 256, 0], [0, 0, -1.0], [0, 1.0, 0]], f32)
EPIPOLE = (600.0, 0.0)
CW = np.array([(EPIPOLE[0] - CX) / FX * Z, (EPIPOLE[1] - CY) / FY * Z, Z], f32)


def tri_case(sizes=NODE_SIZES, ties=False, extras=True, only_stereo=False, check_ori=False,
             geometry=True):
    """SearchForTriangulation over node_scene: the last minimum wins, 50 passes,
    no ratio test and no claims.  geometry adds to the first node of 65+
    features: has_mp on either side, the epipole-distance gate on both sides
    (and skipped for a u_right of exactly 0.0: >= 0 is stereo), den == 0, and
    dsqr on either side of 3.84 * sigma2."""
    ns = node_scene(sizes, ties, extras)
    _node_check(ns)
    rng = np.random.default_rng(60)
    n1, n2 = len(ns["d1"]), len(ns["d2"])
    x1 = (np.arange(n1) % 200 + 1.0).astype(f32)
    x2 = (np.arange(n2) % 400 + 1.0).astype(f32)
    y1, y2 = np.zeros(n1, f32), np.zeros(n2, f32)
    ur1, ur2 = np.full(n1, -1.0, f32), np.full(n2, -1.0, f32)
    st = rng.random(n1) < 0.4
    ur1[st] = x1[st] - f32(8.0)
    st2 = rng.random(n2) < 0.4
    ur2[st2] = x2[st2] - f32(8.0)
    has1, has2 = np.zeros(n1, np.uint8), np.zeros(n2, np.uint8)
    exp = {}
    for i1, kind, e in ns["probes"]:
        if "d" in e and e["d"] > 50:
            continue
        exp[i1] = e["tri"] if "tri" in e else (e["last"] if "last" in e else e["any"])
    if geometry and not ties:
        # probes with a single planted feature
        want = [p for p in ns["probes"] if p[1] in ("d49", "d50", "best", "masked")]
        assert len(want) >= 8
        lim = 3.84
        e_out = _search(f32(math.sqrt(lim)) - f32(4e-6), 3.0,
                        lambda x: not float(f32(f32(x * x) / f32(1.0))) < lim * 1.0)
        e_in = np.nextafter(e_out, f32(0))
        assert float(f32(e_in * e_in)) < lim
        edits = [("has1", None), ("has2", None), ("den0", None), ("dsqr_in", e_in),
                 ("dsqr_out", e_out), ("epi_in", None), ("epi_out", None), ("epi_zero", None)]
        for (i1, kind, e), (name, val) in zip(want, edits):
            i2 = exp[i1]
            if name == "has1":
                has1[i1] = 1; exp.pop(i1)
            elif name == "has2":
                has2[i2] = 1; exp.pop(i1)
            elif name == "den0":
                x1[i1] = 256.0; exp.pop(i1)
            elif name.startswith("dsqr"):
                x1[i1] = 0.0; y2[i2] = val
                if name == "dsqr_out":
                    exp.pop(i1)
            else:   # mono-mono pairs near the epipole: squared distance < 100 * scale[0] skips
                ur1[i1] = -1.0
                ur2[i2] = -1.0
                x2[i2] = EPIPOLE[0] - 10.0
                if name == "epi_in":
                    x2[i2] = np.nextafter(f32(EPIPOLE[0] - 10.0), f32(EPIPOLE[0]))
                    exp.pop(i1)
                if name == "epi_zero":
                    x2[i2] = EPIPOLE[0] - 2.0
                    ur1[i1] = ur2[i2] = 0.0
    if only_stereo:
        for i1 in list(exp):
            if not (ur1[i1] >= 0 and ur2[exp[i1]] >= 0):
                exp.pop(i1)
    m12 = np.full(n1, -1, np.int32)
    for i1, i2 in exp.items():
        m12[i1] = i2
    kf = lambda x, y, d, ur, has: dict(keys=keypoints(x, y), desc=d, scale=SCALE, width=W,
                                       height=H, u_right=ur, has_mp=has)
    return _case("tri", kf1=kf(x1, y1, ns["d1"], ur1, has1), kf2=kf(x2, y2, ns["d2"], ur2, has2),
                 F12=F12, Cw=CW, fv1=_fv(ns["node1"]), fv2=_fv(ns["node2"]),
                 only_stereo=only_stereo, check_ori=check_ori,
                 expect=None if only_stereo else m12)


# --------------------------------------------------------- E: rotation histogram
# bins reachable with factor 1/30 are 0..12 (rot * (1/30) for rot in [0, 360])
HIST_SHAPES = {
    "four_tied": {2: 3, 5: 3, 9: 3, 11: 3},      # strict '>' scan keeps 2, 5, 9
    "ten_one_one": {0: 10, 7: 1, 12: 1},          # max2 * 10 == max1: 1 < 0.1f * 10 is false
    "eleven_one_one": {0: 11, 7: 1, 12: 1},       # max2 * 10 == max1 - 1: second and third go
    "ten_two_one": {4: 10, 1: 2, 12: 1},          # max3 * 10 == max1: kept
    "eleven_two_one": {4: 11, 1: 2, 12: 1},       # max3 * 10 == max1 - 1: third goes
    "one_bin": {6: 5},
}


def hist_keep(shape):
    c = [0] * 30
    for b, k in HIST_SHAPES[shape].items():
        c[b] = k
    return [b for b in pyref._three_maxima(c) if b >= 0]


def _hist_angles(shape):
    """(angle1, angle2, bin) per match.  Bin 12's first entry has a rotation
    that is negative by less than half an ulp of 360: rot + 360 rounds to 360."""
    out = []
    for b, k in HIST_SHAPES[shape].items():
        for j in range(k):
            if b == 12 and j == 0:
                out.append((0.0, 1e-6, 12))
            else:
                out.append((30.0 * b + 40.0, 40.0, b))
    for a1, a2, b in out:
        assert pyref._rot_bin(f32(a1), f32(a2)) == b
    return out


def hist_reloc(shape):
    sc = Scene(70)
    keep = hist_keep(shape)
    pairs = []
    for a1, a2, b in _hist_angles(shape):
        i = sc.lone(d=3, angle=a1, kp_angle=a2)
        pairs.append((sc.pair[i], i if b in keep else -2))
    keys, desc, _ = sc.frame()
    mps, md, ang = sc.points()
    km = np.full(len(keys), -1, np.int32)
    for k, val in pairs:
        km[k] = val
    win = [(sc.kx[k] - 1.0, sc.ky[k], f32(10.0), -1, 1) for k in sc.pair]  # lone: kp at u + 1
    return reloc_case(keys, desc, mps, md, ang, check_ori=True, expect=km, windows=win)


def hist_frame(shape):
    sc = Scene(72)
    keep = hist_keep(shape)
    ang = _hist_angles(shape)
    u, v, q, kidx = [], [], [], []
    for a1, a2, b in ang:
        x, y = sc.next_site()
        d = sc.rng.integers(0, 256, 32, dtype=np.uint8)
        kidx.append(sc.kp(x + 1.0, y, flip_bits(d, 3), 0, a2))
        u.append(x); v.append(y); q.append(d)
    keys, desc, _ = sc.frame()
    last = last_points(u, v, 0, [a for a, _, _ in ang])
    km = np.full(len(keys), -1, np.int32)
    for i, (k, (_, _, b)) in enumerate(zip(kidx, ang)):
        km[k] = last["mp_id"][i] if b in keep else -2
    win = [(x, y, f32(10.0), -1, 1) for x, y in zip(u, v)]
    return frame_case(keys, desc, last, np.array(q, np.uint8), check_ori=True, expect=km,
                      windows=win)


def hist_bow(shape, form="frame"):
    """All matches in one node of 70 features, planted from the last position
    down (second trip of the lane loop)."""
    rng = np.random.default_rng(71)
    ang = _hist_angles(shape)
    keep = hist_keep(shape)
    size, n1 = 70, len(ang)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, (size, 32), dtype=np.uint8)
    a1, a2 = np.zeros(n1, f32), np.zeros(size, f32)
    pairs = []
    for i, (x1, x2, b) in enumerate(ang):
        p = size - 1 - 2 * i
        d2[p] = flip_bits(d1[i], 3)
        a1[i], a2[p] = x1, x2
        pairs.append((i, p, b in keep))
    mp1 = (np.arange(n1) + 5000).astype(np.int32)
    fv1, fv2 = _fv(np.full(n1, 3)), _fv(np.full(size, 3))
    n_exp = sum(k for _, _, k in pairs)
    if form == "frame":
        exp = np.full(size, -1, np.int32)
        for i, p, k in pairs:
            if k:
                exp[p] = mp1[i]
        return _case("bow", kf_desc=d1, kf_angle=a1, kf_mp=mp1, kf_bad=np.zeros(n1, np.uint8),
                     kf_fv=fv1, f_desc=d2, f_angle=a2, f_fv=fv2, nnratio=0.75, check_ori=True,
                     expect=exp, n_expect=n_exp)
    exp = np.full(n1, -1, np.int32)
    for i, p, k in pairs:
        if k:
            exp[i] = p
    kf = lambda d, a: dict(keys=keypoints(np.arange(len(d), dtype=f32) + 1, np.zeros(len(d), f32),
                                          0, a), desc=d, scale=SCALE, width=W, height=H,
                           u_right=np.full(len(d), -1.0, f32), has_mp=np.zeros(len(d), np.uint8))
    return _case("tri", kf1=kf(d1, a1), kf2=kf(d2, a2), F12=F12, Cw=CW, fv1=fv1, fv2=fv2,
                 only_stereo=False, check_ori=True, expect=exp)


# ------------------------------------------------------------- counts and LDS tiers
COUNTS_NKEYS = (1, 31, 32, 33, 65)
COUNTS_N = (1, 63, 64, 65, 255, 256, 257)


def counts_case(family, nkeys, n):
    """Keypoint counts around the lock bitmap's word edge and point counts around
    the batch edge, one cluster so that windows overlap."""
    kw = dict(nkeys=nkeys, n=n, seed=100 + nkeys * 7 + n, clusters=((320.0, 240.0),), side=40.0)
    return {"reloc": crowded_reloc, "sim3": crowded_sim3, "frame": crowded_frame}[family](**kw)


def resolve_lds_pp(nkeys, n):
    """orb_k_pp_resolve_lds: lock words and claimBy per keypoint (both padded to 4),
    accIdx per point, plus the kernel's static hist[32]."""
    words = (nkeys + 31) // 32
    return 4 * (((words + 3) & ~3) + ((nkeys + 3) & ~3) + max(n, 1)) + 128


def resolve_lds_frame(nkeys, n):
    """orb_k_frame_resolve_lds: as above with lastWriter per keypoint as well."""
    words = (nkeys + 31) // 32
    return 4 * (((words + 3) & ~3) + 2 * ((nkeys + 3) & ~3) + max(n, 1)) + 128


LDS_LIMIT = 160 * 1024
# (nkeys, n): below 64 KiB, between 64 KiB and 160 KiB, the largest admitted, one more
LDS_TIERS = {
    "pp": ((3000, 2000), (12000, 5000), (20000, 20300), (20000, 20301)),
    "frame": ((3000, 2000), (6000, 6000), (12000, 16552), (12000, 16553)),
}
assert resolve_lds_pp(20000, 20300) == LDS_LIMIT and resolve_lds_frame(12000, 16552) == LDS_LIMIT
assert 65536 < resolve_lds_pp(12000, 5000) < LDS_LIMIT > resolve_lds_frame(6000, 6000) > 65536


def lds_case(family, nkeys, n, seed=9):
    """Keypoints spread uniformly over the image, points on (noisy copies of)
    keypoints, radius 2 px: windows stay small however many keypoints."""
    rng = np.random.default_rng(seed)
    kx = (np.round(rng.uniform(2, 630, nkeys) * 4) / 4).astype(f32)
    ky = (np.round(rng.uniform(2, 470, nkeys) * 4) / 4).astype(f32)
    keys = keypoints(kx, ky, 0, rng.choice([0.0, 30.0, 200.0], nkeys))
    desc = rng.integers(0, 256, (nkeys, 32), dtype=np.uint8)
    src = rng.integers(0, nkeys, n)
    pu = kx[src] + rng.choice([-0.5, 0.0, 0.5], n).astype(f32)
    pv = ky[src]
    pd = noisy(rng, desc[src], 0.03)
    if family == "frame":
        last = last_points(pu, pv, 0, rng.choice([0.0, 30.0], n), rng.random(n) < 0.7)
        return frame_case(keys, desc, last, pd, th=2.0, check_ori=True)
    pos = np.stack([(pu - f32(CX)) / f32(FX) * f32(Z), (pv - f32(CY)) / f32(FY) * f32(Z),
                    np.full(n, Z, f32)], 1).astype(f32)
    dist = np.sqrt((pos.astype(np.float64) ** 2).sum(1))
    mps = np.zeros(n, MAP_POINT_DTYPE)
    mps["pos"] = pos
    mps["normal"] = (pos / dist[:, None]).astype(f32)
    mps["max_distance"] = (dist * 0.93).astype(f32)
    mps["min_distance"] = (dist * 0.2).astype(f32)
    ang = rng.choice([0.0, 30.0], n).astype(f32)
    if family == "reloc":
        return reloc_case(keys, desc, mps, pd, ang, th=2.0, check_ori=True)
    return sim3_case(keys, desc, mps, pd, th=2.0)


# ---------------------------------------------------------------------- F: empties
def empty_cases():
    """Every variant with no points, no keypoints, and (node-based) no nodes."""
    sc = Scene(80)
    for _ in range(5):
        sc.lone(d=2)
    keys, desc, ur = sc.frame()
    mps, md, ang = sc.points()
    k0, d0, m0, md0 = keys[:0], desc[:0], mps[:0], md[:0]
    last = last_points([sc.kx[i] - 1 for i in range(5)], [sc.ky[i] for i in range(5)], 0)
    out = []
    for kk, dd, mm, mdd, aa, uu in ((keys, desc, m0, md0, ang[:0], ur),
                                    (k0, d0, mps, md, ang, ur[:0])):
        out += [reloc_case(kk, dd, mm, mdd, aa), sim3_case(kk, dd, mm, mdd),
                fuse_case(kk, dd, uu, mm, mdd), fuse_sim3_case(kk, dd, mm, mdd)]
    out += [frame_case(keys, desc, last[:0], md0), frame_case(k0, d0, last, md)]
    kf = lambda kk, dd, mm, mdd: dict(keys=kk, desc=dd, scale=SCALE, width=W, height=H, Rw=EYE,
                                      tw=ZERO3, mps=mm, mp_desc=mdd,
                                      valid=np.ones(len(kk), np.uint8),
                                      already=np.zeros(len(kk), np.uint8))
    full = kf(keys, desc, np.array([map_point(float(k["x"]), float(k["y"]), 0) for k in keys],
                                   MAP_POINT_DTYPE), desc)
    none = kf(k0, d0, m0, md0)
    for a, b in ((full, none), (none, full)):
        out.append(_case("by_sim3", kf1=a, kf2=b, s12=1.0, R12=EYE, t12=ZERO3, th=7.5))
    nofv = _fv(np.zeros(0))
    b = bow_case("frame", (5,), extras=False)
    out += [dict(b, kf_fv=nofv, expect=None), dict(b, f_fv=nofv, expect=None)]
    b = bow_case("kf", (5,), extras=False)
    out += [dict(b, fv1=nofv, expect=None), dict(b, fv2=nofv, expect=None)]
    t = tri_case((5,), extras=False, geometry=False)
    out += [dict(t, fv1=nofv, expect=None), dict(t, fv2=nofv, expect=None)]
    return out


# ------------------------------------------------------------------------ runners
def run_oracle(o, c):
    f = c["family"]
    if f == "reloc":
        return o.search_by_projection_reloc(c["keys"], c["desc"], SCALE, W, H, pose_record(), CAM,
                                            c["mps"], c["mp_desc"], c["kf_angle"], c["th"],
                                            c["orb_dist"], c["check_ori"], c["locked"], LS)
    if f == "sim3":
        return o.search_by_projection_sim3(c["keys"], c["desc"], SCALE, W, H, scw(), CAM, c["mps"],
                                           c["mp_desc"], c["th"], c["kp_matched"], LS)
    if f == "fuse":
        return o.fuse(c["keys"], c["desc"], SCALE, INV_SIGMA2, W, H, c["u_right"], pose_record(),
                      CAM, c["mps"], c["mp_desc"], c["th"], LS)
    if f == "fuse_sim3":
        return o.fuse_sim3(c["keys"], c["desc"], SCALE, W, H, scw(), CAM, c["mps"], c["mp_desc"],
                           c["th"], LS)
    if f == "by_sim3":
        return o.search_by_sim3(c["kf1"], c["kf2"], CAM, c["s12"], c["R12"], c["t12"], c["th"], LS)
    if f == "frame":
        return o.match_projection_frame(c["keys"], c["desc"], SCALE, W, H, c["last"],
                                        c["last_desc"], CAM, c["tlc_z"], c["th"], c["mono"],
                                        c["check_ori"], c["locked"], c["u_right"])
    if f == "bow":
        return o.match_bow(c["kf_desc"], c["kf_angle"], c["kf_mp"], c["kf_bad"], c["kf_fv"],
                           c["f_desc"], c["f_angle"], c["f_fv"], c["nnratio"], c["check_ori"])
    if f == "bow_kf":
        return o.search_by_bow_kf(c["d1"], c["a1"], c["mp1"], c["bad1"], c["fv1"], c["d2"],
                                  c["a2"], c["mp2"], c["bad2"], c["fv2"], c["nnratio"],
                                  c["check_ori"])
    if f == "tri":
        return o.search_for_triangulation(c["kf1"], c["kf2"], SIGMA2, c["F12"], CAM, c["Cw"], EYE,
                                          ZERO3, c["fv1"], c["fv2"], c["only_stereo"],
                                          c["check_ori"])
    raise KeyError(f)


def run_pyref(c, rules=()):
    f = c["family"]
    if f == "reloc":
        return pyref.search_by_projection_reloc(c["keys"], c["desc"], SCALE, W, H, EYE, ZERO3,
                                                ZERO3, CAM, c["mps"], c["mp_desc"], c["kf_angle"],
                                                c["th"], c["orb_dist"], c["check_ori"],
                                                c["locked"], LS, rules=rules)
    if f == "sim3":
        return pyref.search_by_projection_sim3(c["keys"], c["desc"], SCALE, W, H, scw(), CAM,
                                               c["mps"], c["mp_desc"], c["th"], c["kp_matched"],
                                               LS, rules=rules)
    if f == "fuse":
        return pyref.fuse(c["keys"], c["desc"], SCALE, INV_SIGMA2, W, H, c["u_right"], EYE, ZERO3,
                          ZERO3, CAM, c["mps"], c["mp_desc"], c["th"], LS, rules=rules)
    if f == "by_sim3":
        return pyref.search_by_sim3(c["kf1"], c["kf2"], CAM, c["s12"], c["R12"], c["t12"],
                                    c["th"], LS, rules=rules)
    if f == "frame":
        return pyref.search_by_projection_frame(c["keys"], c["desc"], SCALE, W, H, c["last"],
                                                c["last_desc"], CAM, c["tlc_z"], c["th"],
                                                c["mono"], c["check_ori"], c["locked"],
                                                c["u_right"], rules=rules)
    if f == "bow":
        return pyref.search_by_bow(c["kf_desc"], c["kf_angle"], c["kf_mp"], c["kf_bad"],
                                   c["kf_fv"], c["f_desc"], c["f_angle"], c["f_fv"], c["nnratio"],
                                   c["check_ori"], rules=rules)
    if f == "bow_kf":
        return pyref.search_by_bow_kf(c["d1"], c["a1"], c["mp1"], c["bad1"], c["fv1"], c["d2"],
                                      c["a2"], c["mp2"], c["bad2"], c["fv2"], c["nnratio"],
                                      c["check_ori"], rules=rules)
    if f == "tri":
        return pyref.search_for_triangulation(c["kf1"], c["kf2"], SIGMA2, c["F12"], CAM, c["Cw"],
                                              EYE, ZERO3, c["fv1"], c["fv2"], c["only_stereo"],
                                              c["check_ori"], rules=rules)
    raise KeyError(f)   # fuse_sim3 has no restatement: oracle and construction only


def run_gpu(gpu, matchers, c):
    """The Python entry point of the case's variant on a matcher shared per
    (nnratio, checkOri), so that scratch buffers are reused across cases."""
    f = c["family"]
    key = (c.get("nnratio", 0.6), bool(c.get("check_ori", True)))
    if key not in matchers:
        matchers[key] = gpu.ORBmatcher(*key)
    m = matchers[key]
    fr = lambda keys, desc, ur=None: gpu.Frame(keys, desc, SCALE, W, H, u_right=ur)
    if f == "reloc":
        return m.SearchByProjectionKF(fr(c["keys"], c["desc"]), pose_record(), CAM, float(LS),
                                      c["mps"], c["mp_desc"], c["kf_angle"], c["th"],
                                      c["orb_dist"], c["locked"])
    if f == "sim3":
        return m.SearchByProjectionSim3(fr(c["keys"], c["desc"]), scw(), CAM, float(LS), c["mps"],
                                        c["mp_desc"], c["th"], c["kp_matched"])
    if f == "fuse":
        return m.Fuse(fr(c["keys"], c["desc"], c["u_right"]), INV_SIGMA2, pose_record(), CAM,
                      float(LS), c["mps"], c["mp_desc"], c["th"])
    if f == "fuse_sim3":
        return m.FuseSim3(fr(c["keys"], c["desc"]), scw(), CAM, float(LS), c["mps"], c["mp_desc"],
                          c["th"])
    if f == "by_sim3":
        a, b = c["kf1"], c["kf2"]
        return m.SearchBySim3(fr(a["keys"], a["desc"]), fr(b["keys"], b["desc"]), float(LS), CAM,
                              a["Rw"], a["tw"], b["Rw"], b["tw"], a["mps"], a["valid"],
                              a["already"], a["mp_desc"], b["mps"], b["valid"], b["already"],
                              b["mp_desc"], c["s12"], c["R12"], c["t12"], c["th"])
    if f == "frame":
        return m.SearchByProjectionFrame(fr(c["keys"], c["desc"], c["u_right"]), c["last"],
                                         c["last_desc"], CAM, c["tlc_z"], c["th"], bool(c["mono"]),
                                         c["locked"])
    if f == "bow":
        return m.SearchByBoW(c["kf_desc"], c["kf_angle"], c["kf_mp"], c["kf_bad"], c["kf_fv"],
                             c["f_desc"], c["f_angle"], c["f_fv"])
    if f == "bow_kf":
        return m.SearchByBoWKF(c["d1"], c["a1"], c["mp1"], c["bad1"], c["fv1"], c["d2"], c["a2"],
                               c["mp2"], c["bad2"], c["fv2"])
    if f == "tri":
        a, b = c["kf1"], c["kf2"]
        return m.SearchForTriangulation(fr(a["keys"], a["desc"], a["u_right"]), a["has_mp"],
                                        fr(b["keys"], b["desc"], b["u_right"]), b["has_mp"],
                                        SIGMA2, c["F12"], CAM, c["Cw"], EYE, ZERO3, c["fv1"],
                                        c["fv2"], c["only_stereo"])
    raise KeyError(f)


# ------------------------------------------------------------------------- census
def windows_kf(mps, R, t, ow, cam, scale, th, width, height, reloc, log_scale=LS):
    """Windows of the natural scenes' map points for census_claiming: the
    projection and gates of SearchByProjection(F, pKF, ...) (reloc) or
    SearchByProjection(pKF, Scw, ...) as pyref states them."""
    fx, fy, cx, cy = (f32(c) for c in cam[:4])
    out = []
    for mp in mps:
        out.append(None)
        if mp["bad"] or mp["seen"]:
            continue
        Pc = pyref._xf(R, t, mp["pos"])
        if reloc:
            invz = f32(1.0 / float(Pc[2]))
            u = f32(f32(f32(fx * Pc[0]) * invz) + cx)
            v = f32(f32(f32(fy * Pc[1]) * invz) + cy)
            if pyref._out_frame(u, v, width, height):
                continue
        else:
            if Pc[2] < 0:
                continue
            invz = f32(f32(1) / Pc[2])
            u = f32(f32(fx * f32(Pc[0] * invz)) + cx)
            v = f32(f32(fy * f32(Pc[1] * invz)) + cy)
            if not pyref._in_kf(u, v, width, height):
                continue
        PO = [f32(f32(mp["pos"][k]) - f32(ow[k])) for k in range(3)]
        dist = pyref._norm(PO)
        if dist < f32(f32(0.8) * mp["min_distance"]) or dist > f32(f32(1.2) * mp["max_distance"]):
            continue
        if not reloc and pyref._dotd(PO, mp["normal"]) < 0.5 * float(dist):
            continue
        lvl = pyref._level(mp["max_distance"], dist, log_scale, len(scale))
        out[-1] = (u, v, f32(f32(th) * f32(scale[lvl])), lvl - 1, lvl + 1 if reloc else lvl)
    return out


def windows_frame(last, cam, scale, th):
    """Windows of SearchByProjection(CurrentFrame, LastFrame) in its mono form."""
    fx, fy, cx, cy = (f32(c) for c in cam[:4])
    out = []
    for L in last:
        u = f32(f32(f32(fx * L["xc"]) * L["invzc"]) + cx)
        v = f32(f32(f32(fy * L["yc"]) * L["invzc"]) + cy)
        o = int(L["last_octave"])
        out.append((u, v, f32(f32(th) * f32(scale[o])), o - 1, o + 1) if L["valid"] else None)
    return out


def census_claiming(c, width=W, height=H):
    """Sequential replay of a claiming variant (reloc, sim3, frame) over the
    case's `windows` (u, v, radius, minLevel, maxLevel per point, None = the
    point never opens a window):
      slow   points with more than TOPK candidates whose TOPK nearest in
             (distance, scan order) are locked when the point is reached
      near   points with an earlier point, at most WAVE - 1 places before,
             accepted onto one of their TOPK nearest (a conflict if both sit in
             one batch)
      multi  keypoints written more than once (frame: writers without
             observations do not lock)
    plus windows opened, largest candidate count, points accepted, rejected by
    the distance threshold, and with their best free candidate exactly at the
    threshold and one above it; with the rotation filter on, the histogram's
    shape and the entries and keypoints it resets (partial_reset: keypoints
    that lose some but not all of their writers, Frame variant only).  Frame
    candidates exclude keypoints locked on entry and those failing the u_right
    gate, as k_frame_candidates does; the other two keep entry locks in the list."""
    f = c["family"]
    keys, desc = c["keys"], c["desc"]
    cells, invW, invH = pyref.grid_cells(keys, width, height)
    if f == "sim3":
        entry = np.asarray(c["kp_matched"]) >= 0
        qd, thr = c["mp_desc"], 50
        locks = np.ones(len(qd), bool)
    elif f == "reloc":
        entry = np.asarray(c["locked"], bool)
        qd, thr = c["mp_desc"], c["orb_dist"]
        locks = np.ones(len(qd), bool)
    else:
        entry = np.asarray(c["locked"], bool)
        qd, thr = c["last_desc"], 100
        locks = np.asarray(c["last"]["has_obs"], bool)
    angle = None    # the rotation filter's first angle per point, where the call applies it
    if c.get("check_ori") and f == "reloc":
        angle = c["kf_angle"]
    elif c.get("check_ori") and f == "frame":
        angle = c["last"]["last_angle"]
    lock = entry.copy()
    taker = {}      # keypoint -> index of the last point accepted onto it
    writers = {}    # keypoint -> histogram bins of the points written onto it
    writes = np.zeros(len(keys), np.int64)
    out = dict(points=len(qd), windows=0, max_cands=0, slow=0, near=0, multi=0, accepted=0,
               rejected=0, at_thr=0, at_thr_plus_1=0)
    for i, w in enumerate(c["windows"]):
        if w is None:
            continue
        u, v, r, lo, hi = w
        if f == "frame" and c["last"]["invzc"][i] < 0:
            continue
        check = f != "sim3"   # sim3 filters levels in its loop, the others in GetFeaturesInArea
        idx = pyref.features_in_area(keys, cells, invW, invH, u, v, r, lo if check else -1,
                                     hi if check else -1)
        cand = []
        for j in idx:
            if not check and not (lo <= keys[j]["octave"] <= hi):
                continue
            if f == "frame":
                if entry[j]:
                    continue
                ur = c["u_right"]
                if ur is not None and ur[j] > 0 and abs(f32(f32(f32(u) - f32(BF / Z)) - ur[j])) > r:
                    continue
            cand.append((pyref.hamming(qd[i], desc[j]), len(cand), j))
        out["windows"] += 1
        out["max_cands"] = max(out["max_cands"], len(cand))
        top = sorted(cand)[:TOPK]
        if len(cand) > TOPK and all(lock[j] for _, _, j in top):
            out["slow"] += 1
        if any(j in taker and i - taker[j] < WAVE for _, _, j in top):
            out["near"] += 1
        free = [(d, o, j) for d, o, j in cand if not lock[j]]
        if free:
            d, _, j = min(free)
            if d == thr:
                out["at_thr"] += 1
            if d == thr + 1:
                out["at_thr_plus_1"] += 1
            if d <= thr:
                out["accepted"] += 1
                writes[j] += 1
                taker[j] = i
                if locks[i]:
                    lock[j] = True
                if angle is not None:
                    writers.setdefault(j, []).append(pyref._rot_bin(angle[i], keys[j]["angle"]))
            else:
                out["rejected"] += 1
    out["multi"] = int((writes > 1).sum())
    if angle is not None:
        # histogram shape (entries per bin, descending) and what the three-maxima
        # rule does to it: entries reset, keypoints with every writer reset, and
        # keypoints with some but not all writers reset
        counts = [0] * 30
        for bins in writers.values():
            for b in bins:
                counts[b] += 1
        keep = pyref._three_maxima(counts)
        gone = {j: [b not in keep for b in bins] for j, bins in writers.items()}
        out["hist"] = sorted((k for k in counts if k), reverse=True)
        out["reset"] = sum(sum(g) for g in gone.values())
        out["all_reset"] = sum(all(g) for g in gone.values())
        out["partial_reset"] = sum(any(g) and not all(g) for g in gone.values())
    return out


def census_mutual(c):
    """SearchBySim3 (both poses the identity, s12 = 1, as every by_sim3 input here
    has them): per direction the points that open a window, are accepted
    (best <= 100) and rejected, then the pairs that agree both ways (mutual) and
    those accepted in one direction whose partner points elsewhere (one_way)."""
    th = c["th"]
    best = []
    out = {}
    for tag, A, B in (("12", c["kf1"], c["kf2"]), ("21", c["kf2"], c["kf1"])):
        cells, invW, invH = pyref.grid_cells(B["keys"], W, H)
        win = windows_kf(A["mps"], EYE, ZERO3, ZERO3, CAM, SCALE, th, W, H, False)
        m = np.full(len(A["keys"]), -1, np.int64)
        opened = rejected = 0
        for i, w in enumerate(win):
            if w is None or not A["valid"][i] or A["already"][i]:
                continue
            u, v, r, lo, hi = w
            opened += 1
            cand = [(pyref.hamming(A["mp_desc"][i], B["desc"][j]), k, j) for k, j in enumerate(
                pyref.features_in_area(B["keys"], cells, invW, invH, u, v, r, -1, -1))
                if lo <= B["keys"][j]["octave"] <= hi]
            if cand and min(cand)[0] <= 100:
                m[i] = min(cand)[2]
            elif cand:
                rejected += 1
        best.append(m)
        out["windows_" + tag], out["accepted_" + tag] = opened, int((m >= 0).sum())
        out["rejected_" + tag] = rejected
    m1, m2 = best
    out["mutual"] = int(sum(j >= 0 and m2[j] == i for i, j in enumerate(m1)))
    out["one_way"] = int(sum(j >= 0 and m2[j] != i for i, j in enumerate(m1)) +
                         sum(i >= 0 and m1[i] != j for j, i in enumerate(m2)))
    return out


def census_thresholds(c, out):
    """Gate scenes (points tagged with their descriptor distance `d`): the answer
    of the call per distance, as {d: "accepted" | "rejected"}.  Points behind a
    gate other than the distance threshold are left out."""
    res = {}
    plain = ("d", "behind")
    for i, tag in enumerate(c["tags"]):
        if tag["behind"] or any(k not in plain for k in tag):
            continue
        hit = (out[i] >= 0) if c["family"] in ("fuse", "fuse_sim3") else bool((out == i).any())
        res[tag["d"]] = "accepted" if hit else "rejected"
    return res


def census_nodes(c):
    """Node-based variants: features per shared node on the scanned side, the
    trips of the 64-lane loop they need, the position of the best candidate,
    ties for the minimum by position class (same trip / different trips), and
    first-vector features whose best distance is within TH_LOW, above it, and
    exactly 49, 50 and 51.
    Claims and masks are ignored: this describes the input, not the outcome."""
    f = c["family"]
    if f == "bow":
        fv1, fv2, d1, d2 = c["kf_fv"], c["f_fv"], c["kf_desc"], c["f_desc"]
    elif f == "bow_kf":
        fv1, fv2, d1, d2 = c["fv1"], c["fv2"], c["d1"], c["d2"]
    else:
        fv1, fv2, d1, d2 = c["fv1"], c["fv2"], c["kf1"]["desc"], c["kf2"]["desc"]
    n2 = {int(fv2[0][k]): fv2[2][fv2[1][k]:fv2[1][k + 1]] for k in range(len(fv2[0]))}
    out = dict(nodes1=len(fv1[0]), nodes2=len(fv2[0]), shared=0, only1=0, sizes=[], max_size=0,
               best_beyond_first_trip=0, ties_same_trip=0, ties_cross_trip=0, tie_positions=set(),
               best_le_50=0, best_above_50=0, best_at={49: 0, 50: 0, 51: 0})
    for k in range(len(fv1[0])):
        ff = n2.get(int(fv1[0][k]))
        if ff is None:
            out["only1"] += 1
            continue
        out["shared"] += 1
        out["sizes"].append(len(ff))
        for i1 in fv1[2][fv1[1][k]:fv1[1][k + 1]]:
            ds = [pyref.hamming(d1[i1], d2[j]) for j in ff]
            best = min(ds)
            if best in out["best_at"]:
                out["best_at"][best] += 1
            out["best_le_50" if best <= 50 else "best_above_50"] += 1
            if best > 50:
                continue
            pos = [p for p, d in enumerate(ds) if d == best]
            if pos[0] >= WAVE:
                out["best_beyond_first_trip"] += 1
            if len(pos) > 1:
                cross = pos[0] // WAVE != pos[-1] // WAVE
                out["ties_cross_trip" if cross else "ties_same_trip"] += 1
                out["tie_positions"] |= set(pos)
    out["max_size"] = max(out["sizes"], default=0)
    out["sizes"] = sorted(out["sizes"])
    out["tie_positions"] = sorted(out["tie_positions"])
    return out


# ----------------------------------------------------------------------- registry
# name -> (builder, minimums).  Minimums are conditions on the input (census) and
# on the reference's answer (`matches`), chosen so that the reference alone
# meets them with room to spare; they are not measurements of the kernels.
CASES = {
    "crowded_reloc": (crowded_reloc, dict(slow=10, near=10, matches=100)),
    "crowded_reloc_th5_d64": (lambda: crowded_reloc(th=5.0, orb_dist=64, check_ori=False, seed=12),
                              dict(near=10, matches=50)),
    "crowded_reloc_all_locked": (lambda: crowded_reloc(locked_frac=2.0), dict(matches=0)),
    "crowded_reloc_none_locked": (lambda: crowded_reloc(locked_frac=-1.0),
                                  dict(slow=10, near=10, matches=100)),
    "crowded_sim3": (crowded_sim3, dict(slow=10, near=10, matches=100)),
    "crowded_sim3_none_matched": (lambda: crowded_sim3(matched_frac=-1.0),
                                  dict(slow=10, near=10, matches=100)),
    "crowded_sim3_all_matched": (lambda: crowded_sim3(matched_frac=2.0), dict(matches=0)),
    "crowded_frame": (crowded_frame, dict(slow=10, near=10, multi=10, partial_reset=10,
                                          all_reset=10, matches=100)),
    "crowded_frame_no_ori": (lambda: crowded_frame(check_ori=False, seed=13),
                             dict(slow=10, near=10, multi=10, matches=100)),
    "crowded_frame_stereo_fwd": (lambda: crowded_frame(stereo=True, tlc_z=1.0, seed=4),
                                 dict(slow=10, near=10, multi=10, partial_reset=10, matches=100)),
    "crowded_frame_stereo_bwd": (lambda: crowded_frame(stereo=True, tlc_z=-1.0, seed=5),
                                 dict(slow=10, near=10, multi=10, partial_reset=10, matches=100)),
    "crowded_fuse": (crowded_fuse, dict(matches=50)),
    "crowded_fuse_sim3": (lambda: crowded_fuse(sim3=True), dict(matches=50)),
    "chain_reloc": (chain_reloc, dict(slow=100, matches=130)),
    "chain_sim3": (chain_sim3, dict(slow=100, matches=130)),
    "chain_frame": (chain_frame, dict(slow=100, matches=130)),
    "gates_sim3": (gates_sim3, dict(matches=10)),
    "gates_fuse": (gates_fuse, dict(matches=10)),
    "gates_fuse_sim3": (gates_fuse_sim3, dict(matches=10)),
    "gates_frame": (gates_frame, dict(matches=8, at_thr=1, at_thr_plus_1=1)),
    "by_sim3": (by_sim3_case, dict(matches=20, mutual=20, one_way=10)),
    "by_sim3_no_masks": (lambda: by_sim3_case(n=65, seed=15, with_masks=False), dict(matches=5)),
    "by_sim3_thresholds": (by_sim3_thresholds, dict(matches=4)),
}
for _o in ("cs", "sc"):
    CASES["mixed_reloc_" + _o] = (lambda o=_o: mixed_reloc(o), dict(slow=1, near=1, matches=7))
    CASES["mixed_sim3_" + _o] = (lambda o=_o: mixed_sim3(o), dict(slow=1, near=1, matches=7))
    CASES["mixed_frame_" + _o] = (lambda o=_o: mixed_frame(o), dict(slow=1, near=1, matches=7))
for _f in ("reloc", "sim3"):
    CASES["entry_slow_" + _f] = (lambda f=_f: entry_slow(f), dict(slow=1, near=1, matches=4))
for _d in (50, 64, 100):
    CASES["gates_reloc_%d" % _d] = (lambda d=_d: gates_reloc(d), dict(matches=10))
for _dir in ("fwd", "bwd", "mono"):
    for _oc in (0, 7):
        CASES["levels_frame_%s_%d" % (_dir, _oc)] = (lambda d=_dir, o=_oc: levels_frame(d, o),
                                                     dict(matches=1))
# vocabulary nodes: all sizes; 1, 4 and 5 first-vector nodes (a block of the
# kernels holds four waves, one node each)
NODE_SETS = {"": NODE_SIZES, "_nodes1": (65,), "_nodes4": (1, 63, 64, 65),
             "_nodes5": (1, 63, 64, 65, 128)}
for _s, _sizes in NODE_SETS.items():
    _ex = _s == ""
    for _form in ("frame", "kf"):
        CASES["bow_%s%s" % (_form, _s)] = (
            lambda f=_form, s=_sizes, e=_ex: bow_case(f, s, extras=e),
            dict(sizes=_sizes, matches=len(_sizes)))
    CASES["tri" + _s] = (lambda s=_sizes, e=_ex: tri_case(s, extras=e, geometry=e),
                         dict(sizes=_sizes, matches=len(_sizes)))
for _form in ("frame", "kf"):
    CASES["bow_%s_ties" % _form] = (lambda f=_form: bow_case(f, ties=True),
                                    dict(sizes=NODE_SIZES[1:], tie_positions=TIE_POS, matches=10))
CASES["tri_ties"] = (lambda: tri_case(ties=True), dict(sizes=NODE_SIZES[1:],
                                                       tie_positions=TIE_POS, matches=10))
CASES["tri_only_stereo"] = (lambda: tri_case(only_stereo=True), dict(sizes=NODE_SIZES, matches=5))
CASES["tri_ori"] = (lambda: tri_case(check_ori=True, geometry=False), dict(matches=10))
CASES["bow_frame_ori"] = (lambda: bow_case("frame", check_ori=True), dict(matches=10))
for _sh in HIST_SHAPES:
    _n = len(hist_keep(_sh))
    _h = sorted(HIST_SHAPES[_sh].values(), reverse=True)
    CASES["hist_reloc_" + _sh] = (lambda s=_sh: hist_reloc(s), dict(matches=_n, hist=_h))
    CASES["hist_frame_" + _sh] = (lambda s=_sh: hist_frame(s), dict(matches=_n, hist=_h))
    CASES["hist_bow_" + _sh] = (lambda s=_sh: hist_bow(s), dict(matches=_n))
    CASES["hist_tri_" + _sh] = (lambda s=_sh: hist_bow(s, "tri"), dict(matches=_n))
CLAIMING = ("reloc", "sim3", "frame")
NODE_BASED = ("bow", "bow_kf", "tri")
