"""Directed inputs for Frame::ComputeStereoMatches (k_stereo_rows, k_stereo_match2,
k_stereo_prune), built where the natural synthetic pairs never go: each CASES
entry is (builder, census minimum).  A case is a dict of hand-made pyramids
(uint8 arrays per level, passed to the host entry point), directed keypoints and
descriptors, intrinsics, and -- where the construction knows it -- its own
expected answer.

Two sets of intrinsics: EXACT (bf 32, fx 64: maxD = 64 exactly, so a gate can be
met on the float) and KITTI (scenarios.BF / FX, where bf / (bf / fx) rounds).

Defined domain (check_domain asserts it for every case): octaves inside
[0, nLevels); every right band [floor(y - 2s), ceil(y + 2s)] inside [0, H - 1];
every left keypoint's 11x11 window inside its level; every right keypoint that
can win for a left keypoint (row, octave and u gates passed) at scaled x >= 10,
because the 11 shifts reach 10 columns left of round(uR * inv).  Outside it the
reference itself reads out of bounds, so no case goes there.

test_stereo_edge_cases.py shows on the CPU that the oracle equals pyref on these
inputs, that the census minimums hold and that every wrong neighbour of a rule
(pyref.stereo_match's `rules`) changes a named case's answer;
test_gpu_stereo_edges.py runs them through the kernels."""
import math

import numpy as np

import pyref
import scenarios as S
from matcher_edge_cases import KEYPOINT_DTYPE

f32 = np.float32
N_LEVELS = 8
SCALE = np.ones(N_LEVELS, f32)
for _i in range(1, N_LEVELS):
    SCALE[_i] = f32(SCALE[_i - 1] * f32(1.2))
INV = (f32(1.0) / SCALE).astype(f32)
W0, H0 = 320, 120
EXACT = (32.0, 64.0)      # bf, fx: mb = 0.5, maxD = 64
KITTI = (S.BF, S.FX)


def level_sizes(w, h):
    return [(int(round(w * float(INV[l]))), int(round(h * float(INV[l])))) for l in range(N_LEVELS)]


def flip_bits(desc, nbits):
    """`desc` with its first nbits bits flipped: Hamming distance exactly nbits."""
    bits = np.unpackbits(np.asarray(desc, np.uint8).reshape(32))
    bits[:nbits] ^= 1
    return np.packbits(bits)


def level0(level, s):
    """A level-0 coordinate whose roundf(x * inv[level]) is the integer s."""
    x = f32(f32(s) * SCALE[level])
    assert pyref._roundf(x * INV[level]) == s, (level, s)
    return x


class Scene:
    """Pyramids of independent random texture (left and right unrelated, so an
    unpasted window pair has a SAD in the thousands) plus directed keypoints."""

    def __init__(self, name, intr=KITTI, w=W0, h=H0, seed=1):
        self.name, self.intr, self.w, self.h = name, intr, w, h
        self.rng = np.random.default_rng(seed)
        self.sizes = level_sizes(w, h)
        self.lpyr = [self.rng.integers(0, 256, (lh, lw), dtype=np.uint8) for lw, lh in self.sizes]
        self.rpyr = [self.rng.integers(0, 256, (lh, lw), dtype=np.uint8) for lw, lh in self.sizes]
        self.lk, self.ld, self.rk, self.rd = [], [], [], []
        self.pasted = [[] for _ in range(N_LEVELS)]
        self.matched, self.sad, self.exact = {}, {}, {}

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def left(self, x, y, octave, desc=None):
        self.lk.append((f32(x), f32(y), int(octave)))
        self.ld.append(self.desc() if desc is None else desc)
        return len(self.lk) - 1

    def right(self, x, y, octave, desc=None):
        self.rk.append((f32(x), f32(y), int(octave)))
        self.rd.append(self.desc() if desc is None else desc)
        return len(self.rk) - 1

    def paste(self, level, xl, yl, xr, inc=0, sad=0):
        """The right window of shift `inc` around scaled xr becomes the left window
        around scaled (xl, yl): SAD 0 at that shift, then exactly `sad` by moving
        pixels off the centre row (each by at most 255)."""
        IL, IR = self.lpyr[level], self.rpyr[level]
        c = xr + inc
        rect = (yl - 5, yl + 6, c - 5, c + 6)
        for r in self.pasted[level]:
            assert rect[1] <= r[0] or r[1] <= rect[0] or rect[3] <= r[2] or r[3] <= rect[2], \
                (self.name, "pasted windows overlap", rect, r)
        self.pasted[level].append(rect)
        IR[yl - 5:yl + 6, c - 5:c + 6] = IL[yl - 5:yl + 6, xl - 5:xl + 6]
        px = [(yl - 3, c + 2), (yl + 3, c - 2), (yl - 4, c - 4)]
        assert sad <= 255 * len(px)
        for (yy, xx) in px:
            d = min(sad, 255)
            sad -= d
            v = int(IR[yy, xx])
            IR[yy, xx] = v + d if v + d <= 255 else v - d

    def match(self, level, xl, yl, xr, inc=0, hd=10, sad=40, roct=None, dy=0.0, expect=True,
              y=None, paste=True):
        """A left keypoint at scaled (xl, yl) of `level` and a right one at scaled
        xr whose descriptor is hd bits away, with the window pasted for shift inc."""
        d = self.desc()
        yy = level0(level, yl) if y is None else f32(y)
        iL = self.left(level0(level, xl), yy, level, d)
        iR = self.right(level0(level, xr), f32(yy + f32(dy)), level if roct is None else roct,
                        flip_bits(d, hd))
        if paste:
            self.paste(level, xl, yl, xr, inc, sad)
        if expect is not None:
            self.matched[iL] = bool(expect)
            if expect and paste:
                self.sad[iL] = sad
        return iL, iR

    def case(self, **extra):
        def keys(rows):
            k = np.zeros(len(rows), KEYPOINT_DTYPE)
            for i, (x, y, o) in enumerate(rows):
                k[i]["x"], k[i]["y"], k[i]["octave"] = x, y, o
            k["size"], k["angle"] = 31.0, 0.0
            return k
        c = dict(name=self.name, lk=keys(self.lk), rk=keys(self.rk),
                 ld=np.array(self.ld, np.uint8).reshape(-1, 32),
                 rd=np.array(self.rd, np.uint8).reshape(-1, 32),
                 lpyr=self.lpyr, rpyr=self.rpyr, bf=self.intr[0], fx=self.intr[1], w=self.w,
                 h=self.h, matched=dict(self.matched), sad=dict(self.sad), exact=dict(self.exact))
        c.update(extra)
        check_domain(c)
        return c


# ---------------------------------------------------------------- entry points
def args(c):
    return (c["lk"], c["ld"], c.get("scale", SCALE), c["rk"], c["rd"], c["lpyr"], c["rpyr"],
            c.get("inv", INV), c["bf"], c["fx"], c["w"], c["h"])


def run_oracle(o, c):
    return o.stereo_match(*args(c), with_sad=True)


def run_pyref(c, rules=(), trace=None):
    return pyref.stereo_match(*args(c), rules=rules, trace=trace)


def run_gpu(gpu, matcher, c):
    F = gpu.Frame(c["lk"], c["ld"], SCALE, c["w"], c["h"])
    return matcher.ComputeStereoMatches(F, c["rk"], c["rd"], c["lpyr"], c["rpyr"], INV, c["bf"],
                                        c["fx"])


def check_expect(c, out):
    """The construction's own answer, where it states one."""
    ur, dp, sad = out
    for iL, m in c["matched"].items():
        assert (ur[iL] >= 0) == m and (dp[iL] >= 0) == m, (c["name"], iL, m, ur[iL], dp[iL])
    for iL, s in c["sad"].items():
        assert sad[iL] == s, (c["name"], iL, s, sad[iL])
    for iL, (u, d) in c["exact"].items():
        assert ur[iL] == f32(u) and dp[iL] == f32(d), (c["name"], iL, u, d, ur[iL], dp[iL])


# ------------------------------------------------------------- defined domain
def check_domain(c):
    lk, rk = c["lk"], c["rk"]
    H = c["lpyr"][0].shape[0]
    assert len(c["lpyr"]) == len(c["rpyr"]) == N_LEVELS
    for a, b in zip(c["lpyr"], c["rpyr"]):
        assert a.shape == b.shape and a.dtype == b.dtype == np.uint8
    for k in (lk, rk):
        assert ((k["octave"] >= 0) & (k["octave"] < N_LEVELS)).all(), c["name"]
    r = f32(2.0) * SCALE[rk["octave"]]
    lo, hi = np.floor(rk["y"] - r), np.ceil(rk["y"] + r)
    assert (lo >= 0).all() and (hi <= H - 1).all(), (c["name"], "right band leaves the image")
    mb = f32(c["bf"]) / f32(c["fx"])
    maxD = f32(c["bf"]) / mb
    for i in range(len(lk)):
        l = int(lk["octave"][i])
        lh, lw = c["lpyr"][l].shape
        assert 0 <= int(lk["y"][i]) <= H - 1, (c["name"], i)
        su, sv = pyref._roundf(lk["x"][i] * INV[l]), pyref._roundf(lk["y"][i] * INV[l])
        assert 5 <= su <= lw - 6 and 5 <= sv <= lh - 6, (c["name"], i, "left window", su, sv)
        row = int(lk["y"][i])
        can = (lo <= row) & (row <= hi) & (np.abs(rk["octave"] - l) <= 1) & \
              (rk["x"] >= lk["x"][i] - maxD) & (rk["x"] <= lk["x"][i])
        sx = np.array([pyref._roundf(x * INV[l]) for x in rk["x"][can]])
        assert (sx >= 10).all(), (c["name"], i, "right candidate left of scaled x 10")


# --------------------------------------------------------------------- census
def scratch_capacity(c):
    """Row-list entries per pair by the rule of orb_k_stereo_scratch, for the
    stride the host entry point uses (max(NL, NR, 1))."""
    stride = max(len(c["lk"]), len(c["rk"]), 1)
    return stride * int(math.ceil(4.0 * float(SCALE.max())) + 3)


def census(c):
    """What the input reaches, counted from the restatement's trace."""
    tr = {}
    out = run_pyref(c, trace=tr)
    kp = tr["kp"]
    H = tr["nrows"]
    cen = dict(NL=len(c["lk"]), NR=len(c["rk"]), V=tr["prune"]["V"],
               kept=int((out[0] >= 0).sum()), reset=tr["prune"].get("reset", 0),
               median=tr["prune"].get("median"), at_th=tr["prune"].get("at_th", 0))
    for k in ("ur_eq_minu", "ur_eq_maxu", "ur_below_minu", "ur_above_maxu", "halves"):
        cen[k] = sum(t.get(k, 0) for t in kp)
    cen["best_dist"] = sorted(set(t["best_dist"] for t in kp if "best_dist" in t))
    cen["row_lens"] = sorted(set(t.get("row_len", 0) for t in kp))
    cen["win_trips"] = sorted(set(t["best_pos"] // 16 for t in kp if t["stage"] != "none"))
    cen["dist_ties"] = sum(t.get("n_tied", 1) > 1 for t in kp if t["stage"] != "none")
    cen["oct"] = sorted(set((t["level"], t["best_oct_delta"]) for t in kp if "level" in t))
    cen["oct_seen"] = sorted(set(d for t in kp for d in t.get("oct_delta", ())))
    cen["border"] = sum(t["stage"] == "border" for t in kp)
    cen["endu_last"] = sum(t.get("endu") == t.get("cols", 0) - 1 for t in kp)
    cen["endu_last_levels"] = sorted(set(t["level"] for t in kp
                                         if t.get("endu") == t.get("cols", 0) - 1))
    cen["sx_10"] = sum(t.get("sx") == 10.0 for t in kp)
    sads = [t["sads"] for t in kp if "sads" in t]
    cen["max_sad"] = max((max(s) for s in sads), default=0)
    cen["big_low"] = sum(v >= 32768 for s in sads for v in s[0::2])    # low half of a packed word
    cen["big_high"] = sum(v >= 32768 for s in sads for v in s[1::2])   # high half
    cen["sad_ties"] = sum(t.get("sad_ties", 1) > 1 for t in kp)
    cen["incs"] = sorted(set(t["inc"] for t in kp if "inc" in t))
    cen["edge_inc"] = sum(t["stage"] == "edge_inc" for t in kp)
    cen["delta_half"] = sum(t.get("delta") == 0.5 for t in kp)
    cen["zero_branch"] = sum(bool(t.get("zero_branch")) for t in kp)
    cen["disp_neg"] = sum(t["stage"] == "disparity" and t["disparity"] < 0 for t in kp)
    cen["disp_ge_maxd"] = sum(t["stage"] == "disparity" and t["disparity"] >= t["maxd"] for t in kp)
    cen["disp_eq_maxd"] = sum(t.get("disparity") == t.get("maxd", -1) for t in kp)
    cen["band_row0"] = sum(lo == 0 for lo, hi in tr["bands"])
    cen["band_last_row"] = sum(hi == H - 1 for lo, hi in tr["bands"])
    cen["band_rows_max"] = max((hi - lo + 1 for lo, hi in tr["bands"]), default=0)
    cen["fill"] = sum(hi - lo + 1 for lo, hi in tr["bands"]) / scratch_capacity(c)
    return cen


# ---------------------------------------------------------------------- cases
def _fillers(sc, n, level=0, y0=100, x0=30, sad0=40):
    """n plain matches (SAD sad0, sad0 + 1, ...) that keep the median positive."""
    return [sc.match(level, x0 + 24 * i, y0, x0 + 24 * i - 4, sad=sad0 + i)[0] for i in range(n)]


def hamming_gates():
    sc = Scene("hamming_gates", EXACT)
    for i, hd in enumerate((73, 74, 75, 76, 99, 100)):
        sc.match(0, 40 + 30 * i, 20, 34 + 30 * i, hd=hd, sad=40 + i, expect=hd < 75)
    # a 75 listed before a 74: the 74 wins, and matches
    d = sc.desc()
    iL = sc.left(60, 50, 0, d)
    sc.right(30, 50, 0, flip_bits(d, 75))
    sc.right(52, 50, 0, flip_bits(d, 74))
    sc.paste(0, 60, 50, 52, 0, 50)
    sc.matched[iL], sc.sad[iL] = True, 50
    _fillers(sc, 3)
    return sc.case()


def u_gates():
    """uR == minU and uR == maxU are candidates, their float neighbours outside
    are not (maxD = 64 exactly; uL = 100 and 200)."""
    sc = Scene("u_gates", EXACT)
    below, above = lambda v: np.nextafter(f32(v), f32(-np.inf)), lambda v: np.nextafter(f32(v), f32(np.inf))
    rows = iter(range(10, 110, 12))
    # (uL, uR, shift that puts the disparity inside [0, 64), expected)
    for uL, uR, inc, ok in ((100, f32(36), 2, True), (100, below(36), 2, False),
                            (100, f32(100), -2, True), (100, above(100), -2, False),
                            (200, f32(136), 3, True), (200, below(136), 3, False),
                            (200, f32(200), -3, True), (200, above(200), -3, False)):
        y = next(rows)
        d = sc.desc()
        iL = sc.left(uL, y, 0, d)
        sc.right(uR, y, 0, flip_bits(d, 12))
        sc.paste(0, uL, y, int(pyref._roundf(uR)), inc, 40 + iL)
        sc.matched[iL] = ok
        if ok:
            sc.sad[iL] = 40 + iL
    return sc.case()


def u_gates_kitti():
    """The same with the KITTI intrinsics, where maxD = bf / (bf / fx) rounds:
    a 1000 x 40 level 0, uL = 900."""
    sc = Scene("u_gates_kitti", KITTI, w=1000, h=40)
    mb = f32(S.BF) / f32(S.FX)
    maxD = f32(S.BF) / mb
    uL = f32(900.0)
    minU = uL - maxD
    for j, (uR, ok) in enumerate(((minU, True), (np.nextafter(minU, f32(-np.inf)), False))):
        y = 12 + 14 * j
        d = sc.desc()
        iL = sc.left(uL, y, 0, d)
        sc.right(uR, y, 0, flip_bits(d, 12))
        sc.paste(0, 900, y, int(pyref._roundf(uR)), 3, 40 + j)   # disparity about maxD - 3
        sc.matched[iL] = ok
    iL, _ = sc.match(0, 500, 12, 480, sad=41)
    return sc.case()


def octave_gates():
    sc = Scene("octave_gates")
    for lvl, roct in ((0, 0), (0, 1), (0, 2), (7, 7), (7, 6), (7, 5), (3, 1), (3, 2), (3, 4),
                      (3, 5), (1, 0), (6, 7)):
        lw, lh = sc.sizes[lvl]
        n = sum(1 for k in sc.lk if k[2] == lvl)
        xl = 24 + 20 * n
        yl = lh // 2
        sc.match(lvl, xl, yl, xl - 6, roct=roct, sad=40 + len(sc.lk), expect=abs(roct - lvl) <= 1)
    return sc.case()


def row_lists():
    """Row lists of 1, 16, 17 and 200 candidates (one and several trips of the
    16-lane loop), the winner in the first, a middle and the last trip, and equal
    best distances inside a trip and across trips (the smaller iR wins)."""
    sc = Scene("row_lists")
    # (row, list length, winner position, tie partner position or None)
    plan = ((8, 1, 0, None), (20, 16, 15, None), (32, 17, 16, None), (44, 17, 3, 16),
            (56, 200, 5, None), (68, 200, 100, 190), (80, 200, 199, None), (92, 200, 17, 18),
            (104, 16, 2, 9))
    for y, n, win, tie in plan:
        d = sc.desc()
        xl = 150
        iL = sc.left(xl, y, 0, d)
        xs = np.linspace(12, 140, n).astype(f32) if n > 1 else np.array([100], f32)
        for j in range(n):
            if j == win or j == tie:
                sc.right(xs[j], y, 0, flip_bits(d, 30))
            else:
                sc.right(xs[j], y, 0, flip_bits(d, 31 + (j % 40)))
        sc.paste(0, xl, y, int(pyref._roundf(xs[win])), 0, 40 + iL)
        sc.matched[iL] = True
        sc.sad[iL] = 40 + iL
    return sc.case()


def bands():
    sc = Scene("bands")
    # level 0, r = 2: y -+ r integral; the left row on the first and last band
    # row, and one row outside each
    for j, dy in enumerate((-3, -2, 2, 3)):
        sc.match(0, 30 + 40 * j, 20, 24 + 40 * j, dy=float(dy), sad=40 + j, expect=abs(dy) <= 2)
    # octave 2, y = 50.3: band [47, 54].  Left rows 47, 46 (out), 54.99 -> 54 (in:
    # truncated, not rounded) and 55 (out), on level 1 with fractional y
    for j, (vl, ok) in enumerate(((47.0, True), (46.99, False), (54.99, True), (55.0, False))):
        d = sc.desc()
        xs = 30 + 40 * j
        iL = sc.left(level0(1, xs), vl, 1, d)
        sc.right(level0(1, xs - 6), 50.3, 2, flip_bits(d, 9))
        sc.paste(1, xs, int(pyref._roundf(f32(vl) * INV[1])), xs - 6, 0, 44 + j)
        sc.matched[iL] = ok
    # a band whose first row is 0 and one whose last row is H - 1 (octave 1,
    # r = 2.4), each with a level-0 left keypoint on its far row
    sc.match(0, 200, 5, 190, roct=1, y=5.0, dy=-2.5, sad=48)
    sc.match(0, 240, 114, 230, roct=1, y=114.0, dy=2.5, sad=49)
    _fillers(sc, 2, y0=80)
    return sc.case()


def border():
    sc = Scene("border")
    # level 0: round(uR0) + 11 == cols - 1 kept, == cols dropped
    sc.match(0, 314, 20, 308, sad=40)
    sc.match(0, 314, 40, 309, sad=41, expect=False, paste=False)
    # level 2 (222 wide) and level 5 (129 wide) with their own widths
    for lvl, y in ((2, 20), (5, 20)):
        lw = sc.sizes[lvl][0]
        sc.match(lvl, lw - 6, y, lw - 12, sad=42 + lvl)
        sc.match(lvl, lw - 6, y + 14, lw - 11, sad=43 + lvl, expect=False, paste=False)
    # scaled x exactly 10, levels 0 and 3
    sc.match(0, 30, 60, 10, sad=50)
    sc.match(3, 30, 40, 10, sad=51)
    # x * inv exactly at .5 (level 0) for uL, vL and uR0: away from zero
    d = sc.desc()
    iL = sc.left(100.5, 80, 0, d)
    sc.right(80.0, 80, 0, flip_bits(d, 5))
    sc.paste(0, 101, 80, 80, 0, 52)
    sc.matched[iL], sc.sad[iL] = True, 52
    d = sc.desc()
    iL = sc.left(150, 80.5, 0, d)
    sc.right(130.0, 80.5, 0, flip_bits(d, 5))
    sc.paste(0, 150, 81, 130, 0, 53)
    sc.matched[iL], sc.sad[iL] = True, 53
    d = sc.desc()
    iL = sc.left(200, 100, 0, d)
    sc.right(180.5, 100, 0, flip_bits(d, 5))
    sc.paste(0, 200, 100, 181, 0, 54)
    sc.matched[iL], sc.sad[iL] = True, 54
    return sc.case()


def _stripes(sc, level, phase):
    lw, lh = sc.sizes[level]
    col = (((np.arange(lw) + phase) & 1) * 255).astype(np.uint8)
    return np.tile(col, (lh, 1))


def sad_magnitudes():
    """SADs of 2^15 and more in the low and in the high halves of the packed
    words, up to 60,180 (the bound for any window pair is 120 * 510 = 61,200)."""
    sc = Scene("sad_magnitudes")
    # level 0: column-parity stripes, left = right.  The 11 SADs alternate
    # 66 * 510 = 33,660 (odd shifts) and 0; the five even shifts tie and the
    # first, -4, wins
    sc.lpyr[0], sc.rpyr[0] = _stripes(sc, 0, 0), _stripes(sc, 0, 0)
    d = sc.desc()
    a = sc.left(100, 20, 0, d)
    sc.right(90.0, 20, 0, flip_bits(d, 7))
    sc.matched[a] = True
    # level 1: the same with the right keypoint one column over, so the even
    # shifts are the large ones (high halves); a pixel that only the window of
    # shift -5 holds makes -3 the strict first minimum
    sc.lpyr[1], sc.rpyr[1] = _stripes(sc, 1, 0), _stripes(sc, 1, 0)
    d = sc.desc()
    b = sc.left(level0(1, 100), level0(1, 20), 1, d)
    sc.right(level0(1, 89), level0(1, 20), 1, flip_bits(d, 7))
    sc.rpyr[1][17, 89 - 10] ^= 255
    sc.matched[b] = True
    # level 2: left window 255 with centre 0; right rows 0 with the centre row
    # 255 and one centre-row pixel 254 (shift +1).  SADs 58,651 / 58,530 at that
    # shift / 58,650 where the window misses the pixel: 2^15 in both halves, and
    # read as signed 16 bit the odd words' values would win
    sc.lpyr[2][:28, :] = 255
    sc.lpyr[2][14, 100] = 0
    sc.rpyr[2][:28, :] = 0
    sc.rpyr[2][14, :] = 255
    sc.rpyr[2][14, 91] = 254
    d = sc.desc()
    e = sc.left(level0(2, 100), level0(2, 14), 2, d)
    sc.right(level0(2, 90), level0(2, 14), 2, flip_bits(d, 7))
    sc.matched[e], sc.sad[e] = True, 58530
    # level 3: the same left window; right centre row 255 / 0 by column parity,
    # other rows 0.  SADs alternate 60,180 (centre 255) and 29,070; -4 is first
    sc.lpyr[3][:28, :] = 255
    sc.lpyr[3][14, 100] = 0
    sc.rpyr[3][:28, :] = 0
    sc.rpyr[3][14, :] = ((np.arange(sc.sizes[3][0]) & 1) * 255).astype(np.uint8)
    d = sc.desc()
    g = sc.left(level0(3, 100), level0(3, 14), 3, d)
    sc.right(level0(3, 90), level0(3, 14), 3, flip_bits(d, 7))
    sc.matched[g], sc.sad[g] = True, 29070
    # level 4: dist3 == dist2, deltaR exactly 0.5: two centre-row pixels at 254
    sc.lpyr[4][:28, :] = 255
    sc.lpyr[4][14, 100] = 0
    sc.rpyr[4][:28, :] = 0
    sc.rpyr[4][14, :] = 255
    sc.rpyr[4][14, 90:92] = 254
    d = sc.desc()
    k = sc.left(level0(4, 100), level0(4, 14), 4, d)
    sc.right(level0(4, 90), level0(4, 14), 4, flip_bits(d, 7))
    sc.matched[k], sc.sad[k] = True, 58531
    s = SCALE[4] * ((f32(90) + f32(0)) + f32(0.5))
    sc.exact[k] = (s, f32(S.BF) / (level0(4, 100) - s))
    return sc.case()


def shifts():
    """Best shift at -L and +L (rejected) and at -4 / +4 (accepted)."""
    sc = Scene("shifts")
    for j, inc in enumerate((-5, -4, 4, 5)):
        for lvl, y in ((0, 20), (2, 20)):
            sc.match(lvl, 40 + 44 * j, y, 26 + 44 * j, inc=inc, sad=40 + j + lvl,
                     expect=abs(inc) < 5)
    _fillers(sc, 2, y0=60)
    return sc.case()


def _triangle(lw, lh, centre, amp=8):
    x = np.arange(lw)
    row = np.abs(((x - centre) % 32) - 16) * amp
    return np.tile(row.astype(np.uint8), (lh, 1))


def disparity():
    """A triangle wave in x (period 32, left = right): about a crest every SAD
    is symmetric in the shift, so deltaR = 0 exactly.  maxD = 64."""
    sc = Scene("disparity", EXACT)
    sc.lpyr[0], sc.rpyr[0] = _triangle(W0, H0, 100), _triangle(W0, H0, 100)

    def pair(uL, uR, y, ok):
        d = sc.desc()
        iL = sc.left(uL, y, 0, d)
        sc.right(uR, y, 0, flip_bits(d, 6))
        sc.matched[iL] = ok
        return iL
    # same x: disparity 0 -> 0.01f, uR = (float)((double)uL - 0.01)
    z = pair(148.0, 148.0, 12, True)
    sc.exact[z] = (f32(np.float64(f32(148.0)) - 0.01), f32(32.0) / f32(0.01))
    sc.sad[z] = 0
    # the shift -1 window made worse than +1: deltaR > 0, disparity < 0
    pair(212.0, 212.0, 28, False)
    sc.rpyr[0][25, 212 - 6] += 40
    # uR0 == minU: disparity == maxD exactly (rejected), one float below (kept)
    pair(100.0, 36.0, 44, False)
    k = pair(np.nextafter(f32(100.0), f32(0)), 36.0, 60, True)
    sc.exact[k] = (f32(36.0), f32(32.0) / (np.nextafter(f32(100.0), f32(0)) - f32(36.0)))
    # disparity 32 between two crests, with SADs 50.. that keep the median positive
    for j in range(4):
        y = 76 + 10 * j if j < 3 else 112
        iL = pair(244.0, 212.0, y, True)
        v = int(sc.rpyr[0][y - 3, 214])
        sc.rpyr[0][y - 3, 214] = v + 50 + j
        sc.sad[iL] = 50 + j
    return sc.case()


def _prune_case(name, sads, nl_extra=0, expect=None):
    sc = Scene(name)
    ids = []
    for j, s in enumerate(sads):
        ids.append(sc.match(0, 30 + 26 * (j % 11), 10 + 14 * (j // 11), 24 + 26 * (j % 11), sad=s,
                            expect=None)[0])
    for j in range(nl_extra):   # left keypoints without a candidate
        sc.left(20 + (j % 29) * 10, 70 + (j // 29) * 4, 0)
    for iL, s, m in zip(ids, sads, expect if expect is not None else [None] * len(sads)):
        sc.sad[iL] = s
        if m is not None:
            sc.matched[iL] = m
    return sc


def prune_v0():
    sc = Scene("prune_v0")
    for j in range(3):
        sc.match(0, 30 + 30 * j, 20, 24 + 30 * j, hd=80, expect=False, paste=False)
    return sc.case()


def prune_v1():
    return _prune_case("prune_v1", [40], expect=[True]).case()


def prune_v1_zero():
    return _prune_case("prune_v1_zero", [0], expect=[False]).case()


def prune_v2():
    """Median = the upper of the two (index V / 2): 30, threshold 63."""
    return _prune_case("prune_v2", [10, 30], expect=[True, True]).case()


def prune_v3():
    return _prune_case("prune_v3", [10, 12, 50], expect=[True, True, False]).case()


def prune_median0():
    """Median 0: thDist 0, and no SAD is < 0, so every match is reset."""
    return _prune_case("prune_median0", [0, 0, 0, 40], expect=[False] * 4).case()


def prune_threshold():
    """Median 10: thDist = 1.5f * 1.4f * 10 = 21.0f exactly (the product
    20.99999905 is a tie between two floats and rounds to even), so 21 is reset
    and 20 kept."""
    return _prune_case("prune_threshold", [5, 8, 10, 20, 21],
                       expect=[True, True, True, True, False]).case()


def prune_strided():
    """NL = 300 with five matches, at indices 0, 255, 256, 257 and 299: the
    prune's 256-thread strided loops."""
    sc = Scene("prune_strided")
    at = {0: 10, 255: 12, 256: 30, 257: 11, 299: 13}
    j = 0
    for i in range(300):
        if i in at:
            iL, _ = sc.match(0, 40 + 50 * j, 20, 30 + 50 * j, sad=at[i], expect=at[i] != 30)
            j += 1
        else:
            sc.left(20 + (i % 29) * 10, 50 + (i // 29) * 6, 0)
    return sc.case()


def counts_case(nl, nr_extra=0, nr_matching=None):
    """nl left keypoints on a grid, the first nr_matching with their right
    keypoint; nr_extra further right keypoints that match nothing."""
    sc = Scene("counts_%d_%d_%s" % (nl, nr_extra, nr_matching), seed=nl + 1)
    nm = nl if nr_matching is None else nr_matching
    for i in range(nl):
        xl, yl = 18 + 16 * (i % 18), 6 + 12 * (i // 18)
        if i < nm:
            sc.match(0, xl, yl, xl - 3, sad=40 + i % 30, expect=None)
        else:
            sc.left(xl, yl, 0)
    for j in range(nr_extra):
        sc.right(12 + (j * 7) % 290, 4 + (j * 5) % 110, (j % 3))
    return sc.case()


COUNTS_NL = (1, 15, 16, 17, 63, 64, 65)


def counts_nr0():
    return counts_case(5, 0, 0)


def counts_nr_many():
    return counts_case(3, 400)


def counts_nl_many():
    return counts_case(160, 0, 2)


def capacity():
    """NR == the stride, every right keypoint at octave 7 with y - r just below
    an integer, so each band has 17 rows of the 18 the scratch rule allows."""
    sc = Scene("capacity")
    r = f32(2.0) * SCALE[7]
    # four matches at level 7 and four at level 6, right keypoints at octave 7
    n = 0
    for lvl in (7, 6):
        for j in range(4):
            xl = 24 + 14 * j
            yl = 10 + 3 * (j % 2) if lvl == 7 else 14 + 4 * (j % 2)
            sc.match(lvl, xl, yl, xl - 4, roct=7, sad=40 + n)
            n += 1
    while len(sc.rk) < 64:
        j = len(sc.rk)
        sc.right(40 + 4 * j, 10 + (j * 13) % 100, 7)
    # slide every right y so that frac(y - r) = 0.8 (17 rows), keeping its row
    for i, (x, y, o) in enumerate(sc.rk):
        base = math.floor(float(f32(y) - r))
        sc.rk[i] = (x, f32(f32(base) + f32(0.8) + r), o)
    return sc.case()


def tiny():
    """One left and one right keypoint (the in-between call of the GPU test)."""
    sc = Scene("tiny", seed=9)
    sc.match(0, 60, 30, 50, sad=40)
    return sc.case()


# name -> (builder, census minimum: key -> lower bound, or a set that must be covered)
CASES = {
    "hamming_gates": (hamming_gates, dict(best_dist={73, 74, 75, 76}, kept=5)),
    "u_gates": (u_gates, dict(ur_eq_minu=2, ur_eq_maxu=2, ur_below_minu=2, ur_above_maxu=2,
                              kept=4)),
    "u_gates_kitti": (u_gates_kitti, dict(ur_eq_minu=1, ur_below_minu=1, kept=2)),
    "octave_gates": (octave_gates, dict(oct={(0, 0), (0, 1), (7, 0), (7, -1), (3, -1), (3, 1), (1, -1),
                                             (6, 1)}, oct_seen={-2, -1, 0, 1, 2}, kept=8)),
    "row_lists": (row_lists, dict(row_lens={1, 16, 17, 200}, win_trips={0, 1, 6, 12},
                                  dist_ties=4, kept=9)),
    "bands": (bands, dict(band_row0=1, band_last_row=1, kept=8)),
    "border": (border, dict(border=3, endu_last=3, endu_last_levels={0, 2, 5}, sx_10=2,
                            halves=3, kept=8)),
    "sad_magnitudes": (sad_magnitudes, dict(max_sad=60180, big_low=10, big_high=10, sad_ties=3,
                                            delta_half=1, kept=5)),
    "shifts": (shifts, dict(incs={-5, -4, 4, 5}, edge_inc=4, kept=6)),
    "disparity": (disparity, dict(zero_branch=1, disp_neg=1, disp_ge_maxd=1, disp_eq_maxd=1,
                                  kept=6)),
    "prune_v0": (prune_v0, dict(V=0)),
    "prune_v1": (prune_v1, dict(V=1, kept=1)),
    "prune_v1_zero": (prune_v1_zero, dict(V=1, reset=1)),
    "prune_v2": (prune_v2, dict(V=2, kept=2)),
    "prune_v3": (prune_v3, dict(V=3, reset=1)),
    "prune_median0": (prune_median0, dict(V=4, reset=4)),
    "prune_threshold": (prune_threshold, dict(V=5, at_th=1, reset=1)),
    "prune_strided": (prune_strided, dict(NL=300, V=5, reset=1)),
    "counts_nr0": (counts_nr0, dict(NL=5)),
    "counts_nr_many": (counts_nr_many, dict(NR=403, kept=3)),
    "counts_nl_many": (counts_nl_many, dict(NL=160, kept=2)),
    "capacity": (capacity, dict(band_rows_max=17, fill=0.9, kept=8)),
    "tiny": (tiny, dict(kept=1)),
}
for _n in COUNTS_NL:
    CASES["counts_nl_%d" % _n] = ((lambda n=_n: counts_case(n)), dict(NL=_n, kept=max(1, _n // 2)))
# census values that must equal the minimum (not merely reach it)
EXACT_KEYS = ("V", "NL", "NR")
