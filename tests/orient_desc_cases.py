"""Directed frames for IC_Angle, the blur's clamp and rBRIEF (k_orient_desc),
shared by the CPU and GPU tests (test infrastructure).

The unit is a stamp: one 255 pixel on a 0 field.  All 16 pixels of its FAST
ring are darker, so it is a corner, the only one near it, and the keypoint
sits exactly on it; its own contribution to the IC_Angle moments is zero
(u = v = 0).  "Weight" pixels of value <= 6 inside the 31-px patch then set
the moments to any small target: they are below minThFAST = 7 against the 0
field, so they are no corners themselves.  A weight of value w at patch
offset (u, v) adds u * w to m_10 and v * w to m_01 (src/ORBextractor.cc:77-110).
In inverse polarity (field 255, dot 0, weights 255 - w) the uniform field
contributes nothing by symmetry and the same weights give the negated target.

Every case carries tags; tests/test_orient_desc_cases.py shows on the CPU,
with the restatement of tests/orient_desc_ref.py on the oracle's keypoints,
that each case holds what its tags claim, and the GPU tests assert the same
census before they compare.
"""
import numpy as np

import orient_desc_ref as odr

W, H = 400, 300
NF, SF, NL, INI_TH, MIN_TH = 1000, 1.2, 8, 20, 7
K = 12                     # the moment magnitude of the axis and diagonal stamps
STEP, EDGE = 44, 40        # stamps at least 44 px apart and 40 px from the frame edge
SLOTS = [(EDGE + STEP * i, EDGE + STEP * j) for j in range((H - 2 * EDGE) // STEP + 1)
         for i in range((W - 2 * EDGE) // STEP + 1)]   # 8 x 6

# the circular patch of IC_Angle: (u, v) with |u| <= umax[|v|]
PATCH = [(u, v) for v in range(-15, 16) for u in range(-odr.UMAX[abs(v)], odr.UMAX[abs(v)] + 1)]
# the largest m_10 weights of value <= 6 allow: every patch pixel right of the
# centre column at 6 (rows +v and -v cancel in m_01)
M = 6 * sum(u for u, _ in PATCH if u > 0)


def _axis_weight(k):
    """(offset, value) with offset * value == k, 4 <= offset <= 15 (clear of
    the FAST ring), 1 <= value <= 6."""
    for a in range(15, 3, -1):
        if k % a == 0 and 1 <= k // a <= 6:
            return a, k // a
    raise ValueError(k)


def _weights(m01, m10):
    """Weight pixels [(u, v, value)] whose moments are exactly (m01, m10)."""
    out = []
    if abs(m10) == M:
        out += [(u, v, 6) for u, v in PATCH if u > 0]
    elif m10:
        a, w = _axis_weight(abs(m10))
        out.append((a if m10 > 0 else -a, 0, w))
    if abs(m01) == 1:
        out.append((0, m01, 1))
    elif m01:
        a, w = _axis_weight(abs(m01))
        out.append((0, a if m01 > 0 else -a, w))
    assert sum(v * w for _, v, w in out) == m01 and sum(u * w for u, _, w in out) == m10
    return out


def moment_targets():
    """[(m01, m10)] of the moments cases, level 0."""
    k = K
    t = [(0, 0), (0, k), (0, -k), (k, 0), (-k, 0)]
    t += [(sy * k, sx * k) for sy in (1, -1) for sx in (1, -1)]
    t += [(sy * k, sx * (k + 1)) for sy in (1, -1) for sx in (1, -1)]
    t += [(sy * (k + 1), sx * k) for sy in (1, -1) for sx in (1, -1)]
    t += [(1, M), (-1, M)]
    return t


# slots of the 19 moment stamps: spread over the frame, so that every octree
# split separates some of them and none is dropped
_MOMENT_SLOTS = [(5 * i) % len(SLOTS) for i in range(19)]


def _moments_image(white):
    img = np.zeros((H, W), np.int64)
    stamps = []
    for slot, (m01, m10) in zip(_MOMENT_SLOTS, moment_targets()):
        x, y = SLOTS[slot]
        for u, v, w in _weights(m01, m10):
            img[y + v, x + u] = w
        img[y, x] = 255
        stamps.append(dict(x=x, y=y, target=(-m01, -m10) if white else (m01, m10)))
    if white:
        img = 255 - img
    return img.astype(np.uint8), stamps


def _binary_blocks(seed=3, b=4):
    rng = np.random.default_rng(seed)
    a = (rng.integers(0, 2, (-(-H // b), -(-W // b))) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.kron(a, np.ones((b, b), np.uint8))[:H, :W])


NOISE_SEED = 12   # seeds 0 .. 4 give no tie at this size, 12 gives 7


def _noise(seed=None):
    rng = np.random.default_rng(NOISE_SEED if seed is None else seed)
    return rng.integers(0, 256, (H, W), np.uint8)


CONES = [(101, 93), (287, 111)]
SPARSE_DOTS = [(19, 19, 255), (330, 250, 8)]


def _sparse_levels():
    """Cone blobs max(0, 120 - 2 r): their slope of 2 per pixel is below
    minThFAST over the 3-px FAST ring until the pyramid has steepened it.  Two
    dots are keypoints on level 0 only: one at (19, 19), the first pixel a
    keypoint can take, which every coarser level leaves outside its border,
    and one inside the frame of value 8, a corner at minThFAST that the first
    resize takes below it (a 255 dot stays a corner down to level 4)."""
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.zeros((H, W), np.int64)
    for cx, cy in CONES:
        r = np.sqrt((xx - cx) ** 2 + (yy - cy) ** 2)
        img = np.maximum(img, np.maximum(0, 120 - 2 * r).astype(np.int64))
    for x, y, v in SPARSE_DOTS:
        img[y, x] = v
    return img.astype(np.uint8)


COUNTS = (1, 2, 3, 7, 8, 9, 31, 32, 33)


def _interleave(slots, x0, x1, y0, y1):
    """The slots of box [x0, x1) x [y0, y1) in an order whose every prefix is
    spread evenly over the four children DivideNode would make of the box
    (src/ORBextractor.cc:504-560), and so on down: round-robin over the
    children's own orders."""
    if len(slots) <= 1:
        return list(slots)
    mx, my = x0 + -(-(x1 - x0) // 2), y0 + -(-(y1 - y0) // 2)
    boxes = [(x0, mx, y0, my), (mx, x1, y0, my), (x0, mx, my, y1), (mx, x1, my, y1)]
    kids = [_interleave([s for s in slots if b[0] <= SLOTS[s][0] < b[1] and b[2] <= SLOTS[s][1] < b[3]],
                        *b) for b in boxes]
    out = []
    for i in range(max(len(k) for k in kids)):
        out += [k[i] for k in kids if i < len(k)]
    return out


# slot order of the count_n dots.  The reference's octree stops when a pass of
# splits does not grow its node list, so two dots that a split leaves together
# can come back as one; with this order every node that holds two or more dots
# has them in at least two of its children (16 is the FAST border the octree's
# root box starts at).
_COUNT_ORDER = _interleave(range(len(SLOTS)), 16, W - 16, 16, H - 16)


def _count_order():
    return _COUNT_ORDER


def _count_image(n):
    """n dots on a field of noise in 0 .. 6 (below minThFAST, so no corners of
    its own), which gives every dot moments and a descriptor of its own."""
    rng = np.random.default_rng(100 + n)
    img = rng.integers(0, 7, (H, W), np.uint8)
    dots = [SLOTS[s] for s in _count_order()[:n]]
    for x, y in dots:
        img[y, x] = 255
    return img, dots


class Case:
    def __init__(self, name, img, tags, nl=NL, nf=NF, stamps=None):
        img = np.ascontiguousarray(img, np.uint8)
        img.setflags(write=False)
        self.name, self.img, self.tags, self.nl, self.nf = name, img, frozenset(tags), nl, nf
        self.stamps = stamps or []

    @property
    def params(self):
        return (self.nf, SF, self.nl, INI_TH, MIN_TH)

    def __repr__(self):
        return f"Case({self.name})"


_cases = None


def cases():
    """{name: Case}, built once per process."""
    global _cases
    if _cases is None:
        out = []
        dark, stamps = _moments_image(False)
        out.append(Case("moments_dark", dark, {"moments"}, stamps=stamps))
        out.append(Case("moments_dark_1level", dark, {"moments"}, nl=1, stamps=stamps))
        white, stamps = _moments_image(True)
        out.append(Case("moments_white", white, {"moments", "presat", "clamp_bits"}, stamps=stamps))
        out.append(Case("binary_blocks", _binary_blocks(), {"presat", "clamp_bits", "equal_every_level"}))
        out.append(Case("noise_ties", _noise(), {"ties"}))
        out.append(Case("sparse_levels", _sparse_levels(), {"empty_level", "odd_level"}))
        for n in COUNTS:
            img, dots = _count_image(n)
            out.append(Case(f"count_{n}", img, {"count"}, nl=1,
                            stamps=[dict(x=x, y=y, target=None) for x, y in dots]))
        out.append(Case("flat", np.full((H, W), 128, np.uint8), {"flat"}))
        _cases = {c.name: c for c in out}
    return _cases


EIGHT_LEVEL = ("moments_dark", "moments_white", "binary_blocks", "noise_ties", "sparse_levels")
COUNT_CASES = tuple(f"count_{n}" for n in COUNTS)


def white_field(w=403, h=301):
    """A white frame of odd size with three 0 dots: the blur of every level
    reaches 256 / 257 before its clamp."""
    img = np.full((h, w), 255, np.uint8)
    for x, y in ((60, 60), (w - 70, 90), (w // 2, h - 60)):
        img[y, x] = 0
    return img


# --------------------------------------------------------- oracle and census
_oracle_cache = {}


def case_oracle(oracle, name):
    """(image, keypoints, descriptors, per-level counts) of a case from the
    oracle, computed once per process, read-only."""
    if name not in _oracle_cache:
        c = cases()[name]
        k, d, per = oracle.extract(c.img, *c.params)
        for a in (k, d, per):
            a.setflags(write=False)
        _oracle_cache[name] = (c.img, k, d, per)
    return _oracle_cache[name]


_restate_cache = {}


def case_restated(oracle, name):
    """(angles, descriptors, traces) of orient_desc_ref.restate on the oracle's
    keypoints and pyramid of a case, once per process."""
    if name not in _restate_cache:
        c = cases()[name]
        img, k, _, _ = case_oracle(oracle, name)
        levels = oracle.pyramid(img, SF, c.nl)
        scale = oracle.params(c.nf, SF, c.nl)["scale"]
        _restate_cache[name] = odr.restate(levels, k, scale)
    return _restate_cache[name]


def assert_census(oracle, name):
    """What the tags of case `name` claim, shown on the oracle's output alone
    (every threshold is "at least one")."""
    c = cases()[name]
    _, keys, _, per = case_oracle(oracle, name)
    per = per.tolist()
    if "flat" in c.tags:
        assert len(keys) == 0 and per == [0] * c.nl, (name, per)
        return
    _, _, traces = case_restated(oracle, name)
    total = odr.census(traces)
    at = {(t["x"], t["y"]): (t, keys["angle"][i]) for i, t in enumerate(traces) if t["level"] == 0}
    if "moments" in c.tags:
        k = K
        exact = {(0, 0): 0.0, (0, k): 0.0, (k, 0): 90.0, (0, -k): 180.0, (-k, 0): 270.0}
        quadrants = set()
        for s in c.stamps:
            assert (s["x"], s["y"]) in at, (name, s)   # one keypoint exactly on the stamp
            t, angle = at[(s["x"], s["y"])]
            assert (t["m01"], t["m10"]) == s["target"], (name, s, t)
            quadrants.add(t["k"])
            if s["target"] in exact:
                assert angle == np.float32(exact[s["target"]]), (name, s, angle)
            if s["target"] == (-1, M):
                assert 359.5 < angle < 360.0 and t["k"] == 4, (name, s, angle, t["k"])
        assert {0, 1, 2, 3} <= quadrants, (name, quadrants)   # every branch of the A.6 quadrant switch
    if "presat" in c.tags:
        assert total["n_presat"] > 0, (name, total)
    if "clamp_bits" in c.tags:
        assert total["n_clamp_bits"] > 0, (name, total)
    if "equal_every_level" in c.tags:
        for l in range(c.nl):
            assert sum(t["n_equal"] for t in traces if t["level"] == l) > 0, (name, l)
    if "ties" in c.tags:
        assert total["n_ties"] > 0, (name, total)
    if "empty_level" in c.tags:
        assert any(per[l] == 0 and any(per[:l]) and any(per[l + 1:]) for l in range(c.nl)), (name, per)
        for x, y, _ in SPARSE_DOTS:
            assert (x, y) in at, (name, x, y)
    if "odd_level" in c.tags:
        assert any(per[l] % 2 == 1 and any(per[l + 1:]) for l in range(c.nl)), (name, per)
    if "count" in c.tags:
        assert per == [len(c.stamps)], (name, per)
        assert sorted(at) == sorted((s["x"], s["y"]) for s in c.stamps), name
