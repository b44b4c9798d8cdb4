"""CPU checks of the orientation / rBRIEF restatement and its directed frames.

tests/orient_desc_ref.py states IC_Angle and computeOrbDescriptor
(src/ORBextractor.cc:77-164) a second time; here it must give, for every
keypoint the oracle returns, the oracle's angle as float32 and all 32
descriptor bytes -- on every directed case of tests/orient_desc_cases.py, on
a stock synthetic frame and on two border images -- and the census of every
case must show what its tags claim on the oracle's output alone, so that the
GPU comparison of tests/test_gpu_orient_desc_edges.py stands on inputs that
hold their edge.  No tolerances: every comparison is exact, every census
threshold is "at least one".  No GPU needed.

Census of the oracle's output, for comparison after a change of inputs
(per-level counts; n_ties, n_presat, n_clamp_bits, n_equal over the frame):

  moments_dark         [19, 19, 19, 18, 16, 10, 8, 1]       0      0     0  24050
  moments_dark_1level  [19]                                 0      0     0   4168
  moments_white        [19, 19, 19, 18, 16, 10, 8, 1]       0  52830  1281  26229
  binary_blocks        [49, 181, 151, 127, 106, 88, 74, 62] 0    982     5   1776
  noise_ties           [217, 181, 151, 127, 106, 87, 73, 42] 7     0     0  10788
  sparse_levels        [2, 0, 1, 0, 1, 1, 0, 2]             0      0     0    501
  count_n              [n] for n in 1, 2, 3, 7, 8, 9, 31, 32, 33
  flat                 [0, 0, 0, 0, 0, 0, 0, 0]
"""
import numpy as np
import pytest

import border_cases as bc
import orient_desc_cases as oc
import orient_desc_ref as odr
import pyref

ALL = list(oc.cases())


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _agree(keys, desc, angles, rdesc, what):
    bad = np.nonzero(_bits(angles) != _bits(keys["angle"]))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} angles differ, first keypoint {bad[0]}: "
                           f"oracle {keys[bad[0]]} restated {angles[bad[0]]!r}")
    bad = np.nonzero((rdesc != desc).any(1))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} descriptors differ, first keypoint {bad[0]}: "
                           f"{keys[bad[0]]}, {int(np.unpackbits(rdesc[bad[0]] ^ desc[bad[0]]).sum())} bits")


# ------------------------------------------------------------- the pieces
def test_umax_by_the_reference_formula(oracle):
    assert odr.UMAX == oracle.params()["umax"].tolist()
    assert len(oc.PATCH) == 749


@pytest.mark.parametrize("name", ["moments_white", "binary_blocks", "noise_ties"])
def test_blur_unclamped_clamps_to_blur7(oracle, name):
    img = oc.cases()[name].img
    for l, lv in enumerate(oracle.pyramid(img, oc.SF, oc.NL)):
        raw = odr.blur_unclamped(lv)
        assert raw.dtype == np.int64 and raw.min() >= 0
        assert np.array_equal(np.minimum(raw, 255), pyref.blur7(lv)), (name, l)
        assert np.array_equal(pyref.blur7(lv), oracle.blur7(lv)), (name, l)


def test_white_field_blurs_past_255():
    """The integer kernel sums to 257 per axis: a white field is 257 before the clamp."""
    assert sum(pyref.gaussian_kernel_int()) == 257
    raw = odr.blur_unclamped(np.full((40, 50), 255, np.uint8))
    assert raw.min() == raw.max() == (255 * 257 * 257 + (1 << 15)) >> 16 == 257


def test_pinned_sincos_is_the_oracles(oracle):
    deg = np.concatenate([np.arange(0, 361, 15, dtype=np.float32),
                          np.float32([359.5, 359.99, np.nextafter(np.float32(360), np.float32(0)),
                                      44.999996, 45.000004, 89.99999, 90.00001, 0.0036, 179.99, 180.01]),
                          np.random.default_rng(0).uniform(0, 360, 500).astype(np.float32)])
    ks = set()
    for d in deg:
        rad = np.float32(d * odr.FACTOR_PI)
        s, c, k = odr.pinned_sincos(rad)
        so, co = oracle.sincos(float(rad))
        assert _bits(s) == _bits(np.float32(so)) and _bits(c) == _bits(np.float32(co)), d
        ks.add(k)
    assert ks == {0, 1, 2, 3, 4}
    assert odr.FACTOR_PI == np.float32(np.pi / 180)


def test_moment_weights_hit_their_targets():
    """The weights of every stamp give its target exactly, stay inside the
    patch and below minThFAST; the stamps keep their distances."""
    t = oc.moment_targets()
    assert len(t) == len(set(t)) == 19
    for m01, m10 in t:
        ws = oc._weights(m01, m10)
        assert all((u, v) in oc.PATCH and (u, v) != (0, 0) and 1 <= w < oc.MIN_TH for u, v, w in ws)
    assert oc.M == 14688
    for name in ("moments_dark", "moments_white") + oc.COUNT_CASES:
        pts = [(s["x"], s["y"]) for s in oc.cases()[name].stamps]
        assert len(set(pts)) == len(pts)
        for i, (x, y) in enumerate(pts):
            assert oc.EDGE <= x <= oc.W - oc.EDGE and oc.EDGE <= y <= oc.H - oc.EDGE
            assert all(max(abs(x - a), abs(y - b)) >= oc.STEP for a, b in pts[:i])


# ------------------------------------------- restatement against the oracle
@pytest.mark.parametrize("name", ALL)
def test_restatement_equals_oracle_on_case(oracle, name):
    _, keys, desc, _ = oc.case_oracle(oracle, name)
    if name == "flat":
        assert len(keys) == 0
        return
    angles, rdesc, traces = oc.case_restated(oracle, name)
    assert len(keys) > 0
    _agree(keys, desc, angles, rdesc, name)
    assert all(t["reach"] <= 18 for t in traces)   # samples stay inside the 37 x 37 window


def test_restatement_equals_oracle_on_stock_frame(oracle):
    img = oracle.synth_image(1, 0, 400, 300)
    keys, desc, _ = oracle.extract(img, oc.NF, oc.SF, oc.NL, oc.INI_TH, oc.MIN_TH)
    assert len(keys) > 300
    scale = oracle.params(oc.NF, oc.SF, oc.NL)["scale"]
    angles, rdesc, _ = odr.restate(oracle.pyramid(img, oc.SF, oc.NL), keys, scale)
    _agree(keys, desc, angles, rdesc, "synth_image(1, 0, 400, 300)")


@pytest.mark.parametrize("i", [0, 3])
def test_restatement_equals_oracle_on_border_images(oracle, i):
    """Images 0 and 3 of border_set(380, 230): keypoints at distance 0 and 1
    from every side of every level (tests/test_border_inputs.py), where the
    sampled windows reach the level's first and last rows and columns."""
    w, h = 380, 230
    img, keys, desc = bc.border_oracle(oracle, w, h)[i]
    scale = oracle.params(bc.NF, bc.SF, bc.NL)["scale"]
    angles, rdesc, _ = odr.restate(oracle.pyramid(img, bc.SF, bc.NL), keys, scale)
    _agree(keys, desc, angles, rdesc, f"border image {i}")
    assert not bc.EDGE_BINS - bc.bins_of(oracle, w, h, [bc.border_oracle(oracle, w, h)[j] for j in (0, 3)])


# ------------------------------------------------------------------ census
@pytest.mark.parametrize("name", ALL)
def test_census(oracle, name):
    oc.assert_census(oracle, name)


def test_census_counts_cover_the_slot_pairing():
    """Level counts 1, 2, 3 (half a pair, one pair, a pair and a repeated
    half-wave); 7, 8, 9 around the 4 pairs of a k_orient_desc<1> workgroup and
    31, 32, 33 around the 4 * DESC_PPW = 16 pairs of a k_orient_desc<DESC_PPW>
    one."""
    assert oc.COUNTS == (1, 2, 3, 7, 8, 9, 31, 32, 33)
    assert all(oc.cases()[f"count_{n}"].nl == 1 for n in oc.COUNTS)


def test_white_field_presaturates_every_level(oracle):
    for name, img in (("moments_white", oc.cases()["moments_white"].img), ("white_field", oc.white_field())):
        for l, lv in enumerate(oracle.pyramid(img, oc.SF, oc.NL)):
            assert odr.blur_unclamped(lv).max() > 255, (name, l)


def test_clamp_and_ties_decide_bits(oracle):
    """What the census counts is what a wrong kernel would get wrong: without
    the clamp moments_white's descriptors differ from the oracle's, and with
    ties rounded away from zero noise_ties' sampling offsets differ."""
    c = oc.cases()["moments_white"]
    _, keys, desc, _ = oc.case_oracle(oracle, "moments_white")
    _, _, traces = oc.case_restated(oracle, "moments_white")
    levels = oracle.pyramid(c.img, oc.SF, c.nl)
    hit = next(i for i, t in enumerate(traces) if t["n_clamp_bits"])
    t = traces[hit]
    raw = odr.blur_unclamped(levels[t["level"]])
    _, d_raw, _ = odr.describe(levels[t["level"]], raw, raw, t["x"], t["y"])
    assert int(np.unpackbits(d_raw ^ desc[hit]).sum()) == t["n_clamp_bits"]
    _, keys, _, _ = oc.case_oracle(oracle, "noise_ties")
    _, _, traces = oc.case_restated(oracle, "noise_ties")
    hit = next(i for i, t in enumerate(traces) if t["n_ties"])
    rad = np.float32(keys["angle"][hit] * odr.FACTOR_PI)
    b, a, _ = odr.pinned_sincos(rad)
    px, py = odr._PATTERN[:, 0].astype(np.float32), odr._PATTERN[:, 1].astype(np.float32)
    fx, fy = px * a - py * b, px * b + py * a
    away = lambda v: np.copysign(np.floor(np.abs(v) + np.float32(0.5)), v)
    assert ((away(fx) != np.rint(fx)) | (away(fy) != np.rint(fy))).sum() > 0
