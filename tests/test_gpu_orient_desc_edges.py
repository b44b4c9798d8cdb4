"""k_orient_desc (IC_Angle + 7 x 7 blur + rBRIEF) on the directed frames of
tests/orient_desc_cases.py: all 7 keypoint fields, their order and all 256
descriptor bits against oracle.extract, which tests/test_orient_desc_cases.py
shows equal to a second statement of the arithmetic on the same frames.

  aimed at                             case                      launch
  m_01 == m_10 == 0, axes, diagonals   moments_dark / _white     <1> and <DESC_PPW>
    both sides of |m_01| == |m_10|,
    sincos reduction with k = 4
  the blur's min(., 255)               moments_white,            <1>, <DESC_PPW>,
                                       binary_blocks, white 403  blurred_levels()
  cvRound of x.5 by the float adder    noise_ties                <1> and <DESC_PPW>
  empty levels between full ones,      sparse_levels, flat in    <1> (B = 2),
    a frame with no keypoints            the middle of a batch   <DESC_PPW> (B = 6)
  level counts 1 .. 33, odd counts     count_n                   <1>, <DESC_PPW> (B = 9)
    (half-wave 1 repeats half-wave 0)

Each test first asserts the census of its cases (orient_desc_cases.assert_census,
on the oracle's output alone), so that a pass cannot come from inputs that
lost their edge.  Every comparison is exact.
"""
import numpy as np
import pytest

import orient_desc_cases as oc
import orient_desc_ref as odr
import pyref
from test_gpu_extractor_borders import _batch, _same

pytestmark = pytest.mark.gpu


def _ref(oracle, name):
    oc.assert_census(oracle, name)
    img, k, d, _ = oc.case_oracle(oracle, name)
    return img, k, d


def _compare(oracle, got, ref, what):
    _same(oracle, oc.W, oc.H, got, ref, what)


def _handle(gpu, nl):
    return gpu.ORBextractor(oc.NF, oc.SF, nl, oc.INI_TH, oc.MIN_TH)


@pytest.mark.parametrize("nl", [8, 1])
def test_one_frame_at_a_time(gpu, oracle, nl):
    """Every case of one parameter set on one handle, one call each
    (k_orient_desc<1>), flat between the others."""
    names = [n for n, c in oc.cases().items() if c.nl == nl]
    if nl == 8:
        names.remove("flat")
        names.insert(2, "flat")
    refs = [_ref(oracle, n) for n in names]
    ext = _handle(gpu, nl)
    for name, ref in zip(names, refs):
        k, d = ext(ref[0])
        _compare(oracle, (k, d), ref, name)


def test_batch_of_two(gpu, oracle):
    """moments_white and sparse_levels in one call: the batch entry point with
    k_orient_desc<1>, presaturated windows beside levels without keypoints."""
    names = ["moments_white", "sparse_levels"]
    refs = [_ref(oracle, n) for n in names]
    got, fast = _batch(gpu, _handle(gpu, 8), [r[0] for r in refs])
    assert fast == "k_fast_band"
    for name, g, ref in zip(names, got, refs):
        _compare(oracle, g, ref, name)


@pytest.mark.parametrize("layout", ["tight", "odd_stride_shift_1"])
def test_batch_of_all_eight_level_cases(gpu, oracle, layout):
    """The five 8-level cases with flat in the middle, B = 6:
    k_orient_desc<DESC_PPW>, a frame without keypoints between frames with
    them, rows packed tight or at an odd stride from a base one byte past a
    4-byte boundary."""
    names = list(oc.EIGHT_LEVEL)
    names.insert(len(names) // 2, "flat")
    refs = [_ref(oracle, n) for n in names]
    w, h = oc.W, oc.H
    stride, pitch, shift = (w, w * h, 0) if layout == "tight" else (w + 5, (w + 5) * h + 3, 1)
    got, _ = _batch(gpu, _handle(gpu, 8), [r[0] for r in refs], stride, pitch, shift)
    assert len(got[names.index("flat")][0]) == 0
    for name, g, ref in zip(names, got, refs):
        _compare(oracle, g, ref, f"{name} ({layout})")


def test_count_frames(gpu, oracle):
    """Level counts 1, 2, 3, 7, 8, 9, 31, 32, 33 on one level: one by one
    (k_orient_desc<1>) and as one batch of nine (k_orient_desc<DESC_PPW>,
    a different count per image in one launch)."""
    names = list(oc.COUNT_CASES)
    refs = [_ref(oracle, n) for n in names]
    assert [len(r[1]) for r in refs] == list(oc.COUNTS)
    ext = _handle(gpu, 1)
    for name, ref in zip(names, refs):
        _compare(oracle, ext(ref[0]), ref, f"{name}, one frame")
    got, _ = _batch(gpu, ext, [r[0] for r in refs])
    for name, g, ref in zip(names, got, refs):
        _compare(oracle, g, ref, f"{name}, batch of nine")


@pytest.mark.parametrize("name", ["moments_white", "binary_blocks", "white_field_403x301"])
def test_blurred_levels_at_the_clamp(gpu, oracle, name):
    """blurred_levels() after ext(img) equals pyref.blur7 of every oracle
    pyramid level; on the white frames the unclamped blur exceeds 255 on every
    level compared, so the kernel's min(., 255) is what is compared."""
    white = name != "binary_blocks"
    if name in oc.cases():
        oc.assert_census(oracle, name)
        img = oc.cases()[name].img
    else:
        img = oc.white_field(403, 301)
    ext = _handle(gpu, 8)
    k, d = ext(img)
    kr, dr, _ = oracle.extract(img, oc.NF, oc.SF, 8, oc.INI_TH, oc.MIN_TH)
    h, w = img.shape
    _same(oracle, w, h, (k, d), (img, kr, dr), name)
    got = ext.blurred_levels()
    levels = oracle.pyramid(img, oc.SF, 8)
    assert len(got) == len(levels) == 8
    for l, (a, lv) in enumerate(zip(got, levels)):
        raw = odr.blur_unclamped(lv)
        if white:
            assert raw.max() > 255, (name, l)
        b = pyref.blur7(lv)
        assert a.shape == b.shape, (name, l)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (f"{name} level {l}: {len(bad)} px differ, first {bad[:5].tolist()}, "
                               f"unclamped there {[int(raw[y, x]) for y, x in bad[:5]]}")
