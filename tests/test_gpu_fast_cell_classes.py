"""k_fast_cells reads per cell class (level, rows, cols) what it used to derive
per cell, and a wave walks four consecutive cells: the batch path (B >= 4)
against the oracle, bit for bit, at the shapes where the class logic can go
wrong.  Every case asserts that the FAST stage ran k_fast_cells.

  case                     what it exercises
  200 x 150, 321 x 243     last-row / last-column cells differ from the interior
                           ones: a wave's four cells change class (every level
                           >= 33 px; 321 x 243: the launches of levels 1-2 and
                           of levels >= 3 each hold waves that cross a level)
  219 x 131, 8 levels      levels of 10, 4, 3 and 2 cells: a wave runs across a
                           level boundary in both of those launches; three
                           levels without a cell
  stride w + 5, shift 1-3  a caller stride that is no multiple of 4
  flat + textured corner,  cells that find nothing at iniThFAST (phase B; on the
  faint + textured corner  faint background they find corners at minThFAST) beside
                           cells of the same class that do (phase A)
  noise, 2 x 2 blocks      the fullest candidate queues (flushes in mid-pass) and
                           corner lists a cell can meet
  526 x 1012, 2 levels     level 1 (438 x 843) ends in a row of 5-px cells (tiny)
"""
import numpy as np
import pytest

import border_cases as bc
from test_gpu_extractor_borders import _batch, _same

pytestmark = pytest.mark.gpu

NF, SF, INI, MIN = 20000, 1.2, 20, 7
_refs = {}


def _noise(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), np.uint8)


def _faint(seed, w, h):
    """2 x 2 blocks of 100 / 112: corners above minThFAST, none above iniThFAST."""
    return (100 + 12 * (bc.blocky(seed, w, h, 2) >> 7)).astype(np.uint8)


def _corner(seed, w, h):
    """Faint everywhere, full contrast in the top-left 45 %: phase-B cells beside phase-A cells."""
    img = _faint(seed, w, h)
    ch, cw = int(h * 0.45), int(w * 0.45)
    img[:ch, :cw] = bc.blocky(seed + 1, cw, ch, 2)
    return img


def _flat_corner(seed, w, h):
    """One grey level everywhere but a textured top-left corner: the other cells find nothing at
    either threshold.  (The corner reaches past the middle: with every key in one quadrant the
    reference's octree stops at its first pass and keeps one keypoint per level.)"""
    img = np.full((h, w), 100, np.uint8)
    ch, cw = int(h * 0.6), int(w * 0.6)
    img[:ch, :cw] = bc.blocky(seed + 1, cw, ch, 2)
    return img


def _images(w, h, B):
    kinds = [_noise, lambda s, a, b: bc.blocky(s, a, b, 2), _corner, _faint, _flat_corner,
             lambda s, a, b: bc.blocky(s, a, b, 3)[:, ::-1].copy()]
    return [np.ascontiguousarray(kinds[i % len(kinds)](7000 + 131 * w + h + i, w, h)) for i in range(B)]


def _oracle(oracle, w, h, nl, B):
    key = (w, h, nl, B)
    if key not in _refs:
        res = []
        for img in _images(w, h, B):
            k, d, _ = oracle.extract(img, NF, SF, nl, INI, MIN)
            for a in (img, k, d):
                a.setflags(write=False)
            res.append((img, k, d))
        _refs[key] = res
    return _refs[key]


def _check(gpu, oracle, w, h, nl, B, **layout):
    refs = _oracle(oracle, w, h, nl, B)
    ext = gpu.ORBextractor(NF, SF, nl, INI, MIN)
    got, fast = _batch(gpu, ext, [r[0] for r in refs], **layout)
    assert fast == "k_fast_cells"
    for i, ref in enumerate(refs):
        _same(oracle, w, h, got[i], ref, f"{w} x {h}, {nl} levels, image {i} of {B} {layout}")
    return refs


@pytest.mark.parametrize("w,h,nl,B", [(200, 150, 3, 5), (321, 243, 6, 5), (219, 131, 8, 6)])
def test_class_changes_inside_a_wave(gpu, oracle, w, h, nl, B):
    refs = _check(gpu, oracle, w, h, nl, B)
    sizes = oracle.level_sizes(w, h, SF, nl)
    assert min(min(s) for s in sizes) >= 33
    # the faint image: every keypoint from phase B; the corner image: both phases
    # (the response is the largest threshold the corner passes: >= iniThFAST from phase A)
    resp = [r[1]["response"] for r in refs]
    assert len(refs[0][1]) > 0 and resp[3].size and resp[3].max() < INI
    l0 = refs[2][1]["octave"] == 0
    assert (resp[2][l0] >= INI).any() and (resp[2][l0] < INI).any()
    flat = refs[4][1]  # keypoints in the textured corner only
    assert len(flat) > 50 and flat["x"].max() < 0.6 * w + 4 and flat["y"].max() < 0.6 * h + 4


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_odd_stride(gpu, oracle, shift):
    w, h = 200, 150
    _check(gpu, oracle, w, h, 3, 5, stride=w + 5, pitch=(w + 5) * h + 3, shift=shift)


def test_tiny_last_row(gpu, oracle):
    w, h, nl = 526, 1012, 2
    assert tuple(oracle.level_sizes(w, h, SF, nl)[1]) == (438, 843)
    assert bc.last_cell(843, "y") == (5, 0)  # a 5-px row of cells: no window, no keypoint
    _check(gpu, oracle, w, h, nl, 4)
