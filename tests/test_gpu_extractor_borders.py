"""GPU extractor parity at the level borders and the FAST cell-grid edges.

k_orient_desc stages a 43 x 43 window per keypoint: it reflects rows
(REFLECT_101) within 2 px of the top and bottom keypoint rows and patches
columns through LDS within 2 px of the left and right keypoint columns; level
0 is read from the caller's image at its stride, levels 1-7 from the arena at
a padded pitch.  The inputs of tests/border_cases.py put oracle keypoints at
every such place of every level (tests/test_border_inputs.py shows it on the
CPU); here every kernel path that can serve them is compared with the oracle,
all 7 keypoint fields, their order and all 256 descriptor bits:

  path                               case                          shown by
  k_fast_band, k_orient_desc<1>      one frame; batch of 2         profile stage 2, B <= 2
  k_fast_cells                       batches of 4 / 20, 380 x 230  profile stage 2
  k_fast_band for a batch            batches of 4 / 20, 260 x 230  profile stage 2
  k_orient_desc<DESC_PPW>            batches of 4 / 20             B >= 3
  octree keys in registers           batches of 2 / 4              B <= 16
  octree keys in LDS / global        batch of 20                   B > 16
  level 0 at byte shifts 0-3,        batch of 20                   the call's arguments
    tight and odd stride
  arena levels 1-7                   every case (8 levels); level 1 of 940 x 1048
"""
import numpy as np
import pytest

import border_cases as bc
from test_gpu_extractor import _diff_report

pytestmark = pytest.mark.gpu


def _batch(gpu, ext, imgs, stride=None, pitch=None, shift=0):
    """One extract_batch call over imgs packed at (stride, pitch), the first
    image `shift` bytes past a 4-byte boundary.  Returns ([(keys, desc)], the
    FAST stage's kernel name)."""
    torch = pytest.importorskip("torch")
    B = len(imgs)
    h, w = imgs[0].shape
    stride = stride or w
    pitch = pitch or stride * h
    buf = np.zeros(pitch * B + stride + 16, np.uint8)
    for f, im in enumerate(imgs):
        rows = np.lib.stride_tricks.as_strided(buf[shift + f * pitch:], (h, w), (stride, 1))
        rows[:] = im
    cap = ext.capacity(w, h)
    assert cap > 0
    d_buf = torch.from_numpy(buf).cuda()
    assert d_buf.data_ptr() % 4 == 0
    d_kps = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ext.profile(True)
    ext.extract_batch(d_buf.data_ptr() + shift, B, w, h, stride, pitch, d_kps.data_ptr(),
                      d_desc.data_ptr(), cap, d_cnt.data_ptr())
    torch.cuda.synchronize()
    name, _, _ = ext.profile_read(2)
    ext.profile(False)
    kps = d_kps.cpu().numpy().view(gpu.KEYPOINT_DTYPE).reshape(B, cap)
    desc = d_desc.cpu().numpy()
    cnt = d_cnt.cpu().numpy()
    assert (cnt >= 0).all() and (cnt <= cap).all(), cnt
    return [(kps[f, :cnt[f]], desc[f, :cnt[f]]) for f in range(B)], name


def _same(oracle, w, h, got, ref, what):
    (k, d), (_, kr, dr) = got, ref
    ok = len(k) == len(kr) and k.tobytes() == kr.tobytes() and d.tobytes() == dr.tobytes()
    assert ok, (f"{what}\n{_diff_report(k, d, kr, dr)}\n"
                f"{bc.describe_first_diff(oracle, w, h, k, d, kr, dr)}")


def _covered(oracle, w, h, refs, bins):
    missing = bins - bc.bins_of(oracle, w, h, refs)
    assert not missing, sorted(missing, key=str)  # the oracle output compared with holds the cases


@pytest.mark.parametrize("w,h", bc.SIZES)
def test_border_one_frame(gpu, oracle, w, h):
    """The 20 images one by one on one handle (k_fast_band, k_orient_desc<1>),
    and the pyramid the calls leave behind."""
    refs = bc.border_oracle(oracle, w, h)
    _covered(oracle, w, h, refs, bc.ALL_BINS)
    ext = gpu.ORBextractor(bc.NF, bc.SF, bc.NL, 20, 7)
    for i, ref in enumerate(refs):
        _same(oracle, w, h, ext(ref[0]), ref, f"image {i}")
        if i in (0, len(refs) - 1):
            for l, (a, b) in enumerate(zip(ext.mvImagePyramid, oracle.pyramid(ref[0], bc.SF, bc.NL))):
                assert a.shape == b.shape and np.array_equal(a, b), f"image {i} level {l}"


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("layout", ["tight", "odd_stride"])
@pytest.mark.parametrize("w,h", bc.SIZES)
def test_border_batch_of_20(gpu, oracle, w, h, layout, shift):
    """All 20 images in one call: more than 16, so the octree keeps its keys in
    LDS / global scratch, and k_orient_desc<DESC_PPW>; level 0 read at each
    byte alignment of the image base, rows packed tight or at an odd stride."""
    refs = bc.border_oracle(oracle, w, h)
    _covered(oracle, w, h, refs, bc.ALL_BINS)
    stride, pitch = (w, w * h + 4) if layout == "tight" else (w + 5, (w + 5) * h + 3)
    ext = gpu.ORBextractor(bc.NF, bc.SF, bc.NL, 20, 7)
    got, fast = _batch(gpu, ext, [r[0] for r in refs], stride, pitch, shift)
    assert fast == bc.FAST_KERNEL[(w, h)]
    for i, ref in enumerate(refs):
        _same(oracle, w, h, got[i], ref, f"image {i}")


@pytest.mark.parametrize("B", [4, 2])
@pytest.mark.parametrize("w,h", bc.SIZES)
def test_border_small_batch(gpu, oracle, w, h, B):
    """4 images: the smallest batch that takes k_fast_cells, octree keys in
    registers.  2 images: the batch entry point with k_fast_band and
    k_orient_desc<1>."""
    refs = bc.border_subset(oracle, w, h, B)
    _covered(oracle, w, h, refs, bc.EDGE_BINS)
    ext = gpu.ORBextractor(bc.NF, bc.SF, bc.NL, 20, 7)
    got, fast = _batch(gpu, ext, [r[0] for r in refs])
    assert fast == ("k_fast_band" if B < 4 else bc.FAST_KERNEL[(w, h)])
    for i, ref in enumerate(refs):
        _same(oracle, w, h, got[i], ref, f"image {bc.SUBSET[B][i]}")


@pytest.mark.parametrize("w,h,nl", bc.GRID_CASES)
def test_fast_cell_grid_edges(gpu, oracle, w, h, nl):
    """Level dimensions whose last cell column is 7-12 px wide or skipped and
    whose last cell row is 4-12 px high (a row of 4-6 px exists but holds no
    FAST corner): noise, 2 x 2 blocks and their mirror images, one frame at a
    time and as a batch of 4 through k_fast_cells."""
    lw, lh = oracle.level_sizes(w, h, bc.SF, nl)[nl - 1]
    if nl == 2:
        assert (lw, lh) == (783, 873)
    col, _ = bc.GRID_DIMS[lw]
    _, row = bc.GRID_DIMS[lh]
    size_x, skip_x = bc.last_cell(lw, "x")
    assert skip_x == 1 if col is None else (size_x, skip_x) == (col, 0)
    assert bc.last_cell(lh, "y") == (row, 0)
    refs = bc.grid_oracle(oracle, w, h, nl)
    scale = oracle.params(bc.GRID_NF, bc.SF, nl)["scale"]
    for i, (_, k, _) in enumerate(refs):
        c = bc.grid_edge_counts(k, lw, lh, nl - 1, scale)
        assert c["beyond"] == 0 and c["bottom"] > 0 and (col is None or c["right"] > 0), (i, c)
    ext = gpu.ORBextractor(bc.GRID_NF, bc.SF, nl, 20, 7)
    for i, ref in enumerate(refs):
        _same(oracle, w, h, ext(ref[0]), ref, f"one frame, image {i}")
    got, fast = _batch(gpu, ext, [r[0] for r in refs])
    assert fast == "k_fast_cells"
    for i, ref in enumerate(refs):
        _same(oracle, w, h, got[i], ref, f"batch of 4, image {i}")
