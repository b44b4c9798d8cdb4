"""k_pyr_resize's kept row taps and top-byte pack against the oracle's pyramid.

A thread of the batch resize builds four output rows; a row whose first staged
source row is the previous row's second keeps that row's horizontal taps, and
the vertical stage takes the result byte as the top byte of the scaled sum with
no shift and no clamp (extractor_kernels.hip).  Every level of every image must
still equal the oracle's cv::resize chain bit for bit:

* scale factors 1.1, 1.2 and 1.25 -- the two-row source step falls at a
  different cadence in each, 1.25 is the narrow window's limit;
* per scale factor two image sizes (SIZES) whose levels have a width that is
  no multiple of 4, a width just past a multiple of 128 and a height = 1 and
  = 31 mod 32: partial tiles, the y >= dh break and the clamped last source row
  next to a kept tap (the test checks the sizes still have these properties);
* batches of 9 and 17 images: more than 8 takes one launch per level, and past
  16 the launch has two workgroups per tile that walk alternate images (9 and
  8 of them), each reusing the row decisions it made before its loop;
* a source stride equal to the (odd) width -- the unaligned staging on level 1 --
  and a 16-aligned one, with the row padding filled with junk;
* images: all 255 (the removed clamp and the 2^32 bound), all 0, 0/255
  checkerboards of 1 px and 3 px period (the largest tap swings), seeded noise.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NLEVELS = 4
# scale factor -> two sizes, chosen from the level sizes the extractor derives
SIZES = {1.1: ((157, 107), (311, 105)),
         1.2: ((157, 113), (311, 109)),
         1.25: ((161, 101), (251, 99))}
CONTENTS = ("ones", "zeros", "check1", "check3", "noise")


def _image(kind, w, h, seed):
    if kind == "ones":
        return np.full((h, w), 255, np.uint8)
    if kind == "zeros":
        return np.zeros((h, w), np.uint8)
    if kind in ("check1", "check3"):
        p = 1 if kind == "check1" else 3
        y, x = np.mgrid[0:h, 0:w]
        return (((x // p + y // p) & 1) * 255).astype(np.uint8)
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _batch_kinds(B):
    """Content of each image: the five kinds in turn, so every workgroup's
    image loop meets every kind; noise images differ by seed."""
    return [(CONTENTS[i % len(CONTENTS)], i) for i in range(B)]


@functools.lru_cache(maxsize=None)
def _reference(kind, seed, w, h, sf):
    import oracle
    return tuple(oracle.pyramid(_image(kind, w, h, seed), sf, NLEVELS))


@pytest.mark.parametrize("sf", sorted(SIZES))
def test_sizes_reach_the_tile_edges(gpu, sf):
    """The two sizes of a scale factor put, on some level >= 1, a width that is
    no multiple of 4, a width 1-3 past a multiple of 128, a height = 1 and a
    height = 31 mod 32 (read from the extractor's own levels)."""
    ws, hs = [], []
    for w, h in SIZES[sf]:
        ext = gpu.ORBextractor(500, sf, NLEVELS, 20, 7)
        ext(_image("noise", w, h, 1))
        for lv in ext.mvImagePyramid[1:]:
            hs.append(lv.shape[0])
            ws.append(lv.shape[1])
    assert any(x % 4 for x in ws), ws
    assert any(x % 128 in (1, 2, 3) for x in ws), ws
    assert any(y % 32 == 1 for y in hs) and any(y % 32 == 31 for y in hs), hs


@pytest.mark.parametrize("aligned", [False, True], ids=["stride_w", "stride_16"])
@pytest.mark.parametrize("B", [9, 17])
@pytest.mark.parametrize("size", [0, 1])
@pytest.mark.parametrize("sf", sorted(SIZES))
def test_batch_levels_equal_oracle(gpu, oracle, sf, size, B, aligned):
    torch = pytest.importorskip("torch")
    w, h = SIZES[sf][size]
    assert w % 2 == 1  # stride == width is the unaligned path
    stride = ((w + 15) & ~15) + 16 if aligned else w
    kinds = _batch_kinds(B)
    buf = np.full((B, h, stride), 0xA5, np.uint8)  # junk in the row padding
    for i, (kind, seed) in enumerate(kinds):
        buf[i, :, :w] = _image(kind, w, h, seed)
    ext = gpu.ORBextractor(500, sf, NLEVELS, 20, 7)
    cap = ext.capacity(w, h)
    d_img = torch.from_numpy(buf).cuda()
    d_k = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ext.profile(True)
    ext.extract_batch(d_img.data_ptr(), B, w, h, stride, stride * h, d_k.data_ptr(),
                      d_d.data_ptr(), cap, d_n.data_ptr())
    torch.cuda.synchronize()
    name, _, n = ext.profile_read(0)
    ext.profile(False)
    # one launch per level: the kernel under test, not the level pairs
    assert name == "k_pyr_resize" and n == NLEVELS - 1, (name, n)
    for i, (kind, seed) in enumerate(kinds):
        ref = _reference(kind, seed, w, h, sf)
        for l in range(1, NLEVELS):
            got = ext.batch_level(i, l)
            assert got.shape == ref[l].shape, (i, kind, l, got.shape, ref[l].shape)
            bad = got != ref[l]
            assert not bad.any(), (
                f"image {i} ({kind}) level {l} {got.shape}: {bad.sum()} px differ, first at "
                f"(y, x) = {tuple(np.argwhere(bad)[0])}")
