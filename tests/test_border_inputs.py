"""The border inputs of tests/border_cases.py reach the cases they are built
for, shown with the CPU oracle alone: every (level, side, distance) and
(level, corner) bin at both test sizes, the sub-lists the small GPU batches
use, and the FAST cell-grid geometry of the grid-edge sizes."""
import numpy as np
import pytest

import border_cases as bc


@pytest.mark.parametrize("w,h", bc.SIZES)
def test_border_set_hits_every_bin(oracle, w, h):
    """The oracle's keypoints over border_set(w, h) hit all 8 x (24 + 4) = 224
    bins: no level, side, distance or corner excluded."""
    assert len(bc.ALL_BINS) == 224
    res = bc.border_oracle(oracle, w, h)
    assert len(res) == 20
    missing = bc.ALL_BINS - bc.bins_of(oracle, w, h, res)
    assert not missing, sorted(missing, key=str)


@pytest.mark.parametrize("w,h", bc.SIZES)
@pytest.mark.parametrize("n", sorted(bc.SUBSET))
def test_small_batch_images_hit_every_edge(oracle, w, h, n):
    """The images of the batches of 4 and 2 alone put keypoints at distance 0
    and 1 from every side of every level."""
    res = bc.border_subset(oracle, w, h, n)
    assert len(res) == n
    missing = bc.EDGE_BINS - bc.bins_of(oracle, w, h, res)
    assert not missing, sorted(missing, key=str)


def test_dropin_image_hits_every_edge(oracle):
    w, h = bc.SIZES[0]
    res = bc.border_oracle(oracle, w, h)
    assert np.array_equal(res[bc.DROPIN_IMAGE][0], bc.blocky(3, w, h, 3))  # the first b = 3 image
    missing = bc.EDGE_BINS - bc.bins_of(oracle, w, h, [res[bc.DROPIN_IMAGE]])
    assert not missing, sorted(missing, key=str)


def test_level_sizes_select_the_fast_kernel(oracle):
    """380 x 230: every level's cell ROI is at most 43 px wide (a 16-byte-load
    row of k_fast_cells); 260 x 230: level 6 (87 x 77) is one cell of 55 px."""
    def widest(w, h):
        out = []
        for lw, lh in oracle.level_sizes(w, h, bc.SF, bc.NL):
            cx, _ = bc.cell_grid(lw, "x")
            cy, _ = bc.cell_grid(lh, "y")
            assert cx and cy
            out.append(max(b - a for a, b in cx))
        return out
    assert max(widest(380, 230)) <= 43
    assert oracle.level_sizes(380, 230)[5:] == [(153, 92), (127, 77), (106, 64)]
    wide = widest(260, 230)
    assert oracle.level_sizes(260, 230)[6:] == [(87, 77), (73, 64)]
    assert wide[6] == 55 and len(bc.cell_grid(87, "x")[0]) == 1


@pytest.mark.parametrize("n", sorted(bc.GRID_DIMS))
def test_cell_grid_table(n):
    """Level dimension -> size of the last cell that exists, as a column and as
    a row.  A row starting 4-6 px before the border exists where the column is
    skipped: 'iniX >= maxBorderX - 6' against 'iniY >= maxBorderY - 3'."""
    col, row = bc.GRID_DIMS[n]
    size_x, skip_x = bc.last_cell(n, "x")
    size_y, skip_y = bc.last_cell(n, "y")
    if col is None:
        assert skip_x == 1 and size_x >= 31   # the last column is skipped: a full cell is last
    else:
        assert (size_x, skip_x) == (col, 0)
    if row is None:
        assert skip_y == 1 and size_y >= 31
    else:
        assert (size_y, skip_y) == (row, 0)
    # cells tile the level at one step, each reaching 6 px into the next or the border
    for axis in "xy":
        cells, _ = bc.cell_grid(n, axis)
        assert cells[0][0] == 16 and cells[-1][1] == n - 16
        step = cells[1][0] - cells[0][0]
        assert all(b[0] - a[0] == step and a[1] == min(b[0] + 6, n - 16)
                   for a, b in zip(cells, cells[1:]))


@pytest.mark.parametrize("w,h,nl", bc.GRID_CASES)
def test_grid_case_geometry(oracle, w, h, nl):
    """Each grid-edge size carries the last-cell geometry it is listed for, on
    its last level, and the oracle's keypoints sit where that geometry says."""
    lw, lh = oracle.level_sizes(w, h, bc.SF, nl)[nl - 1]
    if nl == 2:
        assert (lw, lh) == (783, 873)
    col, _ = bc.GRID_DIMS[lw]
    _, row = bc.GRID_DIMS[lh]
    size_x, skip_x = bc.last_cell(lw, "x")
    assert skip_x == 1 if col is None else (size_x, skip_x) == (col, 0)
    assert bc.last_cell(lh, "y") == (row, 0)
    scale = oracle.params(bc.GRID_NF, bc.SF, nl)["scale"]
    for i, (_, k, _) in enumerate(bc.grid_oracle(oracle, w, h, nl)):
        c = bc.grid_edge_counts(k, lw, lh, nl - 1, scale)
        assert c["beyond"] == 0, (i, c)
        # a last cell of >= 7 px holds FAST candidates up to the last column / row;
        # under a 4-6 px last row the row above reaches the border itself
        assert c["bottom"] > 0, (i, c)
        if col is not None:
            assert c["right"] > 0, (i, c)
