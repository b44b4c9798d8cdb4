"""Extractor inputs that put keypoints on every level's borders, and the FAST
cell grid restated, shared by the CPU and GPU tests (test infrastructure).

Keypoints exist only at 19 <= x <= lw - 20 and 19 <= y <= lh - 20 of a level
(the 16-px FAST border plus its 3-px ring, src/ORBextractor.cc:797-800).  A
descriptor window is 43 px wide, so it overhangs a column edge exactly at
x in {19, 20, lw - 21, lw - 20} and reflects rows at y in {19, 20, lh - 21,
lh - 20}.  The bins below name those places per level; the tests assert that
the oracle's keypoints reach them before comparing the GPU's with them.
"""
import numpy as np

NF, SF, NL = 20000, 1.2, 8   # quota far above the candidate count: the octree keeps border keypoints
SIDES = ("L", "R", "T", "B")
CORNERS = ("TL", "TR", "BL", "BR")
DEPTH = 6                    # side bins d = 0 .. 5
ALL_BINS = frozenset([(l, s, d) for l in range(NL) for s in SIDES for d in range(DEPTH)] +
                     [(l, c) for l in range(NL) for c in CORNERS])
EDGE_BINS = frozenset((l, s, d) for l in range(NL) for s in SIDES for d in (0, 1))

# every level's cells fit k_fast_cells / level 6 (87 x 77) is one 55-px-wide cell: k_fast_band
SIZES = [(380, 230), (260, 230)]
FAST_KERNEL = {(380, 230): "k_fast_cells", (260, 230): "k_fast_band"}


def blocky(seed, w, h, b):
    """Uniform noise in b x b blocks at a random phase.  Plain noise (b = 1)
    loses its FAST corners by level 5-6 of the pyramid; the coarser blocks
    keep them dense on the high levels."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (-(-h // b) + 1, -(-w // b) + 1), np.uint8)
    ox, oy = rng.integers(0, b, 2)
    img = np.kron(a, np.ones((b, b), np.uint8))[oy:oy + h, ox:ox + w]
    return np.ascontiguousarray(img, np.uint8)


def border_set(w, h):
    """The 20 images of one size: b = 1 .. 5, seed = 10 * s + b for s = 0 .. 3."""
    return [blocky(10 * s + b, w, h, b) for s in range(4) for b in range(1, 6)]


def _level_xy(keys, scale):
    s = np.asarray(scale, np.float32)[keys["octave"]]
    return (np.rint(keys["x"] / s).astype(np.int64), np.rint(keys["y"] / s).astype(np.int64))


def key_bins(keys, sizes, scale):
    """Per keypoint the list of bins it falls in (most keypoints: none)."""
    lx, ly = _level_xy(keys, scale)
    out = []
    for l, x, y in zip(keys["octave"].tolist(), lx.tolist(), ly.tolist()):
        lw, lh = sizes[l]
        d = {"L": x - 19, "R": lw - 20 - x, "T": y - 19, "B": lh - 20 - y}
        assert min(d.values()) >= 0, (l, x, y, lw, lh)  # no keypoint lies outside the FAST border
        b = [(l, s, d[s]) for s in SIDES if d[s] < DEPTH]
        b += [(l, c) for c in CORNERS if d[c[1]] <= 1 and d[c[0]] <= 1]
        out.append(b)
    return out


def border_bins(keys, sizes, scale):
    """The set of bins the keypoints hit: (level, side, d) for a keypoint d px
    inside the extreme coordinate of that side (level x = 19 + d for L,
    lw - 20 - d for R; level y = 19 + d for T, lh - 20 - d for B; d = 0 .. 5),
    and (level, corner) for one within 2 px of both extreme coordinates, whose
    window overhangs a column edge and reflects rows at once."""
    return {b for kb in key_bins(keys, sizes, scale) for b in kb}


_cache = {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def border_oracle(oracle, w, h):
    """[(image, keypoints, descriptors)] of border_set(w, h) from the oracle,
    computed once per size and process, read-only."""
    if (w, h) not in _cache:
        res = []
        for img in border_set(w, h):
            k, d, _ = oracle.extract(img, NF, SF, NL, 20, 7)
            res.append(_frozen(img, k, d))
        _cache[(w, h)] = res
    return _cache[(w, h)]


def bins_of(oracle, w, h, results):
    sizes = oracle.level_sizes(w, h, SF, NL)
    scale = oracle.params(NF, SF, NL)["scale"]
    bins = set()
    for _, k, _ in results:
        bins |= border_bins(k, sizes, scale)
    return bins


# Sub-lists of border_set for the small batches: images whose keypoints alone
# hit every EDGE_BINS bin at both sizes (tests/test_border_inputs.py checks
# it).  The first four do; the first two miss two bins at 260 x 230, the first
# and the fourth (b = 1 and b = 4) do not.  Image 2 is the set's first b = 3
# image, which does so alone at 380 x 230 (the drop-in case).
SUBSET = {4: (0, 1, 2, 3), 2: (0, 3)}
DROPIN_IMAGE = 2


def border_subset(oracle, w, h, n):
    res = border_oracle(oracle, w, h)
    return [res[i] for i in SUBSET[n]]


def describe_first_diff(oracle, w, h, k_gpu, d_gpu, k_ref, d_ref):
    """The first keypoint of the oracle's list that the GPU's differs at
    (any field, or a descriptor bit), with its border bins."""
    n = min(len(k_gpu), len(k_ref))
    bad = np.nonzero((k_gpu[:n] != k_ref[:n]) | (d_gpu[:n] != d_ref[:n]).any(1))[0]
    if len(bad) == 0:
        return f"lists agree over their first {n} keypoints (gpu {len(k_gpu)}, ref {len(k_ref)})"
    i = int(bad[0])
    sizes = oracle.level_sizes(w, h, SF, NL)
    scale = oracle.params(NF, SF, NL)["scale"]
    bins = key_bins(k_ref[i:i + 1], sizes, scale)[0]
    bits = int(np.unpackbits(d_gpu[i] ^ d_ref[i]).sum())
    return (f"first differing keypoint {i}: ref {k_ref[i]} gpu {k_gpu[i]}, {bits} descriptor bits, "
            f"border bins {bins or 'none'}")


# ------------------------------------------------------------ FAST cell grid
def cell_grid(n, axis):
    """The reference's cell loop over one level dimension of n px
    (src/ORBextractor.cc:797-839): ([(ini, max)] of the cells that exist, the
    number skipped).  Columns ("x") are skipped from iniX >= maxBorderX - 6,
    rows ("y") from iniY >= maxBorderY - 3, so a row of 4-6 px exists (too
    short for a FAST corner, which needs 7) where a column would be skipped."""
    lo, hi = 16, n - 16
    span = np.float32(hi - lo)
    count = int(span / np.float32(30))
    if count <= 0:
        return [], 0
    cell = int(np.ceil(span / np.float32(count)))
    margin = {"x": 6, "y": 3}[axis]
    cells, skipped = [], 0
    for i in range(count):
        ini = lo + i * cell
        if ini >= hi - margin:
            skipped += 1
            continue
        cells.append((ini, min(ini + cell + 6, hi)))
    return cells, skipped


def last_cell(n, axis):
    """Size of the last cell that exists and the number of cells skipped."""
    cells, skipped = cell_grid(n, axis)
    return cells[-1][1] - cells[-1][0], skipped


# level dimension -> (last column px or None where it is skipped, last row px)
GRID_DIMS = {783: (7, 7), 753: (8, 8), 723: (9, 9), 693: (10, 10), 663: (11, 11), 633: (12, 12),
             873: (None, 4), 843: (None, 5), 813: (None, 6), 1241: (None, None)}
# (w, h, nlevels): the level that carries the geometry is the last one
GRID_CASES = [(783, 873, 1), (753, 843, 1), (723, 813, 1),   # 7/8/9-px last column, 4/5/6-px last row
              (693, 783, 1), (663, 753, 1), (633, 723, 1),   # 10/11/12-px last column, 7/8/9-px last row
              (813, 693, 1), (843, 663, 1), (873, 633, 1),   # last column skipped, 10/11/12-px last row
              (940, 1048, 2)]                                # level 1 is 783 x 873, read from the arena
GRID_NF = 30000


def grid_images(w, h):
    """Uniform noise, blocky(b = 2) and their left-right flips."""
    noise = np.random.default_rng(1000 * w + h).integers(0, 256, (h, w), np.uint8)
    blk = blocky(1000 * w + h, w, h, 2)
    return [noise, blk, np.ascontiguousarray(noise[:, ::-1]), np.ascontiguousarray(blk[:, ::-1])]


def grid_oracle(oracle, w, h, nl):
    key = (w, h, nl)
    if key not in _cache:
        res = []
        for img in grid_images(w, h):
            k, d, _ = oracle.extract(img, GRID_NF, SF, nl, 20, 7)
            res.append(_frozen(img, k, d))
        _cache[key] = res
    return _cache[key]


def grid_edge_counts(keys, lw, lh, level, scale):
    """Keypoints of `level` at the last column / last row a keypoint can take,
    and beyond them (must be none)."""
    k = keys[keys["octave"] == level]
    lx, ly = _level_xy(k, scale)
    return dict(right=int((lx == lw - 20).sum()), bottom=int((ly == lh - 20).sum()),
                beyond=int(((lx > lw - 20) | (ly > lh - 20)).sum()))
