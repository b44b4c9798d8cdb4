"""SearchByProjection(F, localMap) where the window walk can go wrong.

The candidate scan (k_proj_candidates) and for_features_in_area read a window
as per-column runs of the column-major cell table: rows nMinCellY..nMaxCellY
of column ix are the entries [cs[ix*48 + nMinCellY], cs[ix*48 + nMaxCellY + 1]).
The staged scan takes four columns at a time and runs one loop over their
concatenated runs.  These cases put the run bounds at the table's edges
(windows clamped to column 0 / 63 and row 0 / 47, windows wholly outside),
make runs empty (leading, trailing, all), make them long (past the top-K and
past the candidate lists' capacity, so the overflow-list second walk and the
resolves' exact re-scan are taken), cross the four-column chunk (th 3 and 8),
take the unstaged scan (more than 4,096 keypoints) and the batch entry point.
Every case is index-exact against the CPU oracle (src/ORBmatcher.cc:47-133
with src/Frame.cc:368-424) and first checks, in numpy, that its inputs hold
the situation it names.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 640, 480
COLS, ROWS = 64, 48          # FRAME_GRID_COLS / FRAME_GRID_ROWS
TOPK, OVF_CAP = 4, 16        # matcher_common.h
PROJ_STAGE = 4096            # matcher_kernels.hip: larger frames are scanned unstaged
CHUNK = 4                    # columns per flat loop of the staged scan
SCALE = np.float32(1.2) ** np.arange(8, dtype=np.float32)
NNRATIO = 0.8


def _oracle():
    import oracle as o  # oracle/oracle.py (tests/conftest.py puts it on the path)
    o.lib()
    return o


def _radius(mps, th):
    r = np.where(mps["view_cos"].astype(np.float64) > 0.998, np.float32(2.5), np.float32(4.0))
    return (r * np.float32(th) * SCALE[mps["level"]]).astype(np.float32)


def _windows(keys, mps, th):
    """GetFeaturesInArea's cell bounds of every usable map point and the run
    length of each of its columns (src/Frame.cc:368-400)."""
    cs, _ = _oracle().grid(keys, W, H)
    cs = cs.astype(np.int64)
    r = _radius(mps, th)
    inv_w, inv_h = np.float32(COLS) / np.float32(W), np.float32(ROWS) / np.float32(H)
    x, y = mps["proj_x"], mps["proj_y"]
    ux0 = np.floor((x - r) * inv_w).astype(np.int64)
    ux1 = np.ceil((x + r) * inv_w).astype(np.int64)
    uy0 = np.floor((y - r) * inv_h).astype(np.int64)
    uy1 = np.ceil((y + r) * inv_h).astype(np.int64)
    usable = (mps["in_view"] != 0) & (mps["bad"] == 0)
    outside = (ux0 >= COLS) | (ux1 < 0) | (uy0 >= ROWS) | (uy1 < 0)
    x0, x1 = np.maximum(ux0, 0), np.minimum(ux1, COLS - 1)
    y0, y1 = np.maximum(uy0, 0), np.minimum(uy1, ROWS - 1)
    visited = usable & ~outside
    ncols = np.where(visited, x1 - x0 + 1, 0)
    k = np.arange(COLS)[None, :]
    col = np.clip(x0[:, None] + k, 0, COLS - 1)
    yy0, yy1 = np.clip(y0, 0, ROWS - 1)[:, None], np.clip(y1, 0, ROWS - 1)[:, None]
    runs = cs[col * ROWS + yy1 + 1] - cs[col * ROWS + yy0]
    runs = np.where((k < ncols[:, None]), runs, 0)
    return dict(ux0=ux0, ux1=ux1, uy0=uy0, uy1=uy1, usable=usable, outside=outside & usable,
                visited=visited, ncols=ncols, runs=runs, r=r)


def _noisy(desc, rng, p=0.1):
    flips = rng.random((len(desc), 256)) < p
    return desc ^ np.packbits(flips, axis=1, bitorder="little")


def _synth_keys(rng, x, y, octave):
    o = _oracle()
    k = np.zeros(len(x), o.KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"] = x, y, octave
    k["size"] = 31.0 * SCALE[octave]
    k["angle"] = rng.uniform(0, 360, len(x))
    k["response"] = rng.uniform(20, 200, len(x))
    k["class_id"] = -1
    return k, rng.integers(0, 256, (len(x), 32), dtype=np.uint8)


def _onto(rng, k, d, src, jitter, has_obs=0.8):
    """Map points projected onto the keypoints `src`."""
    m = len(src)
    mps = np.zeros(m, _oracle().MP_TRACK_DTYPE)
    mps["proj_x"] = k["x"][src] + rng.uniform(-jitter, jitter, m).astype(np.float32)
    mps["proj_y"] = k["y"][src] + rng.uniform(-jitter, jitter, m).astype(np.float32)
    mps["proj_xr"] = -1.0
    mps["level"] = np.minimum(k["octave"][src] + rng.integers(0, 2, m), 7)
    mps["view_cos"] = np.where(rng.random(m) < 0.5, 0.999, 0.9).astype(np.float32)
    mps["in_view"] = 1
    mps["has_obs"] = rng.random(m) < has_obs
    return mps, _noisy(d[src], rng)


def _check(gpu, k, d, mps, mpd, th, locked=None, ur=None, matcher=None):
    o = _oracle()
    n_ref, km_ref = o.match_projection_local(k, d, SCALE, W, H, mps, mpd, th, NNRATIO, locked, ur)
    assert n_ref > 0
    m = matcher or gpu.ORBmatcher(NNRATIO)
    n, km = m.SearchByProjection(gpu.Frame(k, d, SCALE, W, H, u_right=ur), mps, mpd, th, locked)
    assert n == n_ref, (n, n_ref)
    assert np.array_equal(km, km_ref), np.nonzero(km != km_ref)[0][:10]
    return n_ref, km_ref


# ------------------------------------------------------------ clamps and borders
@functools.lru_cache(maxsize=None)
def _extracted_frame():
    o = _oracle()
    k, d, _ = o.extract(o.synth_image(1, 0, W, H), 1000, 1.2, 8, 20, 7)
    return k, d


def _border_map(k, d, th):
    """A 48 x 48 lattice from one level-7 radius outside the image to the same
    distance past the far border (half of the in-image points moved onto their
    nearest keypoint, so that the map matches), plus, for every level, view
    class and border, a point half a radius inside, one half a radius outside
    and one clear of the grid."""
    o = _oracle()
    rng = np.random.default_rng(int(th * 10))
    rmax = 4.0 * th * float(SCALE[7])
    gx, gy = np.meshgrid(np.linspace(-rmax, W + rmax, 48), np.linspace(-rmax, H + rmax, 48))
    x, y = gx.ravel().astype(np.float32), gy.ravel().astype(np.float32)
    m = len(x)
    near = np.argmin((k["x"][None, :] - x[:, None]) ** 2 + (k["y"][None, :] - y[:, None]) ** 2, 1)
    inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    snap = inside & (rng.random(m) < 0.5)
    x = np.where(snap, k["x"][near] + rng.uniform(-1, 1, m), x).astype(np.float32)
    y = np.where(snap, k["y"][near] + rng.uniform(-1, 1, m), y).astype(np.float32)
    level = np.where(snap, np.minimum(k["octave"][near] + rng.integers(0, 2, m), 7),
                     rng.integers(0, 8, m)).astype(np.int32)
    cos = np.where(rng.random(m) < 0.5, 0.999, 0.9).astype(np.float32)
    ex, ey, el, ec = [], [], [], []
    for lv in range(8):
        for c, base in ((0.999, 2.5), (0.9, 4.0)):
            r = base * th * float(SCALE[lv])
            far = r + 2 * W / COLS  # the window's last cell lies outside the grid
            for off in (0.5 * r, -0.5 * r, -far):
                # off > 0: inside the border; < 0: beyond it
                ex += [off, W - off, 97.0 + lv, 331.0 + lv]
                ey += [211.0 + lv, 143.0 + lv, off, H - off]
                el += [lv] * 4
                ec += [c] * 4
    x = np.concatenate([x, np.float32(ex)])
    y = np.concatenate([y, np.float32(ey)])
    level = np.concatenate([level, np.int32(el)])
    cos = np.concatenate([cos, np.float32(ec)])
    near = np.concatenate([near, np.argmin((k["x"][None, :] - x[m:, None]) ** 2 +
                                           (k["y"][None, :] - y[m:, None]) ** 2, 1)])
    mps = np.zeros(len(x), o.MP_TRACK_DTYPE)
    mps["proj_x"], mps["proj_y"], mps["proj_xr"] = x, y, -1.0
    mps["level"], mps["view_cos"] = level, cos
    mps["in_view"] = 1
    mps["has_obs"] = rng.random(len(x)) < 0.8
    return mps, _noisy(d[near], rng)


@pytest.mark.parametrize("th", [1.0, 3.0, 8.0])
def test_clamped_and_outside_windows(gpu, th):
    k, d = _extracted_frame()
    mps, mpd = _border_map(k, d, th)
    w = _windows(k, mps, th)
    v = w["visited"]
    assert 2300 <= len(mps) <= 2700
    assert set(mps["level"]) == set(range(8))
    for c in (0.999, 0.9):
        assert (mps["view_cos"] == np.float32(c)).any()
    # windows cut by each border and still visited; windows that visit nothing
    assert (v & (w["ux0"] < 0)).any() and (v & (w["ux1"] > COLS - 1)).any()
    assert (v & (w["uy0"] < 0)).any() and (v & (w["uy1"] > ROWS - 1)).any()
    for side in (w["ux0"] >= COLS, w["ux1"] < 0, w["uy0"] >= ROWS, w["uy1"] < 0):
        assert (w["usable"] & side).any()
    # points beyond each border whose window still reaches into the grid
    x, y = mps["proj_x"], mps["proj_y"]
    for beyond in (x < 0, x >= W, y < 0, y >= H):
        assert (v & beyond).any()
    # clamped windows that hold entries (the extractor keeps 16+ px clear of the
    # image border, which a th = 1 window at the border does not span)
    total = w["runs"].sum(1)
    if th > 1.0:
        for cut in (w["ux0"] < 0, w["ux1"] > COLS - 1, w["uy0"] < 0, w["uy1"] > ROWS - 1):
            assert (v & cut & (total > 0)).any()
    nc = w["ncols"][v & (total > 0)]
    assert nc.min() <= CHUNK < nc.max()          # the one-chunk and the chunked walk
    assert (nc % CHUNK != 0).any() and w["ncols"][v].min() == 1
    if th == 8.0:
        assert nc.max() >= 24
    _check(gpu, k, d, mps, mpd, th)


# ------------------------------------------------------------ empty runs
def test_empty_runs(gpu):
    """Keypoints in the left half only: windows with no entry at all, windows
    whose leading columns are empty and whose last is not, and the reverse."""
    rng = np.random.default_rng(11)
    n, m = 800, 1500
    k, d = _synth_keys(rng, rng.uniform(2, W / 2 - 2, n).astype(np.float32),
                       rng.uniform(2, H - 2, n).astype(np.float32), rng.integers(0, 4, n))
    mps, mpd = _onto(rng, k, d, rng.integers(0, n, m), 1.5)
    free = rng.random(m) < 0.5  # anywhere in the image
    mps["proj_x"][free] = rng.uniform(0, W, free.sum())
    mps["proj_y"][free] = rng.uniform(0, H, free.sum())
    mps["level"][free] = rng.integers(0, 5, free.sum())
    # along the edge of the populated half: leading columns filled, trailing empty
    edge = np.nonzero(free)[0][:200]
    mps["proj_x"][edge] = rng.uniform(W / 2 - 12, W / 2 + 12, len(edge))
    w = _windows(k, mps, 1.0)
    v, runs, nc = w["visited"], w["runs"], w["ncols"]
    total = runs.sum(1)
    last = runs[np.arange(m), np.maximum(nc - 1, 0)]
    assert (k["x"] < W / 2).all() and nc[v].max() <= COLS
    assert (v & (total == 0)).sum() > 100                          # all runs empty
    assert (v & (nc > 1) & (runs[:, 0] == 0) & (last > 0)).any()   # leading empty
    assert (v & (nc > 1) & (runs[:, 0] > 0) & (last == 0)).any()   # trailing empty
    inner = (runs[:, 1:-1] == 0) & (np.arange(1, COLS - 1)[None, :] < nc[:, None] - 1)
    assert (v & (runs[:, 0] > 0) & (last > 0) & inner.any(1)).any()  # empty between two
    _check(gpu, k, d, mps, mpd, 1.0)


# ------------------------------------------------------------ dense runs
@functools.lru_cache(maxsize=None)
def _dense_case():
    """900 keypoints in the six cells (20..21, 10..12); 1,500 map points
    projected onto them, every one of them locking what it claims."""
    rng = np.random.default_rng(23)
    n, m = 900, 1500
    k, d = _synth_keys(rng, rng.uniform(195.5, 214.4, n).astype(np.float32),
                       rng.uniform(95.5, 124.4, n).astype(np.float32), rng.integers(0, 8, n))
    locked = (rng.random(n) < 0.05).astype(np.uint8)
    mps, mpd = _onto(rng, k, d, rng.integers(0, n, m), 1.0, has_obs=2.0)
    n_ref, km_ref = _oracle().match_projection_local(k, d, SCALE, W, H, mps, mpd, 1.0, NNRATIO,
                                                     locked)
    return k, d, locked, mps, mpd, n_ref, km_ref


@pytest.mark.parametrize("schedule", [0, 1, 2, 3])
def test_dense_runs(gpu, schedule):
    k, d, locked, mps, mpd, n_ref, km_ref = _dense_case()
    m = len(mps)
    cs, _ = _oracle().grid(k, W, H)
    cells = np.nonzero(np.diff(cs))[0]
    assert len(cells) == 6 and set(cells // ROWS) == {20, 21} and set(cells % ROWS) == {10, 11, 12}
    w = _windows(k, mps, 1.0)
    assert w["visited"].all() and w["runs"].max() > OVF_CAP
    # candidates of a point: level, window and lock tests (every distance is < 256)
    r = w["r"][:, None]
    cand = ((k["octave"][None, :] >= mps["level"][:, None] - 1) &
            (k["octave"][None, :] <= mps["level"][:, None]) &
            (np.abs(k["x"][None, :] - mps["proj_x"][:, None]) < r) &
            (np.abs(k["y"][None, :] - mps["proj_y"][:, None]) < r) & (locked[None, :] == 0))
    count = cand.sum(1)
    listed = (count > TOPK) & (count <= OVF_CAP)   # overflow list: the second walk
    beyond = count > OVF_CAP                       # no list: the grid re-scan
    assert listed.sum() > 50 and beyond.sum() > 50
    # a point's top-K has run dry when its K nearest candidates were claimed by
    # earlier points (all of them lock: has_obs), which the final assignment
    # shows: km_ref[i] = j < m
    assert mps["has_obs"].all()
    bits = np.unpackbits(d, axis=1)
    dry = np.zeros(m, bool)
    for i in np.nonzero(count > TOPK)[0]:
        c = np.nonzero(cand[i])[0]
        dist = (bits[c] != np.unpackbits(mpd[i])[None, :]).sum(1)
        assert dist.max() < 256
        top = c[np.argsort(dist, kind="stable")[:TOPK]]
        dry[i] = ((km_ref[top] >= 0) & (km_ref[top] < i)).all()
    assert (dry & listed).any() and (dry & beyond).any()
    assert n_ref > 0
    mt = gpu.ORBmatcher(NNRATIO)
    mt.set_resolve(schedule, 6)
    n, km = mt.SearchByProjection(gpu.Frame(k, d, SCALE, W, H), mps, mpd, 1.0, locked)
    assert n == n_ref, (n, n_ref)
    assert np.array_equal(km, km_ref), np.nonzero(km != km_ref)[0][:10]


# ------------------------------------------------------------ unstaged scan
def test_unstaged_scan(gpu):
    """More keypoints than the staged scan holds: for_features_in_area over the
    global grid, with stereo gating and locked keypoints."""
    rng = np.random.default_rng(31)
    n, m = 5000, 3000
    k, d = _synth_keys(rng, rng.uniform(1, W - 1, n).astype(np.float32),
                       rng.uniform(1, H - 1, n).astype(np.float32), rng.integers(0, 8, n))
    ur = np.where(rng.random(n) < 0.4, k["x"] - rng.uniform(5, 40, n), -1).astype(np.float32)
    locked = (rng.random(n) < 0.1).astype(np.uint8)
    src = rng.integers(0, n, m)
    mps, mpd = _onto(rng, k, d, src, 1.5)
    rs = _radius(mps, 1.0)
    mps["proj_xr"] = np.where(ur[src] > 0, ur[src] + rng.uniform(-2, 2, m) * rs,
                              mps["proj_x"] - 20).astype(np.float32)
    assert n > PROJ_STAGE
    assert (ur > 0).sum() > n // 4 and locked.sum() > n // 20
    er = np.abs(mps["proj_xr"] - ur[src])
    assert ((ur[src] > 0) & (er > rs)).any() and ((ur[src] > 0) & (er <= rs)).any()
    w = _windows(k, mps, 1.0)
    assert w["visited"].all() and (w["runs"].sum(1) > OVF_CAP).any()
    _check(gpu, k, d, mps, mpd, 1.0, locked, ur)


# ------------------------------------------------------------ batch entry point
def test_batch_entry_point(gpu):
    """search_by_projection_batch, three problems of different sizes under one
    stride, one of them without keypoints."""
    torch = pytest.importorskip("torch")
    o = _oracle()
    rng = np.random.default_rng(41)
    ns, ms = (700, 0, 300), (1200, 800, 500)
    cap, stride, B = max(ns), max(ms), 3
    keys = np.zeros((B, cap), o.KEYPOINT_DTYPE)
    desc = np.zeros((B, cap, 32), np.uint8)
    lk = np.zeros((B, cap), np.uint8)
    mps = np.zeros((B, stride), o.MP_TRACK_DTYPE)
    mpd = np.zeros((B, stride, 32), np.uint8)
    want = []
    for p, (n, m) in enumerate(zip(ns, ms)):
        if n == 0:  # a map, and nothing to match it to
            mps[p, :m]["proj_x"] = rng.uniform(0, W, m)
            mps[p, :m]["proj_y"] = rng.uniform(0, H, m)
            mps[p, :m]["in_view"] = 1
            want.append(None)
            continue
        k, d = _synth_keys(rng, rng.uniform(1, W - 1, n).astype(np.float32),
                           rng.uniform(1, H - 1, n).astype(np.float32), rng.integers(0, 8, n))
        mp, md = _onto(rng, k, d, rng.integers(0, n, m), 1.5)
        locked = (rng.random(n) < 0.1).astype(np.uint8)
        keys[p, :n], desc[p, :n], lk[p, :n], mps[p, :m], mpd[p, :m] = k, d, locked, mp, md
        want.append(o.match_projection_local(k, d, SCALE, W, H, mp, md, 1.0, NNRATIO, locked))
        assert want[-1][0] > 0
    assert len(set(ns)) == 3 and 0 in ns and len(set(ms)) == 3 and stride == max(ms)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(B, -1)).cuda()
    d_keys, d_desc, d_lk, d_mps, d_mpd = dev(keys), dev(desc), dev(lk), dev(mps), dev(mpd)
    d_n = torch.tensor(ns, dtype=torch.int32, device="cuda")
    d_m = torch.tensor(ms, dtype=torch.int32, device="cuda")
    km = torch.full((B, cap), -7, dtype=torch.int32, device="cuda")
    nm = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gpu.ORBmatcher(NNRATIO).search_by_projection_batch(
        B, d_keys.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), d_lk.data_ptr(), cap,
        d_mps.data_ptr(), d_mpd.data_ptr(), d_m.data_ptr(), stride, W, H, SCALE, 1.0,
        km.data_ptr(), nm.data_ptr())
    torch.cuda.synchronize()
    got_km, got_n = km.cpu().numpy(), nm.cpu().numpy()
    for p, ref in enumerate(want):
        if ref is None:
            assert got_n[p] == 0
            continue
        assert got_n[p] == ref[0], (p, got_n[p], ref[0])
        assert np.array_equal(got_km[p, :ns[p]], ref[1]), p
