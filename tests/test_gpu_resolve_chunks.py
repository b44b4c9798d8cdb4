"""The prefix resolve k_proj_resolve<NW> around the edges of its input ring.

The kernel keeps four blocks of W = 64 * NW points' inputs in LDS and the four
after them in flight in registers; a window [start, start + W) of points is
evaluated per round and the ring slides one block at a time as the window
moves on.  What can go wrong is a window reading a block that is not (yet, or
any more) resident, a prefetch past a problem's points, and the order of a
round's LDS accesses.  So: map sizes around the window (W) and ring (4 W)
edges, a different size for every problem of a call, and contents that move
the window in steps of 1 (a chain in which every point looks at the keypoint
its predecessor locks), in full windows (no shared candidates), and in
between; points whose top-K runs dry, with a candidate list and with the
list pool used up; pre-locked keypoints; has_obs mixed.  Every problem is
compared index-exactly (kp_match and nmatches) with the CPU oracle
(src/ORBmatcher.cc:47-133), and the call's kernel is asserted.

The last test makes more than 4,095 calls on one matcher: the candidate-list
counters are tagged with a 12-bit call generation and are cleared when it
wraps.
"""
import functools
import importlib.util
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 640, 480
TOPK, OVF_CAP, OVF_SLOTS = 4, 16, 512  # matcher_common.h
SCALE = np.float32(1.2) ** np.arange(8, dtype=np.float32)
NNRATIO = 0.8
SIZES_W1 = (0, 1, 63, 64, 65, 255, 256, 257, 320, 511, 512, 513, 1000)
SIZES_W4 = (0, 1, 255, 256, 257, 1023, 1024, 1025, 1280, 2047, 2048, 2049, 4000)
STYLES = ("disjoint", "chain", "mixed", "clusters")


def _oracle():
    import oracle as o
    o.lib()
    return o


@functools.lru_cache(maxsize=None)
def _rounds():
    """tools/attribution/resolve_rounds.py: the kernel's schedule on the CPU."""
    path = Path(__file__).resolve().parents[1] / "tools" / "attribution" / "resolve_rounds.py"
    spec = importlib.util.spec_from_file_location("resolve_rounds", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _keys(rng, x, y, octave):
    o = _oracle()
    k = np.zeros(len(x), o.KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"] = x, y, octave
    k["size"] = 31.0 * SCALE[octave]
    k["angle"] = rng.uniform(0, 360, len(x))
    k["response"] = rng.uniform(20, 200, len(x))
    k["class_id"] = -1
    return k, rng.integers(0, 256, (len(x), 32), dtype=np.uint8)


def _points(rng, x, y, level, desc, has_obs, flip=0.08):
    m = len(x)
    mps = np.zeros(m, _oracle().MP_TRACK_DTYPE)
    mps["proj_x"], mps["proj_y"], mps["proj_xr"] = x, y, -1.0
    mps["level"] = level
    mps["view_cos"] = 0.9  # radius 4 * scale[level]
    mps["in_view"] = 1
    mps["has_obs"] = has_obs
    flips = rng.random((m, 256)) < flip
    return mps, desc ^ np.packbits(flips, axis=1, bitorder="little")


def _disjoint(rng, m):
    """300 keypoints on a 20 px lattice; every point lies on a lattice site of
    its own while sites last, then on empty ones: no candidate is shared."""
    sites = np.stack(np.meshgrid(np.arange(30) * 20 + 30, np.arange(22) * 20 + 30), -1).reshape(-1, 2)
    sites = sites[rng.permutation(len(sites))].astype(np.float32)
    n = 300
    k, d = _keys(rng, sites[:n, 0], sites[:n, 1], rng.integers(0, 3, n))
    site = np.concatenate([rng.permutation(len(sites)),
                           rng.integers(n, len(sites), max(m - len(sites), 0))])[:m]
    on = site < n
    lvl = np.where(on, k["octave"][np.minimum(site, n - 1)], 1)
    desc = np.where(on[:, None], d[np.minimum(site, n - 1)], rng.integers(0, 256, (m, 32), dtype=np.uint8))
    mps, mpd = _points(rng, sites[site, 0] + rng.uniform(-1, 1, m).astype(np.float32),
                       sites[site, 1] + rng.uniform(-1, 1, m).astype(np.float32), lvl,
                       desc.astype(np.uint8), rng.random(m) < 0.7)
    return k, d, None, mps, mpd


def _chain(rng, m):
    """Keypoints 3.5 px apart along rows; point i lies 1 px before keypoint i
    (its best, a near copy of its descriptor) and sees keypoint i - 1 as well,
    which point i - 1 locks: every window commits one point.  Past the 300
    keypoints the points land on locked keypoints only."""
    n = 300
    i = np.arange(n)
    k, d = _keys(rng, (40 + 3.5 * (i % 100)).astype(np.float32), (60 + 40 * (i // 100)).astype(np.float32),
                 np.zeros(n, np.int64))
    j = np.arange(m) % n
    mps, mpd = _points(rng, k["x"][j] - 1.0, k["y"][j], np.zeros(m, np.int64), d[j], np.ones(m, bool))
    return k, d, None, mps, mpd


def _mixed(rng, m):
    """Random keypoints, points projected near random keypoints: shared
    candidates, has_obs mixed, a tenth of the keypoints locked beforehand."""
    n = int(rng.integers(60, 301))
    k, d = _keys(rng, rng.uniform(20, W - 20, n).astype(np.float32),
                 rng.uniform(20, H - 20, n).astype(np.float32), rng.integers(0, 8, n))
    src = rng.integers(0, n, m)
    mps, mpd = _points(rng, k["x"][src] + rng.uniform(-2, 2, m).astype(np.float32),
                       k["y"][src] + rng.uniform(-2, 2, m).astype(np.float32),
                       np.minimum(k["octave"][src] + rng.integers(0, 2, m), 7), d[src],
                       rng.random(m) < 0.6)
    mps["view_cos"] = np.where(rng.random(m) < 0.5, 0.999, 0.9)
    mps["in_view"] = rng.random(m) < 0.95
    return k, d, (rng.random(n) < 0.1).astype(np.uint8), mps, mpd


def _clusters(rng, m):
    """18 clusters of 10 keypoints and 2 of 20, each within 2 px: a point on a
    cluster has 10 candidates (listed) or 20 (past the lists' capacity), and
    once a cluster's keypoints are locked every later point's top-K is dry."""
    cx = np.repeat(60 + 60 * (np.arange(20) % 10), [10] * 18 + [20] * 2)
    cy = np.repeat(100 + 200 * (np.arange(20) // 10), [10] * 18 + [20] * 2)
    n = len(cx)
    k, d = _keys(rng, (cx + rng.uniform(-1, 1, n)).astype(np.float32),
                 (cy + rng.uniform(-1, 1, n)).astype(np.float32), np.full(n, 2))
    c = rng.integers(0, 20, m)
    src = np.array([rng.choice(np.nonzero((cx == 60 + 60 * (q % 10)) & (cy == 100 + 200 * (q // 10)))[0])
                    for q in c], np.int64).reshape(m)
    mps, mpd = _points(rng, (60 + 60 * (c % 10)).astype(np.float32),
                       (100 + 200 * (c // 10)).astype(np.float32), np.full(m, 2), d[src],
                       np.ones(m, bool), flip=0.15)
    return k, d, None, mps, mpd


@functools.lru_cache(maxsize=None)
def _problem(style, m):
    """One problem and its oracle result (computed once, shared by the cases)."""
    rng = np.random.default_rng(1000 * STYLES.index(style) + m)
    k, d, locked, mps, mpd = globals()["_" + style](rng, m)
    assert 60 <= len(k) <= 300
    n_ref, km_ref = _oracle().match_projection_local(k, d, SCALE, W, H, mps, mpd, 1.0, NNRATIO, locked)
    for a in (k, d, mps, mpd, km_ref):
        a.setflags(write=False)
    return k, d, locked, mps, mpd, n_ref, km_ref


def _cands(style, m):
    k, d, locked, mps, mpd, _, _ = _problem(style, m)
    return _rounds().candidate_lists(_oracle(), k, d, SCALE, W, H, mps, mpd, 1.0, locked)


def _dry(style, m):
    """Points whose top-K entries are all locked when their turn comes, split
    into those with a candidate list's worth of candidates and those past it."""
    k, _, _, mps, _, _, km_ref = _problem(style, m)
    assert mps["has_obs"].all()  # then km_ref[j] = i means: locked from point i on
    listed = beyond = 0
    for i, c in enumerate(_cands(style, m)):
        if c is None or len(c) <= TOPK:
            continue
        top = [e[0] for e in sorted(c, key=lambda e: e[1])[:TOPK]]
        if all(0 <= km_ref[j] < i for j in top):
            listed += len(c) <= OVF_CAP
            beyond += len(c) > OVF_CAP
    return listed, beyond


def _check_contents(style, sizes):
    """On the CPU: the inputs hold the situation their style names."""
    big = max(sizes)
    if style == "disjoint":
        for m in (257, big):
            seen = [e[0] for c in _cands(style, m) if c for e in c]
            assert len(seen) == len(set(seen)) and len(seen) >= min(m, 600) // 4
    elif style == "chain":
        k, _, _, mps, _, n_ref, km_ref = _problem(style, big)
        cands = _cands(style, big)
        assert mps["has_obs"].all()
        assert all(c[0][0] == i % 300 or c[1][0] == i % 300 for i, c in enumerate(cands[:300]) if len(c) > 1)
        km, n, rounds, _, commits = _rounds().replay(cands, mps["has_obs"], len(k), NNRATIO, 1)
        assert n == n_ref and np.array_equal(km, km_ref)
        # one point per round along each row of the chain (the first of a row has no predecessor)
        assert commits[:min(big, 300) - 3].count(1) >= min(big, 300) - 6, commits[:20]
    elif style == "mixed":
        k, _, locked, mps, _, n_ref, _ = _problem(style, big)
        assert locked.any() and 0 < mps["has_obs"].sum() < len(mps) and n_ref > 0
        seen = [e[0] for c in _cands(style, big) if c for e in c]
        assert len(seen) > len(set(seen))
    else:
        small = [m for m in sizes if 250 <= m <= OVF_SLOTS][-1]
        listed, _ = _dry(style, small)        # every listed point of this problem has a list
        assert listed > 0
        listed, beyond = _dry(style, big)     # more dry listed points than the pool has lists
        assert listed > OVF_SLOTS and beyond > 0, (listed, beyond)


def _run_batch(gpu, style, sizes, kernel, schedule, mp_stride=None):
    torch = pytest.importorskip("torch")
    o = _oracle()
    B = len(sizes)
    with ThreadPoolExecutor(max_workers=16) as ex:  # the oracle's calls release the GIL
        probs = list(ex.map(lambda m: _problem(style, m), sizes))
    cap = max(len(p[0]) for p in probs)
    stride = mp_stride or max(max(sizes), 1)
    keys = np.zeros((B, cap), o.KEYPOINT_DTYPE)
    desc = np.zeros((B, cap, 32), np.uint8)
    lk = np.zeros((B, cap), np.uint8)
    mps = np.zeros((B, stride), o.MP_TRACK_DTYPE)
    mpd = np.zeros((B, stride, 32), np.uint8)
    # (rows past a problem's points stay searchable: a read past nmps would match them)
    mps["in_view"] = 1
    for p, (k, d, locked, mp, md, _, _) in enumerate(probs):
        n, m = len(k), len(mp)
        keys[p, :n], desc[p, :n], mps[p, :m], mpd[p, :m] = k, d, mp, md
        if locked is not None:
            lk[p, :n] = locked
        if n:
            mps[p, m:]["proj_x"], mps[p, m:]["proj_y"] = k["x"][0], k["y"][0]
            mps[p, m:]["level"] = k["octave"][0]
            mpd[p, m:] = d[0]
    assert len({len(p[3]) for p in probs}) > 1 or B == 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(B, -1)).cuda()
    d_keys, d_desc, d_lk, d_mps, d_mpd = dev(keys), dev(desc), dev(lk), dev(mps), dev(mpd)
    d_n = torch.tensor([len(p[0]) for p in probs], dtype=torch.int32, device="cuda")
    d_m = torch.tensor([len(p[3]) for p in probs], dtype=torch.int32, device="cuda")
    km = torch.full((B, cap), -7, dtype=torch.int32, device="cuda")
    nm = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    mt = gpu.ORBmatcher(NNRATIO)
    mt.set_resolve(schedule, 6)
    assert mt.resolve_kernel(B, cap, stride) == kernel
    torch.cuda.synchronize()
    mt.search_by_projection_batch(B, d_keys.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(),
                                  d_lk.data_ptr(), cap, d_mps.data_ptr(), d_mpd.data_ptr(),
                                  d_m.data_ptr(), stride, W, H, SCALE, 1.0, km.data_ptr(),
                                  nm.data_ptr())
    torch.cuda.synchronize()
    got_km, got_n = km.cpu().numpy(), nm.cpu().numpy()
    for p, (k, _, _, mp, _, n_ref, km_ref) in enumerate(probs):
        assert got_n[p] == n_ref, (p, len(mp), got_n[p], n_ref)
        assert np.array_equal(got_km[p, :len(k)], km_ref), \
            (p, len(mp), np.nonzero(got_km[p, :len(k)] != km_ref)[0][:10])
    assert sum(p[5] for p in probs) > 0


@pytest.mark.parametrize("style", STYLES)
def test_one_wave_128_problems(gpu, style):
    """RESOLVE_W1_MIN problems: the smallest call that takes k_proj_resolve<1>."""
    _check_contents(style, SIZES_W1)
    sizes = [SIZES_W1[(p * 5) % len(SIZES_W1)] for p in range(128)]
    assert set(sizes) == set(SIZES_W1)
    _run_batch(gpu, style, sizes, "k_proj_resolve<1>", 0)


@pytest.mark.parametrize("style", STYLES)
def test_four_waves(gpu, style):
    """k_proj_resolve<4>: 16 problems by shape, and 4 problems under the prefix
    schedule (by shape a call that small takes the fixed-point kernel)."""
    _check_contents(style, SIZES_W4)
    _run_batch(gpu, style, list(SIZES_W4) + [257, 1025, 2049], "k_proj_resolve<4>", 0)
    _run_batch(gpu, style, [1025, 257, 4000, 2049], "k_proj_resolve<4>", 1)


def test_eight_waves(gpu):
    """k_proj_resolve<8> (512-point windows, 2,048-point ring): the prefix
    schedule on a map stride of 20,000."""
    for style in ("chain", "clusters"):
        _run_batch(gpu, style, [2049, 513, 4000], "k_proj_resolve<8>", 1, mp_stride=20000)


def test_kpmatch_in_global_memory(gpu):
    """A frame whose 8 B per keypoint the host keeps out of LDS: kpMatch takes
    global atomics, as it did before the result was kept in LDS."""
    rng = np.random.default_rng(77)
    n, m = 6000, 1500
    k, d = _keys(rng, rng.uniform(20, W - 20, n).astype(np.float32),
                 rng.uniform(20, H - 20, n).astype(np.float32), rng.integers(0, 8, n))
    src = rng.integers(0, n, m)
    mps, mpd = _points(rng, k["x"][src] + rng.uniform(-2, 2, m).astype(np.float32),
                       k["y"][src] + rng.uniform(-2, 2, m).astype(np.float32),
                       np.minimum(k["octave"][src] + rng.integers(0, 2, m), 7), d[src],
                       rng.random(m) < 0.6)
    locked = (rng.random(n) < 0.1).astype(np.uint8)
    n_ref, km_ref = _oracle().match_projection_local(k, d, SCALE, W, H, mps, mpd, 1.0, NNRATIO, locked)
    assert n_ref > 0 and n * 8 + 4 * 5200 > 64 * 1024
    mt = gpu.ORBmatcher(NNRATIO)
    mt.set_resolve(mt.RESOLVE_PREFIX, 6)
    assert mt.resolve_kernel(1, n, m) == "k_proj_resolve<4>"
    got_n, km = mt.SearchByProjection(gpu.Frame(k, d, SCALE, W, H), mps, mpd, 1.0, locked)
    assert got_n == n_ref and np.array_equal(km, km_ref)


def test_generation_wrap(gpu):
    """More than 4,095 calls on one matcher, each with listed points whose
    top-K runs dry, exact before and after the 12-bit generation wraps."""
    k, d, locked, mps, mpd, n_ref, km_ref = _problem("clusters", 320)
    listed, _ = _dry("clusters", 320)
    assert listed > 0 and n_ref > 0
    mt = gpu.ORBmatcher(NNRATIO)
    mt.set_resolve(mt.RESOLVE_PREFIX, 6)
    assert mt.resolve_kernel(1, len(k), len(mps)) == "k_proj_resolve<4>"
    F = gpu.Frame(k, d, SCALE, W, H)
    bad = []
    for call in range(4200):
        n, km = mt.SearchByProjection(F, mps, mpd, 1.0, locked)
        if n != n_ref or not np.array_equal(km, km_ref):
            bad.append(call)
    assert not bad, bad[:10]
