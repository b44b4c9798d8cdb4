"""Directed inputs for ORBmatcher::SearchForInitialization (k_init_prep,
k_init_candidates, k_init_resolve) and MapPoint::ComputeDistinctiveDescriptors
(k_distinctive), built where the natural frames and the random crowds never
go: each CASES entry is (builder, census minimum).

A SearchForInitialization case is dict(kind="init", problems=[...]); a problem
holds the arguments of one call (k1, d1, k2, d2, prev, w, h, window, nnratio,
check) and, for the shifted_bounds case, the grid bounds and the shift of the
batch entry.  The distinctive case is dict(kind="distinctive", offs, desc, init).

census() is computed from the reference loop alone: it replays
pyref.search_for_initialization with a trace (per query: its candidates in scan
order and the vMatchedDistance of each when the query is processed) and derives
from that, by the rules written in mapping_kernels.hip, which path every query
must take: committed from its top-K list, exact although the top-K ran dry,
resolved wave-wide from its list, or rescanned on one lane; which lane of which
batch holds a conflict, and on which of its two keypoints.  While it does so it
checks that what the speculative batches would commit is what the sequential
loop did.  It never reads the kernels' scratch.

test_mapping_edge_cases.py shows on the CPU that the oracle equals pyref on
these inputs, that the census minimums hold and that every wrong neighbour of a
rule (the `rules` of pyref.search_for_initialization / distinctive_descriptor)
changes a named case's answer; test_gpu_mapping_edges.py runs them through the
kernels."""
import math

import numpy as np

import pyref
from matcher_edge_cases import KEYPOINT_DTYPE, _hist_angles

f32 = np.float32
W, H = 640, 480
WAVE = 64   # queries per speculative batch of k_init_resolve
_LIMITS = None


def limits():
    """topk, list, stage and max_stride of the build (16, 256, 1536, 10232)."""
    global _LIMITS
    if _LIMITS is None:
        from conftest import load_pkg
        _LIMITS = load_pkg().ORBmatcher.search_init_limits()
    return _LIMITS


# ------------------------------------------------------------------ the scene
class Scene:
    """One SearchForInitialization problem under construction.  Sites are
    window centres on a lattice of pitch 4 * window, so that the windows of two
    sites never share a keypoint; all coordinates are integers unless a builder
    says otherwise."""

    def __init__(self, name, window, nnratio=0.9, check=False, seed=1, interleave=0):
        self.name, self.window, self.nnratio, self.check = name, window, nnratio, check
        self.rng = np.random.default_rng(seed)
        self.k1, self.d1, self.prev, self.k2, self.d2 = [], [], [], [], []
        self.pitch = 4 * window
        self.cols = (W - self.pitch) // self.pitch
        self.nsite = 0
        self.interleave, self.nq = interleave, 0

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def near(self, d, dist, lo=0, hi=256):
        """A descriptor exactly `dist` bits from d, the bits drawn from [lo, hi)."""
        bits = np.unpackbits(np.asarray(d, np.uint8))
        bits[lo + self.rng.permutation(hi - lo)[:dist]] ^= 1
        return np.packbits(bits)

    def site(self):
        i = self.nsite
        self.nsite += 1
        c = (self.pitch * (1 + i % self.cols), self.pitch * (1 + i // self.cols))
        assert c[1] + self.pitch <= H, (self.name, "out of sites")
        return c

    def f2(self, x, y, desc, octave=0, angle=0.0):
        self.k2.append((f32(x), f32(y), int(octave), f32(angle)))
        self.d2.append(np.asarray(desc, np.uint8))
        return len(self.k2) - 1

    def f1(self, px, py, desc, octave=0, angle=0.0):
        """A keypoint of F1 whose vbPrevMatched entry is (px, py).  With
        `interleave`, every interleave-th level-0 query is preceded by a copy
        at octave 1, so that query slots differ from keypoint indices and the
        copy would take the match first if the level filter were dropped."""
        if octave == 0:
            if self.interleave and self.nq % self.interleave == 0:
                self.f1(px, py, desc, 1, angle)
            self.nq += 1
        self.k1.append((f32(px), f32(py), int(octave), f32(angle)))
        self.d1.append(np.asarray(desc, np.uint8))
        self.prev.append((f32(px), f32(py)))
        return len(self.k1) - 1

    def place(self, centre, a, queries, offsets=None, angles2=None):
        """Keypoints of F2 at centre + offsets[i], keypoint i a base descriptor
        with a private block of a[i] bits flipped, and one descriptor per entry
        (s, p) of `queries`: the base with s[i] bits of block i and p private
        bits flipped, which is a[i] - 2 s[i] + sum(s) + p bits from keypoint i.
        Returns (F2 indices, query descriptors, the distance matrix)."""
        k = len(a)
        offsets = offsets or [(i - k // 2, (i * 2) % 3 - 1) for i in range(k)]
        at = np.concatenate([[0], np.cumsum(a)]).astype(int)
        assert at[-1] + max(p for _, p in queries) <= 256
        base = np.unpackbits(self.desc())
        ids, qs = [], []
        for i in range(k):
            b = base.copy()
            b[at[i]:at[i + 1]] ^= 1
            ids.append(self.f2(centre[0] + offsets[i][0], centre[1] + offsets[i][1], np.packbits(b),
                               angle=0.0 if angles2 is None else angles2[i]))
        for s, p in queries:
            b = base.copy()
            for i in range(k):
                assert 0 <= s[i] <= a[i]
                b[at[i]:at[i] + s[i]] ^= 1
            b[at[-1]:at[-1] + p] ^= 1
            qs.append(np.packbits(b))
        D = [[pyref.hamming(q, self.d2[i]) for i in ids] for q in qs]
        for (s, p), row in zip(queries, D):
            assert row == [a[i] - 2 * s[i] + sum(s) + p for i in range(k)]
        return ids, qs, D

    def one(self, centre, dists, offsets=None, angles2=None):
        """Keypoints at exactly `dists` from one query descriptor (the base)."""
        ids, qs, D = self.place(centre, dists, [((0,) * len(dists), 0)], offsets, angles2)
        assert D[0] == list(dists)
        return ids, qs[0]

    def solo(self, d1=10, d2=40, a1=0.0, a2=0.0):
        """A site of its own: two keypoints at d1 and d2 and one query."""
        c = self.site()
        ids, q = self.one(c, (d1, d2), angles2=[a2, a2])
        return self.f1(c[0], c[1], q, angle=a1), ids[0]

    def crowd(self, dists, kill, lone=False):
        """A site of len(dists) keypoints on the integer lattice inside the
        window, in random scan positions, keypoint j at dists[j] from the
        query Q.  For every j in `kill` an earlier query with keypoint j's own
        descriptor takes it at distance 0, so Q meets it with
        vMatchedDistance 0.  With `lone`, the flipped bits of the killed
        keypoints are disjoint blocks and a keypoint with Q's own descriptor is
        added: every killer's second best is that keypoint, which nobody claims,
        so the killers do not conflict in a batch.  Returns the call that
        appends Q to F1 (after the killers, wherever the builder wants it)."""
        c, r = self.site(), self.window - 1
        spots = [(dx, dy) for dx in range(-r, r + 1) for dy in range(-r, r + 1)]
        spots = [spots[i] for i in self.rng.permutation(len(spots))]
        q = self.desc()
        n = len(dists)
        assert n + lone <= len(spots)
        descs, at = [], 0
        for j, dj in enumerate(dists):
            if lone and j in kill:
                descs.append(self.near(q, dj, at, at + dj))
                at += dj
            elif lone:
                descs.append(self.near(q, dj, 128, 256))
            else:
                descs.append(self.near(q, dj))
        assert at <= 128
        for j in range(n):
            self.f2(c[0] + spots[j][0], c[1] + spots[j][1], descs[j])
        if lone:
            self.f2(c[0] + spots[n][0], c[1] + spots[n][1], q)
        for j in kill:
            self.f1(c[0], c[1], descs[j])
        return lambda: self.f1(c[0], c[1], q)

    def problem(self, **extra):
        def keys(rows):
            k = np.zeros(len(rows), KEYPOINT_DTYPE)
            for i, (x, y, o, a) in enumerate(rows):
                k[i]["x"], k[i]["y"], k[i]["octave"], k[i]["angle"] = x, y, o, a
            k["size"] = 31.0
            return k
        p = dict(name=self.name, k1=keys(self.k1), k2=keys(self.k2),
                 d1=np.array(self.d1, np.uint8).reshape(-1, 32),
                 d2=np.array(self.d2, np.uint8).reshape(-1, 32),
                 prev=np.array(self.prev, f32).reshape(-1, 2), w=W, h=H, window=self.window,
                 nnratio=self.nnratio, check=self.check)
        p.update(extra)
        return p


# ---------------------------------------------------------------- entry points
def _args(p):
    return (p["k1"], p["d1"], p["k2"], p["d2"], p["w"], p["h"], p["prev"], p["window"],
            p["nnratio"], p["check"])


def _unshifted(p):
    return p.get("base", p)


def run_oracle(o, p):
    """(n, m12, prev) of one problem.  A shifted problem's answer is that of
    the scene it was shifted from, with prev moved by the (exact) shift."""
    n, m12, prev = o.search_for_initialization(*_args(_unshifted(p)))
    return n, m12, (prev + f32(p.get("shift", 0.0))).astype(f32)


def run_pyref(p, rules=(), trace=None):
    n, m12, prev = pyref.search_for_initialization(*_args(_unshifted(p)), rules=rules, trace=trace)
    return n, m12, (prev + f32(p.get("shift", 0.0))).astype(f32)


def run_gpu(gpu, p):
    """The single-frame call (grid bounds 0..w, 0..h: unshifted problems only)."""
    assert "bounds" not in p
    m = gpu.ORBmatcher(p["nnratio"], p["check"])
    F1 = gpu.Frame(p["k1"], p["d1"], np.ones(8, f32), p["w"], p["h"])
    F2 = gpu.Frame(p["k2"], p["d2"], np.ones(8, f32), p["w"], p["h"])
    return m.SearchForInitialization(F1, F2, p["prev"], p["window"])


def batch_key(p):
    """Problems that one batch call can hold share these."""
    return (p["window"], float(p["nnratio"]), bool(p["check"]),
            tuple(p.get("bounds", (0.0, float(p["w"]), 0.0, float(p["h"])))))


JUNK_M12, JUNK_PREV = -7, -7777.0


class Batch:
    """The device arrays of one orb_search_for_initialization_batch call over
    `problems` (one batch_key).  Slots past each count hold junk."""

    def __init__(self, torch, problems, stride):
        self.key = batch_key(problems[0])
        assert all(batch_key(p) == self.key for p in problems)
        self.problems, self.stride, self.torch = problems, stride, torch
        P = self.P = len(problems)
        rng = np.random.default_rng(99)
        K1 = rng.integers(0, 1 << 30, (P, stride, 7), dtype=np.int32)    # junk keypoints
        K2 = rng.integers(0, 1 << 30, (P, stride, 7), dtype=np.int32)
        D1 = rng.integers(0, 256, (P, stride, 32), dtype=np.uint8)
        D2 = rng.integers(0, 256, (P, stride, 32), dtype=np.uint8)
        PR = np.full((P, stride, 2), JUNK_PREV, f32)
        n1 = np.array([len(p["k1"]) for p in problems], np.int32)
        n2 = np.array([len(p["k2"]) for p in problems], np.int32)
        assert max(n1.max(), n2.max()) <= stride
        for i, p in enumerate(problems):
            K1[i, :n1[i]] = np.ascontiguousarray(p["k1"]).view(np.int32).reshape(-1, 7)
            K2[i, :n2[i]] = np.ascontiguousarray(p["k2"]).view(np.int32).reshape(-1, 7)
            D1[i, :n1[i]], D2[i, :n2[i]], PR[i, :n1[i]] = p["d1"], p["d2"], p["prev"]
        self.PR0 = PR
        self.t = {k: torch.from_numpy(v).to("cuda")
                  for k, v in dict(K1=K1, K2=K2, D1=D1, D2=D2, PR=PR, n1=n1, n2=n2).items()}
        self.m12 = torch.full((P, stride), JUNK_M12, dtype=torch.int32, device="cuda")
        self.nm = torch.full((P,), JUNK_M12, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def launch(self, matcher, stream=0, n_problems=None, stride=None, bounds=None):
        t, b = self.t, bounds or self.key[3]
        matcher.search_for_initialization_batch(
            self.P if n_problems is None else n_problems, t["K1"].data_ptr(), t["D1"].data_ptr(),
            t["n1"].data_ptr(), t["K2"].data_ptr(), t["D2"].data_ptr(), t["n2"].data_ptr(),
            self.stride if stride is None else stride, b[0], b[1], b[2], b[3], self.key[0],
            t["PR"].data_ptr(), self.m12.data_ptr(), self.nm.data_ptr(), stream)

    def reset(self):
        """prev as it was given, junk in the outputs."""
        self.t["PR"].copy_(self.torch.from_numpy(self.PR0))
        self.m12.fill_(JUNK_M12)
        self.nm.fill_(JUNK_M12)
        self.torch.cuda.synchronize()

    def fetch(self):
        """(n [P], m12 [P, stride], prev [P, stride, 2]) as the device holds them."""
        self.torch.cuda.synchronize()
        return self.nm.cpu().numpy(), self.m12.cpu().numpy(), self.t["PR"].cpu().numpy()

    def untouched(self):
        nm, m12, prev = self.fetch()
        return (nm == JUNK_M12).all() and (m12 == JUNK_M12).all() and all(
            prev[i, :len(p["k1"])].tobytes() == p["prev"].tobytes() and
            (prev[i, len(p["k1"]):] == f32(JUNK_PREV)).all() for i, p in enumerate(self.problems))


def run_gpu_batch(gpu, torch, problems, stride, matcher=None, stream=0):
    """One batch call; the matcher's nnratio and orientation check are the
    problems'.  Returns Batch.fetch()."""
    b = Batch(torch, problems, stride)
    b.launch(matcher or gpu.ORBmatcher(b.key[1], b.key[2]), stream)
    return b.fetch()


def check_batch(problems, refs, got, what=""):
    """n, m12 and the prev bytes of every problem; junk past N1 untouched."""
    nm, m12, prev = got
    for i, (p, (rn, rm, rp)) in enumerate(zip(problems, refs)):
        n1 = len(p["k1"])
        tag = (what, p["name"], i)
        assert nm[i] == rn, tag + (int(nm[i]), rn)
        assert np.array_equal(m12[i, :n1], rm), tag + (np.nonzero(m12[i, :n1] != rm)[0][:10],)
        assert prev[i, :n1].tobytes() == rp.tobytes(), tag + ("prev",)
        assert (m12[i, n1:] == JUNK_M12).all(), tag + ("m12 written past N1",)
        assert (prev[i, n1:] == f32(JUNK_PREV)).all(), tag + ("prev written past N1",)


def distinctive_pyref(c, rules=()):
    offs = c["offs"]
    return np.array([pyref.distinctive_descriptor(c["desc"][offs[i]:offs[i + 1]], rules)
                     for i in range(len(offs) - 1)], np.int32)


def distinctive_expected_out(c, best):
    """Row p = the chosen descriptor; rows of empty lists keep their input."""
    out = c["init"].copy()
    has = best >= 0
    out[has] = c["desc"][c["offs"][:-1][has] + best[has]]
    return out


# --------------------------------------------------------------------- census
def _cell_range(p, x, y):
    """GetFeaturesInArea's cell range for a window centre, or the exit taken."""
    invW, invH, r = f32(f32(64) / f32(p["w"])), f32(f32(48) / f32(p["h"])), f32(p["window"])
    x, y = f32(x), f32(y)
    x0 = max(0, int(math.floor(float(f32(f32(x - r) * invW)))))
    if x0 >= 64:
        return "x0"
    x1 = min(63, int(math.ceil(float(f32(f32(x + r) * invW)))))
    if x1 < 0:
        return "x1"
    y0 = max(0, int(math.floor(float(f32(f32(y - r) * invH)))))
    if y0 >= 48:
        return "y0"
    y1 = min(47, int(math.ceil(float(f32(f32(y + r) * invH)))))
    if y1 < 0:
        return "y1"
    return x0, x1, y0, y1


def census(p, traced=None):
    """What one problem reaches (see the module docstring).  `traced`: the
    (n, trace) of a run_pyref call already made on p, to spare a second one."""
    L = limits()
    TOPK, LIST = L["topk"], L["list"]
    p = _unshifted(p)
    if traced is None:
        tr = []
        n = pyref.search_for_initialization(*_args(p), trace=tr)[0]
    else:
        n, tr = traced
    k1, k2, r, nn = p["k1"], p["k2"], f32(p["window"]), p["nnratio"]
    cells, _, _ = pyref.grid_cells(k2, p["w"], p["h"])
    ns = sum(1 for v in cells.values() for i in v if k2[i]["octave"] == 0)
    cen = dict(N1=len(k1), N2=len(k2), nq=len(tr), ns=ns, staged=ns <= L["stage"], n=int(n),
               slot_ne_index=sum(t["i1"] != k for k, t in enumerate(tr)))
    # ---- per query, at the moment the sequential loop processes it
    nc_set, dry, accepts, steals = set(), {}, 0, 0
    eq = dict(mdist_eq=0, mdist_above=0, b1_50=0, b1_51=0, ratio_eq=0, ratio_below=0, win_eq_x=0,
              win_eq_y=0, win_inside=0, tie_best=0, tie_accept=0)
    edges = dict(col0=0, col63=0, row0=0, row47=0)
    exits = set()
    order_of = []
    # the level-0 keypoints of F2 that the grid holds, with their cells
    grid = [(i, cx, cy) for (cx, cy), ids in cells.items() for i in ids if k2[i]["octave"] == 0]
    g_i, g_cx, g_cy = (np.array(v, np.int64) for v in zip(*grid)) if grid else (np.zeros(0, np.int64),) * 3
    g_x, g_y = k2["x"][g_i].astype(f32), k2["y"][g_i].astype(f32)
    for t in tr:
        cand, md = t["cand"], t["mdist"]
        nc = len(cand)
        nc_set.add(nc)
        order = sorted(range(nc), key=lambda j: (cand[j][1], j))     # (distance, scan order)
        order_of.append(order)
        alive = [md[j] > cand[j][1] for j in order]
        t["rank"] = [i for i, a in enumerate(alive) if a][:2]        # first and second survivor
        if sum(alive[:TOPK]) < 2:
            dry[nc] = dry.get(nc, 0) + 1
        accepts += t["accept"]
        steals += t["stole"] >= 0
        eq["mdist_eq"] += any(md[j] == cand[j][1] for j in range(nc))
        eq["mdist_above"] += any(md[j] == cand[j][1] + 1 for j in range(nc))
        if t["bi"] >= 0:
            lim = f32(f32(t["b2"]) * f32(nn))
            ok = f32(t["b1"]) < lim
            eq["b1_50"] += t["b1"] == 50 and t["accept"]
            eq["b1_51"] += t["b1"] == 51 and bool(ok)    # only TH_LOW rejects it
            if t["b1"] <= 50 and t["b2"] < (1 << 31):
                eq["ratio_eq"] += f32(t["b1"]) == lim
                eq["ratio_below"] += f32(t["b1"] + 1) == lim
            if t["b1"] == t["b2"]:
                eq["tie_best"] += 1
                eq["tie_accept"] += t["accept"]
        x, y = p["prev"][t["i1"]]
        cr = _cell_range(p, x, y)
        if isinstance(cr, str):
            exits.add(cr)
            continue
        edges["col0"] += cr[0] == 0
        edges["col63"] += cr[1] == 63
        edges["row0"] += cr[2] == 0
        edges["row47"] += cr[3] == 47
        dx, dy = np.abs(g_x - f32(x)), np.abs(g_y - f32(y))
        inr = (cr[0] <= g_cx) & (g_cx <= cr[1]) & (cr[2] <= g_cy) & (g_cy <= cr[3])
        eq["win_eq_x"] += int((inr & (dx == r) & (dy < r)).sum())
        eq["win_eq_y"] += int((inr & (dy == r) & (dx < r)).sum())
        eq["win_inside"] += int((inr & (np.maximum(dx, dy) == r - f32(0.125))).sum())
    # steal chains: how often one keypoint changes hands
    taken = {}
    for t in tr:
        if t["stole"] >= 0:
            taken[t["bi"]] = taken.get(t["bi"], 0) + 1
    cen.update(nc=sorted(nc_set), dry=dry, accepts=accepts, steals=steals,
               chain=max(taken.values(), default=0), exits=sorted(exits), **eq, **edges)
    # ---- the speculative batches of k_init_resolve, from the same trace
    md, start = {}, 0
    paths = dict(topk=0, dry_exact=0, list=0, rescan=0)
    conflict_lanes, slow_lanes, si_only, full_clean, batches, chunks = set(), set(), 0, 0, 0, set()
    while start < len(tr):
        batches += 1
        lanes, claim = [], {}
        for lane in range(min(WAVE, len(tr) - start)):
            t = tr[start + lane]
            cand = t["cand"]
            got = [cand[j] for j in order_of[start + lane][:TOPK]
                   if md.get(cand[j][0], 1 << 31) > cand[j][1]][:2]
            b1, bi = (got[0][1], got[0][0]) if got else (1 << 31, -1)
            b2, si = (got[1][1], got[1][0]) if len(got) > 1 else (1 << 31, -1)
            slow = len(got) < 2 and len(cand) > TOPK
            acc = not slow and bi >= 0 and b1 <= 50 and f32(b1) < f32(f32(b2) * f32(nn))
            if acc:
                claim[bi] = min(claim.get(bi, WAVE), lane)
            lanes.append((slow, acc, bi, si, len(got), len(cand)))
        commit = WAVE
        for lane, (slow, acc, bi, si, found, nc) in enumerate(lanes):
            on_bi = bi >= 0 and claim.get(bi, WAVE) < lane
            on_si = si >= 0 and claim.get(si, WAVE) < lane
            if slow or on_bi or on_si:
                commit = lane
                if slow:
                    slow_lanes.add(lane)
                    paths["list" if nc <= LIST else "rescan"] += 1
                    if nc <= LIST:      # list positions (scan order) of the two survivors
                        t = tr[start + lane]
                        pos = [order_of[start + lane][i] for i in t["rank"]]
                        chunks.add(tuple(q // WAVE for q in pos))
                else:
                    conflict_lanes.add(lane)
                    si_only += on_si and not on_bi
                break
        for lane in range(min(commit, len(lanes))):
            slow, acc, bi, si, found, nc = lanes[lane]
            t = tr[start + lane]
            # what the batch commits is what the sequential loop did
            assert acc == t["accept"] and (not acc or bi == t["bi"]), (p["name"], start, lane)
            paths["dry_exact" if found < 2 and nc > 0 else "topk"] += 1
        full_clean += commit == WAVE and len(lanes) == WAVE
        advance = commit + 1 if commit < len(lanes) and lanes[commit][0] else min(commit, len(lanes))
        for t in tr[start:start + advance]:
            if t["accept"]:
                md[t["bi"]] = t["b1"]
        start += advance
    cen.update(paths=paths, conflict_lanes=sorted(conflict_lanes), slow_lanes=sorted(slow_lanes),
               si_only=si_only, full_clean=full_clean, batches=batches, list_chunks=sorted(chunks))
    # ---- the histogram: do the votes of stolen queries decide the kept bins?
    if p["check"]:
        votes, stolen = [0] * 30, [0] * 30
        owner = {}
        for t in tr:
            if t["accept"]:
                b = pyref._rot_bin(k1[t["i1"]]["angle"], k2[t["bi"]]["angle"])
                votes[b] += 1
                if t["bi"] in owner:
                    stolen[owner[t["bi"]]] += 1
                owner[t["bi"]] = b
        live = [v - s for v, s in zip(votes, stolen)]
        cen.update(stolen_votes=sum(stolen),
                   stolen_votes_decide=pyref._three_maxima(votes) != pyref._three_maxima(live))
    return cen


# ---------------------------------------------------------------------- cases
def _counts(nnratio):
    sc = Scene("counts_nn%g" % nnratio, 10, nnratio, seed=3)
    later = []
    q = sc.desc()
    c = sc.site()                                       # 0 candidates: nothing there
    sc.f1(c[0], c[1], q)
    c = sc.site()                                       # 0 candidates: only an octave-1 keypoint
    sc.f2(c[0] + 1, c[1], q, octave=1)
    sc.f1(c[0], c[1], q)
    c = sc.site()                                       # 1 candidate
    sc.f2(c[0], c[1] + 2, sc.near(q, 20))
    sc.f1(c[0], c[1], q)
    sc.solo()                                           # 2 candidates
    L = limits()
    TOPK, LIST = L["topk"], L["list"]
    low = list(range(1, TOPK + 1))
    far = lambda n: [int(v) for v in sc.rng.integers(60, 121, n)]
    # 16 candidates, 15 taken: exact although the top-K ran dry (accepts, b2 = inf)
    later.append(sc.crowd(low[:-1] + [30], range(TOPK - 1)))
    later.append(sc.crowd(low, range(TOPK)))            # 16, all taken: nothing survives
    later.append(sc.crowd(low[:-2] + [30, 33], range(TOPK - 2)))   # 16, two survive: 30 vs 33 rejects
    later.append(sc.crowd(low + [30], range(TOPK)))     # 17, the survivor at rank 16: first slow
    # 17, survivors at ranks 15 and 16 (35 vs 38 rejects; with the top-K alone 35 would pass)
    later.append(sc.crowd(list(range(20, 20 + TOPK)) + [38], range(TOPK - 1)))
    for n in (LIST, LIST + 1):                          # the list and the lane-0 rescan
        later.append(sc.crowd(low + [30, 40] + far(n - TOPK - 2), range(TOPK)))
        later.append(sc.crowd(low + [30, 30] + far(n - TOPK - 2), range(TOPK)))   # tied survivors
    for q_ in later:
        q_()
    return sc.problem()


def counts():
    """One scene under nnratio 0.9 and 1.25 (the latter accepts tied bests)."""
    return dict(kind="init", problems=[_counts(0.9), _counts(1.25)])


def _solos(sc, n):
    for i in range(n):
        sc.solo(10 + 2 * (i % 5), 40 + 2 * (i % 7))


def batch_lanes():
    probs = []
    # 63 queries: slots 0 and 1 want the same keypoint; lane 1 would accept A at 7,
    # but the sequential loop skips A (5 <= 7) and takes B
    sc = Scene("lanes_63", 5, seed=4, interleave=3)
    c = sc.site()
    _, qs, D = sc.place(c, (5, 17, 40), [((0, 0, 0), 0), ((0, 2, 0), 0)])
    assert D == [[5, 17, 40], [7, 15, 42]]
    sc.f1(c[0], c[1], qs[0])
    sc.f1(c[0], c[1], qs[1])
    _solos(sc, 61)
    probs.append(sc.problem())
    # 64 queries, no shared keypoint: one full batch commits
    sc = Scene("lanes_64", 5, seed=5, interleave=2)
    c = sc.site()
    sc.f1(c[0], c[1], sc.desc())                                  # no candidate
    c = sc.site()
    q = sc.desc()
    sc.f2(c[0], c[1], sc.near(q, 12))                             # one candidate
    sc.f1(c[0], c[1], q)
    _solos(sc, 62)
    probs.append(sc.problem())
    # 65 queries: slot 63 conflicts with slot 0 on its best (lane 63); the next
    # batch starts there, and slot 64 (lane 1) has its second best claimed by
    # lane 0: with B at 30 still alive 28 vs 30 rejects, without it 28 vs 88 accepts
    sc = Scene("lanes_65", 5, seed=6, interleave=4)
    c = sc.site()
    _, qs, D = sc.place(c, (4, 18, 40, 60),
                        [((0, 0, 0, 0), 0), ((0, 2, 0, 0), 0), ((0, 8, 20, 0), 0)])
    assert D == [[4, 18, 40, 60], [6, 16, 42, 62], [32, 30, 28, 88]]
    sc.f1(c[0], c[1], qs[0])
    _solos(sc, 62)
    sc.f1(c[0], c[1], qs[1])
    sc.f1(c[0], c[1], qs[2])
    probs.append(sc.problem())
    # 129 queries: 15 killers and 49 others fill batch one without a conflict;
    # slot 64 is slow at lane 0 (17 candidates, one survivor in its top 16);
    # slots 65..128 are a second full batch
    sc = Scene("lanes_129", 5, seed=7, interleave=5)
    slow = sc.crowd(list(range(1, 16)) + [20], range(15), lone=True)
    _solos(sc, 49)
    slow()
    _solos(sc, 64)
    probs.append(sc.problem())
    return dict(kind="init", problems=probs)


def _equalities(nnratio, snap=True):
    sc = Scene("equalities_nn%g" % nnratio, 10, nnratio, seed=8)
    r = 10
    # vMatchedDistance == d: skipped; one above: stolen
    for s_b, second in ((20, [20, 30]), (19, [19, 31])):
        c = sc.site()
        _, qs, D = sc.place(c, (0, 50), [((0, 0), 20), ((0, s_b), 0)])
        assert D == [[20, 70], second]
        sc.f1(c[0], c[1], qs[0])
        sc.f1(c[0], c[1], qs[1])
    for t in ((50, 100), (51, 101), (45, 50), (44, 50)):   # TH_LOW and the ratio, both sides
        c = sc.site()
        _, q = sc.one(c, t)
        sc.f1(c[0], c[1], q)
    # |dx| == r, |dy| == r (outside) and one eighth less (inside); the near
    # keypoint is the better match, the centre one the fallback
    for off in ((r, 0), (r - 0.125, 0), (0, -r), (0, -r + 0.125), (-r, 3), (2, r - 0.125)):
        c = sc.site()
        _, q = sc.one(c, (10, 45), offsets=[off, (0, 0)])
        sc.f1(c[0], c[1], q)
    # equal best distances at two scan positions; the keypoint with the lower
    # index lies in the later grid column, so scan order is not index order
    for t in ((20, 20, 60), (20, 20, 20)):
        c = sc.site()
        _, q = sc.one(c, t, offsets=[(7, 0), (-7, 0), (0, 3)])
        sc.f1(c[0], c[1], q)
    _solos(sc, 6)
    return sc.problem()


def equalities():
    return dict(kind="init", problems=[_equalities(0.9), _equalities(1.25)])


SHIFT = -16.0


def shifted_bounds():
    """The equalities scenes moved by (-16, -16) under the grid bounds
    (-16, w - 16, -16, h - 16).  Every coordinate is a multiple of 1/8 below
    1024, so both the shift and the kernels' subtraction of minX are exact:
    m12 is that of the unshifted scene and prev the unshifted one moved."""
    probs = []
    for base in equalities()["problems"]:
        p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        for k in (p["k1"], p["k2"]):
            for ax in ("x", "y"):
                assert (k[ax] * 8 == np.round(k[ax] * 8)).all() and (np.abs(k[ax]) < 1024).all()
                k[ax] = k[ax] + f32(SHIFT)
        assert (p["prev"] * 8 == np.round(p["prev"] * 8)).all()
        p["prev"] = (p["prev"] + f32(SHIFT)).astype(f32)
        for a, b in ((p["k2"], base["k2"]), (p["k1"], base["k1"])):
            assert np.array_equal(a["x"] - f32(SHIFT), b["x"]) and np.array_equal(a["y"] - f32(SHIFT), b["y"])
        p.update(name="shifted_" + base["name"], base=base, shift=SHIFT,
                 bounds=(SHIFT, W + SHIFT, SHIFT, H + SHIFT))
        probs.append(p)
    return dict(kind="init", problems=probs)


# bins of the three stolen votes of the chain, and of its last owner
CHAIN_BINS = {"four_tied": ((11, 11, 20), 2), "ten_two_one": ((4, 4, 4), 1)}


def steal_hist():
    """Orientation check on.  The live matches fill the histogram as
    matcher_edge_cases.HIST_SHAPES says; one keypoint is taken at 30 and
    stolen at 20, 10 and 4, and the three stolen queries' votes stay
    (src/ORBmatcher.cc:524-527).  four_tied: bin 11 rises from 3 to 5 and
    displaces bin 9.  ten_two_one: bin 4 rises from 10 to 13, and bin 12's
    single vote falls below a tenth of it."""
    probs = []
    for shape, (stolen, last) in sorted(CHAIN_BINS.items()):
        sc = Scene("steal_hist_" + shape, 5, check=True, seed=9, interleave=4)
        ang = _hist_angles(shape)
        for a1, a2, b in ang[:len(ang) // 2]:
            sc.solo(a1=a1, a2=a2)
        c = sc.site()
        _, qs, D = sc.place(c, (0, 60), [((0, 0), t) for t in (30, 20, 10, 4)],
                            angles2=[40.0, 40.0])
        assert D == [[30, 90], [20, 80], [10, 70], [4, 64]]
        for q, b in zip(qs, stolen + (last,)):
            sc.f1(c[0], c[1], q, angle=30.0 * b + 40.0)
        for a1, a2, b in ang[len(ang) // 2:]:
            sc.solo(a1=a1, a2=a2)
        probs.append(sc.problem())
    return dict(kind="init", problems=probs)


def _stage(n_level0):
    """n_level0 level-0 keypoints of F2 inside the grid, 150 above level 0 mixed
    in, descriptors from a pool of 20 with 5% noise; window 40 (about 30
    candidates).  The first queries' windows touch the grid's four edges or
    lie wholly outside it (the four exits of GetFeaturesInArea)."""
    rng = np.random.default_rng(1000 + n_level0)
    n2 = n_level0 + 150
    k2 = np.zeros(n2, KEYPOINT_DTYPE)
    k2["x"], k2["y"] = rng.uniform(0, 634, n2), rng.uniform(0, 474, n2)
    k2["angle"], k2["size"] = rng.uniform(0, 360, n2), 31.0
    k2["octave"][rng.permutation(n2)[:150]] = rng.integers(1, 4, 150)
    edge = [(5, 240), (635, 240), (320, 5), (320, 475), (3, 3), (636, 476),        # touching
            (-50.5, 240), (700, 240), (320, -50.5), (320, 540),                    # outside
            (-45, 240), (320, -45), (679.5, 240), (320, 519.5)]                    # nearly outside
    n1 = 260
    k1 = np.zeros(n1, KEYPOINT_DTYPE)
    k1["x"], k1["y"] = rng.uniform(0, 634, n1), rng.uniform(0, 474, n1)
    k1["x"][:len(edge)], k1["y"][:len(edge)] = zip(*edge)
    k1["angle"], k1["size"] = rng.uniform(0, 360, n1), 31.0
    k1["octave"][len(edge)::5] = 1
    pool = rng.integers(0, 256, (20, 32), dtype=np.uint8)
    d1, d2 = pool[rng.integers(0, 20, n1)].copy(), pool[rng.integers(0, 20, n2)].copy()
    for d in (d1, d2):
        bits = np.unpackbits(d, axis=1)
        bits ^= (rng.random(bits.shape) < 0.05).astype(np.uint8)
        d[:] = np.packbits(bits, axis=1)
    # above level 0 in F2: exact copies of queries' descriptors right at their
    # window centres -- the best match by far if the level filter were dropped
    up = np.nonzero(k2["octave"] > 0)[0]
    qs = np.nonzero(k1["octave"] == 0)[0][len(edge):len(edge) + len(up)]
    m = min(len(up), len(qs))
    k2["x"][up[:m]], k2["y"][up[:m]], d2[up[:m]] = k1["x"][qs[:m]], k1["y"][qs[:m]], d1[qs[:m]]
    return dict(name="stage_%d" % n_level0, k1=k1, d1=d1, k2=k2, d2=d2,
                prev=np.stack([k1["x"], k1["y"]], 1).astype(f32), w=W, h=H, window=40,
                nnratio=0.9, check=True)


def stage_boundary():
    return dict(kind="init", problems=[_stage(1536), _stage(1537)])


def _small(seed, n=10, interleave=3):
    sc = Scene("small_%d" % seed, 5, check=True, seed=seed, interleave=interleave)
    _solos(sc, n)
    return sc.problem()


def empty():
    """N1 = 0, N2 = 0, no level-0 keypoint in F1, none in F2: each between two
    ordinary problems of one batch."""
    def cut(p, **kw):
        p = dict(p)
        p.update(kw)
        return p
    a, b, c, d = _small(21), _small(22), _small(23), _small(24)
    up1, up2 = a["k1"].copy(), b["k2"].copy()
    up1["octave"], up2["octave"] = 1, 2
    probs = [_small(20),
             cut(a, name="N1=0", k1=a["k1"][:0], d1=a["d1"][:0], prev=a["prev"][:0]),
             a,
             cut(b, name="N2=0", k2=b["k2"][:0], d2=b["d2"][:0]),
             b,
             cut(a, name="F1 above level 0", k1=up1),
             c,
             cut(b, name="F2 above level 0", k2=up2),
             d]
    return dict(kind="init", problems=probs)


DISTINCTIVE_N = (0, 1, 2, 3, 4, 0, 63, 64, 65, 128, 129, 200)


def distinctive():
    """One CSR call: the lengths of DISTINCTIVE_N (an empty list first and
    between two others), then the directed lists named in `names`, then an
    empty list last."""
    rng = np.random.default_rng(31)

    def noisy(n, flip=0.08):
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        bits = np.unpackbits(np.tile(base, (n, 1)), axis=1)
        return np.packbits(bits ^ (rng.random(bits.shape) < flip), axis=1).reshape(n, 32)

    def block(x, i, w):
        b = np.unpackbits(x)
        b[w * i:w * (i + 1)] ^= 1
        return np.packbits(b)
    x = rng.integers(0, 256, 32, dtype=np.uint8)
    inv = ~x
    lists = [noisy(n) for n in DISTINCTIVE_N]
    names = ["n%d" % n if i != 5 else "n0_between" for i, n in enumerate(DISTINCTIVE_N)]
    directed = [
        ("identical", [x] * 5),                                            # median 0 at row 0
        ("tied_rows", [block(x, 0, 60), block(x, 1, 60), x, x, x, block(x, 2, 60)]),   # rows 2,3,4
        ("last_wins", [block(x, i, 40) for i in range(5)] + [x]),
        ("median_255", [x, inv, block(inv, 0, 1)]),                        # row 0: median 255
        ("median_256", [x, inv, inv, inv]),                                # row 0: median 256
        ("median_256_long", [x] + [inv] * 69),                             # the chunked path
        ("even_median", [block(x, 0, 10), x, block(x, 1, 10), block(x, 1, 100)]),
        ("tied_long", [block(x, i % 4, 50) for i in range(97)] + [x, x, x]),   # rows 97,98,99
    ]
    for nm, rows in directed:
        names.append(nm)
        lists.append(np.array(rows, np.uint8).reshape(-1, 32))
    names.append("empty_last")
    lists.append(np.zeros((0, 32), np.uint8))
    counts = [len(l) for l in lists]
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    desc = np.concatenate(lists).astype(np.uint8)
    init = rng.integers(0, 256, (len(lists), 32), dtype=np.uint8)
    return dict(kind="distinctive", offs=offs, desc=desc, init=init, names=names)


def census_distinctive(c):
    n = np.diff(c["offs"])
    best = distinctive_pyref(c)
    offs = c["offs"]
    med0, ties, last = 0, 0, 0
    top = 0
    for i in range(len(n)):
        rows = c["desc"][offs[i]:offs[i + 1]]
        if len(rows) == 0:
            continue
        bits = np.unpackbits(rows, axis=1).astype(np.int32)
        D = (bits[:, None, :] != bits[None, :, :]).sum(-1)
        med = np.sort(D, axis=1)[:, (len(rows) - 1) // 2]
        med0 += med.min() == 0
        ties += (med == med.min()).sum() > 1 and best[i] > 0
        last += best[i] == len(rows) - 1 and len(rows) > 1
        top = max(top, int(med.max()))
    return dict(lengths=sorted(set(int(v) for v in n)), long_lengths=sorted(set(int(v) for v in n if v > 64)),
                median0=int(med0), ties_not_row0=int(ties), last_row_wins=int(last), max_median=top,
                empty_first=bool(n[0] == 0), empty_last=bool(n[-1] == 0),
                empty_between=bool(((n[1:-1] == 0) & (n[:-2] > 0) & (n[2:] > 0)).any()))


# ------------------------------------------- the inputs of test_gpu_mapping.py
def crowd_collisions():
    """Few distinct descriptors in a small area (test_gpu_mapping.py)."""
    rng = np.random.default_rng(11)
    n1, n2 = 700, 500
    k1 = np.zeros(n1, KEYPOINT_DTYPE)
    k2 = np.zeros(n2, KEYPOINT_DTYPE)
    for k, n in ((k1, n1), (k2, n2)):
        k["x"] = rng.uniform(200, 260, n)
        k["y"] = rng.uniform(200, 260, n)
        k["angle"] = rng.uniform(0, 360, n)
        k["octave"] = np.where(rng.random(n) < 0.8, 0, 1)
    base = rng.integers(0, 256, (12, 32), dtype=np.uint8)
    d1 = base[rng.integers(0, 12, n1)].copy()
    d2 = base[rng.integers(0, 12, n2)].copy()
    for d in (d1, d2):
        bits = np.unpackbits(d, axis=1)
        bits ^= (rng.random(bits.shape) < rng.uniform(0, 0.12, (len(d), 1))).astype(np.uint8)
        d[:] = np.packbits(bits, axis=1)
    prev = np.stack([k1["x"], k1["y"]], 1) + rng.uniform(-5, 5, (n1, 2)).astype(np.float32)
    return dict(k1=k1, d1=d1, k2=k2, d2=d2, prev=prev.astype(np.float32), w=640, h=480)


def crowd_unstaged():
    """More level-0 F2 keypoints than the LDS stage holds (test_gpu_mapping.py)."""
    rng = np.random.default_rng(12)
    n = 2600
    k1 = np.zeros(n, KEYPOINT_DTYPE)
    k2 = np.zeros(n, KEYPOINT_DTYPE)
    for k in (k1, k2):
        k["x"] = rng.uniform(0, 640, n)
        k["y"] = rng.uniform(0, 480, n)
        k["angle"] = rng.uniform(0, 360, n)
    base = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    d1 = base[rng.integers(0, 40, n)].copy()
    d2 = base[rng.integers(0, 40, n)].copy()
    for d in (d1, d2):
        bits = np.unpackbits(d, axis=1)
        bits ^= (rng.random(bits.shape) < 0.05).astype(np.uint8)
        d[:] = np.packbits(bits, axis=1)
    return dict(k1=k1, d1=d1, k2=k2, d2=d2, prev=np.stack([k1["x"], k1["y"]], 1), w=640, h=480)


def as_problem(s, name, window, nnratio=0.9, check=True):
    p = dict(s)
    p.update(name=name, window=window, nnratio=nnratio, check=check,
             prev=np.asarray(s["prev"], f32))
    return p


# name -> (builder, census minimum).  For "init" cases the minimum is a list,
# one dict per problem; a value is a lower bound, a set or dict that must be
# covered, or (for EXACT_KEYS) the value itself.
_DRY = {16: 1, 17: 1, 256: 1, 257: 1}
_COUNTS_MIN = dict(nc={0, 1, 2, 16, 17, 256, 257}, dry=_DRY,
                   paths=dict(topk=20, dry_exact=2, list=3, rescan=2), staged=True)
CASES = {
    "counts": (counts, [dict(_COUNTS_MIN, tie_best=2, list_chunks={(0, 0)}),
                        dict(_COUNTS_MIN, tie_accept=2)]),
    "batch_lanes": (batch_lanes, [
        dict(nq=63, conflict_lanes={1}, slot_ne_index=60, accepts=63),
        dict(nq=64, full_clean=1, batches=1, conflict_lanes=set(), slow_lanes=set(), nc={0, 1, 2}),
        dict(nq=65, conflict_lanes={1, 63}, si_only=1, batches=3, accepts=65),
        dict(nq=129, full_clean=2, slow_lanes={0}, batches=3, conflict_lanes=set(),
             paths=dict(list=1))]),
    "equalities": (equalities, [
        dict(mdist_eq=1, mdist_above=1, b1_50=1, b1_51=1, ratio_eq=1, ratio_below=1, win_eq_x=2,
             win_eq_y=1, win_inside=3, tie_best=2, tie_accept=0),
        dict(mdist_eq=1, b1_50=1, win_eq_x=2, win_eq_y=1, tie_best=2, tie_accept=2)]),
    "shifted_bounds": (shifted_bounds, [dict(mdist_eq=1, win_eq_x=2, win_eq_y=1, tie_best=2),
                                        dict(mdist_eq=1, win_eq_x=2, win_eq_y=1, tie_accept=2)]),
    "steal_hist": (steal_hist, [dict(chain=3, steals=3, stolen_votes=3, stolen_votes_decide=True,
                                     slot_ne_index=10)] * 2),
    "stage_boundary": (stage_boundary, [
        dict(ns=1536, staged=True, col0=1, col63=1, row0=1, row47=1,
             exits={"x0", "x1", "y0", "y1"}, accepts=20, steals=1),
        dict(ns=1537, staged=False, col0=1, col63=1, row0=1, row47=1,
             exits={"x0", "x1", "y0", "y1"}, accepts=20, steals=1)]),
    "empty": (empty, [dict(nq=10), dict(N1=0, nq=0), dict(nq=10), dict(N2=0, nq=10, accepts=0),
                      dict(nq=10), dict(nq=0, N1=14), dict(nq=10), dict(ns=0, accepts=0),
                      dict(nq=10)]),
    "distinctive": (distinctive, dict(
        lengths={0, 1, 2, 3, 4, 63, 64, 65, 128, 129, 200}, long_lengths={65, 128, 129, 200},
        median0=3, ties_not_row0=2, last_row_wins=1, max_median=256, empty_first=True,
        empty_last=True, empty_between=True)),
}
EXACT_KEYS = ("nq", "ns", "N1", "N2", "staged", "batches", "conflict_lanes", "slow_lanes",
              "tie_accept", "stolen_votes_decide", "empty_first", "empty_last", "empty_between")


def meets(cen, minimum):
    """Assert that a census meets its minimum."""
    for k, v in minimum.items():
        got = cen[k]
        if k in EXACT_KEYS:
            want = sorted(v) if isinstance(v, set) else v
            assert got == want, (k, v, got)
        elif isinstance(v, set):
            assert v <= set(got), (k, v, got)
        elif isinstance(v, dict):
            for kk, vv in v.items():
                assert got.get(kk, 0) >= vv, (k, kk, vv, got)
        else:
            assert got >= v, (k, v, got)
