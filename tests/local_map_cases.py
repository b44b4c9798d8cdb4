"""Small directed maps for Tracking::UpdateLocalMap (tests/local_map_ref.py,
orb_update_local_map_batch).  Every input draws its keyframe ranks as a random
permutation, so index order and rank order differ; a case has at most 130
keyframes and 64 slots per keyframe unless its docstring says otherwise.

An input is dict(name, map, kp_match, local_kf, mp_stride): the map in the
layout of local_map_ref, the frame's matches, the list the previous frame left
and a local-map capacity that holds every local point unless the case is about
the capacity.  combine() lays several inputs side by side in ONE map (keyframe
and point numbers shifted, ranks interleaved at random with each input's own
order kept), which is what a batch call takes.
"""
import functools

import numpy as np

import local_map_ref as R

HASH_CAP = 9216      # distinct point ids k_local_map's LDS table takes (include/orb_abi.h)
CHILD_STAGE = 16     # children per visited keyframe it stages in LDS


class MapBuilder:
    def __init__(self, n_kf, seed):
        self.rng = np.random.default_rng(seed)
        self.n_kf = n_kf
        self.rank = self.rng.permutation(n_kf).astype(np.int32)
        while n_kf > 1 and np.array_equal(self.rank, np.arange(n_kf)):
            self.rank = self.rng.permutation(n_kf).astype(np.int32)
        self.bad = np.zeros(n_kf, np.uint8)
        self.parent = np.full(n_kf, -1, np.int32)
        self.cov = [[] for _ in range(n_kf)]
        self.child = [[] for _ in range(n_kf)]
        self.kf_mp = [[] for _ in range(n_kf)]
        self.obs = []
        self.pts = []
        self.next = 0

    def take(self, n):
        out = list(range(self.next, self.next + n))
        self.next += n
        assert self.next <= self.n_kf
        return out

    def by_rank(self, kfs):
        return sorted(kfs, key=lambda k: self.rank[k])

    def point(self, obs=(), in_kfs=None, bad=0, has_obs=1, seen=0):
        """A map point observed by `obs` (its votes) and listed in the
        kf_mp of `in_kfs` (default: the observers)."""
        pid = len(self.pts)
        self.obs.append([int(k) for k in obs])
        self.pts.append((bad, seen, has_obs))
        for k in (obs if in_kfs is None else in_kfs):
            self.kf_mp[k].append(pid)
        return pid

    def votes(self, kf, n):
        """n points seen by kf alone; matching them gives kf n votes."""
        return [self.point([kf]) for _ in range(n)]

    def map(self):
        n = len(self.pts)
        pts = np.zeros(n, R.MAP_POINT_DTYPE)
        r = self.rng
        pts["pos"] = r.standard_normal((n, 3)).astype(np.float32)
        pts["normal"] = r.standard_normal((n, 3)).astype(np.float32)
        pts["min_distance"] = r.random(n).astype(np.float32)
        pts["max_distance"] = (r.random(n) + 2).astype(np.float32)
        if n:
            pts["bad"], pts["seen"], pts["has_obs"] = np.array(self.pts, np.uint8).T
        pts["_pad"] = r.integers(0, 256, n, dtype=np.uint8)
        desc = r.integers(0, 256, (n, 32), dtype=np.uint8)
        return dict(rank=self.rank, bad=self.bad, parent=self.parent, cov=self.cov,
                    child=self.child, kf_mp=[list(x) for x in self.kf_mp], obs=self.obs,
                    points=pts, desc=desc)


def _inp(name, b, kp_match, local_kf=(), mp_stride=None):
    m = b.map()
    inp = dict(name=name, map=m, kp_match=np.array(kp_match, np.int32).reshape(-1),
               local_kf=np.array(local_kf, np.int32).reshape(-1))
    n = R.update_local_map(m, inp["kp_match"], inp["local_kf"], 1 << 30)["n_local_points"]
    inp["mp_stride"] = mp_stride if mp_stride is not None else max(n + 3, 4)
    return inp


# ------------------------------------------------------------- tiny, by hand
def tiny():
    """Five keyframes with fixed ranks (keyframe -> rank 2 0 4 1 3); answers
    worked out by hand in tests/test_local_map_ref.py."""
    b = MapBuilder(5, 1)
    b.rank = np.array([2, 0, 4, 1, 3], np.int32)
    p0 = b.point([0, 1])            # votes: kf0, kf1
    p1 = b.point([1])               # votes: kf1
    p2 = b.point([3], bad=1)        # matched and bad: nulled, no vote
    p3 = b.point([0, 2])            # not matched; in kf0 and kf2
    p4 = b.point([], in_kfs=[4], has_obs=0)
    b.kf_mp[0].append(-1)
    b.kf_mp[1].append(p3)           # kf1 is walked first: p3's first occurrence is here
    b.cov[1] = [0, 2]               # kf0 is voted; kf2 is the first free covisible
    b.child[0] = [4]
    b.parent[0] = 3
    return _inp("tiny", b, [p0, -1, p1, p2, -2, p0])


def tiny_empty():
    """No match at all and a stale list [3, 1]: the list is kept (:1462)."""
    b = MapBuilder(5, 2)
    b.rank = np.array([2, 0, 4, 1, 3], np.int32)
    a = b.point([3])
    c = b.point([1, 3])
    b.point([0])
    assert (a, c) == (0, 1)
    return _inp("tiny_empty", b, [-1, -2, -1], local_kf=[3, 1])


# ---------------------------------------------------------------- keyframes
def empty_stale():
    """Zero matched points and a non-empty stale list; one listed keyframe is
    bad by now and is not re-checked."""
    b = MapBuilder(12, 3)
    k = b.take(12)
    for q in k:
        for _ in range(3):
            b.point([q])
    b.point([k[2], k[5]])
    b.bad[k[5]] = 1
    return _inp("empty_stale", b, [-1] * 7 + [-2, -1], local_kf=[k[5], k[2], k[9]])


def all_voted_bad():
    b = MapBuilder(8, 4)
    k = b.take(8)
    km = b.votes(k[1], 2) + b.votes(k[4], 3) + [-1]
    b.bad[k[1]] = b.bad[k[4]] = 1
    b.cov[k[1]] = [k[0]]
    return _inp("all_voted_bad", b, km, local_kf=[k[6]])


def tie_max():
    """Two keyframes share the largest count; the one of smaller rank has the
    larger index.  A third, of still smaller rank, has fewer votes."""
    b = MapBuilder(9, 5)
    pair = next((i, j) for i in range(9) for j in range(i + 1, 9) if b.rank[i] > b.rank[j])
    lo, hi = pair                                  # lo < hi, rank[lo] > rank[hi]
    rest = [q for q in range(9) if q not in pair]
    km = b.votes(lo, 4) + b.votes(hi, 4) + b.votes(rest[0], 2) + b.votes(rest[1], 4 - 1)
    return _inp("tie_max", b, km)


def voted(n_voted):
    """n_voted keyframes with one vote each, 130 keyframes in all.  In rank
    order the first voted keyframe has a free covisible, the second a free
    covisible and a free child, the third a free covisible; with 80 voted the
    first also has a free child and a free parent.  79 -> 82 entries (the third
    is not visited), 80 -> 83, 81 and above -> no additions."""
    b = MapBuilder(130, 100 + n_voted)
    v = b.take(n_voted)
    free = b.take(6)
    km = []
    for q in v:
        km += b.votes(q, 1)
    o = b.by_rank(v)
    b.cov[o[0]] = [o[5], free[0]]
    b.cov[o[1]] = [free[1]]
    b.child[o[1]] = [free[2]]
    b.cov[o[2]] = [free[3]]
    if n_voted == 80:
        b.child[o[0]] = [free[4]]
        b.parent[o[0]] = free[5]
    for q in free:
        b.point([], in_kfs=[q])
    return _inp("voted%d" % n_voted, b, km)


def neigh_11th():
    """Eleven covisibles: ten voted or bad, only the eleventh qualifies."""
    b = MapBuilder(16, 6)
    v = b.take(9)
    badk = b.take(2)
    free = b.take(1)
    km = []
    for q in v:
        km += b.votes(q, 2)
    b.bad[badk] = 1
    a = b.by_rank(v)[0]
    b.cov[a] = [q for q in v if q != a] + badk + free   # 8 + 2 + 1
    b.point([], in_kfs=free)
    return _inp("neigh_11th", b, km)


def neighbours():
    """A bad covisible skipped; a covisible already added by an earlier
    iteration; a keyframe with two free covisibles (only the first is taken)."""
    b = MapBuilder(14, 7)
    v = b.by_rank(b.take(3))
    x, y, z1, z2, bd = b.take(5)
    km = []
    for q in v:
        km += b.votes(q, 1)
    b.bad[bd] = 1
    b.cov[v[0]] = [bd, x]
    b.cov[v[1]] = [x, y]
    b.cov[v[2]] = [z1, z2]
    for q in (x, y, z1, z2):
        b.point([], in_kfs=[q])
    return _inp("neighbours", b, km)


def children(n_children=5):
    """Several qualifying children listed in descending rank; the one of
    smallest rank among the whole list is bad, the next is voted already.
    n_children 16 / 17 sits on either side of the kernel's staged-children
    bound (above it the pass reads the list from memory)."""
    b = MapBuilder(n_children + 6, 8 + n_children)
    v = b.by_rank(b.take(2))
    ch = b.take(n_children)
    km = b.votes(v[0], 2) + b.votes(v[1], 1)
    o = b.by_rank(ch)
    b.bad[o[0]] = 1
    lst = o[::-1]                     # list order: descending rank
    b.child[v[0]] = lst + [v[1]]      # v[1] is included already
    b.child[v[1]] = list(lst)         # the next smallest
    for q in ch:
        b.point([], in_kfs=[q])
    return _inp("children%d" % n_children, b, km)


def parent_break():
    """The first visited keyframe's parent is added and ends the pass: the
    second's free covisible is never looked at."""
    b = MapBuilder(10, 9)
    v = b.by_rank(b.take(3))
    par, x = b.take(2)
    km = []
    for q in v:
        km += b.votes(q, 1)
    b.parent[v[0]] = par
    b.cov[v[1]] = [x]
    b.point([], in_kfs=[par])
    b.point([], in_kfs=[x])
    return _inp("parent_break", b, km)


def parent_included():
    """The first keyframe's parent is voted (no push, no break); the second's
    parent is bad and is added all the same."""
    b = MapBuilder(10, 10)
    v = b.by_rank(b.take(3))
    par, x = b.take(2)
    km = []
    for q in v:
        km += b.votes(q, 1)
    b.parent[v[0]] = v[2]
    b.cov[v[0]] = [x]
    b.parent[v[1]] = par
    b.bad[par] = 1
    b.point([], in_kfs=[par])
    b.point([], in_kfs=[x])
    return _inp("parent_included", b, km)


# ------------------------------------------------------------------- points
def points_mix(mp_stride=None, name="points_mix"):
    """A keyframe with no points, -1 slots, a point in several keyframes and
    twice in one, bad points, a matched point without observations, a matched
    bad point, -2 matches, map `seen` bytes that disagree with the frame."""
    b = MapBuilder(9, 11)
    k = b.take(9)
    km = []
    shared = b.point([k[0], k[1], k[2]], seen=1)
    twice = b.point([k[1]])
    b.kf_mp[k[1]] += [-1, twice, -1]
    km += [shared, twice, -2]
    km += [b.point([k[3]], has_obs=0)]
    km += [b.point([k[2]], bad=1), -1]
    for q in k[:4]:
        for j in range(6):
            b.point([q], bad=(j == 2), seen=(j == 4))
    km += b.votes(k[0], 2)
    b.cov[k[0]] = [k[6]]               # k[6] has no points at all
    b.child[k[1]] = [k[7]]
    b.point([k[7]], seen=1)
    b.kf_mp[k[7]] += [shared, -5]
    km += [-2]
    return _inp(name, b, km, mp_stride=mp_stride)


def over_mp_stride():
    return points_mix(mp_stride=5, name="over_mp_stride")


def _fill(b, kfs, n_points, per_kf, bad_every=0):
    """n_points new points over kfs, per_kf slots each -> (ids, matches that
    give every used keyframe a vote)."""
    ids, km, q = [], [], 0
    while len(ids) < n_points:
        take = min(n_points - len(ids), per_kf)
        own = [b.point([kfs[q]], bad=int(bad_every and (len(ids) + j) % bad_every == 3))
               for j in range(take)]
        km.append(next(i for i in own if not b.pts[i][0]))
        ids += own
        q += 1
    return ids, km


def count(n_points, per_kf=40):
    """Exactly n_points local points (per_kf slots per keyframe; 1,023-1,025
    use keyframes of 300 slots), some held by the frame."""
    b = MapBuilder(8, 2000 + n_points)
    ids, km = _fill(b, b.take(8), n_points, per_kf)
    km += ids[::17]
    return _inp("count%d" % n_points, b, km, mp_stride=n_points + 2)


def tier(n_distinct, extra=False, name=None):
    """n_distinct distinct point ids over keyframes of 1,024 slots (above the
    64 of the other cases): the LDS table takes HASH_CAP of them, one more runs
    on the scratch table; this is the smallest slot total that does.  extra
    adds repeats, -1 slots and bad points."""
    n_kf = (n_distinct + 1023) // 1024 + 2
    b = MapBuilder(n_kf, 3000 + n_distinct + int(extra))
    k = b.take(n_kf)
    ids, km = _fill(b, k, n_distinct, 1024, bad_every=11 if extra else 0)
    km += ids[5::97]
    if extra:
        b.kf_mp[k[-1]] += ids[::-1][:300] + [-1, -1] + ids[:20]
        km += b.votes(k[-1], 1) + [-2]
    return _inp(name or "tier%d" % n_distinct, b, km)


SMALL = {
    "tiny": tiny, "tiny_empty": tiny_empty, "empty_stale": empty_stale,
    "all_voted_bad": all_voted_bad, "tie_max": tie_max,
    "voted79": lambda: voted(79), "voted80": lambda: voted(80), "voted81": lambda: voted(81),
    "voted82": lambda: voted(82), "voted100": lambda: voted(100),
    "neigh_11th": neigh_11th, "neighbours": neighbours, "children5": lambda: children(5),
    "children16": lambda: children(16), "children17": lambda: children(17),
    "parent_break": parent_break, "parent_included": parent_included,
    "points_mix": points_mix, "over_mp_stride": over_mp_stride,
    "count63": lambda: count(63), "count64": lambda: count(64), "count65": lambda: count(65),
    "count1023": lambda: count(1023, 300), "count1024": lambda: count(1024, 300),
    "count1025": lambda: count(1025, 300),
}
LARGE = {
    "tier%d" % HASH_CAP: lambda: tier(HASH_CAP),
    "tier%d" % (HASH_CAP + 1): lambda: tier(HASH_CAP + 1),
    "tier_mix": lambda: tier(HASH_CAP + 90, extra=True, name="tier_mix"),
}
ALL = dict(SMALL, **LARGE)


@functools.lru_cache(maxsize=None)
def get(name):
    return ALL[name]()


def combine(inputs, seed=0):
    """The inputs side by side in one map -> (map, problems): problem i is
    input i's frame with its keyframe and point numbers shifted."""
    rng = np.random.default_rng(seed)
    keys, kf0, mp0 = [], [], []
    nk = nm = 0
    for inp in inputs:
        m = inp["map"]
        n = len(m["rank"])
        ks = np.sort(rng.random(n))
        keys.append(ks[m["rank"]])        # the input's own order survives
        kf0.append(nk)
        mp0.append(nm)
        nk += n
        nm += len(m["points"])
    allkeys = np.concatenate(keys) if keys else np.zeros(0)
    rank = np.empty(nk, np.int32)
    rank[np.argsort(allkeys, kind="stable")] = np.arange(nk, dtype=np.int32)
    sh = lambda lst, o: [int(x) + o if x >= 0 else int(x) for x in lst]
    out = dict(rank=rank, bad=np.concatenate([i["map"]["bad"] for i in inputs]),
               parent=np.concatenate([np.where(i["map"]["parent"] >= 0, i["map"]["parent"] + o,
                                               -1).astype(np.int32)
                                      for i, o in zip(inputs, kf0)]),
               cov=[], child=[], kf_mp=[], obs=[],
               points=np.concatenate([i["map"]["points"] for i in inputs]),
               desc=np.concatenate([i["map"]["desc"] for i in inputs]))
    probs = []
    for inp, ko, mo in zip(inputs, kf0, mp0):
        m = inp["map"]
        out["cov"] += [sh(x, ko) for x in m["cov"]]
        out["child"] += [sh(x, ko) for x in m["child"]]
        out["kf_mp"] += [sh(x, mo) for x in m["kf_mp"]]
        out["obs"] += [sh(x, ko) for x in m["obs"]]
        probs.append(dict(name=inp["name"], kp_match=np.array(sh(inp["kp_match"], mo), np.int32),
                          local_kf=np.array(sh(inp["local_kf"], ko), np.int32),
                          mp_stride=inp["mp_stride"]))
    return out, probs


def csr(lists):
    offs = np.zeros(len(lists) + 1, np.int32)
    offs[1:] = np.cumsum([len(x) for x in lists])
    vals = np.array([v for x in lists for v in x], np.int32)
    return offs, vals


def view_arrays(m):
    """The keyword arguments of orb_amd.MapView for a map."""
    co, cv = csr(m["cov"])
    ho, hv = csr(m["child"])
    mo, mv = csr(m["kf_mp"])
    oo, ov = csr(m["obs"])
    return dict(kf_rank=m["rank"], kf_bad=m["bad"], kf_parent=m["parent"], kf_cov_offs=co,
                kf_cov=cv, kf_child_offs=ho, kf_child=hv, kf_mp_offs=mo, kf_mp=mv,
                mp_obs_offs=oo, mp_obs=ov, points=m["points"], mp_desc=m["desc"])
