"""The directed inputs of matcher_edge_cases.py on the CPU: the oracle equals the
independent restatement (pyref) exactly, and the construction's own answer
where it has one; the census of each input meets the minimum stated next to its
generator (printed, run with -s to read it); and every family's inputs separate
the reference rule from its plausible wrong neighbours (pyref's rule switches).

Also the cross-check of the two restatements added with these tests,
pyref.search_by_projection_frame and pyref.search_by_bow, on the natural
frame_pair / bow_pair scenes."""
import functools

import numpy as np
import pytest

import matcher_edge_cases as E
import pyref
import scenarios as S


@functools.lru_cache(maxsize=None)
def case(name):
    return E.CASES[name][0]()


@functools.lru_cache(maxsize=None)
def reference(name):
    import oracle as o
    o.lib()
    return E.run_oracle(o, case(name))


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_oracle_matches_restatement_and_census(name):
    c, minimum = case(name), E.CASES[name][1]
    n, out = reference(name)
    if c["family"] != "fuse_sim3":   # no restatement of FuseSim3: oracle and construction
        pn, pout = E.run_pyref(c)
        assert pn == n, (pn, n)
        assert np.array_equal(pout, out), np.nonzero(pout != out)[0][:10]
    if c.get("expect") is not None:
        assert np.array_equal(out, c["expect"]), np.nonzero(out != c["expect"])[0][:10]
        assert n == c.get("n_expect", int((c["expect"] >= 0).sum()))
    if minimum["matches"] == 0:
        assert n == 0
    assert n >= minimum["matches"], (n, minimum["matches"])
    if c["family"] in E.CLAIMING and "windows" in c:
        cen = E.census_claiming(c)
        print(name, "matches", n, "reset", int((out == -2).sum()), cen)
        for k in ("slow", "near", "multi", "partial_reset", "all_reset", "at_thr",
                  "at_thr_plus_1"):
            assert cen.get(k, 0) >= minimum.get(k, 0), (k, cen.get(k), minimum[k])
        if "hist" in minimum:
            assert cen["hist"] == minimum["hist"], (cen["hist"], minimum["hist"])
        if "reset" in cen:   # the replay's bookkeeping is the reference's
            assert cen["accepted"] - cen["reset"] == n
    if "tags" in c:   # gate scenes: both sides of the distance threshold are present
        thr = {"reloc": c.get("orb_dist"), "sim3": 50, "fuse": 50, "fuse_sim3": 50}[c["family"]]
        per_d = E.census_thresholds(c, out)
        print(name, "by distance", per_d)
        assert per_d[thr] == "accepted" and per_d[thr + 1] == "rejected"
        assert all((d <= thr) == (r == "accepted") for d, r in per_d.items())
    if c["family"] == "by_sim3":
        cen = E.census_mutual(c)
        print(name, "matches", n, cen)
        assert cen["mutual"] == n
        for k in ("mutual", "one_way"):
            assert cen[k] >= minimum.get(k, 0), (k, cen[k], minimum[k])
    if c["family"] in E.NODE_BASED:
        cen = E.census_nodes(c)
        print(name, "matches", n, cen)
        for s in minimum.get("sizes", ()):
            assert s in cen["sizes"], (s, cen["sizes"])
        for p in minimum.get("tie_positions", ()):
            assert p in cen["tie_positions"], (p, cen["tie_positions"])
        if "tie_positions" in minimum:
            assert cen["ties_cross_trip"] >= 3 and cen["ties_same_trip"] >= 1
        if name in ("bow_frame", "bow_kf", "tri"):   # best distance 49, 50 and 51 in every big node
            assert all(cen["best_at"][d] >= 5 for d in (49, 50, 51)), cen["best_at"]
        if max(minimum.get("sizes", (0,))) > E.WAVE:
            assert cen["best_beyond_first_trip"] >= 1


@pytest.mark.parametrize("family", E.CLAIMING)
@pytest.mark.parametrize("nkeys,n", [(k, 65) for k in E.COUNTS_NKEYS] +
                         [(65, m) for m in E.COUNTS_N if m != 65])
def test_counts(oracle, family, nkeys, n):
    c = E.counts_case(family, nkeys, n)
    assert _same(E.run_oracle(oracle, c), E.run_pyref(c))


def test_empty_inputs(oracle):
    for c in E.empty_cases():
        n, out = E.run_oracle(oracle, c)
        assert n == 0 and (out < 0).all(), c["family"]
        if c["family"] != "fuse_sim3":
            assert _same((n, out), E.run_pyref(c)), c["family"]


# Which input separates which wrong rule, per family.  A rule that no input of
# its family changes would not be tested by these inputs at all.
SENSITIVITY = {
    "reloc": dict(th_strict="gates_reloc_64", tie_flip="chain_reloc", top4="chain_reloc",
                  bounds_flip="gates_reloc_100", hist_ge="hist_reloc_four_tied"),
    "sim3": dict(th_strict="gates_sim3", tie_flip="chain_sim3", top4="chain_sim3",
                 bounds_flip="gates_sim3"),
    "fuse": dict(th_strict="gates_fuse", tie_flip="gates_fuse", stereo_flip="gates_fuse",
                 bounds_flip="gates_fuse"),
    "by_sim3": dict(th_strict="by_sim3_thresholds", tie_flip="by_sim3_thresholds",
                    bounds_flip="by_sim3_thresholds"),
    "frame": dict(th_strict="gates_frame", tie_flip="chain_frame", top4="chain_frame",
                  stereo_flip="gates_frame", bounds_flip="gates_frame",
                  hist_ge="hist_frame_four_tied"),
    "bow": dict(th_strict="bow_frame", tie_flip="bow_frame_ties", no_claims="bow_frame",
                hist_ge="hist_bow_four_tied"),
    "bow_kf": dict(th_strict="bow_kf", tie_flip="bow_kf_ties", no_claims="bow_kf"),
    "tri": dict(th_strict="tri", tie_flip="tri_ties", stereo_flip="tri",
                hist_ge="hist_tri_four_tied"),
}


@pytest.mark.parametrize("family,rule", [(f, r) for f in sorted(SENSITIVITY)
                                         for r in sorted(SENSITIVITY[f])])
def test_sensitivity(family, rule):
    name = SENSITIVITY[family][rule]
    c = case(name)
    assert c["family"] == family
    ref = reference(name)
    wrong = E.run_pyref(c, rules=(rule,))
    diff = np.nonzero(wrong[1] != ref[1])[0]
    print(family, rule, name, "n", ref[0], "->", wrong[0], "entries changed", len(diff))
    assert len(diff) > 0 or wrong[0] != ref[0]


def test_crowded_inputs_feel_top4_rule():
    """Not only the chain: on the crowded inputs as well, treating TOPK
    exhaustion as "no match" changes the answer."""
    for name in ("crowded_reloc", "crowded_sim3", "crowded_frame"):
        assert not _same(reference(name), E.run_pyref(case(name), rules=("top4",)))


# ------------------------------------------ the two restatements on natural scenes
@pytest.mark.parametrize("mono,tlc,th,ori", [(1, 0.0, 15.0, 1), (0, 1.0, 7.0, 1),
                                             (0, -1.0, 7.0, 0), (0, 0.0, 14.0, 1)])
def test_frame_restatement_on_frame_pair(oracle, mono, tlc, th, ori):
    fp = S.frame_pair(oracle, 2, rng_seed=int(th))
    rng = np.random.default_rng(7)
    n = len(fp["kb"])
    ur = None if mono else np.where(rng.random(n) < 0.6,
                                    fp["kb"]["x"] - rng.uniform(3, 60, n), -1).astype(np.float32)
    locked = (rng.random(n) < 0.1).astype(np.uint8)
    args = (fp["kb"], fp["db"], fp["scale"], fp["w"], fp["h"], fp["last"], fp["last_desc"],
            S.camera(), tlc, th, mono, ori, locked, ur)
    ref = oracle.match_projection_frame(*args)
    assert ref[0] > 100
    assert _same(ref, pyref.search_by_projection_frame(*args))


@pytest.mark.parametrize("seed,nnratio,ori", [(4, 0.75, 1), (6, 0.9, 0)])
def test_bow_restatement_on_bow_pair(oracle, seed, nnratio, ori):
    bp = S.bow_pair(oracle, seed)
    args = (bp["kf_desc"], bp["kf_angle"], bp["kf_mp"], bp["kf_bad"], bp["kf_fv"], bp["f_desc"],
            bp["f_angle"], bp["f_fv"], nnratio, ori)
    ref = oracle.match_bow(*args)
    assert ref[0] > 50
    assert _same(ref, pyref.search_by_bow(*args))


def test_natural_scene_census(oracle):
    """The census of the natural scenes the older GPU tests use, in the columns
    of the directed inputs' (printed; run with -s): what those scenes leave
    uncovered.  Asserted: their vocabulary nodes need one trip of the 64-lane loop
    only, which is why the directed node inputs exist."""
    import math
    ls = np.float32(math.log(np.float32(1.2)))
    kf0, kf1 = S.keyframe_pair(oracle, 3, rng_seed=1)
    rng = np.random.default_rng(11)
    mps = kf0["mps"].copy()
    mps["bad"] |= kf0["valid"] == 0
    mps["seen"] = rng.random(len(mps)) < 0.1
    lk = (rng.random(len(kf1["keys"])) < 0.2).astype(np.uint8)
    ow = S.pose_record(oracle, kf1["Rw"], kf1["tw"])["ow"][0]
    for th, od in ((10, 100), (3, 64), (5, 50)):
        win = E.windows_kf(mps, kf1["Rw"], kf1["tw"], ow, S.camera(), kf1["scale"], th, 1241, 376,
                           True, ls)
        c = dict(family="reloc", keys=kf1["keys"], desc=kf1["desc"], locked=lk,
                 mp_desc=kf0["mp_desc"], orb_dist=od, windows=win)
        print("keyframe_pair reloc th", th, E.census_claiming(c, 1241, 376))
    fp = S.frame_pair(oracle, 2, rng_seed=15)
    c = dict(family="frame", keys=fp["kb"], desc=fp["db"], last=fp["last"], u_right=None,
             last_desc=fp["last_desc"], locked=np.zeros(len(fp["kb"]), np.uint8),
             windows=E.windows_frame(fp["last"], S.camera(), fp["scale"], 15.0))
    print("frame_pair mono th 15", E.census_claiming(c, 1241, 376))
    bp = S.bow_pair(oracle, 4)
    cen = E.census_nodes(dict(family="bow", kf_fv=bp["kf_fv"], f_fv=bp["f_fv"],
                              kf_desc=bp["kf_desc"], f_desc=bp["f_desc"]))
    print("bow_pair(4)", {k: v for k, v in cen.items() if k != "sizes"})
    assert cen["max_size"] <= E.WAVE and cen["best_beyond_first_trip"] == 0
    fv0 = oracle.feature_vector(S.vocab_nodes(kf0["desc"]))
    fv1 = oracle.feature_vector(S.vocab_nodes(kf1["desc"]))
    cen = E.census_nodes(dict(family="bow_kf", fv1=fv0, fv2=fv1, d1=kf0["desc"], d2=kf1["desc"]))
    print("keyframe_pair nodes", {k: v for k, v in cen.items() if k != "sizes"})
    assert cen["max_size"] <= E.WAVE and cen["best_beyond_first_trip"] == 0


def test_lds_tier_sizes():
    """The tier inputs sit where they claim to, by the documented rule."""
    for tier, lds in (("pp", E.resolve_lds_pp), ("frame", E.resolve_lds_frame)):
        small, mid, top, over = (lds(*s) for s in E.LDS_TIERS[tier])
        assert small <= 65536 < mid < top == E.LDS_LIMIT < over == E.LDS_LIMIT + 4
