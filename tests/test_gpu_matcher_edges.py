"""The ORBmatcher variant kernels (k_pp_match / k_pp_resolve / k_sim3_mutual,
k_frame_candidates / k_frame_resolve, k_bow_match / k_bow_finish, k_tri_match /
k_tri_finish) on the directed inputs of matcher_edge_cases.py, against the CPU
oracle: counts, arrays and -2 marks exact.

Every input runs three times on a matcher shared by the whole module: once,
then again after a call of the same variant with a different size, so that
reused scratch (top-K lists, candidate counts, the buffer pools) meets stale
contents.  test_matcher_edge_cases.py shows on the CPU that these inputs reach
the kernels' branches (census) and separate the reference rules from their
wrong neighbours."""
import functools

import numpy as np
import pytest

import matcher_edge_cases as E

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(name):
    return E.CASES[name][0]()


@functools.lru_cache(maxsize=None)
def reference(name):
    import oracle as o
    o.lib()
    return E.run_oracle(o, case(name))


@pytest.fixture(scope="module")
def matchers():
    return {}


# a call of each family with sizes unlike any directed input's, run in between
OTHER = {"reloc": "crowded_reloc_th5_d64", "sim3": "crowded_sim3_none_matched",
         "fuse": "crowded_fuse", "fuse_sim3": "crowded_fuse_sim3", "by_sim3": "by_sim3_no_masks",
         "frame": "crowded_frame_no_ori", "bow": "bow_frame_nodes4", "bow_kf": "bow_kf_nodes4",
         "tri": "tri_nodes4"}
OTHER_ALT = {"reloc": "crowded_reloc", "sim3": "crowded_sim3", "fuse": "gates_fuse",
             "fuse_sim3": "gates_fuse_sim3", "by_sim3": "by_sim3", "frame": "crowded_frame",
             "bow": "bow_frame_nodes1", "bow_kf": "bow_kf_nodes1", "tri": "tri_nodes1"}


def _check(got, ref, what):
    n, out = got
    rn, rout = ref
    assert np.array_equal(out, rout), (what, np.nonzero(out != rout)[0][:10],
                                       out[out != rout][:10], rout[out != rout][:10])
    assert n == rn, (what, n, rn)


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_directed_input(gpu, matchers, name):
    c = case(name)
    ref = reference(name)
    if c.get("expect") is not None:
        assert np.array_equal(ref[1], c["expect"])
    _check(E.run_gpu(gpu, matchers, c), ref, name)
    other = OTHER[c["family"]]
    if other == name:
        other = OTHER_ALT[c["family"]]
    # the in-between call shares the matcher only if its (nnratio, checkOri) agree
    oc = dict(case(other))
    for k in ("nnratio", "check_ori"):
        if k in c:
            oc[k] = c[k]
    E.run_gpu(gpu, matchers, oc)
    _check(E.run_gpu(gpu, matchers, c), ref, name + " (after another size)")
    _check(E.run_gpu(gpu, matchers, c), ref, name + " (repeated)")


@pytest.mark.parametrize("family", E.CLAIMING)
def test_counts(gpu, oracle, matchers, family):
    """nkeys around the lock bitmap's word edge, n around the batch edge."""
    sizes = [(k, 65) for k in E.COUNTS_NKEYS] + [(65, m) for m in E.COUNTS_N if m != 65]
    for nkeys, n in sizes:
        c = E.counts_case(family, nkeys, n)
        _check(E.run_gpu(gpu, matchers, c), E.run_oracle(oracle, c), (family, nkeys, n))


def test_empty_inputs(gpu, oracle, matchers):
    for c in E.empty_cases():
        n, out = E.run_gpu(gpu, matchers, c)
        assert n == 0 and (out < 0).all(), c["family"]
        _check((n, out), E.run_oracle(oracle, c), c["family"])


# ------------------------------------------------------------------- LDS tiers
def _raw_call(gpu, matchers, c):
    """The claiming variant of case `c` through the C ABI with outputs preset to
    junk: (status, kp_match, nmatches, kp_match as passed in)."""
    import ctypes
    L = gpu.lib()
    m = next(iter(matchers.values()))
    F = gpu.Frame(c["keys"], c["desc"], E.SCALE, E.W, E.H)
    f, cam = F._c(), gpu._Camera(*E.CAM)
    nm = ctypes.c_int32(5)
    ptr = lambda a: a.ctypes.data
    if c["family"] == "sim3":
        km = np.where(np.arange(F.N) % 3 == 0, 7, -1).astype(np.int32)
    else:
        km = np.full(F.N, 7, np.int32)
    entry = km.copy()
    if c["family"] == "frame":
        last = np.ascontiguousarray(c["last"], gpu.LAST_MP_DTYPE)
        st = L.orb_match_projection_frame(m.handle, ctypes.byref(f), None, len(last), ptr(last),
                                          ptr(c["last_desc"]), ctypes.byref(cam), c["tlc_z"],
                                          c["th"], int(c["mono"]), int(c["check_ori"]), ptr(km),
                                          ctypes.byref(nm))
        return st, km, nm.value, entry
    mps = np.ascontiguousarray(c["mps"], gpu.MAP_POINT_DTYPE)
    if c["family"] == "reloc":
        pose = np.ascontiguousarray(E.pose_record(), gpu.POSE_DTYPE)
        st = L.orb_search_by_projection_reloc(m.handle, ctypes.byref(f), None, ptr(pose),
                                              ctypes.byref(cam), float(E.LS), len(mps), ptr(mps),
                                              ptr(c["mp_desc"]), ptr(c["kf_angle"]), c["th"],
                                              int(c["orb_dist"]), int(c["check_ori"]), ptr(km),
                                              ctypes.byref(nm))
    else:
        S = np.ascontiguousarray(E.scw(), np.float32).reshape(12)
        st = L.orb_search_by_projection_sim3(m.handle, ctypes.byref(f), ptr(S), ctypes.byref(cam),
                                             float(E.LS), len(mps), ptr(mps), ptr(c["mp_desc"]),
                                             c["th"], ptr(km), ctypes.byref(nm))
    return st, km, nm.value, entry
@pytest.mark.parametrize("family,tier", [("reloc", "pp"), ("sim3", "pp"), ("frame", "frame")])
def test_resolve_lds_tiers(gpu, oracle, matchers, family, tier):
    """Dynamic LDS of the one-block resolve kernels below 64 KiB, between 64 KiB
    and 160 KiB, at the largest size the documented rule admits (dynamic plus the
    kernels' 128 B of static LDS = 160 KiB) and one element beyond, where the call
    must be refused on the host with ORB_ECAPACITY."""
    small, mid, top, over = E.LDS_TIERS[tier]
    for nkeys, n in (small, mid, top, small):
        c = E.lds_case(family, nkeys, n)
        ref = E.run_oracle(oracle, c)
        assert ref[0] > n // 4
        _check(E.run_gpu(gpu, matchers, c), ref, (family, nkeys, n))
    c = E.lds_case(family, *over)
    with pytest.raises(gpu.OrbError) as err:
        E.run_gpu(gpu, matchers, c)
    assert err.value.status == gpu.ORB_ECAPACITY
    # the documented outputs of a refused call, through the C ABI (the Python
    # wrapper raises and drops them): kp_match all -1 (kp_matched as on entry
    # for Sim3), *nmatches 0
    st, km, nm, entry = _raw_call(gpu, matchers, c)
    assert st == gpu.ORB_ECAPACITY and nm == 0
    assert np.array_equal(km, entry if family == "sim3" else np.full(len(km), -1, np.int32))
    # the matcher is as usable as before
    c = E.lds_case(family, *small)
    _check(E.run_gpu(gpu, matchers, c), E.run_oracle(oracle, c), (family, "after refusal"))
