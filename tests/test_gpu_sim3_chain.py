"""LoopClosing::ComputeSim3 over a batch of loop candidates as one device-resident
chain on one stream, with no host read until the end:
orb_match_bow_kf_batch -> orb_sim3_solver_setup_batch -> rounds of
{ orb_sim3_solver_iterate_batch(5) -> orb_search_by_sim3_batch (the solver's
d_result and d_inliers12 as they stand) -> orb_optimize_sim3_batch }, against
the host loop oracle.search_by_bow_kf -> sim3_ref -> oracle.search_by_sim3 with
the host merge -> sim3opt_ref (tests/sim3_chain_ref.chain_reference).  Every
row, state, result and the optimiser's output bit for bit, the gated and the
Sim3-less candidates included."""
import numpy as np
import pytest

import sim3_chain_ref as R
import tri_batch_ref as T
from test_gpu_sim3opt import same

pytestmark = pytest.mark.gpu
SENT = 0x5A5A5A5A
ROUNDS = 2


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def test_chain_of_a_batch_of_candidates_on_one_stream(torch, gpu, oracle):
    sides, pairs, points, mp_desc, host, draws = R.chain_scene(oracle)
    ref = R.chain_reference(oracle, sides, pairs, points, mp_desc, host, draws, ROUNDS)
    assert [r["bow"][2][4] for r in ref] == [1, 0, 1]                       # one candidate gated
    assert [int(r["rounds"][0]["result"]["has_sim3"]) for r in ref] == [1, 0, 0]
    m = gpu.ORBmatcher(0.75, True)
    P, S = len(pairs), max(len(s["desc"]) for s in sides) + 3
    arr = T.pack_slots(sides, S, with_u_right=False)
    d = {k: _dev(torch, v) for k, v in arr.items() if v is not None}
    p = lambda t: t.data_ptr()
    junk = lambda n: torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    s1, s2 = (_dev(torch, np.array([q[i] for q in pairs], np.int32)) for i in (0, 1))
    dpts, ddesc, ddraws = _dev(torch, points), _dev(torch, mp_desc), _dev(torch, draws)
    m12, ix2 = junk(P * S * 4), junk(P * S * 4)
    binfo = junk(P * 20)
    state, corr = junk(P * gpu.SIM3_STATE_DTYPE.itemsize), junk(P * S * gpu.SIM3_CORR_DTYPE.itemsize)
    per_round = [dict(res=junk(P * gpu.SIM3_RESULT_DTYPE.itemsize), inl=junk(P * S),
                      sinfo=junk(P * 20), new12=junk(P * S * 4),
                      opt=junk(P * gpu.SIM3_OPT_RESULT_DTYPE.itemsize)) for _ in range(ROUNDS)]
    cam = host["cam"]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    st = stream.cuda_stream
    m.search_by_bow_kf_batch(P, p(s1), p(s2), p(d["keys"]), p(d["desc"]), p(d["nkeys"]),
                             p(d["pidx"]), p(d["fv_nodes"]), p(d["fv_offs"]), p(d["fv_feats"]),
                             p(d["n_fv_nodes"]), S, p(dpts), 20, p(m12), p(ix2), p(binfo), stream=st)
    m.sim3_solver_setup_batch(P, p(s1), p(s2), p(d["keys"]), p(d["nkeys"]), p(d["pidx"]),
                              p(d["pose"]), S, p(dpts), p(m12), 0, p(ix2), host["sigma2"], cam, cam,
                              False, p(state), p(corr), stream=st)
    with torch.cuda.stream(stream):
        state0 = state.clone()    # a device copy on the same stream; no host read
    for r in per_round:
        m.sim3_solver_iterate_batch(P, S, p(state), p(corr), p(ddraws), draws.shape[1], 5,
                                    p(r["inl"]), p(r["res"]), stream=st)
        m.search_by_sim3_batch(P, p(s1), p(s2), p(d["keys"]), p(d["desc"]), p(d["nkeys"]),
                               p(d["pidx"]), p(d["pose"]), S, p(dpts), p(ddesc), p(m12), p(ix2),
                               p(r["inl"]), p(r["res"]), cam,
                               (0.0, float(host["width"]), 0.0, float(host["height"])),
                               host["scale"], float(host["log_scale"]), p(r["sinfo"]),
                               th=host["th"], d_new12=p(r["new12"]), stream=st)
        m.optimize_sim3_batch(P, p(s1), p(s2), p(d["keys"]), p(d["nkeys"]), p(d["pidx"]),
                              p(d["pose"]), S, p(dpts), p(m12), p(ix2), p(r["res"]),
                              host["inv_sigma2"], cam, cam, p(r["opt"]), th2=10.0, fix_scale=False,
                              stream=st)
    torch.cuda.synchronize()

    host_of = lambda t, dt: t.cpu().numpy().view(dt)
    rows = lambda t: host_of(t, np.int32).reshape(P, S)
    g_m12, g_ix2 = rows(m12), rows(ix2)
    g_binfo = host_of(binfo, R.B.INFO_DTYPE)
    g_state0, g_state = host_of(state0, gpu.SIM3_STATE_DTYPE), host_of(state, gpu.SIM3_STATE_DTYPE)
    ran = 0
    for c, (want, (k1, _)) in enumerate(zip(ref, pairs)):
        n1 = len(sides[k1]["desc"])
        assert tuple(int(g_binfo[c][f]) for f in R.BOW_FIELDS) == want["bow"][2], c
        same(g_state0[c], want["state0"], f"candidate {c} setup")
        same(g_state[c], want["state"], f"candidate {c} state")
        for k, r in enumerate(per_round):
            w = want["rounds"][k]
            tag = f"candidate {c} round {k}"
            same(host_of(r["res"], gpu.SIM3_RESULT_DTYPE)[c], w["result"], tag)
            sinfo = host_of(r["sinfo"], R.SEARCH_INFO_DTYPE)
            new12 = rows(r["new12"])
            opt = r["opt"].cpu().numpy().reshape(P, -1)
            if w["search"] is None:     # no Sim3: the search and the optimiser skipped it
                assert (sinfo[c:c + 1].view(np.uint8) == 0x5A).all(), tag
                assert (new12[c] == SENT).all() and (opt[c] == 0x5A).all(), tag
                continue
            ran += 1
            assert np.array_equal(host_of(r["inl"], np.uint8).reshape(P, S)[c, :n1], w["inliers"]), tag
            assert tuple(int(sinfo[c][f]) for f in R.SEARCH_FIELDS) == w["search"][3], tag
            assert np.array_equal(new12[c, :n1], w["search"][2]), tag
            assert (new12[c, n1:] == SENT).all(), tag
            same(opt[c].view(gpu.SIM3_OPT_RESULT_DTYPE)[0], w["opt"], tag + " optimiser")
        assert np.array_equal(g_m12[c, :n1], want["match12"]), f"candidate {c} match12"
        assert np.array_equal(g_ix2[c, :n1], want["index2"]), f"candidate {c} index2"
        assert (g_m12[c, n1:] == SENT).all() and (g_ix2[c, n1:] == SENT).all()
    assert ran == ROUNDS
    # the gated candidate: empty rows, N = 0, no_more at once
    assert (g_m12[1, :len(sides[0]["desc"])] == -1).all() and g_state[1]["n"] == 0
    assert host_of(per_round[0]["res"], gpu.SIM3_RESULT_DTYPE)[1]["no_more"] == 1
