"""GPU parity of place recognition on the directed inputs of
placerec_edge_cases.py: every score case through the host call (score_pairs)
and the device call (score_batch), every database script through the device
database, against the restatement's answers (tests/placerec_ref.py; the oracle
is held to the same answers on the CPU by test_oracle_placerec.py).  After
every query lKFsSharingWords (ids, word counts, scored flags, score bits) and
the candidates are compared exactly; any NaN equals any NaN."""
import numpy as np
import pytest

import placerec_edge_cases as ec
import placerec_ref as ref
import scenarios
from test_gpu_placerec import _tree, _voc

pytestmark = pytest.mark.gpu

DB_NAMES = list(ec.DB_CASES)
SCORE_NAMES = list(ec.SCORE_CASES)
_vocs = {}


def _vocabulary(gpu, L, scoring):
    """One device vocabulary per (depth, scoring), shared by the cases."""
    key = (L, scoring)
    if key not in _vocs:
        _vocs[key] = _voc(gpu, _tree(L, 40 + L), scoring)
    return _vocs[key]


def _csr(torch, vs):
    dev = torch.device("cuda:0")
    offs = np.zeros(len(vs) + 1, np.int32)
    offs[1:] = np.cumsum([len(x[0]) for x in vs])
    w = np.concatenate([x[0] for x in vs] + [np.zeros(1, np.uint32)]).astype(np.uint32).view(np.int32)
    x = np.concatenate([x[1] for x in vs] + [np.zeros(1)]).astype(np.float64)
    return [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (offs, w, x)]


def _score_batch(torch, voc, al, bl):
    ao, aw, av = _csr(torch, al)
    bo, bw, bv = _csr(torch, bl)
    out = torch.full((len(al),), -7.0, dtype=torch.float64, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    voc.score_batch(len(al), ao.data_ptr(), aw.data_ptr(), av.data_ptr(), bo.data_ptr(),
                    bw.data_ptr(), bv.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


# --------------------------------------------------------------------- score
@pytest.mark.parametrize("scoring", ec.SCORINGS)
def test_directed_scores_host(gpu, scoring):
    pairs, want = ec.score_pairs_by_scoring(scoring)
    voc = _vocabulary(gpu, 3, scoring)
    al, bl = [a for _, a, _ in pairs], [b for _, _, b in pairs]
    got = voc.score_pairs(al, bl)
    bad = [(i, pairs[i][0]) for i in range(len(pairs)) if not ec.same_doubles(got[i:i + 1], want[i:i + 1])]
    assert not bad, bad
    for n in ec.PAIR_COUNTS:                        # 1, 4 and 5 pairs: a workgroup takes four
        for start in (0, len(pairs) - n):
            got = voc.score_pairs(al[start:start + n], bl[start:start + n])
            assert ec.same_doubles(got, want[start:start + n]), (n, start)


@pytest.mark.parametrize("scoring", ec.SCORINGS)
def test_directed_scores_device_batch(gpu, scoring):
    torch = pytest.importorskip("torch")
    pairs, want = ec.score_pairs_by_scoring(scoring)
    voc = _vocabulary(gpu, 3, scoring)
    al, bl = [a for _, a, _ in pairs], [b for _, _, b in pairs]
    got = _score_batch(torch, voc, al, bl)
    bad = [(i, pairs[i][0]) for i in range(len(pairs)) if not ec.same_doubles(got[i:i + 1], want[i:i + 1])]
    assert not bad, bad
    for n in ec.PAIR_COUNTS:
        for start in (0, len(pairs) - n):
            got = _score_batch(torch, voc, al[start:start + n], bl[start:start + n])
            assert ec.same_doubles(got, want[start:start + n]), (n, start)


def test_every_score_case_is_run():
    n = sum(len(ec.score_pairs_by_scoring(s)[0]) for s in ec.SCORINGS)
    assert n == sum(len(ec.score_case(name)) for name in SCORE_NAMES)


def test_score_batch_on_strided_transform_output(gpu, oracle):
    """orb_vocabulary_score_batch on orb_vocabulary_transform_batch outputs left
    where the transform wrote them: frame f at [f * stride, f * stride +
    d_n_words[f]).  One offsets array describes back-to-back vectors, so the
    offsets are built on the device as the pair (f * stride, f * stride + n_f)
    per frame, and each pair of frames is one call with n_pairs = 1 whose
    offsets pointers address those two entries."""
    torch = pytest.importorskip("torch")
    v = _tree(4, 44)
    voc = _voc(gpu, v)
    stride, counts = 300, np.array([300, 170, 233], np.int32)   # not a power of two
    F = len(counts)
    desc = np.zeros((F, stride, 32), np.uint8)
    for f in range(F):
        desc[f, :counts[f]] = scenarios.vocab_features(v, int(counts[f]), rng_seed=60 + f)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    z = lambda n, dt: torch.full((n,), -7, dtype=dt, device=dev)
    d_counts, d_desc = t(counts), t(desc)
    fw, fwt, fn = z(F * stride, torch.int32), z(F * stride, torch.float64), z(F * stride, torch.int32)
    bw, bv, nw = z(F * stride, torch.int32), z(F * stride, torch.float64), z(F, torch.int32)
    fvn, fvo, fvf, nfv = (z(F * stride, torch.int32), z(F * (stride + 1), torch.int32),
                          z(F * stride, torch.int32), z(F, torch.int32))
    torch.cuda.synchronize()
    voc.transform_batch(F, d_counts.data_ptr(), d_desc.data_ptr(), stride, 4, fw.data_ptr(),
                        fwt.data_ptr(), fn.data_ptr(), bw.data_ptr(), bv.data_ptr(),
                        nw.data_ptr(), fvn.data_ptr(), fvo.data_ptr(), fvf.data_ptr(),
                        nfv.data_ptr())
    # offsets[2 f] = f * stride, offsets[2 f + 1] = f * stride + n_words[f]; nothing leaves the device
    start = torch.arange(F, dtype=torch.int32, device=dev) * stride
    offs = torch.stack([start, start + nw], 1).reshape(-1).contiguous()
    out = z(F * F, torch.float64)
    torch.cuda.synchronize()
    for fa in range(F):
        for fb in range(F):
            voc.score_batch(1, offs.data_ptr() + 8 * fa, bw.data_ptr(), bv.data_ptr(),
                            offs.data_ptr() + 8 * fb, bw.data_ptr(), bv.data_ptr(),
                            out.data_ptr() + 8 * (fa * F + fb))
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(F, F)
    bows = [oracle.vocab_transform(v, desc[f, :counts[f]], 4)[:2] for f in range(F)]
    assert all(0 < len(b[0]) < stride for b in bows[1:])         # gaps behind frames 1 and 2
    want = np.array([[ref.score(bows[fa], bows[fb]) for fb in range(F)] for fa in range(F)])
    assert ec.same_doubles(got, want)
    assert (np.diag(want) > 0.99).all() and (want[0, 1:] < 0.9).all()


# ------------------------------------------------------------------ database
@pytest.mark.parametrize("name", DB_NAMES)
def test_directed_database(gpu, name):
    case = ec.db_case(name)
    want = ec.ref_answers(name)
    voc = _vocabulary(gpu, case["L"], case["scoring"])
    if case["L"] == 4:
        assert voc.n_words >= 9000
    assert voc.n_words >= ec.voc_size(case)
    db = gpu.KeyFrameDatabase(voc)
    try:
        got = ec.replay(case, db, lambda tag, d: dict(n_db=len(d)))
    finally:
        db.close()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        tag = w["tag"]
        assert np.array_equal(g["ids"], w["ids"]), tag
        assert np.array_equal(g["common"], w["common"]), tag
        assert np.array_equal(g["scored"], w["scored"]), tag
        assert ec.same_floats(g["scores"], w["scores"]), tag
        assert g["out"] == w["out"], tag
        assert g["seen"]["n_db"] == w["seen"]["n_db"], tag
