"""ORBmatcher::SearchForInitialization (k_init_prep, k_init_candidates,
k_init_resolve) and MapPoint::ComputeDistinctiveDescriptors (k_distinctive) on
the GPU, on the directed inputs of mapping_edge_cases.py, against the CPU
oracle: n, m12, the prev bytes, best and the out rows, through the single-frame
calls and through the batch calls, with junk past every count that must stay.
test_mapping_edge_cases.py shows on the CPU that these inputs reach the
kernels' branches (census) and separate the reference's rules from their wrong
neighbours.

Also here: two batches on two streams of one handle, the strides around the
64 KiB dynamic-LDS attribute and at the capacity limit, and the argument
checks of the batch entries."""
import ctypes
import functools

import numpy as np
import pytest

import mapping_edge_cases as E

pytestmark = pytest.mark.gpu
INIT = sorted(n for n in E.CASES if n != "distinctive")


@functools.lru_cache(maxsize=None)
def case(name):
    return E.CASES[name][0]()


@functools.lru_cache(maxsize=None)
def reference(name):
    import oracle as o
    o.lib()
    c = case(name)
    if c["kind"] == "init":
        return [E.run_oracle(o, p) for p in c["problems"]]
    return o.distinctive_descriptors(c["offs"], c["desc"])


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


# ------------------------------------------------------------ single-frame calls
@pytest.mark.parametrize("name", [n for n in INIT if n != "shifted_bounds"])
def test_directed_single(gpu, name):
    for p, (rn, rm, rp) in zip(case(name)["problems"], reference(name)):
        n, m12, prev = E.run_gpu(gpu, p)
        assert n == rn, (p["name"], n, rn)
        assert np.array_equal(m12, rm), (p["name"], np.nonzero(m12 != rm)[0][:10])
        assert prev.dtype == rp.dtype and prev.tobytes() == rp.tobytes(), p["name"]


# ------------------------------------------------------------------ batch calls
@functools.lru_cache(maxsize=None)
def groups():
    """Every problem of every case, grouped by what one batch call shares
    (window, nnratio, orientation check, grid bounds)."""
    g = {}
    for name in INIT:
        for p, ref in zip(case(name)["problems"], reference(name)):
            g.setdefault(E.batch_key(p), []).append((p, ref))
    return g


def _group_ids():
    return sorted(set(E.batch_key(p) for name in INIT for p in case(name)["problems"]))


@pytest.mark.parametrize("key", _group_ids(),
                         ids=lambda k: "w%d_nn%g_ori%d_min%g" % (k[0], k[1], k[2], k[3][0]))
def test_directed_batch(gpu, torch, key):
    """All problems of one kind in one batch, kp_stride above every count; then
    the same call again on the first one's scratch."""
    probs, refs = zip(*groups()[key])
    stride = max(max(len(p["k1"]), len(p["k2"])) for p in probs) + 3
    b = E.Batch(torch, list(probs), stride)
    m = gpu.ORBmatcher(key[1], key[2])
    b.launch(m)
    E.check_batch(probs, refs, b.fetch(), "first call")
    b.reset()
    b.launch(m)
    E.check_batch(probs, refs, b.fetch(), "second call")


def test_two_streams_one_handle(gpu, torch):
    """Two batches on two streams through one handle, nothing between them:
    the handle's call-order rule serialises them on its scratch."""
    g = groups()
    key = E.batch_key(case("batch_lanes")["problems"][0])
    probs, refs = zip(*g[key])
    a = E.Batch(torch, list(probs), 300)
    b = E.Batch(torch, list(probs[::-1]), 261)
    m = gpu.ORBmatcher(key[1], key[2])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a.launch(m, stream=s1.cuda_stream)
    b.launch(m, stream=s2.cuda_stream)
    E.check_batch(probs, refs, a.fetch(), "stream 1")
    E.check_batch(probs[::-1], refs[::-1], b.fetch(), "stream 2")


# --------------------------------------------------------- strides and capacity
def _tiny():
    c = case("batch_lanes")["problems"]
    r = reference("batch_lanes")
    return [c[2], c[0]], [r[2], r[0]]     # 65 and 63 queries, a few dozen keypoints each


@pytest.mark.parametrize("stride", [4096, 4097])
def test_stride_around_64k(gpu, torch, stride):
    """kp_stride 4096: 64 KiB of dynamic LDS exactly, launched as it is; 4097:
    the first launch that raises the kernel's dynamic-LDS limit."""
    L = gpu.lib().orb_k_init_lds
    L.restype, L.argtypes = ctypes.c_size_t, [ctypes.c_int]
    assert (L(4096) == 65536) and (L(4097) > 65536)
    probs, refs = _tiny()
    E.check_batch(probs, refs, E.run_gpu_batch(gpu, torch, probs, stride), "stride %d" % stride)


def test_largest_stride(gpu, torch):
    """The largest kp_stride the host accepts launches: 16 B per slot and the
    kernel's 128 static bytes fill the 160 KiB of a workgroup exactly."""
    stride = gpu.ORBmatcher.search_init_limits()["max_stride"]
    probs, refs = _tiny()
    E.check_batch(probs, refs, E.run_gpu_batch(gpu, torch, probs, stride), "stride %d" % stride)


def test_stride_above_capacity(gpu, torch):
    stride = gpu.ORBmatcher.search_init_limits()["max_stride"] + 1
    probs, _ = _tiny()
    b = E.Batch(torch, probs, 200)      # the arrays need not be that long: nothing is launched
    m = gpu.ORBmatcher(0.9, False)
    with pytest.raises(gpu.OrbError) as err:
        b.launch(m, stride=stride)
    assert err.value.status == gpu.ORB_ECAPACITY
    assert b.untouched()


def test_argument_checks(gpu, torch):
    probs, refs = _tiny()
    b = E.Batch(torch, probs, 200)
    m = gpu.ORBmatcher(0.9, False)
    for kw in (dict(n_problems=65536), dict(bounds=(10.0, 10.0, 0.0, 480.0)),
               dict(bounds=(10.0, 5.0, 0.0, 480.0)), dict(bounds=(0.0, 640.0, 3.0, 3.0)),
               dict(stride=0)):
        with pytest.raises(gpu.OrbError) as err:
            b.launch(m, **kw)
        assert err.value.status == gpu.ORB_EINVAL, kw
        assert b.untouched(), kw
    b.launch(m, n_problems=0)           # ORB_OK, no launch
    assert b.untouched()
    b.launch(m)                         # and the same arrays still work
    E.check_batch(probs, refs, b.fetch(), "after the refused calls")


# ------------------------------------------------------- distinctive descriptors
def test_distinctive_single(gpu):
    c, ref = case("distinctive"), reference("distinctive")
    best, out = gpu.ORBmatcher().ComputeDistinctiveDescriptors(c["offs"], c["desc"], c["init"])
    assert np.array_equal(best, ref), [(c["names"][i], best[i], ref[i])
                                       for i in np.nonzero(best != ref)[0]]
    assert np.array_equal(out, E.distinctive_expected_out(c, ref))   # empty lists: input bytes


@pytest.mark.parametrize("with_out", [True, False])
def test_distinctive_batch(gpu, torch, with_out):
    c, ref = case("distinctive"), reference("distinctive")
    n = len(ref)
    d_offs = torch.from_numpy(c["offs"]).to("cuda")
    d_desc = torch.from_numpy(c["desc"]).to("cuda")
    d_best = torch.full((n + 2,), E.JUNK_M12, dtype=torch.int32, device="cuda")
    init = np.concatenate([c["init"], np.full((2, 32), 0xA5, np.uint8)])
    d_out = torch.from_numpy(init).to("cuda")
    torch.cuda.synchronize()
    gpu.ORBmatcher().distinctive_descriptors_batch(n, d_offs.data_ptr(), d_desc.data_ptr(),
                                                   d_best.data_ptr(),
                                                   d_out.data_ptr() if with_out else None)
    torch.cuda.synchronize()
    best, out = d_best.cpu().numpy(), d_out.cpu().numpy()
    assert np.array_equal(best[:n], ref), [(c["names"][i], best[i], ref[i])
                                           for i in np.nonzero(best[:n] != ref)[0]]
    assert (best[n:] == E.JUNK_M12).all()
    want = E.distinctive_expected_out(c, ref) if with_out else c["init"]   # null d_out: best only
    assert np.array_equal(out[:n], want)
    assert (out[n:] == 0xA5).all()
