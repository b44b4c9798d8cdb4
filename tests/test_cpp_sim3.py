"""The C++ host mirror's Sim3Solver (orb_slam2-chinese-annotation_amd/host/
orb_amd.hpp): compiles with plain g++ against the C ABI (CPU test) and gives,
on the GPU, the bits the Python binding gives on the same problem, which are
the restatement's."""
import subprocess

import numpy as np
import pytest

import sim3_cases as C
from conftest import PKG_DIR, ROOT
from sim3_ref import CORR_DTYPE, RESULT_DTYPE, STATE_DTYPE

SRC = ROOT / "tests" / "cpp" / "test_sim3_host.cpp"


def _build(out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", str(SRC), "-o", str(out),
           f"-L{PKG_DIR / 'lib'}", "-lorb_amd", "-L/opt/rocm/lib", "-lamdhip64",
           f"-Wl,-rpath,{PKG_DIR / 'lib'}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_sim3_host_compiles_with_gxx(tmp_path, orb):
    orb.lib()
    _build(tmp_path / "test_sim3_host")
    assert (tmp_path / "test_sim3_host").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["first_of_chunk", "skip_all", "exhaust"])
def test_sim3_host_equals_python_on_gpu(gpu, tmp_path, name):
    torch = pytest.importorskip("torch")
    p = C.directed()[name]
    b = C.Batch([p])
    S, rounds_of = C.STRIDE, 5
    has_i1 = b.index1 is not None
    hdr = np.array([S, len(b.nkeys), len(b.points), C.N_LEVELS, int(p.fix_scale),
                    b.draws.shape[1], int(has_i1), rounds_of], np.int32)
    cam = lambda c: np.array(list(c) + [0.0, 0.0], np.float32)
    parts = [hdr, b.kf1_slot, b.kf2_slot, b.keys, b.nkeys, b.point_index, b.pose, b.points,
             b.match12, b.index2] + ([b.index1] if has_i1 else []) + \
            [b.draws, C.LEVEL_SIGMA2, cam(C.CAM1), cam(C.CAM2)]
    (tmp_path / "in.bin").write_bytes(b"".join(np.ascontiguousarray(a).tobytes() for a in parts))
    exe = tmp_path / "test_sim3_host"
    _build(exe)
    run = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("OK"), run.stdout + run.stderr
    out = (tmp_path / "out.bin").read_bytes()
    sizes = [("state0", 184), ("corr0", S * 56), ("state1", 184), ("corr1", S * 56),
             ("res1", 132), ("inl1", S), ("state2", 184), ("res2", 132), ("getters", 13 * 4)]
    c, o = {}, 0
    for k, n in sizes:
        c[k] = out[o:o + n]
        o += n
    assert o == len(out)

    # the Python binding on the same arrays
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d = {k: dev(getattr(b, k)) for k in ("kf1_slot", "kf2_slot", "keys", "nkeys", "point_index",
                                         "pose", "points", "match12", "index2", "draws")}
    i1 = dev(b.index1) if has_i1 else None
    junk = lambda n: torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    state, corr, inl, res = junk(184), junk(S * 56), junk(S), junk(132)
    m = gpu.ORBmatcher(0.75, True)
    raw = lambda t: (torch.cuda.synchronize(), t.cpu().numpy().tobytes())[1]

    def setup():
        m.sim3_solver_setup_batch(
            1, d["kf1_slot"].data_ptr(), d["kf2_slot"].data_ptr(), d["keys"].data_ptr(),
            d["nkeys"].data_ptr(), d["point_index"].data_ptr(), d["pose"].data_ptr(), S,
            d["points"].data_ptr(), d["match12"].data_ptr(), i1.data_ptr() if has_i1 else 0,
            d["index2"].data_ptr(), C.LEVEL_SIGMA2, C.CAM1, C.CAM2, p.fix_scale,
            state.data_ptr(), corr.data_ptr())

    def iterate(n):
        m.sim3_solver_iterate_batch(1, S, state.data_ptr(), corr.data_ptr(),
                                    d["draws"].data_ptr(), b.draws.shape[1], n, inl.data_ptr(),
                                    res.data_ptr())
        return np.frombuffer(raw(res), RESULT_DTYPE)[0]

    setup()
    # the C++ state bytes hold zeros where Python's buffer held junk before setup: all 184 are written
    assert c["state0"] == raw(state) and c["corr0"] == raw(corr)
    ref = p.solver()
    assert c["state0"] == ref.state_record().tobytes()
    for _ in range(61):
        r = iterate(rounds_of)
        last = ref.iterate(rounds_of)
        if r["has_sim3"] or r["no_more"]:
            break
    assert c["state1"] == raw(state) and c["corr1"] == raw(corr)
    assert c["res1"] == raw(res) and c["inl1"] == raw(inl)
    assert c["res1"] == ref.result_record(last[0], last[1], last[3]).tobytes()
    assert np.frombuffer(c["corr1"], CORR_DTYPE)[:ref.N].tobytes() == ref.corr_records().tobytes()
    setup()
    r = iterate(C.MAX_ITERATIONS)
    assert c["state2"] == raw(state) and c["res2"] == raw(res)
    st = np.frombuffer(c["state2"], STATE_DTYPE)[0]
    g = np.frombuffer(c["getters"], np.float32)
    assert g[:9].tobytes() == st["best_R"].tobytes() and g[9:12].tobytes() == st["best_t"].tobytes()
    assert g[12:].tobytes() == st["best_scale"].tobytes()
    found = run.stdout.split()
    assert found == ["OK", str(int(last[0] is not None)), str(int(st["best_inliers"] > 20))]
