"""The C++ host mirror's device-batched SearchByBoW(KF, F) and strided-count
discard calls (orb_slam2-chinese-annotation_amd/host/orb_amd.hpp): compile with
plain g++ against the C ABI (CPU test) and return, on the GPU, what the Python
mirror returns on the same two problems."""
import subprocess

import numpy as np
import pytest

import bow_batch_ref as B
import matcher_edge_cases as E
import scenarios as S
import track_motion_ref as R
from conftest import PKG_DIR, ROOT

SRC = ROOT / "tests" / "cpp" / "test_bow_batch_host.cpp"
ORDER = ("keys", "desc", "nkeys", "fv_nodes", "fv_offs", "fv_feats", "n_fv_nodes")


def _build(out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", str(SRC), "-o", str(out),
           f"-L{PKG_DIR / 'lib'}", "-lorb_amd", "-L/opt/rocm/lib", "-lamdhip64",
           f"-Wl,-rpath,{PKG_DIR / 'lib'}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_bow_batch_host_compiles_with_gxx(tmp_path, orb):
    orb.lib()
    _build(tmp_path / "test_bow_batch_host")
    assert (tmp_path / "test_bow_batch_host").exists()


@pytest.mark.gpu
def test_bow_batch_host_equals_python_on_gpu(gpu, oracle, tmp_path):
    torch = pytest.importorskip("torch")
    probs = [B.from_bow(S.bow_pair(oracle, 5, nf=60)), B.from_bow(E.hist_bow("eleven_two_one"))]
    P, nnratio, ori, min_matches = len(probs), 0.75, True, 15
    stride = max(len(s["desc"]) for p in probs for s in (p["kf"], p["f"])) + 1
    ka, fa = B.pack_slots([p["kf"] for p in probs], stride), B.pack_slots([p["f"] for p in probs], stride)
    pts, mps = B.pack_points([p["points"] for p in probs])
    pts["pos"], pts["has_obs"] = 0, 1
    blob = np.array([P, stride, mps, min_matches, int(ori)], np.int32).tobytes()
    blob += np.float32(nnratio).tobytes()
    for a in (ka, fa):
        blob += b"".join(a[k].tobytes() for k in ORDER)
    blob += ka["pidx"].tobytes() + pts.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    exe = tmp_path / "test_bow_batch_host"
    _build(exe)
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    out = (tmp_path / "out.bin").read_bytes()
    n_km = P * stride * 4
    c_km = np.frombuffer(out[:n_km], np.int32).reshape(P, stride)
    c_info = np.frombuffer(out[n_km:n_km + P * 20], B.INFO_DTYPE)
    c_out = np.frombuffer(out[n_km + P * 20:n_km + P * 32], R.DISCARD_DTYPE)
    c_km5 = np.frombuffer(out[n_km + P * 32:], np.int32).reshape(P, stride)

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    dk, df = {k: dev(v) for k, v in ka.items()}, {k: dev(v) for k, v in fa.items()}
    d_pts = dev(pts)
    d_km = torch.full((P * stride,), 77, dtype=torch.int32, device="cuda")
    d_info = torch.zeros(P * 5, dtype=torch.int32, device="cuda")
    m = gpu.ORBmatcher(nnratio, ori)
    m.search_by_bow_batch(P, 0, 0, dk["keys"].data_ptr(), dk["desc"].data_ptr(),
                          dk["nkeys"].data_ptr(), dk["pidx"].data_ptr(), dk["fv_nodes"].data_ptr(),
                          dk["fv_offs"].data_ptr(), dk["fv_feats"].data_ptr(),
                          dk["n_fv_nodes"].data_ptr(), df["keys"].data_ptr(), df["desc"].data_ptr(),
                          df["nkeys"].data_ptr(), df["fv_nodes"].data_ptr(), df["fv_offs"].data_ptr(),
                          df["fv_feats"].data_ptr(), df["n_fv_nodes"].data_ptr(), stride,
                          d_pts.data_ptr(), mps, min_matches, d_km.data_ptr(), d_info.data_ptr())
    torch.cuda.synchronize()
    p_km = d_km.cpu().numpy().reshape(P, stride)
    p_info = d_info.cpu().numpy().view(B.INFO_DTYPE)
    assert np.array_equal(c_km, p_km) and c_info.tobytes() == p_info.tobytes()
    for p, q in enumerate(probs):
        km, info = B.expected(oracle, q, nnratio, ori, min_matches)
        B.check(c_km, c_info, p, len(km), km, info, 77, "c++")
        ol = np.zeros(P * stride, np.uint8)
        ol[::3] = 1
        rk, _, _, rout = R.discard_outliers(km, ol.reshape(P, stride)[p, :len(km)],
                                            pts[p * mps:(p + 1) * mps], info[0], True)
        assert np.array_equal(c_km5[p, :len(km)], rk) and c_out[p].tolist() == rout.tolist(), p
    assert c_info["n_matches"].tolist()[0] >= 30 and c_info["enough"].tolist() == [1, 0]
