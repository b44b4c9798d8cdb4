"""The C++ host mirror's two ComputeSim3 matcher batches
(orb_slam2-chinese-annotation_amd/host/orb_amd.hpp): compiles with plain g++
against the C ABI and forwards the capacity functions (CPU tests), and returns,
on the GPU, the reference's rows and records for the BoW batch followed by the
SearchBySim3 batch on its rows."""
import subprocess

import numpy as np
import pytest

import sim3_chain_ref as R
import tri_batch_ref as T
from conftest import PKG_DIR, ROOT

SRC = ROOT / "tests" / "cpp" / "test_sim3_chain_host.cpp"
ORDER = ("keys", "desc", "nkeys", "fv_nodes", "fv_offs", "fv_feats", "n_fv_nodes", "pidx", "pose")


def _build(out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", str(SRC), "-o", str(out),
           f"-L{PKG_DIR / 'lib'}", "-lorb_amd", "-L/opt/rocm/lib", "-lamdhip64",
           f"-Wl,-rpath,{PKG_DIR / 'lib'}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_sim3_chain_host_compiles_and_forwards_the_capacities(tmp_path, orb):
    orb.lib()
    exe = tmp_path / "test_sim3_chain_host"
    _build(exe)
    r = subprocess.run([str(exe), "caps"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert [int(v) for v in r.stdout.split()] == [orb.match_bow_kf_batch_max_stride(),
                                                  orb.search_by_sim3_batch_max_stride(),
                                                  orb.optimize_sim3_max_stride()]


@pytest.mark.gpu
def test_sim3_chain_host_equals_the_reference_on_gpu(gpu, oracle, tmp_path):
    (s1, s2), points, mp_desc, host, rec = R.loop_scene(oracle, nf=300)
    sides, pairs = [s1, s2], [(0, 1), (1, 0)]
    recs = np.array([rec, R.sim3_record()], R.SIM3_RESULT_DTYPE)
    stride = max(len(s["desc"]) for s in sides) + 1
    arr = T.pack_slots(sides, stride, with_u_right=False)
    P, K, ori, nnratio, gate = len(pairs), len(sides), True, 0.75, 20
    blob = np.array([P, K, stride, len(host["scale"]), len(points), int(ori), gate], np.int32).tobytes()
    blob += np.float32(nnratio).tobytes() + np.asarray(host["cam"], np.float32).tobytes()
    blob += np.array([host["width"], host["height"], host["log_scale"], host["th"]],
                     np.float32).tobytes()
    blob += np.asarray(host["scale"], np.float32).tobytes()
    blob += b"".join(arr[k].tobytes() for k in ORDER)
    blob += np.array([p[0] for p in pairs], np.int32).tobytes()
    blob += np.array([p[1] for p in pairs], np.int32).tobytes()
    blob += points.tobytes() + np.ascontiguousarray(mp_desc).tobytes() + recs.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    exe = tmp_path / "test_sim3_chain_host"
    _build(exe)
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    out = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.uint8)
    row = P * stride * 4
    cut = np.cumsum([0, row, row, P * 20, row, row, row, P * 20])
    part = lambda i, dt: out[cut[i]:cut[i + 1]].view(dt)
    rows = lambda i: part(i, np.int32).reshape(P, stride)
    before = {k: np.full((P, stride), 0x5A5A5A5A, np.int32) for k in ("match12", "index2", "new12")}
    for p, (k1, k2) in enumerate(pairs):
        n = len(sides[k1]["desc"])
        bow = R.bow_kf_expected_slot(oracle, arr, k1, k2, stride, points, nnratio, ori, gate)
        R.check_bow(rows(0), rows(1), part(2, R.B.INFO_DTYPE), p, n, bow, 0x5A5A5A5A, "c++ bow")
        want = R.sim3_expected_slot(oracle, arr, k1, k2, stride, points, mp_desc, bow[0], bow[1],
                                    None, recs[p], host)
        R.check_sim3(dict(match12=rows(3), index2=rows(4), new12=rows(5)),
                     part(6, R.SEARCH_INFO_DTYPE), p, n, before, want, 0x5A, "c++ search")
    assert part(2, R.B.INFO_DTYPE)["n_matches"][0] > 20
