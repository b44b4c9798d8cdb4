"""The C++ host mirror's device-batched SearchForTriangulation
(orb_slam2-chinese-annotation_amd/host/orb_amd.hpp): compiles with plain g++
against the C ABI (CPU test) and returns, on the GPU, the reference's rows and
records on three problems over four keyframe slots."""
import subprocess

import numpy as np
import pytest

import matcher_edge_cases as E
import tri_batch_ref as T
from conftest import PKG_DIR, ROOT

SRC = ROOT / "tests" / "cpp" / "test_tri_batch_host.cpp"
ORDER = ("keys", "desc", "nkeys", "fv_nodes", "fv_offs", "fv_feats", "n_fv_nodes", "pidx",
         "u_right", "pose")


def _build(out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", str(SRC), "-o", str(out),
           f"-L{PKG_DIR / 'lib'}", "-lorb_amd", "-L/opt/rocm/lib", "-lamdhip64",
           f"-Wl,-rpath,{PKG_DIR / 'lib'}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_tri_batch_host_compiles_with_gxx(tmp_path, orb):
    orb.lib()
    _build(tmp_path / "test_tri_batch_host")
    assert (tmp_path / "test_tri_batch_host").exists()


@pytest.mark.gpu
def test_tri_batch_host_equals_the_reference_on_gpu(gpu, oracle, tmp_path):
    a1, a2, f_a = T.from_tri_case(E.tri_case(sizes=(1, 63, 64, 65)))
    b1, b2, f_b = T.from_tri_case(E.hist_bow("eleven_two_one", form="kf"))
    sides, pairs, f12 = [a1, a2, b1, b2], [(0, 1), (2, 3), (0, 3)], np.stack([f_a, f_b, f_a])
    stride = max(len(s["desc"]) for s in sides) + 1
    arr = T.pack_slots(sides, stride)
    P, K, ori = len(pairs), len(sides), True
    blob = np.array([P, K, stride, len(E.SCALE), 0, int(ori)], np.int32).tobytes()
    blob += np.asarray(E.CAM, np.float32).tobytes() + E.SCALE.tobytes() + E.SIGMA2.tobytes()
    blob += b"".join(arr[k].tobytes() for k in ORDER)
    blob += np.array([p[0] for p in pairs], np.int32).tobytes()
    blob += np.array([p[1] for p in pairs], np.int32).tobytes() + f12.astype(np.float32).tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    exe = tmp_path / "test_tri_batch_host"
    _build(exe)
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    out = (tmp_path / "out.bin").read_bytes()
    m12 = np.frombuffer(out[:P * stride * 4], np.int32).reshape(P, stride)
    info = np.frombuffer(out[P * stride * 4:], T.INFO_DTYPE)
    for p, (k1, k2) in enumerate(pairs):
        row, want = T.expected_slot(oracle, arr, k1, k2, f12[p], stride, E.CAM, E.SCALE, E.SIGMA2,
                                    False, ori)
        T.check(m12, info, p, len(row), row, want, 77, "c++")
    assert info["n_matches"][0] >= 20 and info["n_matches"][1] == 13
