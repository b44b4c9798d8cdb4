"""The C++ host mirror's ComputeSceneMedianDepth / CreateNewMapPoints
(orb_slam2-chinese-annotation_amd/host/orb_amd.hpp): compiles with plain g++
against the C ABI (CPU test) and gives, on the GPU, the restatement's bits."""
import subprocess

import numpy as np
import pytest

import newpoints_cases as C
import newpoints_ref as R
from conftest import PKG_DIR, ROOT

SRC = ROOT / "tests" / "cpp" / "test_newpoints_host.cpp"


def _build(out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", str(SRC), "-o", str(out),
           f"-L{PKG_DIR / 'lib'}", "-lorb_amd", "-L/opt/rocm/lib", "-lamdhip64",
           f"-Wl,-rpath,{PKG_DIR / 'lib'}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_newpoints_host_compiles_with_gxx(tmp_path, orb):
    orb.lib()
    _build(tmp_path / "test_newpoints_host")
    assert (tmp_path / "test_newpoints_host").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nat_mono_100", "nat_stereo_far_120", "undefined_kinds",
                                  "gate_mono_below"])
def test_newpoints_host_equals_the_restatement_on_gpu(gpu, tmp_path, name):
    c = {x.name: x for x in C.all_cases()}[name]
    n1, n2 = len(c.kf1["keys"]), len(c.kf2["keys"])
    stereo = c.kf1["u_right"] is not None
    exist = c.points if c.points is not None else np.zeros(0, R.MAP_POINT_DTYPE)
    hdr = np.array([n1, n2, C.N_LEVELS, int(c.monocular), int(stereo), c.cursor, c.capacity,
                    len(exist)], np.int32)
    parts = [hdr]
    for kf in (c.kf1, c.kf2):
        parts += [kf["keys"]] + ([kf["u_right"], kf["depth"]] if stereo else []) + \
                 [kf["point_index"], np.array([kf["pose"]])]
    parts += [c.match12, np.array(c.cam1, np.float32), np.array(c.cam2, np.float32),
              C.SCALE_FACTORS, C.LEVEL_SIGMA2, exist, np.array([c.median], np.float32)]
    (tmp_path / "in.bin").write_bytes(b"".join(np.ascontiguousarray(a).tobytes() for a in parts))
    exe = tmp_path / "test_newpoints_host"
    _build(exe)
    run = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("OK"), run.stdout + run.stderr
    out = (tmp_path / "out.bin").read_bytes()
    sizes = [("info", 64), ("cursor", 4), ("status", n1), ("x3d", 12 * n1), ("pairs", 8 * n1),
             ("pidx1", 4 * n1), ("pidx2", 4 * n2), ("points", 36 * c.capacity), ("median", 4),
             ("count", 4)]
    got, o = {}, 0
    for k, n in sizes:
        got[k] = out[o:o + n]
        o += n
    assert o == len(out)
    # the C++ wrapper zero-fills what the call does not write
    ref = c.run(prefill=(np.zeros(n1, np.uint8), np.zeros((n1, 3), np.float32),
                         np.zeros((n1, 2), np.int32), C.junk_points(c.capacity)))
    assert got["info"] == ref["info"].tobytes()
    assert np.frombuffer(got["cursor"], np.int32)[0] == ref["cursor"]
    assert got["status"] == ref["status"].tobytes()
    a, b = np.frombuffer(got["x3d"], np.float32), ref["x3d"].reshape(-1)
    assert ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()
    assert got["pairs"] == ref["pairs"].tobytes()
    assert got["pidx1"] == ref["pidx1"].tobytes() and got["pidx2"] == ref["pidx2"].tobytes()
    assert got["points"] == ref["points"].tobytes()
    if c.monocular:
        med, cnt = R.scene_median_depth(c.kf2["point_index"], c.kf2["pose"],
                                        exist["pos"] if len(exist) else np.zeros((0, 3)), 2)
        m = np.frombuffer(got["median"], np.float32)[0]
        assert (np.isnan(m) and np.isnan(med)) or m.tobytes() == np.float32(med).tobytes()
        assert np.frombuffer(got["count"], np.int32)[0] == cnt
    assert run.stdout.split() == ["OK", str(int(ref["info"]["n_new"])), str(int(ref["info"]["gated"]))]
