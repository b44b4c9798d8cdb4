"""The C++ host mirror's UpdateLocalMap batch, merge and finish calls
(orb_slam2-chinese-annotation_amd/host/orb_amd.hpp): compile with plain g++
against the C ABI (CPU test) and return, on the GPU, what the Python mirror
returns on the same two problems."""
import subprocess

import numpy as np
import pytest

import local_map_cases as C
import local_map_ref as R
from conftest import PKG_DIR, ROOT

SRC = ROOT / "tests" / "cpp" / "test_local_map_host.cpp"
ORDER = ("kf_rank", "kf_by_rank", "kf_bad", "kf_parent", "kf_cov_offs", "kf_cov", "kf_child_offs",
         "kf_child", "kf_mp_offs", "kf_mp", "mp_obs_offs", "mp_obs", "points", "mp_desc")


def _build(out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", str(SRC), "-o", str(out),
           f"-L{PKG_DIR / 'lib'}", "-lorb_amd", "-L/opt/rocm/lib", "-lamdhip64",
           f"-Wl,-rpath,{PKG_DIR / 'lib'}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_local_map_host_compiles_with_gxx(tmp_path, orb):
    orb.lib()
    _build(tmp_path / "test_local_map_host")
    assert (tmp_path / "test_local_map_host").exists()


@pytest.mark.gpu
def test_local_map_host_equals_python_on_gpu(gpu, tmp_path):
    torch = pytest.importorskip("torch")
    m, probs = C.combine([C.get("points_mix"), C.get("voted80")], 4)
    P, NK, NM = len(probs), len(m["rank"]), len(m["points"])
    S, KS, MS = max(len(q["kp_match"]) for q in probs) + 3, NK + 5, 70
    rng = np.random.default_rng(8)
    nk = np.array([len(q["kp_match"]) for q in probs], np.int32)
    km = np.full((P, S), 77, np.int32)
    lkf = np.full((P, KS), 77, np.int32)
    for p, q in enumerate(probs):
        km[p, :nk[p]] = q["kp_match"]
    nlkf = np.zeros(P, np.int32)
    kl = rng.integers(-1, 26, (P, S)).astype(np.int32)
    kl[rng.random((P, S)) < 0.6] = -1
    ol = (rng.random((P, S)) < 0.3).astype(np.uint8)
    va = C.view_arrays(m)
    by_rank = np.zeros(NK, np.int32)
    by_rank[va["kf_rank"]] = np.arange(NK, dtype=np.int32)
    va["kf_by_rank"] = by_rank
    hdr = np.array([P, NK, NM, S, KS, MS, len(va["kf_cov"]), len(va["kf_child"]), len(va["kf_mp"]),
                    len(va["mp_obs"])], np.int32)
    blob = hdr.tobytes() + b"".join(np.ascontiguousarray(va[k]).tobytes() for k in ORDER)
    blob += b"".join(a.tobytes() for a in (nk, km, lkf, nlkf, kl, ol))
    (tmp_path / "in.bin").write_bytes(blob)
    exe = tmp_path / "test_local_map_host"
    _build(exe)
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    out = (tmp_path / "out.bin").read_bytes()
    sizes = [("km", P * S * 4), ("lkf", P * KS * 4), ("nlkf", P * 4), ("li", P * MS * 4),
             ("mps", P * MS * 36), ("desc", P * MS * 32), ("nmps", P * 4), ("locked", P * S),
             ("info", P * 32), ("km_merged", P * S * 4), ("km_final", P * S * 4), ("inl", P * 4)]
    c, o = {}, 0
    for k, n in sizes:
        c[k] = out[o:o + n]
        o += n
    assert o == len(out)

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    view = gpu.MapView(**C.view_arrays(m))
    d = dict(nk=dev(nk), km=dev(km), lkf=dev(lkf), nlkf=dev(nlkf), kl=dev(kl), ol=dev(ol),
             li=torch.full((P * MS,), 77, dtype=torch.int32, device="cuda"),
             mps=torch.zeros(P * MS * 36, dtype=torch.uint8, device="cuda"),
             desc=torch.full((P * MS * 32,), 77, dtype=torch.uint8, device="cuda"),
             nmps=torch.full((P,), 77, dtype=torch.int32, device="cuda"),
             locked=torch.full((P * S,), 77, dtype=torch.uint8, device="cuda"),
             info=torch.zeros(P * 8, dtype=torch.int32, device="cuda"),
             inl=torch.full((P,), 77, dtype=torch.int32, device="cuda"))
    ptr = {k: v.data_ptr() for k, v in d.items()}
    mt = gpu.ORBmatcher(0.8, True)
    mt.update_local_map_batch(P, view, ptr["nk"], ptr["km"], S, ptr["lkf"], ptr["nlkf"], KS,
                              ptr["li"], ptr["mps"], ptr["desc"], ptr["nmps"], MS, ptr["locked"],
                              ptr["info"])
    torch.cuda.synchronize()
    raw = lambda k: d[k].cpu().numpy().tobytes()
    for k in ("km", "lkf", "nlkf", "li", "mps", "desc", "nmps", "locked", "info"):
        assert c[k] == raw(k), k
    mt.track_local_merge_batch(P, ptr["nk"], S, ptr["kl"], ptr["li"], MS, ptr["km"])
    torch.cuda.synchronize()
    assert c["km_merged"] == raw("km")
    mt.track_local_map_finish_batch(P, ptr["nk"], S, ptr["km"], ptr["ol"], view.dev["points"].data_ptr(),
                                    0, False, True, ptr["inl"])
    torch.cuda.synchronize()
    assert c["km_final"] == raw("km") and c["inl"] == raw("inl")
    # and both are the reference's
    info = np.frombuffer(c["info"], R.INFO_DTYPE)
    li = np.frombuffer(c["li"], np.int32).reshape(P, MS)
    kmf = np.frombuffer(c["km_final"], np.int32).reshape(P, S)
    inl = np.frombuffer(c["inl"], np.int32)
    for p, q in enumerate(probs):
        e = R.update_local_map(m, q["kp_match"], [], MS)
        assert info[p].tolist() == e["info"].tolist(), p
        k = len(e["local_index"])
        assert k >= 26 and np.array_equal(li[p, :k], e["local_index"]), p
        merged = R.merge(e["kp_match"], kl[p, :nk[p]], e["local_index"])
        n_in, fin = R.finish(merged, ol[p, :nk[p]], m["points"], False, True)
        assert inl[p] == n_in and np.array_equal(kmf[p, :nk[p]], fin), p
    assert info["n_local_points"].tolist() == [26, 83] and (inl > 0).all()
