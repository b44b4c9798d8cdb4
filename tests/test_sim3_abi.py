"""The Sim3Solver entries are additive: include/orb_abi.h declares them and
their records, the library exports them, the Python wrapper binds them with
the same layouts, ORB_ABI_VERSION stays 1, the capacity is the documented LDS
formula, and the pin list stands identically in its three places."""
import ctypes
import re
import subprocess

import numpy as np

from conftest import ROOT

HEADER = ROOT / "include" / "orb_abi.h"
NEW = ("orb_sim3_solver_setup_batch", "orb_sim3_solver_iterate_batch",
       "orb_sim3_solver_max_stride")
i32, f32, u8 = ctypes.c_int32, ctypes.c_float, ctypes.c_uint8


class Corr(ctypes.Structure):
    _fields_ = [("index1", i32), ("x1", f32 * 3), ("x2", f32 * 3), ("p1", f32 * 2),
                ("p2", f32 * 2), ("max_err1", f32), ("max_err2", f32), ("best_inlier", u8),
                ("_pad", u8 * 3)]


class State(ctypes.Structure):
    _fields_ = [("status", i32), ("n1", i32), ("n", i32), ("max_its", i32), ("iterations", i32),
                ("best_inliers", i32), ("best_iteration", i32), ("min_inliers", i32),
                ("fix_scale", i32), ("best_scale", f32), ("best_R", f32 * 9), ("best_t", f32 * 3),
                ("best_T12", f32 * 16), ("k1", f32 * 4), ("k2", f32 * 4)]


class Result(ctypes.Structure):
    _fields_ = [("has_sim3", i32), ("no_more", i32), ("n_inliers", i32), ("iterations_run", i32),
                ("T12", f32 * 16), ("R", f32 * 9), ("t", f32 * 3), ("scale", f32)]


def _header_fields(code, tag):
    body = re.search(r"typedef struct %s\s*{(.*?)}\s*%s_t;" % (tag, tag), code, re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(None, 1)[1].split(","):
            names.append(re.match(r"\s*(\w+)", part).group(1))
    return names


def test_header_declares_the_entries_and_keeps_the_version():
    text = HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"#define\s+ORB_ABI_VERSION\s+1\b", text)
    for tag, S in (("orb_sim3_corr", Corr), ("orb_sim3_state", State), ("orb_sim3_result", Result)):
        assert _header_fields(code, tag) == [f[0] for f in S._fields_], tag
    head = text[:text.index("#ifndef ORB_ABI_H")]
    for name in NEW[:2]:
        assert name in head, name
    for ref in ("src/Sim3Solver.cc:37-141", ":144-220", ":237-351", ":354-378", ":396-417"):
        assert ref in head, ref
    doc = text[text.index("Sim3Solver on the device"):text.index("/* ---", text.index("orb_sim3_solver_iterate_batch("))]
    doc = " ".join(re.sub(r"\n\s*\*", " ", doc).split())  # comment stars and line breaks dropped
    for phrase in ("NOT checked", "ORB_ECAPACITY", "swap with the back", "bit for bit",
                   "draw_stride < 3 * max_iterations", "unpinned against a real OpenCV",
                   "Thirdparty/DBoW2/DUtils/Random.cpp:47-50"):
        assert phrase in doc, phrase


def test_record_sizes_and_offsets(orb):
    for S, dt, size in ((Corr, orb.SIM3_CORR_DTYPE, 56), (State, orb.SIM3_STATE_DTYPE, 184),
                        (Result, orb.SIM3_RESULT_DTYPE, 132)):
        assert ctypes.sizeof(S) == size == dt.itemsize
        assert [f[0] for f in S._fields_] == list(dt.names)
        for f in S._fields_:
            assert getattr(S, f[0]).offset == dt.fields[f[0]][1], f[0]
            assert getattr(S, f[0]).size == dt.fields[f[0]][0].itemsize, f[0]
    import sim3_ref as R
    assert R.CORR_DTYPE == orb.SIM3_CORR_DTYPE and R.STATE_DTYPE == orb.SIM3_STATE_DTYPE
    assert R.RESULT_DTYPE == orb.SIM3_RESULT_DTYPE
    assert Corr.max_err1.offset == 44 and Corr.best_inlier.offset == 52
    assert State.best_scale.offset == 36 and State.best_T12.offset == 88 and State.k1.offset == 152


def test_library_exports_and_wrapper_binds_them(orb):
    L = orb.lib()
    assert L.orb_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", str(orb.LIB_PATH)], check=True,
                         capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW:
        assert name in syms and getattr(L, name).argtypes is not None, name
    blob = orb.LIB_PATH.read_bytes()
    for kernel in (b"k_sim3_setup", b"k_sim3_iterate"):
        assert kernel in blob, kernel
    assert b"k_bow_batch" in blob and b"k_local_map" in blob      # the other batches stay
    for meth in ("sim3_solver_setup_batch", "sim3_solver_iterate_batch", "sim3_solver_max_stride"):
        assert callable(getattr(orb.ORBmatcher, meth)), meth
    for meth in ("iterate", "find", "GetEstimatedRotation", "GetEstimatedTranslation",
                 "GetEstimatedScale"):
        assert callable(getattr(orb.Sim3Solver, meth)), meth


def test_capacity_is_the_documented_lds_formula(orb):
    cap = orb.sim3_solver_max_stride()      # host-checkable, no device needed
    assert cap == orb.ORBmatcher.sim3_solver_max_stride()
    import sim3_cases as C
    S64 = lambda s: (s + 63) // 64 * 64
    lds = lambda s: 48 * S64(s) + (C.CHUNK + 1) * S64(s) // 8 + 8192
    assert lds(cap) <= 160 * 1024 < lds(cap + 1)
    assert cap >= 2048 and cap % 64 == 0


def test_argument_errors_without_a_device(orb):
    L = orb.lib()
    sig = np.ones(8, np.float32)
    cam = orb._Camera(500, 500, 320, 240, 0, 0)
    one = ctypes.c_void_p(8)  # never dereferenced: the handle is checked first
    st = L.orb_sim3_solver_setup_batch(None, 1, None, None, one, one, one, one, 64, one, one, None,
                                       one, sig.ctypes.data, 8, ctypes.byref(cam),
                                       ctypes.byref(cam), 0, 0.99, 20, 300, one, one, None)
    assert st == orb.ORB_EINVAL
    st = L.orb_sim3_solver_iterate_batch(None, 1, 64, one, one, one, 900, 2147483647, 300, 5, None,
                                         one, one, None)
    assert st == orb.ORB_EINVAL


def _pins(text):
    """The pin list P1..P16 of a document: comment stars and indentation dropped."""
    lines = [re.sub(r"^\s*\*?\s*", "", ln) for ln in text.splitlines()]
    a = next(i for i, ln in enumerate(lines) if ln.startswith("P1 "))
    b = next(i for i, ln in enumerate(lines) if ln.startswith("P16 "))
    return " ".join(" ".join(lines[a:b + 1]).split()).replace("*/", "").strip()


def test_pin_list_stands_identically_in_three_places():
    import sim3_ref
    ref = _pins(sim3_ref.__doc__)
    assert ref.startswith("P1 Rcw * X + tcw") and ref.endswith("(9.210 * (double)sigma2).")
    assert all(f"P{k} " in ref for k in range(1, 17))
    assert _pins(HEADER.read_text()) == ref
    design = (ROOT / "DESIGN.md").read_text()
    assert _pins(design[design.index("### 4.9"):]) == ref
