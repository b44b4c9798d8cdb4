"""The OptimizeSim3 entries are additive: include/orb_abi.h declares them and
their record, the library exports them, the Python wrapper binds them with the
same layout, ORB_ABI_VERSION stays 1, the capacity is the documented LDS
formula, and the pin list stands identically in its three places."""
import ctypes
import re
import subprocess

import numpy as np

from conftest import ROOT

HEADER = ROOT / "include" / "orb_abi.h"
NEW = ("orb_optimize_sim3_batch", "orb_optimize_sim3", "orb_optimize_sim3_max_stride",
       "orb_pinned_exp_batch")
i32, f32, f64 = ctypes.c_int32, ctypes.c_float, ctypes.c_double


class Result(ctypes.Structure):
    _fields_ = [("status", i32), ("n_corr", i32), ("n_bad", i32), ("n_inliers", i32),
                ("q", f64 * 4), ("t", f64 * 3), ("s", f64), ("R", f32 * 9), ("t_f", f32 * 3),
                ("s_f", f32), ("_pad", i32)]


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
    assert _header_fields(code, "orb_sim3_opt_result") == [f[0] for f in Result._fields_]
    # appended: everything older stands before the new section
    sec = text.index("Optimizer::OptimizeSim3 on the device")
    for older in ("orb_sim3_solver_iterate_batch(", "orb_search_for_triangulation_batch(",
                  "orb_status_string("):
        assert text.index(older) < sec, older
    doc = " ".join(re.sub(r"\n\s*\*", " ", text[sec:]).split())
    for phrase in ("src/Optimizer.cc:1130-1326", "NOT-checked", "ORB_ECAPACITY", "has_sim3 == 0",
                   "no scratch tier", "base_binary_edge.hpp:131-200", "sim3.h:70-142",
                   "unpinned against their binaries", "does not synchronise"):
        assert phrase in doc, phrase


def test_record_size_and_offsets(orb):
    dt = orb.SIM3_OPT_RESULT_DTYPE
    assert ctypes.sizeof(Result) == 136 == dt.itemsize
    assert [f[0] for f in Result._fields_] == list(dt.names)
    for f in Result._fields_:
        assert getattr(Result, f[0]).offset == dt.fields[f[0]][1], f[0]
        assert getattr(Result, f[0]).size == dt.fields[f[0]][0].itemsize, f[0]
    import sim3opt_ref as R
    assert R.OPT_RESULT_DTYPE == dt
    assert Result.q.offset == 16 and Result.s.offset == 72 and Result.R.offset == 80
    assert Result.s_f.offset == 128


def test_library_exports_and_wrapper_binds_them(orb):
    L = orb.lib()
    assert L.orb_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", str(orb.LIB_PATH)], check=True,
                         capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW:
        assert name in syms and getattr(L, name).argtypes is not None, name
    blob = orb.LIB_PATH.read_bytes()
    assert b"k_optimize_sim3" in blob and b"k_pinned_exp" in blob
    assert b"k_pose_optimization" in blob and b"k_sim3_iterate" in blob  # the neighbours stay
    for meth in ("optimize_sim3_batch", "OptimizeSim3", "optimize_sim3_max_stride",
                 "pinned_exp_batch"):
        assert callable(getattr(orb.ORBmatcher, meth)), meth


def test_capacity_is_the_documented_lds_formula(orb):
    cap = orb.optimize_sim3_max_stride()  # host-checkable, no device needed
    assert cap == orb.ORBmatcher.optimize_sim3_max_stride()
    tile = (36 * 65 * 8 + 15) // 16 * 16              # one term tile: 36 rows of 64 + 1 doubles
    state = ((36 + 2 * 15 * 8) * 8 + 15) // 16 * 16   # the sums, 15 estimates and 15 inverses
    lds = lambda s: 2 * tile + state + 56 * s
    assert lds(cap) <= 160 * 1024 < lds(cap + 1)
    assert cap >= 2048


def test_argument_errors_without_a_device(orb):
    L = orb.lib()
    inv = np.ones(8, np.float32)
    cam = orb._Camera(500, 500, 320, 240, 0, 0)
    one = ctypes.c_void_p(8)  # never dereferenced: the handle is checked first
    st = L.orb_optimize_sim3_batch(None, 1, None, None, one, one, one, one, 64, one, one, one, one,
                                   None, inv.ctypes.data, 8, ctypes.byref(cam), ctypes.byref(cam),
                                   10.0, 0, one, None)
    assert st == orb.ORB_EINVAL
    st = L.orb_optimize_sim3(None, one, 1, one, one, one, 1, one, one, 1, one, one, one,
                             inv.ctypes.data, 8, ctypes.byref(cam), ctypes.byref(cam), 10.0, 0, one)
    assert st == orb.ORB_EINVAL
    assert L.orb_pinned_exp_batch(None, 1, one, one, None) == orb.ORB_EINVAL


def _pins(text):
    """The pin list O1..O9 of a document: comment stars and indentation dropped."""
    lines = [re.sub(r"^\s*\*?\s*", "", ln) for ln in text.splitlines()]
    a = next(i for i, ln in enumerate(lines) if ln.startswith("O1 "))
    b = next(i for i, ln in enumerate(lines) if ln.startswith("O9 "))
    end = next(i for i in range(b, len(lines)) if "sqrt and / are IEEE." in lines[i])
    return " ".join(" ".join(lines[a:end + 1]).split()).replace("*/", "").strip()


def test_pin_list_stands_identically_in_three_places():
    import sim3opt_ref
    ref = _pins(sim3opt_ref.__doc__)
    assert ref.startswith("O1 P3D1c, P3D2c = Rcw * X + tcw") and ref.endswith("sqrt and / are IEEE.")
    assert all(f"O{k} " in ref for k in range(1, 10))
    text = HEADER.read_text()
    assert _pins(text[text.index("Optimizer::OptimizeSim3 on the device"):]) == ref
    design = (ROOT / "DESIGN.md").read_text()
    assert _pins(design[design.index("### 4.12"):]) == ref
