"""The pose-optimisation entry points of the C ABI: declared in
include/orb_abi.h and exported by the built library (CPU test)."""
import ctypes
import re

from conftest import PKG_DIR, ROOT

SYMBOLS = ("orb_pose_optimization", "orb_pose_optimization_batch",
           "orb_pose_optimization_lds_edges")


def test_header_declares_pose_optimization():
    text = (ROOT / "include" / "orb_abi.h").read_text()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
    m = re.search(r"typedef struct orb_pose_opt_info \{([^}]*)\} orb_pose_opt_info_t;", text)
    assert m, "orb_pose_opt_info_t"
    fields = re.findall(r"\b(n_inliers|n_edges|lm_iterations|rejected_trials)\b", m.group(1))
    assert fields == ["n_inliers", "n_edges", "lm_iterations", "rejected_trials"]
    assert re.search(r"#define ORB_ABI_VERSION 1\b", text)   # additive: the version stays


def test_library_exports_pose_optimization(orb):
    orb.lib()
    L = ctypes.CDLL(str(PKG_DIR / "lib" / "liborb_amd.so"))
    for s in SYMBOLS:
        assert hasattr(L, s), s
    L.orb_pose_optimization_lds_edges.restype = ctypes.c_int
    n = L.orb_pose_optimization_lds_edges()
    assert n >= 1000 and n == orb.ORBmatcher.pose_optimization_lds_edges()
    assert orb.POSE_OPT_INFO_DTYPE.itemsize == 16


def test_pose_optimization_rejects_bad_arguments(orb):
    """Argument checks come before any device work."""
    L = orb.lib()
    bad = orb.ORB_EINVAL
    assert L.orb_pose_optimization(None, 0, None, None, None, None, 12, None, 8, None, None, None,
                                   None, None) == bad
    assert L.orb_pose_optimization_batch(None, 1, None, None, None, 8, None, None, 12, 0, None, 8,
                                         None, None, None, None, None, None) == bad
