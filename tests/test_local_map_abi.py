"""The UpdateLocalMap entries are additive: include/orb_abi.h declares them and
their structs, the library exports them, the Python wrapper binds them,
ORB_ABI_VERSION stays 1, and the capacity is the documented LDS formula."""
import ctypes
import re
import subprocess

import numpy as np

from conftest import ROOT

HEADER = ROOT / "include" / "orb_abi.h"
NEW = ("orb_update_local_map_batch", "orb_update_local_map_max_keyframes",
       "orb_track_local_merge_batch", "orb_track_local_map_finish_batch")
INFO_FIELDS = ["n_local_kf", "n_voted", "n_added", "ref_kf", "max_votes", "n_local_points",
               "n_nulled", "kept"]
VIEW_POINTERS = ["kf_rank", "kf_by_rank", "kf_bad", "kf_parent", "kf_cov_offs", "kf_cov",
                 "kf_child_offs", "kf_child", "kf_mp_offs", "kf_mp", "mp_obs_offs", "mp_obs",
                 "points", "mp_desc"]


def test_header_declares_the_entries_and_keeps_the_version():
    text = HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"#define\s+ORB_ABI_VERSION\s+1\b", text)
    info = re.search(r"typedef struct orb_local_map_info\s*{(.*?)}\s*orb_local_map_info_t;", code,
                     re.S).group(1)
    assert re.findall(r"int32_t\s+(\w+);", info) == INFO_FIELDS
    view = re.search(r"typedef struct orb_map_view\s*{(.*?)}\s*orb_map_view_t;", code, re.S).group(1)
    assert re.findall(r"int32_t\s+n_kf,\s*n_mp;", view)
    assert re.findall(r"\*\s*(\w+);", view) == VIEW_POINTERS
    head = text[:text.index("#ifndef ORB_ABI_H")]
    for name in ("orb_update_local_map_batch", "orb_track_local_merge_batch",
                 "orb_track_local_map_finish_batch"):
        assert name in head, name
    for ref in ("src/Tracking.cc:1395-1404", ":1437-1558", ":1407-1434", ":1333-1354",
                "src/Tracking.cc:1109-1135"):
        assert ref in head, ref
    doc = text[text.index("UpdateLocalMap on the device"):text.index("orb_status_t orb_update_local_map_batch")]
    # what the caller promises, why the list is in/out, the formula, the call order
    assert "NOT checked" in doc and "stays exactly as on entry" in doc
    assert "98,304 + 9,280 + 12 K + K / 8 + 512 <= 163,840" in doc
    assert "call-order" in doc and "ORB_ECAPACITY" in doc


def test_library_exports_and_wrapper_binds_them(orb):
    L = orb.lib()
    assert L.orb_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", str(orb.LIB_PATH)], check=True,
                         capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW:
        assert name in syms and getattr(L, name).argtypes is not None, name
    blob = orb.LIB_PATH.read_bytes()
    for kernel in (b"k_local_map", b"k_track_local_merge", b"k_track_local_finish"):
        assert kernel in blob, kernel
    assert b"k_frame_batch" in blob and b"k_bow_batch" in blob      # the other batches stay
    for meth in ("update_local_map_batch", "track_local_merge_batch",
                 "track_local_map_finish_batch", "update_local_map_max_keyframes"):
        assert callable(getattr(orb.ORBmatcher, meth)), meth
    assert callable(orb.MapView)


def test_info_dtype_and_view_struct_layout(orb):
    dt = orb.LOCAL_MAP_INFO_DTYPE
    assert dt.itemsize == 32 and list(dt.names) == INFO_FIELDS
    assert [dt.fields[k][1] for k in INFO_FIELDS] == list(range(0, 32, 4))
    V = orb._MapView
    assert [f[0] for f in V._fields_] == ["n_kf", "n_mp"] + VIEW_POINTERS
    assert V.n_kf.offset == 0 and V.n_mp.offset == 4 and V.kf_rank.offset == 8
    assert ctypes.sizeof(V) == 8 + 8 * len(VIEW_POINTERS)
    import local_map_ref as R
    assert R.INFO_DTYPE == dt and R.MAP_POINT_DTYPE == orb.MAP_POINT_DTYPE


def test_capacity_is_the_documented_lds_formula(orb):
    cap = orb.update_local_map_max_keyframes()      # host-checkable, no device needed
    assert cap == orb.ORBmatcher.update_local_map_max_keyframes()
    K = lambda s: (s + 32) // 32 * 32
    lds = lambda s: 98304 + 9280 + 12 * K(s) + K(s) // 8 + 512
    assert lds(cap) <= 160 * 1024 < lds(cap + 1)
    assert cap >= 4096
    import local_map_cases as C
    assert C.HASH_CAP == 9216 and C.CHILD_STAGE == 16   # the tiers the directed inputs straddle
