"""The SearchForTriangulation batch entries are additive: include/orb_abi.h
declares them, the library exports them, the Python wrapper binds them,
ORB_ABI_VERSION stays 1 and the one-problem kernels stay in the binary."""
import re
import subprocess

import numpy as np

from conftest import ROOT

HEADER = ROOT / "include" / "orb_abi.h"
NEW = ("orb_search_for_triangulation_batch", "orb_search_for_triangulation_batch_max_stride")
FIELDS = ("n_matches", "n_accepted", "n_common_nodes", "n_tried", "n_shared2", "n_undefined")


def test_header_declares_the_entries_and_keeps_the_version():
    text = HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"\borb_search_for_triangulation\s*\(", code)      # the one-problem entry
    assert re.search(r"#define\s+ORB_ABI_VERSION\s+1\b", text)
    assert re.search(r"}\s*orb_tri_match_info_t;", code)
    fields = re.search(r"typedef struct orb_tri_match_info\s*{(.*?)}", code, re.S).group(1)
    assert tuple(re.findall(r"int32_t\s+(\w+);", fields)) == FIELDS
    head = text[:text.index("#ifndef ORB_ABI_H")]
    assert "orb_search_for_triangulation_batch" in head
    for ref in ("src/ORBmatcher.cc:718-901", "src/LocalMapping.cc:313-318"):
        assert ref in head, ref
    doc = text[text.index("Device-batched SearchForTriangulation"):
               text.index("typedef struct orb_tri_match_info")]
    doc = " ".join(re.sub(r"\n\s*\*", " ", doc).split())
    for phrase in ("NOT checked", "none of the handle's", "8 * ((kp_stride + 3) & ~3) + 1024",
                   "ORB_ECAPACITY before anything is launched", "invz = 1.0f / C2z",
                   "n_matches = -1", "n_undefined"):
        assert phrase in doc, phrase
    # the new-points entry no longer promises what the matcher does not keep
    np_doc = text[text.index("The neighbour loop's gate (src/LocalMapping.cc:289-311)"):
                  text.index("orb_status_t orb_create_new_map_points_batch(")]
    np_doc = " ".join(re.sub(r"\n\s*\*", " ", np_doc).split())
    assert "at most once" not in np_doc
    assert "An index of KF2 may repeat" in np_doc and "largest accepted i1" in np_doc


def test_library_exports_and_wrapper_binds_them(orb):
    L = orb.lib()
    assert L.orb_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", str(orb.LIB_PATH)], check=True,
                         capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW + ("orb_search_for_triangulation",):
        assert name in syms and getattr(L, name).argtypes is not None, name
    assert len(L.orb_search_for_triangulation_batch.argtypes) == 25
    blob = orb.LIB_PATH.read_bytes()
    assert b"k_tri_batch" in blob
    assert b"k_tri_match" in blob and b"k_tri_finish" in blob     # the one-problem kernels stay
    assert callable(orb.ORBmatcher.search_for_triangulation_batch)
    assert callable(orb.ORBmatcher.SearchForTriangulation)
    dt = np.dtype(orb.TRI_MATCH_INFO_DTYPE)
    assert dt.itemsize == 24 and dt.names == FIELDS
    assert [dt.fields[f][1] for f in FIELDS] == [0, 4, 8, 12, 16, 20]


def test_capacity_is_the_documented_lds_formula(orb):
    cap = orb.search_for_triangulation_batch_max_stride()   # host-checkable, no device needed
    assert cap == orb.ORBmatcher.search_for_triangulation_batch_max_stride()
    assert cap >= orb.ORBmatcher.create_new_map_points_max_stride() == 10176
    # 8 bytes per keypoint slot, 1024 bytes static, within 160 KiB
    lds = lambda s: 8 * ((s + 3) // 4 * 4)
    assert lds(cap) + 1024 <= 160 * 1024 < lds(cap + 1) + 1024


def test_refused_on_the_host_without_a_device_call(orb):
    """The argument checks come before anything touches the device."""
    L = orb.lib()
    z = [None] * 25
    assert L.orb_search_for_triangulation_batch(*z[:1], 0, *z[2:14], 64, *z[15:19], 8, 0, 0,
                                                *z[22:]) == orb.ORB_EINVAL     # no handle
