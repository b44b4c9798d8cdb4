"""The BoW batch entries are additive: include/orb_abi.h declares them, the
library exports them, the Python wrapper binds them, ORB_ABI_VERSION stays 1."""
import re
import subprocess

import numpy as np

from conftest import ROOT

HEADER = ROOT / "include" / "orb_abi.h"
NEW = ("orb_match_bow_batch", "orb_match_bow_batch_max_stride",
       "orb_track_discard_outliers_batch_n")


def test_header_declares_the_entries_and_keeps_the_version():
    text = HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"#define\s+ORB_ABI_VERSION\s+1\b", text)
    assert re.search(r"}\s*orb_bow_match_info_t;", code)
    fields = re.search(r"typedef struct orb_bow_match_info\s*{(.*?)}", code, re.S).group(1)
    assert re.findall(r"int32_t\s+(\w+);", fields) == ["n_matches", "n_accepted", "n_common_nodes",
                                                       "n_tried", "enough"]
    # the entry list at the top names both, with the reference lines
    head = text[:text.index("#ifndef ORB_ABI_H")]
    assert "orb_match_bow_batch" in head and "orb_track_discard_outliers_batch_n" in head
    for ref in ("src/ORBmatcher.cc:164-306", "src/Tracking.cc:904-954", ":1592-1616"):
        assert ref in head, ref
    # what the caller promises and what the call does not use is said
    doc = text[text.index("Device-batched SearchByBoW"):text.index("typedef struct orb_bow_match_info")]
    assert "NOT checked" in doc and "none of the handle's" in doc
    assert "8 * ((kp_stride + 3) & ~3) + 512" in doc


def test_library_exports_and_wrapper_binds_them(orb):
    L = orb.lib()
    assert L.orb_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", str(orb.LIB_PATH)], check=True,
                         capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW:
        assert name in syms and getattr(L, name).argtypes is not None, name
    blob = orb.LIB_PATH.read_bytes()
    assert b"k_bow_batch" in blob and b"k_track_discard" in blob
    assert b"k_bow_match" in blob and b"k_bow_finish" in blob     # the one-problem kernels stay
    assert callable(orb.ORBmatcher.search_by_bow_batch)
    assert callable(orb.ORBmatcher.track_discard_outliers_batch_n)
    assert orb.BOW_MATCH_INFO_DTYPE.itemsize == 20
    assert orb.BOW_MATCH_INFO_DTYPE.names == ("n_matches", "n_accepted", "n_common_nodes",
                                              "n_tried", "enough")
    assert np.dtype(orb.BOW_MATCH_INFO_DTYPE).fields["enough"][1] == 16


def test_capacity_is_the_documented_lds_formula(orb):
    cap = orb.match_bow_batch_max_stride()      # host-checkable, no device needed
    assert cap == orb.ORBmatcher.search_by_bow_batch_max_stride()
    assert 8192 <= cap                          # every stride transform_batch accepts
    # 8 bytes per keypoint slot, 512 bytes static, within 160 KiB
    lds = lambda s: 8 * ((s + 3) // 4 * 4)
    assert lds(cap) + 512 <= 160 * 1024 < lds(cap + 1) + 512
