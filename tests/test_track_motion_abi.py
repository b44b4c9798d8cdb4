"""The motion-model batch entries are additive: include/orb_abi.h declares them,
the library exports them, the Python wrapper binds them, ORB_ABI_VERSION stays 1."""
import re
import subprocess

import numpy as np

from conftest import ROOT

HEADER = ROOT / "include" / "orb_abi.h"
NEW = ("orb_match_projection_frame_batch", "orb_match_projection_frame_batch_max_stride",
       "orb_track_discard_outliers_batch")


def test_header_declares_the_entries_and_keeps_the_version():
    text = HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"#define\s+ORB_ABI_VERSION\s+1\b", text)
    for t in ("orb_frame_match_info_t", "orb_track_discard_info_t"):
        assert re.search(r"}\s*%s;" % t, code), t
    # the entry list at the top names both, with the pins
    head = text[:text.index("#ifndef ORB_ABI_H")]
    assert "orb_match_projection_frame_batch" in head and "orb_track_discard_outliers_batch" in head
    assert "src/Tracking.cc:1060-1083" in head and "invzc = 1.0f / z" in head


def test_library_exports_and_wrapper_binds_them(orb):
    L = orb.lib()
    assert L.orb_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", str(orb.LIB_PATH)], check=True,
                         capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW:
        assert name in syms and getattr(L, name).argtypes is not None, name
    assert b"k_frame_batch" in orb.LIB_PATH.read_bytes()
    assert b"k_track_discard" in orb.LIB_PATH.read_bytes()
    assert callable(orb.ORBmatcher.search_by_projection_frame_batch)
    assert callable(orb.ORBmatcher.track_discard_outliers_batch)
    # the records the C structs lay out
    assert orb.FRAME_MATCH_INFO_DTYPE.itemsize == 20 and orb.TRACK_DISCARD_INFO_DTYPE.itemsize == 12
    assert orb.FRAME_MATCH_INFO_DTYPE.names == ("n_matches", "n_matches_first_pass", "retried",
                                                "forward", "backward")
    cap = L.orb_match_projection_frame_batch_max_stride()   # host-checkable, no device needed
    assert 4096 <= cap < (1 << 14)
    # 32 bytes and one lock bit per keypoint slot, 512 bytes static, within 160 KiB
    lds = lambda s: 4 * (8 * ((s + 3) // 4 * 4) + (((s + 3) // 4 * 4 + 31) // 32 + 3) // 4 * 4)
    assert lds(cap) + 512 <= 160 * 1024 < lds(cap + 4) + 512
    assert np.dtype(orb.FRAME_MATCH_INFO_DTYPE).fields["backward"][1] == 16
