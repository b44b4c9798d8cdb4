"""The two ComputeSim3 matcher batches are additive: include/orb_abi.h declares
them, the library exports them, the Python wrapper binds them, ORB_ABI_VERSION
stays 1, the capacity functions are the documented LDS formulas and the
one-problem kernels stay in the binary."""
import re
import subprocess

import numpy as np

from conftest import ROOT

HEADER = ROOT / "include" / "orb_abi.h"
NEW = ("orb_match_bow_kf_batch", "orb_match_bow_kf_batch_max_stride", "orb_search_by_sim3_batch",
       "orb_search_by_sim3_batch_max_stride")
FIELDS = ("n_found", "n_kept", "n_total", "n_best12", "n_best21")


def test_header_declares_the_entries_and_keeps_the_version():
    text = HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW + ("orb_match_bow_kf", "orb_search_by_sim3"):
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"#define\s+ORB_ABI_VERSION\s+1\b", text)
    fields = re.search(r"typedef struct orb_sim3_search_info\s*{(.*?)}", code, re.S).group(1)
    assert tuple(re.findall(r"int32_t\s+(\w+);", fields)) == FIELDS
    doc = text[text.index("LoopClosing::ComputeSim3's two matchers as device batches"):
               text.index("typedef struct orb_sim3_search_info")]
    doc = " ".join(re.sub(r"\n\s*\*", " ", doc).split())
    for phrase in ("src/ORBmatcher.cc: 581-716", "src/ORBmatcher.cc:1212-1458",
                   "src/LoopClosing.cc:338-343", "none of the handle's scratch",
                   "ORB_ECAPACITY before anything is launched",
                   "8 * ((kp_stride + 3) & ~3) + 512",
                   "24,608 + 16 * ((kp_stride + 3) & ~3) + 1,024", "n_matches = -1",
                   "nothing of it is read or written", "NOT checked", "bestDist1 < 50"):
        assert phrase in doc, phrase


def test_library_exports_and_wrapper_binds_them(orb):
    L = orb.lib()
    assert L.orb_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", str(orb.LIB_PATH)], check=True,
                         capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW + ("orb_match_bow_kf", "orb_search_by_sim3"):
        assert name in syms and getattr(L, name).argtypes is not None, name
    assert len(L.orb_match_bow_kf_batch.argtypes) == 21
    assert len(L.orb_search_by_sim3_batch.argtypes) == 29
    blob = orb.LIB_PATH.read_bytes()
    assert b"k_bow_kf_batch" in blob and b"k_sim3_search_batch" in blob
    # the one-problem kernels stay
    assert b"k_pp_match" in blob and b"k_sim3_mutual" in blob and b"k_grid_build" in blob
    for name in ("search_by_bow_kf_batch", "search_by_sim3_batch", "SearchByBoWKF", "SearchBySim3"):
        assert callable(getattr(orb.ORBmatcher, name)), name
    dt = np.dtype(orb.SIM3_SEARCH_INFO_DTYPE)
    assert dt.itemsize == 20 and dt.names == FIELDS
    assert [dt.fields[f][1] for f in FIELDS] == [0, 4, 8, 12, 16]


def test_capacities_are_the_documented_lds_formulas(orb):
    lds_cu = 160 * 1024
    up4 = lambda s: (s + 3) // 4 * 4
    cap = orb.match_bow_kf_batch_max_stride()      # host-checkable, no device needed
    assert cap == orb.ORBmatcher.search_by_bow_kf_batch_max_stride()
    assert 8 * up4(cap) + 512 <= lds_cu < 8 * up4(cap + 1) + 512
    cap = orb.search_by_sim3_batch_max_stride()
    assert cap == orb.ORBmatcher.search_by_sim3_batch_max_stride()
    lds = lambda s: 2 * 4 * (64 * 48 + 4) + 16 * up4(s) + 1024
    assert 2 * 4 * (64 * 48 + 4) == 24608
    assert lds(cap) <= lds_cu < lds(cap + 1)
    # the optimiser stays the chain's binding limit
    assert cap >= orb.optimize_sim3_max_stride() == 2217
    assert orb.match_bow_kf_batch_max_stride() >= orb.optimize_sim3_max_stride()


def test_refused_on_the_host_without_a_device_call(orb):
    """The argument checks come before anything touches the device."""
    L = orb.lib()
    z = [None] * 21
    assert L.orb_match_bow_kf_batch(None, 0, *z[2:12], 64, None, 0.75, 1, 20,
                                    *z[17:]) == orb.ORB_EINVAL            # no handle
    z = [None] * 29
    assert L.orb_search_by_sim3_batch(None, 0, *z[2:9], 64, *z[10:18], 0.0, 640.0, 0.0, 480.0, 8,
                                      None, 0.18, 7.5, None, None, None) == orb.ORB_EINVAL
    # The capacity and null-pointer checks come before the handle is used: a
    # block of zero bytes stands in for it (it is never dereferenced here).
    import ctypes
    fake = ctypes.create_string_buffer(4096)
    h = ctypes.cast(fake, ctypes.c_void_p)
    cam = (ctypes.c_float * 6)(500, 500, 320, 240, 0, 0)
    sf = (ctypes.c_float * 8)(*([1.0] * 8))
    big = orb.match_bow_kf_batch_max_stride() + 1
    bow = lambda n, stride: L.orb_match_bow_kf_batch(h, n, *[None] * 10, stride, None, 0.75, 1, 20,
                                                     None, None, None, None)
    assert bow(1, big) == orb.ORB_ECAPACITY and bow(0, big) == orb.ORB_ECAPACITY
    assert bow(1, 64) == orb.ORB_EINVAL and bow(-1, 64) == orb.ORB_EINVAL
    assert bow(1, 0) == orb.ORB_EINVAL and bow(0, 64) == orb.ORB_OK
    big = orb.search_by_sim3_batch_max_stride() + 1
    s3 = lambda n, stride, levels=8, max_x=640.0: L.orb_search_by_sim3_batch(
        h, n, *[None] * 7, stride, *[None] * 7, cam, 0.0, max_x, 0.0, 480.0, levels, sf, 0.18, 7.5,
        None, None, None)
    assert s3(1, big) == orb.ORB_ECAPACITY and s3(0, big) == orb.ORB_ECAPACITY
    assert s3(1, 64) == orb.ORB_EINVAL and s3(-1, 64) == orb.ORB_EINVAL
    assert s3(0, 0) == orb.ORB_EINVAL and s3(0, 64, levels=0) == orb.ORB_EINVAL
    assert s3(0, 64, levels=17) == orb.ORB_EINVAL and s3(0, 64, max_x=0.0) == orb.ORB_EINVAL
    assert s3(0, 64) == orb.ORB_OK
