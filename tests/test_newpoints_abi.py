"""The CreateNewMapPoints entries are additive: include/orb_abi.h declares them,
their record and the status codes, the library exports them, the Python wrapper
binds them with the same layout, ORB_ABI_VERSION stays 1, the capacities are the
documented LDS formulas, argument errors come back before any launch, and the
pin list stands identically in its three places."""
import ctypes
import re
import subprocess

import numpy as np

from conftest import ROOT

HEADER = ROOT / "include" / "orb_abi.h"
NEW = ("orb_scene_median_depth_batch", "orb_scene_median_depth",
       "orb_scene_median_depth_max_stride", "orb_create_new_map_points_batch",
       "orb_create_new_map_points", "orb_create_new_map_points_max_stride")
i32 = ctypes.c_int32


class Info(ctypes.Structure):
    _fields_ = [("gated", i32), ("overflow", i32), ("n_new", i32), ("first_point", i32),
                ("counts", i32 * 12)]


def test_header_declares_the_entries_and_keeps_the_version():
    import newpoints_ref as R
    text = HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"#define\s+ORB_ABI_VERSION\s+1\b", text)
    body = re.search(r"typedef struct orb_new_point_info\s*{(.*?)}\s*orb_new_point_info_t;", code,
                     re.S).group(1)
    names = [re.match(r"\s*\w+\s+(\w+)", d).group(1) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in Info._fields_]
    codes = dict(re.findall(r"#define\s+ORB_NP_(\w+)\s+(\d+)", text))
    assert int(codes.pop("NSTATUS")) == R.NSTATUS == len(codes)
    assert {k.lower(): int(v) for k, v in codes.items()} == \
        {n: k for k, n in enumerate(R.STATUS_NAMES)}
    head = text[:text.index("#ifndef ORB_ABI_H")]
    for ref in ("orb_scene_median_depth(_batch)", "orb_create_new_map_points(_batch)",
                "src/KeyFrame.cc:658-694", "src/LocalMapping.cc:289-311", ":338-535",
                "src/MapPoint.cc:349-402"):
        assert ref in head, ref
    doc = text[text.index("LocalMapping::CreateNewMapPoints on the device"):
               text.index("DBoW2 vocabulary */")]
    doc = " ".join(re.sub(r"\n\s*\*", " ", doc).split())
    for phrase in ("NOT checked", "ORB_ECAPACITY", "unpinned against a real OpenCV",
                   "share no cursor and no keyframe slot", "does not depend on the "
                   "std::map<KeyFrame*> order", "the current keyframe's mbf (:480)",
                   "`else if` of :372", "overflow = 1", "rejected alternative"):
        assert phrase in doc, phrase


def test_record_size_and_offsets(orb):
    import newpoints_ref as R
    dt = orb.NEW_POINT_INFO_DTYPE
    assert ctypes.sizeof(Info) == 64 == dt.itemsize and dt == R.NEW_POINT_INFO_DTYPE
    assert [f[0] for f in Info._fields_] == list(dt.names)
    for f in Info._fields_:
        assert getattr(Info, f[0]).offset == dt.fields[f[0]][1], f[0]
    assert Info.counts.offset == 16
    assert R.MAP_POINT_DTYPE == orb.MAP_POINT_DTYPE and R.POSE_DTYPE == orb.POSE_DTYPE
    assert R.KEYPOINT_DTYPE == orb.KEYPOINT_DTYPE
    assert (orb.NP_NOT_TRIED, orb.NP_ACCEPTED, orb.NP_UNDEFINED) == (R.NOT_TRIED, R.ACCEPTED,
                                                                      R.UNDEFINED)


def test_library_exports_and_wrapper_binds_them(orb):
    L = orb.lib()
    assert L.orb_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", str(orb.LIB_PATH)], check=True,
                         capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW:
        assert name in syms and getattr(L, name).argtypes is not None, name
    blob = orb.LIB_PATH.read_bytes()
    for kernel in (b"k_median_depth", b"k_new_points"):
        assert kernel in blob, kernel
    assert b"k_sim3_iterate" in blob and b"k_local_map" in blob      # the other batches stay
    for meth in ("scene_median_depth_batch", "create_new_map_points_batch",
                 "ComputeSceneMedianDepth", "CreateNewMapPoints",
                 "create_new_map_points_max_stride", "scene_median_depth_max_stride"):
        assert callable(getattr(orb.ORBmatcher, meth)), meth


def test_capacities_are_the_documented_lds_formulas(orb):
    a = orb.ORBmatcher.create_new_map_points_max_stride()   # host-checkable, no device needed
    b = orb.ORBmatcher.scene_median_depth_max_stride()
    lds = 160 * 1024 - 1024
    assert a == lds // 16 // 64 * 64 and b == lds // 4 // 64 * 64
    assert a >= 8192 and b >= 32768


def _create_args(orb, **kw):
    sf = np.array([1.2 ** k for k in range(8)], np.float32)
    cam = orb._Camera(500, 500, 320, 240, 40, 0.08)
    one = ctypes.c_void_p(8)  # never dereferenced: every check precedes the launch
    a = dict(m=one, n=1, s1=one, s2=one, keys=one, nkeys=one, pidx=one, pose=one, ur=one, dp=one,
             stride=64, m12=one, med=one, c1=ctypes.byref(cam), c2=ctypes.byref(cam),
             sf=sf.ctypes.data, sig=sf.ctypes.data, nl=8, mono=0, pts=one, cap=10, cur=one,
             cidx=one, st=one, x3d=one, pairs=one, info=one, stream=None)
    a.update(kw)
    a["_keep"] = (sf, cam)
    return a


def _create(orb, **kw):
    a = _create_args(orb, **kw)
    return orb.lib().orb_create_new_map_points_batch(
        a["m"], a["n"], a["s1"], a["s2"], a["keys"], a["nkeys"], a["pidx"], a["pose"], a["ur"],
        a["dp"], a["stride"], a["m12"], a["med"], a["c1"], a["c2"], a["sf"], a["sig"], a["nl"],
        a["mono"], a["pts"], a["cap"], a["cur"], a["cidx"], a["st"], a["x3d"], a["pairs"],
        a["info"], a["stream"])


def test_argument_errors_before_any_launch(orb):
    """Every rejected call returns before the handle or any pointer is used: the
    handle here is not a handle and the pointers point nowhere."""
    E, CAP = orb.ORB_EINVAL, orb.ORB_ECAPACITY
    assert _create(orb, m=None) == E
    assert _create(orb, n=-1) == E and _create(orb, stride=0) == E and _create(orb, cap=-1) == E
    assert _create(orb, nl=1) == E and _create(orb, nl=17) == E
    assert _create(orb, c1=None) == E and _create(orb, sf=None) == E and _create(orb, sig=None) == E
    bad = np.array([1, 0, 1, 1, 1, 1, 1, 1], np.float32)
    assert _create(orb, sf=bad.ctypes.data) == E
    bad[1] = np.nan
    assert _create(orb, sig=bad.ctypes.data) == E
    assert _create(orb, ur=None) == E and _create(orb, dp=None) == E   # both or neither
    big = orb.ORBmatcher.create_new_map_points_max_stride() + 1
    assert _create(orb, stride=big) == CAP
    assert _create(orb, n=0) == orb.ORB_OK                 # nothing to do, nothing launched
    assert _create(orb, n=0, ur=None, dp=None, keys=None, info=None) == orb.ORB_OK
    for name in ("s1", "s2", "keys", "nkeys", "pidx", "pose", "m12", "pts", "cur", "cidx", "st",
                 "x3d", "pairs", "info"):
        assert _create(orb, **{name: None}) == E, name
    assert _create(orb, mono=1, med=None, ur=None, dp=None) == E   # the median is read when monocular

    L = orb.lib()
    one = ctypes.c_void_p(8)
    call = lambda **kw: L.orb_scene_median_depth_batch(*[
        {**dict(m=one, n=1, slot=None, nkeys=one, pidx=one, pose=one, stride=64, pts=one, q=2,
                med=one, cnt=one, stream=None), **kw}[k]
        for k in ("m", "n", "slot", "nkeys", "pidx", "pose", "stride", "pts", "q", "med", "cnt",
                  "stream")])
    assert call(m=None) == E and call(n=-1) == E and call(stride=0) == E and call(q=0) == E
    assert call(stride=orb.ORBmatcher.scene_median_depth_max_stride() + 1) == CAP
    assert call(n=0) == orb.ORB_OK
    for name in ("nkeys", "pidx", "pose", "pts", "med", "cnt"):
        assert call(**{name: None}) == E, name
    # the one-problem forms check before they touch the handle as well
    z = np.zeros(1, np.float32)
    assert L.orb_scene_median_depth(None, 0, None, one, None, 0, 2, z.ctypes.data,
                                    z.ctypes.data) == E
    assert L.orb_scene_median_depth(one, 1, None, one, None, 0, 2, z.ctypes.data,
                                    z.ctypes.data) == E
    idx = np.array([3], np.int32)
    assert L.orb_scene_median_depth(one, 1, idx.ctypes.data, one, one, 3, 2, z.ctypes.data,
                                    z.ctypes.data) == E      # an index at n_points


def _pins(text):
    """The pin list N1..N10 of a document: comment stars and indentation dropped."""
    lines = [re.sub(r"^\s*\*?\s*", "", ln) for ln in text.splitlines()]
    a = next(i for i, ln in enumerate(lines) if ln.startswith("N1 "))
    b = next(i for i, ln in enumerate(lines) if ln.startswith("N10 "))
    end = next(i for i in range(b + 1, len(lines))
               if not lines[i] or lines[i].startswith(("libm=True", "orb_status_t", "```", "*/")))
    return " ".join(" ".join(lines[a:end]).split()).replace("*/", "").strip()


def test_pin_list_stands_identically_in_three_places():
    import newpoints_ref
    ref = _pins(newpoints_ref.__doc__)
    assert ref.startswith("N1 Mat::dot of two 3-vectors") and ref.endswith("sf[n_levels - 1]: float.")
    assert all(f"N{k} " in ref for k in range(1, 11))
    assert _pins(HEADER.read_text()) == ref
    design = (ROOT / "DESIGN.md").read_text()
    assert _pins(design[design.index("### 4.10"):]) == ref
