"""Constants the reference embeds -- its only built-in known answers:
the rBRIEF sampling table, umax, per-level quotas, scale tables, Appendix B
level sizes, matcher thresholds.  Checked against what was recorded from the
reference source text (tests/golden/reference_facts.json, written by
tests/golden/make_reference_facts.py; where the reference tree is present the
record is first checked against it), and against the survey's derived values."""
import hashlib
import json
import re

import numpy as np
import pytest

from conftest import PKG_DIR, REFERENCE, reference_present
from orient_desc_ref import pattern_header as _pattern_header

SRC = REFERENCE / "src" / "ORBextractor.cc"
FACTS = json.loads((PKG_DIR.parent / "tests" / "golden" / "reference_facts.json").read_text())
# constants the reference states in its source text: file -> {name: value}
STATED = {"src/ORBmatcher.cc": {"TH_HIGH": 100, "TH_LOW": 50, "HISTO_LENGTH": 30},
          "include/Frame.h": {"FRAME_GRID_ROWS": 48, "FRAME_GRID_COLS": 64},
          "src/ORBextractor.cc": {"EDGE_THRESHOLD": 19, "HALF_PATCH_SIZE": 15, "PATCH_SIZE": 31}}


def pattern_digest(values):
    return hashlib.sha256(" ".join(str(v) for v in values).encode()).hexdigest()


def reference_pattern():
    text = SRC.read_text(encoding="utf-8", errors="replace")
    body = text.split("bit_pattern_31_[256*4] =", 1)[1].split("};", 1)[0]
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    return [int(v) for v in re.findall(r"-?\d+", body)]


def reference_constants():
    """{file: {name: value}} of STATED's names as the reference tree states them."""
    out = {}
    for rel, names in STATED.items():
        text = (REFERENCE / rel).read_text(encoding="utf-8", errors="replace")
        out[rel] = {}
        for n in names:
            m = re.search(r"\b" + n + r"\s*=?\s*(\d+)\b", text)
            out[rel][n] = int(m.group(1)) if m else None
    return out


def test_pattern_table_is_the_reference_table():
    if reference_present("src", "ORBextractor.cc"):
        ref = reference_pattern()
        assert len(ref) == 1024 and pattern_digest(ref) == FACTS["bit_pattern_31_sha256"]
    mine = _pattern_header()
    assert len(mine) == 1024 and pattern_digest(mine) == FACTS["bit_pattern_31_sha256"]


def test_pattern_table_shape():
    p = np.array(_pattern_header()).reshape(512, 2)
    assert p.min() >= -13 and p.max() <= 12 and len(p) == 512
    assert np.sqrt((p.astype(float) ** 2).sum(1)).max() < 18.5  # samples stay within +-18 px


def test_umax(oracle):
    assert oracle.params()["umax"].tolist() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    # 749-pixel circular patch used by IC_Angle
    um = oracle.params()["umax"]
    assert 31 + 2 * sum(2 * int(um[v]) + 1 for v in range(1, 16)) == 749


@pytest.mark.parametrize("nf,quota", [
    (1000, [217, 181, 151, 126, 105, 87, 73, 60]),
    (2000, [434, 362, 302, 251, 209, 175, 145, 122]),
    (4000, [869, 724, 603, 503, 419, 349, 291, 242]),
])
def test_quotas(oracle, nf, quota):
    assert oracle.params(nf)["quota"].tolist() == quota


def test_scale_tables(oracle):
    p = oracle.params()
    sf = np.float64(np.float32(1.2))  # `double scaleFactor` member, include/ORBextractor.h:98
    s = [np.float32(1.0)]
    for _ in range(7):
        s.append(np.float32(np.float64(s[-1]) * sf))
    assert p["scale"].tolist() == [float(v) for v in s]
    assert p["inv_scale"].tolist() == [float(np.float32(1) / v) for v in s]
    assert p["sigma2"].tolist() == [float(v * v) for v in s]
    assert [int(31 * v) for v in p["scale"]] == [31, 37, 44, 53, 64, 77, 92, 111]


@pytest.mark.parametrize("w,h,sizes", [
    (640, 480, [(640, 480), (533, 400), (444, 333), (370, 278), (309, 231), (257, 193), (214, 161), (179, 134)]),
    (1241, 376, [(1241, 376), (1034, 313), (862, 261), (718, 218), (598, 181), (499, 151), (416, 126), (346, 105)]),
    (1920, 1080, [(1920, 1080), (1600, 900), (1333, 750), (1111, 625), (926, 521), (772, 434), (643, 362), (536, 301)]),
])
def test_level_sizes(oracle, w, h, sizes):
    assert oracle.level_sizes(w, h) == sizes


def test_matcher_thresholds_in_reference():
    if reference_present("src", "ORBextractor.cc"):
        assert reference_constants() == FACTS["constants"]
    assert FACTS["constants"] == STATED
    abi = (PKG_DIR.parent / "include" / "orb_abi.h").read_text()
    assert re.search(r"#define ORB_GRID_ROWS 48\b", abi) and re.search(r"#define ORB_GRID_COLS 64\b", abi)
