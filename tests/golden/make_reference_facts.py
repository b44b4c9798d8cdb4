"""Writes tests/golden/reference_facts.json from a reference tree (ORB_REFERENCE):
the digest of the rBRIEF sampling table, the constants the tests name, and
digests of the normalised member declarations of the classes the integration
stubs mirror.  Recorded results only; no reference text is stored."""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import test_integration_compile as tic  # noqa: E402
import test_oracle_constants as toc  # noqa: E402

CLASSES = [("ORBmatcher", "ORBmatcher.h"), ("ORBextractor", "ORBextractor.h"), ("Frame", "Frame.h"),
           ("KeyFrame", "KeyFrame.h"), ("MapPoint", "MapPoint.h")]
facts = {"bit_pattern_31_sha256": toc.pattern_digest(toc.reference_pattern()),
         "constants": toc.reference_constants(),
         "declarations": {n: sorted(tic._digest(d) for d in tic._ref_decls(h, n)) for n, h in CLASSES}}
(HERE / "reference_facts.json").write_text(json.dumps(facts, indent=1) + "\n")
