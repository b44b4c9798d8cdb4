"""The attribution patches (tools/attribution/*.patch) are diffs against the
product's csrc/: each must apply to the source as it stands, with no fuzz and
no failed hunk, or the variant it restores is lost without anyone noticing."""
import glob
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam2-chinese-annotation_amd", "csrc")


def test_attribution_patches_apply_cleanly(tmp_path):
    patches = sorted(glob.glob(os.path.join(ROOT, "tools", "attribution", "*.patch")))
    assert patches, "no patch under tools/attribution/"
    # tools/attribution/build.sh applies them the same way: -p1 from the
    # directory that holds csrc/ (a dry run leaves the copy as it is)
    shutil.copytree(CSRC, tmp_path / "csrc")
    bad = {}
    for patch in patches:
        with open(patch, "rb") as f:
            r = subprocess.run(["patch", "-p1", "--dry-run"], cwd=tmp_path, stdin=f,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0 or "FAILED" in r.stdout or "fuzz" in r.stdout:
            bad[os.path.basename(patch)] = r.stdout
    assert not bad, "\n".join(f"{name}:\n{out}" for name, out in bad.items())
