"""The FAST cell class table of the planner (CPU, no GPU): k_fast_cells reads
per class what it used to derive per cell.  tests/cpp/test_cell_classes_host.cpp
builds the plans below with the planner's own grouping (csrc/orb_plan.h),
checks every cell's class entry against the old per-cell formulas (the float
reciprocal quotients included, over every lane, tile byte and window pixel),
and runs the quotient multipliers exhaustively over their argument ranges."""
import subprocess

from conftest import PKG_DIR, ROOT

SRC = ROOT / "tests" / "cpp" / "test_cell_classes_host.cpp"
SIZES = [(1241, 376), (752, 480), (640, 480), (1920, 1080)]  # the ORB-SLAM2 sequences
FACTORS = [1.1, 1.15, 1.2, 1.25]
# the sizes of test_gpu_fast_cell_classes.py as well, and one whose level 2 is a
# single cell too wide for k_fast_cells (its class must fail the host check)
PLANS = [(w, h, sf, 8) for w, h in SIZES for sf in FACTORS] + \
        [(200, 150, 1.2, 3), (321, 243, 1.2, 6), (219, 131, 1.2, 8), (526, 1012, 1.2, 2),
         (131, 97, 1.2, 4)]


def test_cell_classes_match_per_cell_formulas(tmp_path):
    exe = tmp_path / "test_cell_classes_host"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{PKG_DIR / 'csrc'}", str(SRC),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    args = [str(v) for p in PLANS for v in p]
    run = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("OK"), run.stdout + run.stderr
    ncells, nclasses = int(run.stdout.split()[1]), int(run.stdout.split()[3])
    # a handful of classes per level (interior, last column, last row, corner), many cells each
    assert 0 < nclasses <= 4 * sum(p[3] for p in PLANS) and ncells > 20 * nclasses, run.stdout
