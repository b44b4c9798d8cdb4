"""The weight-pair bound of the pyramid resize tables (CPU, no GPU): the tiled
k_pyr_resize kernels take the result byte as the top byte of four times the
vertical sum, which holds while every table entry's two weights sum to at most
2049 (csrc/orb_resize_tables.h).  tests/cpp/test_resize_tables_host.cpp builds
the planner's tables for the sizes and scale factors of
test_gpu_pyramid_taps.py, and for 1241x376 and 1920x1080 at 1.2 with 8 levels,
and asserts the bound on every entry."""
import subprocess

from conftest import PKG_DIR, ROOT

SRC = ROOT / "tests" / "cpp" / "test_resize_tables_host.cpp"
PLANS = [(157, 107, 1.1, 4), (311, 105, 1.1, 4), (157, 113, 1.2, 4), (311, 109, 1.2, 4),
         (161, 101, 1.25, 4), (251, 99, 1.25, 4), (161, 97, 1.1, 4), (161, 97, 1.2, 4),
         (161, 97, 1.25, 4), (263, 131, 1.1, 4), (263, 131, 1.2, 4), (263, 131, 1.25, 4),
         (1241, 376, 1.2, 8), (1920, 1080, 1.2, 8)]


def test_resize_weight_pairs_bounded(tmp_path):
    exe = tmp_path / "test_resize_tables_host"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{PKG_DIR / 'csrc'}", str(SRC),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    args = [str(v) for p in PLANS for v in p]
    run = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.startswith("OK"), run.stdout + run.stderr
    assert run.stdout.split()[1] == str(sum(p[3] - 1 for p in PLANS)), run.stdout


def test_gpu_test_sizes_are_covered():
    """Every (size, scale factor) of the GPU tap test is among the plans above."""
    import test_gpu_pyramid_taps as T
    want = {(w, h, sf, T.NLEVELS) for sf, sizes in T.SIZES.items() for w, h in sizes}
    assert want <= set(PLANS)
