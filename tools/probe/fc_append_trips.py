#!/usr/bin/env python3
"""Trip count of k_fast_cells' queue-append loop (needs the FC_TRIPS build:
PATCHES=append_trips.patch tools/attribution/build.sh trips -DFC_TRIPS, run with
ORB_AMD_LIB=.../trips.so).  A pretest round (64 lanes x 8 pixels) appends its
candidates with a per-lane serial loop; the wave runs it as many times as the
fullest lane has candidates.  Counted over the first 16 images of one B-frame
batch call at the bench shape: rounds, rounds that append, trips, lanes that
append, entries, and the histogram of trips per round."""
import ctypes
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))
from conftest import load_pkg  # noqa: E402


def main():
    import torch
    orb = load_pkg()
    W, H, B = 1241, 376, int(sys.argv[1]) if len(sys.argv) > 1 else 64
    imgs = np.stack([orb.synth_image(0x4B495454, f, W, H) for f in range(B)])
    ext = orb.ORBextractor(1000, 1.2, 8, 20, 7)
    cap = ext.capacity(W, H)
    d = torch.from_numpy(imgs).cuda()
    k = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    de = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    n = torch.zeros(B, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    L = orb.lib()
    L.orb_k_fc_trips.argtypes = [ctypes.c_void_p, ctypes.c_int]
    ext.extract_batch(d.data_ptr(), B, W, H, W, W * H, k.data_ptr(), de.data_ptr(), cap,
                      n.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert L.orb_k_fc_trips(None, 1) == 0
    ext.extract_batch(d.data_ptr(), B, W, H, W, W * H, k.data_ptr(), de.data_ptr(), cap,
                      n.data_ptr(), s.cuda_stream)
    s.synchronize()
    c = np.zeros(16, np.uint64)
    assert L.orb_k_fc_trips(c.ctypes.data, 0) == 0
    c = c.astype(np.int64)
    rounds, appending, trips, lanes, entries = (int(v) for v in c[:5])
    hist = c[5:14]
    assert rounds > 0 and hist.sum() == rounds, c
    print(f"images counted 16 of {B}; keypoints per image {n.cpu().numpy()[:16].mean():.0f}")
    print(f"pretest rounds {rounds} ({rounds / 16:.0f} per image), appending {appending} "
          f"({appending / rounds:.3f})")
    print(f"loop trips {trips}: {trips / rounds:.3f} per round, {trips / max(appending, 1):.3f} per appending round")
    print(f"entries {entries}: {entries / rounds:.2f} per round, {entries / max(trips, 1):.2f} per trip; "
          f"lanes that append {lanes / rounds:.2f} per round")
    print("trips per round  " + " ".join(f"{i}:{v / rounds:.3f}" for i, v in enumerate(hist)))


if __name__ == "__main__":
    main()
