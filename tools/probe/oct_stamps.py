#!/usr/bin/env python3
"""Per-phase clock sums of k_octree per level (needs the OCT_STAMPS build:
tools/attribution/build.sh octst -DOCT_STAMPS with PATCHES=octree_stamps.patch,
run with ORB_AMD_LIB=.../octst.so).  Thread 0 of every workgroup adds the
s_memtime clocks between phase boundaries to one accumulator per (level,
phase); printed as the mean per workgroup in units of 100 clocks.  The calls
run in the extractor's profile mode (one stage at a time), so the octree's
workgroups share the chip with no other kernel.  Passes over lists of up to
64 nodes (single-wave node steps) book all their node work under
"reg:count+scan", whichever kind of pass they are.
Usage: oct_stamps.py [B]   (B frames per call, default 1024: the batch kernel)"""
import ctypes
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))
from conftest import load_pkg  # noqa: E402

PHASES = ["counts+scan", "gather", "roots", "reg:count+scan", "reg:create", "fin:cand", "fin:rank",
          "fin:jstop+scan", "fin:create", "zero+relabel", "best+out"]


def main():
    import torch
    orb = load_pkg()
    W, H, B = 1241, 376, int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    imgs = np.stack([orb.synth_image(0x4B495454, f, W, H) for f in range(min(B, 64))])
    imgs = np.concatenate([imgs] * ((B + 63) // 64))[:B]
    ext = orb.ORBextractor(1000, 1.2, 8, 20, 7)
    cap = ext.capacity(W, H)
    d = torch.from_numpy(imgs).cuda()
    k = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    de = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    n = torch.zeros(B, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    L = orb.lib()
    L.orb_k_oct_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
    calls = 3
    for i in range(1 + calls):
        if i == 1:  # the first call warms up
            s.synchronize()
            ext.profile(True)
            assert L.orb_k_oct_stamps(None, 1) == 0
        ext.extract_batch(d.data_ptr(), B, W, H, W, W * H, k.data_ptr(), de.data_ptr(), cap,
                          n.data_ptr(), s.cuda_stream)
    s.synchronize()
    acc = np.zeros((16, 16), np.uint64)
    assert L.orb_k_oct_stamps(acc.ctypes.data, 0) == 0
    acc = acc.astype(np.float64)
    for st in range(7):
        name, ms, cnt = ext.profile_read(st)
        if cnt and name == "k_octree":
            print(f"k_octree alone: {ms / calls:.3f} ms per call")
    ext.profile(False)
    print(f"B = {B}, {calls} calls; s_memtime clocks / 100 per workgroup")
    print("lvl    keys  reg  fin ncand " + " ".join(p[:9].rjust(9) for p in PHASES) + "     total")
    tot = np.zeros(len(PHASES))
    for l in range(16):
        wg = acc[l, 14]
        if wg == 0:
            continue
        us = acc[l, :len(PHASES)] / wg / 100.0
        tot += acc[l, :len(PHASES)] / 100.0
        fin = max(acc[l, 13], 1)
        print(f"{l:3d} {acc[l, 11] / wg:7.0f} {acc[l, 12] / wg:4.1f} {acc[l, 13] / wg:4.1f} {acc[l, 15] / fin:5.0f} "
              + " ".join(f"{v:9.2f}" for v in us) + f" {us.sum():9.2f}")
    print("share of all workgroups' time: " + " ".join(f"{p}={v / tot.sum():.3f}" for p, v in zip(PHASES, tot)))


if __name__ == "__main__":
    main()
