#!/usr/bin/env python3
"""Secondary measurements for BASELINE.json's other configs (C1, C2, C3, C5).

bench.py is the driver contract and measures the headline C4 workload; this
script reports the remaining configs, one JSON line each, for BASELINE.md's
results table:

  C1  CPU oracle only: 1241x376, 1000 features, 100-frame synthetic sequence,
      extraction; 1 thread and all host cores (frames/s)
  C2  640x480, 1000 features, GPU extraction only (frames/s) + bit-exact check
  C3  1241x376 stereo pairs, 2000 features per image, both extractions +
      ComputeStereoMatches on the GPU (pairs/s) + bit-exact check
  C5  1920x1080, 4000 features, SearchByProjection against a 50,000-point
      local map (th 1, nnratio 0.8), 16 problems per launch (problems/s for
      extract+match, and the matcher alone with its HBM roofline)
  C4M the headline's matcher alone: 1241x376, 1000 features, 5,000-point local
      maps, 512 problems per launch (same keys as C5)
  F1  SURVEY §8(f): SearchForInitialization, 640x480 frames from the 2000-feature
      initial extractor, window 100, ORBmatcher(0.9, true), 64 pairs per launch
      (pairs/s) + CPU oracle rate + exact check
  F2  SURVEY §8(f): Frame::ComputeBoW (DBoW2 transform, levelsup 4) on an
      ORBvoc-shaped synthetic vocabulary (k 10, L 6, 10^6 words, TF-IDF, L1),
      1000 extracted descriptors per frame, 512 frames per launch (frames/s)
      + CPU oracle rate + exact check
  F3  SURVEY §8(f): ComputeDistinctiveDescriptors over 100,000 map points with
      1..20 observations (points/s) + CPU oracle rate + exact check
  P1  place recognition: DetectRelocalizationCandidates against a database of
      4,096 keyframes of about 1,000 words each on an ORBvoc-shaped synthetic
      vocabulary (k 10, L 6), one query per call (queries/s), each kernel's
      isolated time, bytes/s against 12 B per database entry + exact check
  T1  Optimizer::PoseOptimization: 1,024 problems of the C4 shape per launch
      (1,000 keypoints, about 800 edges, mono and stereo mixed, 1 px noise,
      20 % gross outliers), device-resident (problems/s by device events), the
      one-problem latency through the host-buffer call, the batch's share of
      the headline step + exact check against tests/poseopt_ref.py
  M1  TrackWithMotionModel's SearchByProjection(CurrentFrame, LastFrame): 1,024
      problems of the C4 shape per launch (1241x376, 1,000 keypoints, map
      points on about 80 % of the last frame's keypoints, a rotated predicted
      pose, th 15, retry below 20), device-resident, by device events (median
      of 20), also 1, 64 and 256 problems; against orb_match_projection_frame
      over the same problems one call at a time (host clock; run once more
      with ORB_AMD_LIB naming the parent build for the baseline) + exact check
  B1  TrackReferenceKeyFrame / Relocalization's SearchByBoW(KF, F): B1a 1,024
      problems over 32 distinct bow_pair scenes (1241x376, 1,000 features,
      nnratio 0.7, orientation on, min_matches 15) in one launch, B1b one frame
      slot against 64 keyframe slots (nnratio 0.75); device events around the
      launch (median of 20, minimum, maximum), also 1, 64 and 256 problems;
      against orb_match_bow over the same problems one call at a time (host
      clock; run once more with ORB_AMD_LIB naming the parent build for the
      baseline row alone) + exact check of four problems
  S1  LoopClosing::ComputeSim3's solver: 64 loop candidates of about 150
      correspondences each (256 keypoint slots, 30 % gross outliers, random
      draws), device-resident, by device events (median of 20, minimum,
      maximum): the setup call, one round of iterate(5) over all candidates,
      the rounds to completion with the finished ones discarded, one find();
      against the same calls one problem at a time (64 launches) + exact check
      of four problems against tests/sim3_ref.py
  O1  LoopClosing::ComputeSim3's last stage, Optimizer::OptimizeSim3: 64 loop
      candidates of about 150 correspondences (25 gross outliers each, a start
      from a perturbed true Sim3, th2 10) per launch, device-resident, by
      device events around each launch (median of 20): the time per launch,
      problems/s, one problem alone + exact check against
      tests/sim3opt_ref.py; also written to profiles/sim3opt_O1.json
  N1  LocalMapping::CreateNewMapPoints: 64 (current keyframe, neighbour) pairs
      of about 300 SearchForTriangulation matches each (384 keypoint slots,
      mixed stereo / monocular keypoints, 12 % gross outliers), device-resident,
      through the gate and the body in one launch, by device events (median of
      20, minimum, maximum); the median-depth batch over the 64 neighbours;
      against the same call one pair at a time (64 launches) + exact check of
      four problems against tests/newpoints_ref.py
  G1  LocalMapping::CreateNewMapPoints' matcher, SearchForTriangulation: 64
      keyframe pairs of about 1,000 keypoints in the slot layout, natural
      FeatureVectors (scenarios.vocab_nodes), has_mp 0 % / 50 %, one launch,
      by device events (median of 20, minimum, maximum), also 1 and 16
      problems; against orb_search_for_triangulation over the same pairs one
      blocking call at a time (host clock) + exact check of four problems
      against the oracle and the one-problem entry
  L1  LoopClosing::ComputeSim3's matchers, SearchByBoW(KF, KF) and SearchBySim3:
      64 loop candidates against one current keyframe, about 1,000 keypoints
      per slot, natural FeatureVectors (scenarios.vocab_nodes), by device
      events around each launch (median of 20, minimum, maximum), also 1 and 16
      problems; one full round iterate(5) -> SearchBySim3 -> OptimizeSim3 on
      one stream; against orb_match_bow_kf and orb_search_by_sim3 over the same
      problems one blocking call at a time (host clock; run once more with
      ORB_AMD_LIB naming the parent build for the baseline rows alone) + exact
      check of four problems; each run writes its rows into
      profiles/sim3chain_L1.json (this_build / parent_build)
  R1  RGB-D: 640x480 (TUM1 intrinsics and distortion, DepthMapFactor 5000),
      1000 features, 256 frames per launch, device-resident: extract ->
      undistort -> ComputeStereoFromRGBD -> closest points + UnprojectStereo ->
      stereo batch SearchByProjection against 3,000-point maps (frames/s), the
      same pipeline without the RGB-D stages (monocular matcher), each new
      kernel alone by HIP events with its algorithmic bytes + exact check

Usage: python tools/bench_configs.py [--configs C1,C2,C3,C5,F1,F3,P1,R1,T1,M1,B1,S1,O1,N1,G1,L1] [--steps K]
The oracle (CPU restatement) is used only for the CPU rows and parity checks.
"""
import argparse
import json
import os
import sys
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests")]

import bench  # noqa: E402

SEED = 0x4B495454


def timed(fn, steps, warmup, torch):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def cpu_rate(fn, items, seconds, threads=1):
    """items/s of fn(i) over a bounded sample, on `threads` host threads (the
    oracle's ctypes calls release the GIL)."""
    done = [0]
    lock = threading.Lock()
    stop = time.perf_counter() + seconds

    def worker(t):
        i = t
        while time.perf_counter() < stop:
            fn(i % items)
            with lock:
                done[0] += 1
            i += threads

    t0 = time.perf_counter()
    ths = [threading.Thread(target=worker, args=(t,)) for t in range(threads)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    return done[0] / (time.perf_counter() - t0)


def c1(args, orb, oracle):
    W, H = 1241, 376
    imgs = [oracle.synth_image(SEED, f, W, H) for f in range(100)]
    one = cpu_rate(lambda i: oracle.extract(imgs[i], 1000), 100, args.cpu_seconds, 1)
    nthr = int(os.environ.get("OMP_NUM_THREADS", 0)) or os.cpu_count() or 1  # the box grants 16
    allc = cpu_rate(lambda i: oracle.extract(imgs[i], 1000), 100, args.cpu_seconds, nthr)
    return {"config": "C1", "workload": "1241x376 synthetic 100-frame sequence, 1000 feat, CPU "
            "oracle ORBextractor only", "unit": "frames/s", "cpu_1_thread": one,
            "cpu_all_cores": allc, "cores": nthr, "ms_per_frame_1_thread": 1e3 / one}


def c2(args, orb, oracle, torch):
    W, H, B = 640, 480, args.batch
    imgs = np.stack([orb.synth_image(1 + (f % 3), 0 if f < 3 else f, W, H) for f in range(B)])
    ext = orb.ORBextractor(1000, 1.2, 8, 20, 7)
    cap = ext.capacity(W, H)
    d = torch.from_numpy(imgs).cuda()
    k = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    de = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    n = torch.zeros(B, dtype=torch.int32, device="cuda")
    # an explicit stream: a NULL stream would mean the handle's own stream
    s = torch.cuda.Stream().cuda_stream

    def step():
        ext.extract_batch(d.data_ptr(), B, W, H, W, W * H, k.data_ptr(), de.data_ptr(), cap,
                          n.data_ptr(), s)

    sec = timed(step, args.steps, 2, torch)
    exact = True
    for i in range(3):  # seeds 1..3, frame 0
        kr, dr, _ = oracle.extract(imgs[i], 1000)
        ni = int(n[i].item())
        kg = k[i, :ni].cpu().numpy().view(orb.KEYPOINT_DTYPE).reshape(-1)
        exact &= ni == len(kr) and kg.tobytes() == kr.tobytes() and \
            de[i, :ni].cpu().numpy().tobytes() == dr.tobytes()
    cpu = cpu_rate(lambda i: oracle.extract(imgs[i], 1000), 3, args.cpu_seconds, 1)
    return {"config": "C2", "workload": f"640x480 synthetic, 1000 feat, GPU extraction, batch {B}",
            "unit": "frames/s", "value": B / sec, "ms_per_step": sec * 1e3,
            "bit_exact_seeds_1_3": bool(exact), "cpu_1_thread": cpu}


def c3(args, orb, oracle, torch):
    """bench.c3_workload (the driver line's C3 key, same inputs and schedule)
    plus the oracle check of pair 0 and the oracle's CPU rate."""
    import scenarios

    dev = torch.device("cuda:0")
    r, st = bench.c3_workload(orb, torch, dev, 16, steps=max(args.steps, 40), warmup=5,
                              pairs=args.batch // 2)
    il, ir, s0 = st["il"], st["ir"], st["set0"]
    W, H, NF = 1241, 376, 2000
    p = oracle.params(NF)
    klh, dlh, _ = oracle.extract(il[0], NF)
    krh, drh, _ = oracle.extract(ir[0], NF)
    ur_ref, dp_ref = oracle.stereo_match(klh, dlh, p["scale"], krh, drh, oracle.pyramid(il[0]),
                                         oracle.pyramid(ir[0]), p["inv_scale"], scenarios.BF,
                                         scenarios.FX, W, H)
    n0 = int(s0["nl"][0].item())
    exact = n0 == len(klh) and s0["ur"][0, :n0].cpu().numpy().tobytes() == ur_ref.tobytes() and \
        s0["dp"][0, :n0].cpu().numpy().tobytes() == dp_ref.tobytes()

    def cpu_pair(i):
        a, da, _ = oracle.extract(il[i], NF)
        b, db, _ = oracle.extract(ir[i], NF)
        oracle.stereo_match(a, da, p["scale"], b, db, oracle.pyramid(il[i]), oracle.pyramid(ir[i]),
                            p["inv_scale"], scenarios.BF, scenarios.FX, W, H)

    cpu = cpu_rate(cpu_pair, 4, args.cpu_seconds, 1)
    return dict(config="C3", bit_exact_pair_0=bool(exact), cpu_1_thread=cpu, **r)


def c5(args, orb, oracle, torch):
    return proj_config(args, orb, oracle, torch, "C5", 1920, 1080, 4000, 50000, 16, bench.C5_SEED)


def c4m(args, orb, oracle, torch):
    """the headline's matcher by itself: 512 KITTI-shaped frames, 5,000-point maps"""
    return proj_config(args, orb, oracle, torch, "C4M", 1241, 376, 1000, 5000, 512, 7)


def proj_config(args, orb, oracle, torch, name, W, H, NF, M, B, seed):
    """bench.proj_workload (the driver line's C5 key for C5) plus the oracle
    check of problem 0."""
    dev = torch.device("cuda:0")
    # ~0.1 s timed regions (bench.secondary_configs): short ones are noisy
    steps = max(args.steps, 200 if B <= 64 else 40)
    r, st = bench.proj_workload(orb, torch, dev, 16, W, H, NF, M, B, seed, steps=steps, warmup=10)
    n0 = int(st["nh"][0])
    s0 = st["set0"]
    nr, kmr = oracle.match_projection_local(st["kh"][0, :n0], st["dh"][0, :n0], st["scale"], W, H,
                                            st["mps"][0], st["mpd"][0], 1.0, 0.8, st["lk"][0, :n0])
    exact = int(s0["nm"][0].item()) == nr and np.array_equal(s0["km"][0, :n0].cpu().numpy(), kmr)
    return dict(config=name, bit_exact_problem_0=bool(exact), **r)


def f1(args, orb, oracle, torch):
    import scenarios
    W, H, P, U = 640, 480, 64, 16
    pairs = [scenarios.init_pair(oracle, 100 + i, 1 + i % 3, w=W, h=H, nf=2000) for i in range(U)]
    stride = max(max(len(s["k1"]), len(s["k2"])) for s in pairs)
    K1 = np.zeros((P, stride), orb.KEYPOINT_DTYPE)
    K2 = np.zeros((P, stride), orb.KEYPOINT_DTYPE)
    D1 = np.zeros((P, stride, 32), np.uint8)
    D2 = np.zeros((P, stride, 32), np.uint8)
    PR = np.zeros((P, stride, 2), np.float32)
    n1 = np.zeros(P, np.int32)
    n2 = np.zeros(P, np.int32)
    for i in range(P):
        s = pairs[i % U]
        n1[i], n2[i] = len(s["k1"]), len(s["k2"])
        K1[i, :n1[i]], D1[i, :n1[i]], PR[i, :n1[i]] = s["k1"], s["d1"], s["prev"]
        K2[i, :n2[i]], D2[i, :n2[i]] = s["k2"], s["d2"]
    t = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8)).cuda()
         for k, v in dict(K1=K1, K2=K2, D1=D1, D2=D2, n1=n1, n2=n2).items()}
    pr0 = torch.from_numpy(PR).cuda()
    pr = pr0.clone()
    m12 = torch.zeros((P, stride), dtype=torch.int32, device="cuda")
    nm = torch.zeros(P, dtype=torch.int32, device="cuda")
    mt = orb.ORBmatcher(0.9, True)
    # a real stream shared with torch: the prev-position reset must be ordered
    # before the kernels (handle 0 would select the matcher's own stream)
    ts = torch.cuda.Stream()
    s_ = ts.cuda_stream

    def step():
        with torch.cuda.stream(ts):
            pr.copy_(pr0)  # vbPrevMatched is in/out: restore the initial positions
        mt.search_for_initialization_batch(P, t["K1"].data_ptr(), t["D1"].data_ptr(),
                                           t["n1"].data_ptr(), t["K2"].data_ptr(),
                                           t["D2"].data_ptr(), t["n2"].data_ptr(), stride, 0.0,
                                           float(W), 0.0, float(H), 100, pr.data_ptr(),
                                           m12.data_ptr(), nm.data_ptr(), s_)

    sec = timed(step, args.steps, 2, torch)
    exact = True
    for i in range(U):
        s = pairs[i]
        rn, rm, rp = oracle.search_for_initialization(s["k1"], s["d1"], s["k2"], s["d2"], W, H,
                                                      s["prev"], 100, 0.9, True)
        exact &= int(nm[i].item()) == rn and np.array_equal(m12[i, :n1[i]].cpu().numpy(), rm)
    cpu = cpu_rate(lambda i: oracle.search_for_initialization(
        pairs[i]["k1"], pairs[i]["d1"], pairs[i]["k2"], pairs[i]["d2"], W, H, pairs[i]["prev"],
        100, 0.9, True), U, args.cpu_seconds, 1)
    return {"config": "F1", "workload": f"SearchForInitialization 640x480, 2000-feature initial "
            f"extractor, window 100, {P} pairs per launch", "unit": "pairs/s", "value": P / sec,
            "ms_per_step": sec * 1e3, "cpu_oracle_1_thread": cpu,
            "mean_level0_keypoints": float(np.mean([(s["k1"]["octave"] == 0).sum() for s in pairs])),
            "bit_exact": bool(exact)}


def f3(args, orb, oracle, torch):
    import scenarios
    M = 100000
    rng = np.random.default_rng(9)
    counts = rng.integers(1, 21, M)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    base = rng.integers(0, 256, (M, 32), dtype=np.uint8)
    rows = np.repeat(base, counts, axis=0)
    bits = np.unpackbits(rows, axis=1)
    bits ^= (rng.random(bits.shape) < 0.1).astype(np.uint8)
    desc = np.packbits(bits, axis=1)
    d_offs = torch.from_numpy(offs).cuda()
    d_desc = torch.from_numpy(desc).cuda()
    d_best = torch.zeros(M, dtype=torch.int32, device="cuda")
    d_out = torch.zeros((M, 32), dtype=torch.uint8, device="cuda")
    mt = orb.ORBmatcher()
    s_ = torch.cuda.current_stream().cuda_stream

    def step():
        mt.distinctive_descriptors_batch(M, d_offs.data_ptr(), d_desc.data_ptr(),
                                         d_best.data_ptr(), d_out.data_ptr(), s_)

    sec = timed(step, args.steps, 2, torch)
    ref = oracle.distinctive_descriptors(offs, desc)
    exact = np.array_equal(d_best.cpu().numpy(), ref)
    chunk = 1000
    cpu = cpu_rate(lambda i: oracle.distinctive_descriptors(
        offs[i * chunk:(i + 1) * chunk + 1] - offs[i * chunk],
        desc[offs[i * chunk]:offs[(i + 1) * chunk]]), M // chunk, args.cpu_seconds, 1) * chunk
    alg_bytes = offs[-1] * 32 + (M + 1) * 4 + M * 36
    return {"config": "F3", "workload": "ComputeDistinctiveDescriptors, 100,000 map points, "
            "1..20 observations each", "unit": "points/s", "value": M / sec,
            "ms_per_step": sec * 1e3, "cpu_oracle_1_thread": cpu,
            "alg_GBps": alg_bytes / sec / 1e9, "bit_exact": bool(exact)}


def f2(args, orb, oracle, torch):
    import scenarios
    W, H, NF = 1241, 376, 1000
    voc = scenarios.vocabulary(rng_seed=11, k=10, L=6)
    V = orb.ORBVocabulary(voc["k"], voc["L"], voc["parent"], voc["leaf"], voc["desc"],
                          voc["weight"])
    B = args.batch
    ext = orb.ORBextractor(NF, 1.2, 8, 20, 7)
    frames = []
    for f in range(32):
        _, d = ext(orb.synth_image(SEED, f, W, H))
        frames.append(d[:NF])
    stride = NF + 8
    counts = np.array([len(frames[f % 32]) for f in range(B)], np.int32)
    desc = np.zeros((B, stride, 32), np.uint8)
    for f in range(B):
        desc[f, :counts[f]] = frames[f % 32]
    dev = torch.device("cuda:0")
    d_counts = torch.from_numpy(counts).to(dev)
    d_desc = torch.from_numpy(desc).to(dev)
    n = B * stride
    i32 = lambda m: torch.zeros(m, dtype=torch.int32, device=dev)
    f64 = lambda m: torch.zeros(m, dtype=torch.float64, device=dev)
    fw, fwt, fn, bw, bv, nw = i32(n), f64(n), i32(n), i32(n), f64(n), i32(B)
    fvn, fvo, fvf, nfv = i32(n), i32(B * (stride + 1)), i32(n), i32(B)
    s_ = torch.cuda.current_stream().cuda_stream

    def step():
        V.transform_batch(B, d_counts.data_ptr(), d_desc.data_ptr(), stride, 4, fw.data_ptr(),
                          fwt.data_ptr(), fn.data_ptr(), bw.data_ptr(), bv.data_ptr(),
                          nw.data_ptr(), fvn.data_ptr(), fvo.data_ptr(), fvf.data_ptr(),
                          nfv.data_ptr(), s_)

    sec = timed(step, args.steps, 2, torch)
    exact = True
    h = lambda t: t.cpu().numpy()
    bw_, bv_, nw_, fvn_, fvf_ = h(bw).view(np.uint32), h(bv), h(nw), h(fvn).view(np.uint32), h(fvf)
    for f in range(4):
        r = oracle.vocab_transform(voc, frames[f], 4)
        o = f * stride
        exact &= (np.array_equal(bw_[o:o + nw_[f]], r[0]) and
                  np.array_equal(bv_[o:o + nw_[f]].view(np.uint64), r[1].view(np.uint64)) and
                  np.array_equal(fvn_[o:o + len(r[2])], r[2]) and
                  np.array_equal(fvf_[o:o + len(r[4])].view(np.uint32), r[4]))
    cpu_frames = 8
    cpu_sec = oracle.vocab_time(voc, np.concatenate(frames[:cpu_frames]), cpu_frames, NF, 4)
    feats = int(counts.sum())
    tree_bytes = len(voc["parent"]) * (32 + 8 + 4 + 8 + 4)
    alg_bytes = tree_bytes + feats * (32 + 4 + 8 + 4 + 4 + 8 + 4 + 4 + 4)
    return {"config": "F2", "workload": "Frame::ComputeBoW, ORBvoc-shaped synthetic vocabulary "
            "(k 10, L 6, 10^6 words), 1000 descriptors/frame, levelsup 4", "unit": "frames/s",
            "value": B / sec, "ms_per_step": sec * 1e3, "frames_per_launch": B,
            "features_per_s": feats / sec, "cpu_oracle_1_thread": cpu_frames / cpu_sec,
            "alg_GBps": alg_bytes / sec / 1e9, "bit_exact": bool(exact)}


def p1(args, orb, oracle, torch):
    import placerec_ref
    import scenarios
    NKF, NF, NQ, SCENE = 4096, 1000, 32, 20000
    voc = scenarios.vocabulary(rng_seed=11, k=10, L=6)
    V = orb.ORBVocabulary(voc["k"], voc["L"], voc["parent"], voc["leaf"], voc["desc"],
                          voc["weight"])
    rng = np.random.default_rng(17)
    # one place: every frame sees 1000 of the same 20,000 words (bits flipped)
    scene = rng.choice(np.flatnonzero(voc["leaf"]), SCENE, replace=False)

    def frame_bow():
        bits = np.unpackbits(voc["desc"][rng.choice(scene, NF, replace=False)], axis=1)
        bits ^= (rng.random(bits.shape) < 0.02).astype(np.uint8)
        bw, bv, _ = V.transform(np.packbits(bits, axis=1), 4)
        return bw.copy(), bv.copy()

    db = orb.KeyFrameDatabase(V)
    ref = placerec_ref.KeyFrameDatabase(V.n_words)
    ids = np.arange(1, NKF + 1)
    for i in ids:
        b = frame_bow()
        db.add(int(i), b)
        ref.add(int(i), b)
    for i in ids:  # neighbours in time, as a covisibility graph's best ten are
        nb = [int(j) for j in range(i - 5, i + 6) if j != i and 1 <= j <= NKF]
        db.set_covisibility(int(i), nb)
        ref.set_covisibility(int(i), nb)
    queries = [frame_bow() for _ in range(NQ)]
    entries = sum(len(k.mBowVec[0]) for k in ref.kfs.values())
    qid = [0]

    def step():
        qid[0] += 1
        return db.DetectRelocalizationCandidates(qid[0], queries[qid[0] % NQ])

    exact = True
    for _ in range(2):
        got = step()
        want = ref.DetectRelocalizationCandidates(qid[0], queries[qid[0] % NQ])
        gl, rl = db.last_query(), ref.last_query()
        exact &= got.tolist() == want and all(
            np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
            for a, b in zip(gl, rl))
    steps = max(args.steps, 200)
    sec = timed(step, steps, 10, torch)
    reps = 50
    kernels = {}
    listed = len(db.last_query()[0])
    scored = int(db.last_query()[3].sum())
    for stage in range(5):
        db.profile(stage, 5)
        ms, name = db.profile(stage, reps)
        kernels[name] = ms * 1e3 / reps
    k_us = sum(kernels.values())
    return {"config": "P1", "workload": f"DetectRelocalizationCandidates, {NKF} keyframes, "
            f"{entries / NKF:.0f} words each, k 10 L 6 vocabulary, one query per call",
            "unit": "queries/s", "value": 1.0 / sec, "us_per_query": sec * 1e6,
            "kernel_us_isolated": kernels, "kernel_us_sum": k_us, "database_entries": entries,
            "query_words": int(np.mean([len(q[0]) for q in queries])),
            "last_query_listed": listed, "last_query_scored": scored,
            "alg_bytes": entries * 12, "alg_GBps_per_query": entries * 12 / sec / 1e9,
            "alg_GBps_kernels": entries * 12 / (k_us * 1e-6) / 1e9, "bit_exact": bool(exact)}


def r1(args, orb, oracle, torch):
    import rgbd_ref
    import scenarios
    W, H, NF, B, M, U = 640, 480, 1000, 256, 3000, 16
    K, D = scenarios.cameras()["tum1"]
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    bf, factor = np.float32(40.0), 1.0 / 5000.0
    th_depth = np.float32(bf * np.float32(40.0) / np.float32(fx))  # ThDepth 40 (TUM1.yaml)
    rng = np.random.default_rng(21)
    imgs = np.stack([orb.synth_image(SEED + f % U, f // U, W, H) for f in range(U)])
    # synthetic u16 depth: a slanted plane plus the frame's shapes, about 10 % zeros
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.stack([(5000 + 8 * xx + 12 * yy + 3000 * (imgs[f] > 128)).astype(np.uint16)
                      for f in range(U)])
    depth[rng.random(depth.shape) < 0.1] = 0
    ext = orb.ORBextractor(NF, 1.2, 8, 20, 7)
    mt = orb.ORBmatcher(0.8)
    scale = np.float32(ext.GetScaleFactors())
    cap = ext.capacity(W, H)
    # the local maps: over each unique frame's undistorted keypoints, mTrackProjXR
    # from the depth under the projection
    mps = np.zeros((U, M), orb.MP_TRACK_DTYPE)
    mpd = np.zeros((U, M, 32), np.uint8)
    lk = np.zeros((U, cap), np.uint8)
    host = []
    for f in range(U):
        k, d = ext(imgs[f])
        un = mt.UndistortKeyPoints(k, K, D)
        a, b, c = orb.synth_local_map(SEED + f, un, d, M, W, H)
        px = np.clip(a["proj_x"].astype(np.int64), 0, W - 1)
        py = np.clip(a["proj_y"].astype(np.int64), 0, H - 1)
        z = depth[f][py, px].astype(np.float32) * np.float32(factor)
        a["proj_xr"] = np.where(z > 0, a["proj_x"] - bf / np.where(z > 0, z, 1), a["proj_x"] - 20)
        mps[f], mpd[f], lk[f, :len(k)] = a, b, c
        host.append((k, d, un))
    tile = lambda x: np.ascontiguousarray(np.concatenate([x] * (B // U)))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    d_img, d_depth, d_mps, d_mpd, d_lk = (t(tile(x)) for x in (imgs, depth, mps, mpd, lk))
    d_state = t(rng.choice(np.array([0, 1, 2], np.uint8), (B, cap), p=[0.2, 0.1, 0.7]))
    d_outl = t((rng.random((B, cap)) < 0.05).astype(np.uint8))
    poses = np.zeros(B, orb.POSE_DTYPE)
    for f in range(B):
        R, tt, ow = scenarios.pose(rng)
        poses[f]["rcw"], poses[f]["tcw"], poses[f]["ow"] = R.reshape(9), tt, ow
    d_pose = t(poses)
    z8 = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")
    f32 = lambda n: torch.zeros(n, dtype=torch.float32, device="cuda")
    d_keys, d_un, d_desc, d_n = z8(B * cap * 28), z8(B * cap * 28), z8(B * cap * 32), i32(B)
    d_ur, d_z, d_x3d, d_valid = f32(B * cap), f32(B * cap), f32(B * cap * 3), z8(B * cap)
    d_order, d_create, d_counts = i32(B * cap), z8(B * cap), i32(B * 4)
    d_nm = torch.full((B,), M, dtype=torch.int32, device="cuda")
    d_km, d_nmatch = i32(B * cap), i32(B)
    s = torch.cuda.Stream().cuda_stream
    cam = (fx, fy, cx, cy, float(bf), float(bf) / fx)
    P = lambda x: x.data_ptr()

    def extract():
        ext.extract_batch(P(d_img), B, W, H, W, W * H, P(d_keys), P(d_desc), cap, P(d_n), s)
        mt.undistort_keypoints_batch(B, P(d_n), P(d_keys), cap, K, D, P(d_un), s)

    def rgbd():
        mt.stereo_from_rgbd_batch(B, P(d_n), P(d_keys), P(d_un), cap, P(d_depth),
                                  orb.ORB_DEPTH_U16, W, H, W * 2, W * H * 2, factor, bf, P(d_ur),
                                  P(d_z), s)

    def close():
        mt.close_points_batch(B, P(d_n), P(d_z), P(d_state), P(d_outl), cap, th_depth, P(d_order),
                              P(d_create), P(d_counts), s)

    def unproject():
        mt.unproject_stereo_batch(B, P(d_n), P(d_un), P(d_z), cap, P(d_pose), cam, P(d_x3d),
                                  P(d_valid), s)

    def match_stereo():
        mt.search_by_projection_batch_stereo(B, P(d_un), P(d_desc), P(d_ur), P(d_n), P(d_lk), cap,
                                             P(d_mps), P(d_mpd), P(d_nm), M, W, H, scale, 3.0,
                                             P(d_km), P(d_nmatch), s)

    def match_mono():
        mt.search_by_projection_batch(B, P(d_un), P(d_desc), P(d_n), P(d_lk), cap, P(d_mps),
                                      P(d_mpd), P(d_nm), M, W, H, scale, 3.0, P(d_km),
                                      P(d_nmatch), s)

    def full():
        extract(); rgbd(); close(); unproject(); match_stereo()

    def mono():
        extract(); match_mono()

    steps = max(args.steps, 20)
    sec_mono = timed(mono, steps, 3, torch)
    sec_full = timed(full, steps, 3, torch)
    # parity of frame 0 through the oracle and the restatement
    k, d, un = host[0]
    kr, dr, _ = oracle.extract(imgs[0], NF)
    ur_ref, z_ref = rgbd_ref.stereo_from_rgbd(kr, oracle.undistort_keypoints(kr, K, D), depth[0],
                                              factor, bf)
    n0 = len(kr)
    nr, kmr = oracle.match_projection_local(un, d, scale, W, H, mps[0], mpd[0], 3.0, 0.8,
                                            lk[0, :n0], ur_ref)
    h = lambda x, dt: x.cpu().numpy().view(dt)
    order_ref, create_ref = rgbd_ref.close_points(z_ref, h(d_state, np.uint8)[:n0], th_depth)
    cnt = h(d_counts, np.int32)[:4]
    exact = (int(d_n[0].item()) == n0 and h(d_ur, np.float32)[:n0].tobytes() == ur_ref.tobytes()
             and h(d_z, np.float32)[:n0].tobytes() == z_ref.tobytes()
             and int(d_nmatch[0].item()) == nr and np.array_equal(h(d_km, np.int32)[:n0], kmr)
             and cnt[0] == len(order_ref) and cnt[1] == len(create_ref)
             and np.array_equal(h(d_order, np.int32)[:cnt[0]], order_ref))

    cnts = h(d_counts, np.int32).reshape(B, 4)
    means = {"mean_n_sorted": float(cnts[:, 0].mean()), "mean_n_visit": float(cnts[:, 1].mean()),
             "mean_matches": float(h(d_nmatch, np.int32).mean())}

    enqueue_us = {}  # the host's time to queue one call: a kernel shorter than this is
    # timed at the host's pace, so its figure is an upper bound

    def alone(fn, reps=50):
        """microseconds per call by HIP events on the stream, after a warm-up"""
        ts = torch.cuda.ExternalStream(s)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(5):
            fn()
        e0.record(ts)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        enqueue_us[fn.__name__] = (time.perf_counter() - t0) * 1e6 / reps
        e1.record(ts)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    kp = int(d_n.sum().item())
    slots = B * cap
    # (2,000 launches of the short kernels: a timed window of tens of milliseconds)
    us = {"k_stereo_from_rgbd": alone(rgbd, 2000), "k_unproject_stereo": alone(unproject, 2000),
          "k_close_points": alone(close, 2000), "match_stereo": alone(match_stereo),
          "match_mono": alone(match_mono)}
    # algorithmic bytes: what each kernel must read and write per valid keypoint
    # (rgbd: mvKeys x, y + mvKeysUn x + one u16 + two floats out; unproject: x, y,
    # z + 13 out; close points: z, state, outlier in, order + create out per slot)
    alg = {"k_stereo_from_rgbd": kp * (8 + 4 + 2 + 8), "k_unproject_stereo": kp * (8 + 4 + 13) + B * 60,
           "k_close_points": kp * 6 + slots * 5 + B * 16}
    return {"config": "R1", "workload": f"RGB-D 640x480 TUM1, DepthMapFactor 5000, {NF} feat, "
            f"{B} frames per launch: extract -> undistort -> ComputeStereoFromRGBD -> close "
            f"points + UnprojectStereo -> stereo SearchByProjection, {M}-point maps",
            "unit": "frames/s", "value": B / sec_full, "ms_per_step": sec_full * 1e3,
            "without_rgbd_stages_frames_per_s": B / sec_mono, "without_rgbd_ms_per_step": sec_mono * 1e3,
            "kernel_us_isolated": us, "host_enqueue_us": enqueue_us, "alg_bytes": alg,
            "alg_GBps": {k_: alg[k_] / (us[k_] * 1e-6) / 1e9 for k_ in alg},
            "keypoints_per_launch": kp, "kp_stride": cap, "resolve_kernel": mt.resolve_kernel(B, cap, M),
            "bit_exact_frame_0": bool(exact), **means}


def t1(args, orb, oracle, torch):
    import poseopt_cases as pc
    B, NKP, NE, DISTINCT = 1024, 1000, 800, 128
    cases = [pc.make_case(9000 + i, NKP, NE + (i * 7) % 41 - 20, "mixed", 1.0, 0.2)
             for i in range(DISTINCT)]
    keys = np.zeros((B, NKP), orb.KEYPOINT_DTYPE)
    ur = np.full((B, NKP), -1, np.float32)
    idx = np.full((B, NKP), -1, np.int32)
    poses = np.zeros(B, orb.POSE_DTYPE)
    npts = max(len(c["points"]) for c in cases)
    pts = np.zeros((B, npts, 3), np.float32)
    for p in range(B):  # (the distinct problems repeat 8 times across the batch)
        c = cases[p % DISTINCT]
        keys[p], ur[p], idx[p], poses[p] = c["keys"], c["u_right"], c["point_index"], c["pose"][0]
        pts[p, :len(c["points"])] = c["points"]

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_keys, d_ur, d_idx, d_pin, d_pts = (dev(a) for a in (keys, ur, idx, poses, pts))
    d_nk = torch.full((B,), NKP, dtype=torch.int32, device="cuda")
    d_pout = torch.zeros(B * orb.POSE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_outl = torch.zeros(B * NKP, dtype=torch.uint8, device="cuda")
    d_info = torch.zeros(B * 4, dtype=torch.int32, device="cuda")
    m = orb.ORBmatcher()
    stream = torch.cuda.Stream()  # the launch and its events on one stream

    def run(nprob=B):
        m.pose_optimization_batch(nprob, d_nk.data_ptr(), d_keys.data_ptr(), d_ur.data_ptr(), NKP,
                                  d_idx.data_ptr(), d_pts.data_ptr(), 12, npts,
                                  pc.INV_LEVEL_SIGMA2, pc.CAM, d_pin.data_ptr(), d_pout.data_ptr(),
                                  d_outl.data_ptr(), d_info.data_ptr(), stream=stream.cuda_stream)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(max(args.steps, 5)):  # device events around each launch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        run()
        e1.record(stream)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    batch_ms = ms[len(ms) // 2]
    wall_ms = timed(run, max(args.steps, 5), 1, torch) * 1e3  # host clock, back-to-back launches
    by_size = {}
    for nprob in (1, 64, 256, 768):  # how the launch scales with the problems in flight
        t = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run(nprob)
            e1.record(stream)
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        by_size[str(nprob)] = sorted(t)[2]
    run()
    torch.cuda.synchronize()
    info = d_info.cpu().numpy().view(orb.POSE_OPT_INFO_DTYPE)
    pout = d_pout.cpu().numpy().view(orb.POSE_DTYPE)
    outl = d_outl.cpu().numpy().reshape(B, NKP)
    exact = True
    for p in (0, 1, DISTINCT + 1, B - 1):
        r = pc.run_ref(cases[p % DISTINCT])
        want = np.where(cases[p % DISTINCT]["point_index"] >= 0, r["outlier"], 0)
        exact &= (tuple(int(v) for v in info[p]) ==
                  (r["n_inliers"], r["n_edges"], r["lm_iterations"], r["rejected_trials"]))
        exact &= all(pout[p][k].tobytes() == r[k].tobytes() for k in ("rcw", "tcw", "ow"))
        exact &= bool(np.array_equal(outl[p], want))
    # one problem through the host-buffer call (upload, launch, download, wait)
    c = cases[0]
    one = lambda: m.PoseOptimization(c["keys"], c["u_right"], c["point_index"], c["points"],
                                     pc.INV_LEVEL_SIGMA2, pc.CAM, c["pose"])
    for _ in range(5):
        one()
    lat = []
    for _ in range(50):
        t0 = time.perf_counter()
        one()
        lat.append((time.perf_counter() - t0) * 1e3)
    lat.sort()
    headline_ms = 2.9  # the headline step per 1,024 frames
    return {"config": "T1", "workload": f"PoseOptimization, {B} problems x {NKP} keypoints, "
            f"{int(info['n_edges'].mean())} edges on average, mixed mono / stereo, 1 px noise, "
            f"20% outliers ({DISTINCT} distinct problems)",
            "batch_ms_median": batch_ms, "batch_ms_min": ms[0], "batch_ms_max": ms[-1],
            "batch_ms_host_clock": wall_ms, "launch_ms_by_problems": by_size, "problems_per_s": B / (batch_ms * 1e-3),
            "one_problem_latency_ms_median": lat[len(lat) // 2], "one_problem_latency_ms_min": lat[0],
            "lm_iterations_mean": float(info["lm_iterations"].mean()),
            "rejected_trials_mean": float(info["rejected_trials"].mean()),
            "inliers_mean": float(info["n_inliers"].mean()),
            "share_of_headline_step": batch_ms / headline_ms, "headline_step_ms": headline_ms,
            "lds_edges": m.pose_optimization_lds_edges(), "bit_exact_4_problems": bool(exact)}


def m1(args, orb, oracle, torch):
    import scenarios as S
    import track_motion_ref as R
    B, DISTINCT, TH, RETRY = 1024, 32, 15.0, 20
    W, H = 1241, 376
    rng = np.random.default_rng(SEED)
    probs, scale = [], None
    for i in range(DISTINCT):  # frame_pair scenes: frames 0 and 1 of sequence 40 + i
        fp = S.frame_pair(oracle, 40 + i, rng_seed=i)
        last = fp["last"].copy()
        last["valid"] = rng.random(len(last)) < 0.8
        scale = fp["scale"]
        pr = R.problem_from_records(fp["kb"], fp["db"], last, fp["last_desc"], 0.0)
        Rm, t, _ = S.pose(rng)
        pts = pr["points"].copy()
        pts["pos"] = ((pts["pos"].astype(np.float64) - t.astype(np.float64))
                      @ Rm.astype(np.float64)).astype(np.float32)
        pr["points"], pr["pose_cur"] = pts, R.pose(Rm, t)
        pr["pose_last"] = R.pose(Rm, t + np.array([0, 0, 0.3], np.float32))
        probs.append(pr)
    stride = max(max(len(p["keys"]), len(p["last_keys"])) for p in probs)
    keys = np.zeros((B, stride), orb.KEYPOINT_DTYPE)
    desc = np.zeros((B, stride, 32), np.uint8)
    lkeys = np.zeros((B, stride), orb.KEYPOINT_DTYPE)
    lidx = np.full((B, stride), -1, np.int32)
    pts = np.zeros((B, stride), orb.MAP_POINT_DTYPE)
    md = np.zeros((B, stride, 32), np.uint8)
    nk, ln = np.zeros(B, np.int32), np.zeros(B, np.int32)
    pc, pl = np.zeros(B, orb.POSE_DTYPE), np.zeros(B, orb.POSE_DTYPE)
    for p in range(B):
        pr = probs[p % DISTINCT]
        n, m = len(pr["keys"]), len(pr["last_keys"])
        keys[p, :n], desc[p, :n], nk[p] = pr["keys"], pr["desc"], n
        lkeys[p, :m], lidx[p, :m], ln[p] = pr["last_keys"], pr["last_point_index"], m
        pts[p, :m], md[p, :m] = pr["points"][:m], pr["mp_desc"][:m]
        pc[p], pl[p] = pr["pose_cur"][0], pr["pose_last"][0]
    cam = S.camera()
    m = orb.ORBmatcher(0.9, True)
    # one call at a time through the one-problem entry, host-projected records
    recs = []
    for pr in probs:
        last, ld = R.last_records(pr["pose_cur"], pr["last_keys"], pr["last_point_index"], None,
                                  pr["points"], pr["mp_desc"])
        recs.append((orb.Frame(pr["keys"], pr["desc"], scale, W, H), last, ld,
                     float(R.tlc(pr["pose_cur"], pr["pose_last"])[2])))

    def one(i, th=TH):
        F, last, ld, tz = recs[i]
        return m.SearchByProjectionFrame(F, last, ld, cam, tz, th, True)
    for i in range(DISTINCT):
        one(i)
    lat = []
    for rep in range(4):
        for i in range(DISTINCT):
            t0 = time.perf_counter()
            one(i)
            lat.append((time.perf_counter() - t0) * 1e3)
    lat.sort()
    out = {"config": "M1", "library": str(orb.LIB_PATH),
           "workload": f"SearchByProjection(F, LastF), {B} problems x {stride} keypoint slots, "
                       f"{int(np.mean([(p['last_point_index'] >= 0).sum() for p in probs]))} "
                       f"last-frame map points on average, th {TH}, retry below {RETRY} "
                       f"({DISTINCT} distinct problems)",
           "one_call_ms_median": lat[len(lat) // 2], "one_call_ms_min": lat[0],
           "one_call_ms_max": lat[-1], "one_call_samples": len(lat)}
    if not hasattr(orb.lib(), "orb_match_projection_frame_batch"):
        return out  # a build from before the batch entry: the baseline row only

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d = {k: dev(a) for k, a in dict(keys=keys, desc=desc, lkeys=lkeys, lidx=lidx, pts=pts, md=md,
                                    nk=nk, ln=ln, pc=pc, pl=pl).items()}
    d_km = torch.zeros(B * stride, dtype=torch.int32, device="cuda")
    d_info = torch.zeros(B * 5, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()

    def run(nprob=B):
        m.search_by_projection_frame_batch(
            nprob, d["keys"].data_ptr(), d["desc"].data_ptr(), 0, 0, d["nk"].data_ptr(), stride,
            d["pc"].data_ptr(), d["pl"].data_ptr(), d["lkeys"].data_ptr(), d["ln"].data_ptr(),
            d["lidx"].data_ptr(), 0, d["pts"].data_ptr(), d["md"].data_ptr(), stride, cam, 0.0,
            float(W), 0.0, float(H), scale, TH, True, RETRY, d_km.data_ptr(), d_info.data_ptr(),
            stream=stream.cuda_stream)

    def events(nprob, reps):
        t = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run(nprob)
            e1.record(stream)
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        return sorted(t)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = events(B, 20)
    by_size = {str(n): events(n, 20)[10] for n in (1, 64, 256)}
    run()
    torch.cuda.synchronize()
    km = d_km.cpu().numpy().reshape(B, stride)
    info = d_info.cpu().numpy().view(orb.FRAME_MATCH_INFO_DTYPE)
    exact = True
    for p in (0, 1, DISTINCT + 1, B - 1):
        i = p % DISTINCT
        n1, km1 = one(i)
        if n1 < RETRY:
            n1, km1 = one(i, 2.0 * TH)
        exact &= n1 == int(info[p]["n_matches"]) and bool(np.array_equal(km1, km[p, :len(km1)]))
    batch_ms = ms[len(ms) // 2]
    out.update({"batch_ms_median": batch_ms, "batch_ms_min": ms[0], "batch_ms_max": ms[-1],
                "launch_ms_by_problems": by_size, "problems_per_s": B / (batch_ms * 1e-3),
                "batch_us_per_problem": batch_ms * 1e3 / B,
                "one_call_over_batch_per_problem": lat[len(lat) // 2] / (batch_ms / B),
                "matches_mean": float(info["n_matches"].mean()),
                "retried": int(info["retried"].sum()), "kp_stride": stride,
                "max_stride": m.search_by_projection_frame_batch_max_stride(),
                "exact_vs_one_problem_entry_4_problems": bool(exact)})
    return out


def b1(args, orb, oracle, torch):
    import bow_batch_ref as BR
    import scenarios as S
    B, DISTINCT, K, MIN = 1024, 32, 64, 15
    probs = [BR.from_bow(S.bow_pair(oracle, 40 + i, rng_seed=i)) for i in range(DISTINCT)]
    stride = max(len(s["desc"]) for p in probs for s in (p["kf"], p["f"]))
    ma, mb = orb.ORBmatcher(0.7, True), orb.ORBmatcher(0.75, True)

    def bad_flags(p):
        mp = p["kf"]["pidx"]
        return np.where(mp >= 0, p["points"]["bad"][np.maximum(mp, 0)], 0).astype(np.uint8)
    bad = [bad_flags(p) for p in probs]

    def one(m, k, f):   # keyframe of scene k against the frame of scene f, one blocking call
        kf, fr = probs[k]["kf"], probs[f]["f"]
        return m.SearchByBoW(kf["desc"], kf["angle"], kf["pidx"], bad[k], kf["fv"], fr["desc"],
                             fr["angle"], fr["fv"])

    def latency(m, pairs, reps):
        for k, f in pairs:
            one(m, k, f)
        lat = []
        for _ in range(reps):
            for k, f in pairs:
                t0 = time.perf_counter()
                one(m, k, f)
                lat.append((time.perf_counter() - t0) * 1e3)
        return sorted(lat)
    lat = latency(ma, [(i, i) for i in range(DISTINCT)], 4)
    reloc_pairs = [(k % DISTINCT, 0) for k in range(K)]
    t0 = time.perf_counter()
    for k, f in reloc_pairs:
        one(mb, k, f)
    reloc_serial_ms = (time.perf_counter() - t0) * 1e3
    nodes = [len(p["f"]["fv"][0]) for p in probs]
    out = {"config": "B1", "library": str(orb.LIB_PATH),
           "workload": f"SearchByBoW(KF, F), {B} problems x {stride} keypoint slots, "
                       f"{int(np.mean(nodes))} frame nodes on average, largest node "
                       f"{max(int(np.diff(p['f']['fv'][1]).max()) for p in probs)} features, "
                       f"nnratio 0.7, min_matches {MIN} ({DISTINCT} distinct problems); "
                       f"relocalisation: 1 frame x {K} keyframes, nnratio 0.75",
           "one_call_ms_median": lat[len(lat) // 2], "one_call_ms_min": lat[0],
           "one_call_ms_max": lat[-1], "one_call_samples": len(lat),
           "reloc_serial_ms": reloc_serial_ms}
    if not hasattr(orb.lib(), "orb_match_bow_batch"):
        return out  # a build from before the batch entry: the baseline row only

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    ka = BR.pack_slots([probs[p % DISTINCT]["kf"] for p in range(B)], stride)
    fa = BR.pack_slots([probs[p % DISTINCT]["f"] for p in range(B)], stride)
    pts, mps = BR.pack_points([p["points"] for p in probs])   # scene i's array at i * mps
    dk, df = {k: dev(a) for k, a in ka.items()}, {k: dev(a) for k, a in fa.items()}
    # the 1,024 problems read the 32 point arrays through a per-problem copy
    d_pts = dev(np.concatenate([pts[(p % DISTINCT) * mps:(p % DISTINCT + 1) * mps] for p in range(B)]))
    d_km = torch.zeros(B * stride, dtype=torch.int32, device="cuda")
    d_info = torch.zeros(B * 5, dtype=torch.int32, device="cuda")
    d_zero = torch.zeros(K, dtype=torch.int32, device="cuda")
    d_kidx = dev(np.arange(K, dtype=np.int32))
    stream = torch.cuda.Stream()

    def run(m, nprob, kidx=0, fidx=0, mp_stride=mps):
        m.search_by_bow_batch(
            nprob, kidx, fidx, dk["keys"].data_ptr(), dk["desc"].data_ptr(), dk["nkeys"].data_ptr(),
            dk["pidx"].data_ptr(), dk["fv_nodes"].data_ptr(), dk["fv_offs"].data_ptr(),
            dk["fv_feats"].data_ptr(), dk["n_fv_nodes"].data_ptr(), df["keys"].data_ptr(),
            df["desc"].data_ptr(), df["nkeys"].data_ptr(), df["fv_nodes"].data_ptr(),
            df["fv_offs"].data_ptr(), df["fv_feats"].data_ptr(), df["n_fv_nodes"].data_ptr(),
            stride, d_pts.data_ptr(), mp_stride, MIN, d_km.data_ptr(), d_info.data_ptr(),
            stream=stream.cuda_stream)

    def events(fn, reps):
        t = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        return sorted(t)

    def fetch(n):
        torch.cuda.synchronize()
        return (d_km.cpu().numpy().reshape(B, stride)[:n].copy(),
                d_info.cpu().numpy().view(orb.BOW_MATCH_INFO_DTYPE)[:n].copy())
    for _ in range(3):
        run(ma, B)
    torch.cuda.synchronize()
    ms = events(lambda: run(ma, B), 20)
    by_size = {str(n): events(lambda n=n: run(ma, n), 20)[10] for n in (1, 64, 256)}
    run(ma, B)
    km, info = fetch(B)
    exact = True
    for p in (0, 1, DISTINCT + 1, B - 1):
        n1, fm1 = one(ma, p % DISTINCT, p % DISTINCT)
        want = fm1 if n1 >= MIN else np.full(len(fm1), -1, np.int32)
        exact &= n1 == int(info[p]["n_matches"]) and bool(np.array_equal(want, km[p, :len(fm1)]))
    # B1b: K keyframe slots against frame slot 0, each with its own point array
    reloc = lambda: run(mb, K, d_kidx.data_ptr(), d_zero.data_ptr())
    reloc()
    rms = events(reloc, 20)
    reloc()
    rkm, rinfo = fetch(K)
    for k in (0, 1, K - 1):
        n1, fm1 = one(mb, k % DISTINCT, 0)
        want = fm1 if n1 >= MIN else np.full(len(fm1), -1, np.int32)
        exact &= n1 == int(rinfo[k]["n_matches"]) and bool(np.array_equal(want, rkm[k, :len(fm1)]))
    batch_ms = ms[len(ms) // 2]
    out.update({"batch_ms_median": batch_ms, "batch_ms_min": ms[0], "batch_ms_max": ms[-1],
                "launch_ms_by_problems": by_size, "problems_per_s": B / (batch_ms * 1e-3),
                "batch_us_per_problem": batch_ms * 1e3 / B,
                "one_call_over_batch_per_problem": lat[len(lat) // 2] / (batch_ms / B),
                "matches_mean": float(info["n_matches"].mean()),
                "tried_mean": float(info["n_tried"].mean()),
                "reloc_ms_median": rms[len(rms) // 2], "reloc_ms_min": rms[0],
                "reloc_ms_max": rms[-1], "reloc_enough": int(rinfo["enough"].sum()),
                "reloc_serial_over_batch": reloc_serial_ms / rms[len(rms) // 2],
                "kp_stride": stride, "max_stride": orb.match_bow_batch_max_stride(),
                "exact_vs_one_problem_entry": bool(exact)})
    return out


def s1(args, orb, oracle, torch):
    import sim3_cases as SC
    from sim3_ref import RESULT_DTYPE, STATE_DTYPE
    P, S, MAXI = 64, SC.STRIDE, SC.MAX_ITERATIONS
    rng = np.random.default_rng(31)
    probs = [SC.make_problem(f"s{i}", 3000 + i, n_corr=int(rng.integers(130, 171)),
                             n_outliers=45, n_extra=20, scale=1.05) for i in range(P)]
    b = SC.Batch(probs, S, MAXI)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d = {k: dev(getattr(b, k)) for k in ("kf1_slot", "kf2_slot", "keys", "nkeys", "point_index",
                                         "pose", "points", "match12", "index2", "draws")}
    state = torch.zeros(P * 184, dtype=torch.uint8, device="cuda")
    corr = torch.zeros(P * S * 56, dtype=torch.uint8, device="cuda")
    inl = torch.zeros(P * S, dtype=torch.uint8, device="cuda")
    res = torch.zeros(P * 132, dtype=torch.uint8, device="cuda")
    m = orb.ORBmatcher(0.75, True)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def setup(n=P, p0=0):
        m.sim3_solver_setup_batch(
            n, d["kf1_slot"].data_ptr() + 4 * p0, d["kf2_slot"].data_ptr() + 4 * p0,
            d["keys"].data_ptr(), d["nkeys"].data_ptr(), d["point_index"].data_ptr(),
            d["pose"].data_ptr(), S, d["points"].data_ptr(), d["match12"].data_ptr() + 4 * S * p0,
            0, d["index2"].data_ptr() + 4 * S * p0, SC.LEVEL_SIGMA2, SC.CAM1, SC.CAM2, False,
            state.data_ptr() + 184 * p0, corr.data_ptr() + 56 * S * p0, stream=sp)

    def iterate(k, n=P, p0=0, active=0):
        m.sim3_solver_iterate_batch(
            n, S, state.data_ptr() + 184 * p0, corr.data_ptr() + 56 * S * p0,
            d["draws"].data_ptr() + 4 * 3 * MAXI * p0, 3 * MAXI, k, inl.data_ptr() + S * p0,
            res.data_ptr() + 132 * p0, active, stream=sp)

    def events(prep, fn, reps=20):
        t = []
        for _ in range(reps):
            prep()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        t.sort()
        return {"median": t[len(t) // 2], "min": t[0], "max": t[-1]}

    def results():
        torch.cuda.synchronize()
        return res.cpu().numpy().view(RESULT_DTYPE).copy()

    def serial(fn):
        for p in range(P):
            fn(p)
    for _ in range(3):
        setup()
        iterate(5)
    t_setup = events(lambda: None, setup)
    t_round = events(setup, lambda: iterate(5))
    t_find = events(setup, lambda: iterate(MAXI))
    t_round_serial = events(setup, lambda: serial(lambda p: iterate(5, 1, p)))
    t_find_serial = events(setup, lambda: serial(lambda p: iterate(MAXI, 1, p)))
    t_setup_serial = events(lambda: None, lambda: serial(lambda p: setup(1, p)))
    # ComputeSim3's loop: rounds of iterate(5), the finished candidates discarded
    # (the discard flags are read back every round, as the reference's loop reads them)
    setup()
    active = np.ones(P, np.uint8)
    rounds, t0 = 0, time.perf_counter()
    while active.any() and rounds < 61:
        act = dev(active)
        iterate(5, active=act.data_ptr())
        r = results()
        active &= ((r["no_more"] == 0) & (r["has_sim3"] == 0)).astype(np.uint8)
        rounds += 1
    loop_ms = (time.perf_counter() - t0) * 1e3
    found = int(results()["has_sim3"].sum())
    # exact check: find() on four problems against the restatement
    setup()
    iterate(MAXI)
    r = results()
    st = state.cpu().numpy().view(STATE_DTYPE)
    exact = True
    for p in (0, 1, P // 2, P - 1):
        ref = probs[p].solver()
        T, no_more, vb, n = ref.iterate(MAXI)
        exact &= st[p].tobytes() == ref.state_record().tobytes()
        exact &= r[p].tobytes() == ref.result_record(T, no_more, n).tobytes()
    return {"config": "S1", "library": str(orb.LIB_PATH),
            "workload": f"Sim3Solver, {P} candidates x {int(np.mean(st['n']))} correspondences "
                        f"on average ({int(st['n'].min())}-{int(st['n'].max())}), {S} keypoint "
                        f"slots, 45 gross outliers each, probability 0.99, min_inliers 20, "
                        f"max_iterations {MAXI}",
            "setup_ms": t_setup, "iterate5_ms": t_round, "find_ms": t_find,
            "setup_serial_ms": t_setup_serial, "iterate5_serial_ms": t_round_serial,
            "find_serial_ms": t_find_serial,
            "iterate5_serial_over_batch": t_round_serial["median"] / t_round["median"],
            "find_serial_over_batch": t_find_serial["median"] / t_find["median"],
            "compute_sim3_rounds": rounds, "compute_sim3_loop_host_ms": loop_ms,
            "found": found, "iterations_mean": float(st["iterations"].mean()),
            "iterations_max": int(st["iterations"].max()),
            "max_stride": orb.sim3_solver_max_stride(), "exact_vs_restatement": bool(exact)}


def o1(args, orb, oracle, torch):
    import sim3opt_cases as OC
    from sim3opt_ref import OPT_RESULT_DTYPE, result_record
    P = 64
    rng = np.random.default_rng(41)
    cases = [OC.make(5000 + i, int(rng.integers(135, 166)), 25, noise=0.7) for i in range(P)]
    H = OC.HOSTS["std"]
    S = max(max(c["n1"], c["n2"]) for c in cases)
    keys = np.zeros((2 * P, S), orb.KEYPOINT_DTYPE)
    nkeys = np.zeros(2 * P, np.int32)
    pidx = np.full((2 * P, S), -1, np.int32)
    pose = np.zeros(2 * P, orb.POSE_DTYPE)
    match = np.full((P, S), -1, np.int32)
    index2 = np.full((P, S), -1, np.int32)
    start = np.zeros(P, orb.SIM3_RESULT_DTYPE)
    pts, base = [], 0
    for i, c in enumerate(cases):
        for s_, k, o, n in ((2 * i, c["keys1"], c["octave1"], c["n1"]),
                            (2 * i + 1, c["keys2"], c["octave2"], c["n2"])):
            keys["x"][s_, :n], keys["y"][s_, :n], keys["octave"][s_, :n] = k[:, 0], k[:, 1], o
            nkeys[s_] = n
        pidx[2 * i, :c["n1"]] = np.where(c["point_index1"] >= 0, c["point_index1"] + base, -1)
        match[i, :c["n1"]] = np.where(c["match12"] >= 0, c["match12"] + base, -1)
        index2[i, :c["n1"]] = c["index2"]
        pose["rcw"][2 * i], pose["tcw"][2 * i] = c["pose1"]
        pose["rcw"][2 * i + 1], pose["tcw"][2 * i + 1] = c["pose2"]
        start["has_sim3"][i] = 1
        start["R"][i], start["t"][i], start["scale"][i] = c["start"]
        p = np.zeros(len(c["pos"]), orb.MAP_POINT_DTYPE)
        p["pos"] = c["pos"]
        pts.append(p)
        base += len(p)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    slots = np.arange(2 * P, dtype=np.int32)
    d = dict(kf1=dev(slots[0::2]), kf2=dev(slots[1::2]), keys=dev(keys), nkeys=dev(nkeys),
             pidx=dev(pidx), pose=dev(pose), points=dev(np.concatenate(pts)), match0=dev(match),
             match=dev(match), index2=dev(index2), start=dev(start))
    out = torch.zeros(P * OPT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    m = orb.ORBmatcher(0.75, True)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def run(n=P, p0=0):
        m.optimize_sim3_batch(
            n, d["kf1"].data_ptr() + 4 * p0, d["kf2"].data_ptr() + 4 * p0, d["keys"].data_ptr(),
            d["nkeys"].data_ptr(), d["pidx"].data_ptr(), d["pose"].data_ptr(), S,
            d["points"].data_ptr(), d["match"].data_ptr() + 4 * S * p0,
            d["index2"].data_ptr() + 4 * S * p0, d["start"].data_ptr() + 132 * p0, H["levels"],
            H["K1"], H["K2"], out.data_ptr() + OPT_RESULT_DTYPE.itemsize * p0,
            th2=float(H["th2"]), fix_scale=False, stream=sp)

    def events(fn, reps=20):
        t = []
        for _ in range(reps):
            with torch.cuda.stream(stream):
                d["match"].copy_(d["match0"])  # the call removes matches in place
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        t.sort()
        return {"median": t[len(t) // 2], "min": t[0], "max": t[-1]}

    for _ in range(3):
        run()
    t_batch = events(run)
    t_one = events(lambda: run(1, 0))
    t_serial = events(lambda: [run(1, p) for p in range(P)])
    with torch.cuda.stream(stream):
        d["match"].copy_(d["match0"])
    run()
    torch.cuda.synchronize()
    rec = out.cpu().numpy().view(OPT_RESULT_DTYPE)
    exact = True
    for p in (0, 1, P // 2, P - 1):
        exact &= rec[p].tobytes() == result_record(OC.run_ref(cases[p]))[0].tobytes()
    r = {"config": "O1", "library": str(orb.LIB_PATH),
         "workload": f"OptimizeSim3, {P} candidates x {int(rec['n_corr'].mean())} correspondences "
                     f"on average ({int(rec['n_corr'].min())}-{int(rec['n_corr'].max())}), {S} "
                     f"keypoint slots, 25 gross outliers each, th2 10, scale free",
         "launch_ms": t_batch, "problems_per_s": P / (t_batch["median"] * 1e-3),
         "one_problem_ms": t_one, "serial_ms": t_serial,
         "serial_over_batch": t_serial["median"] / t_batch["median"],
         "n_inliers_mean": float(rec["n_inliers"].mean()), "n_bad_mean": float(rec["n_bad"].mean()),
         "max_stride": orb.optimize_sim3_max_stride(), "exact_vs_restatement": bool(exact)}
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "sim3opt_O1.json").write_text(json.dumps(r, indent=1) + "\n")
    return r


def n1(args, orb, oracle, torch):
    import newpoints_cases as NC
    from newpoints_ref import MAP_POINT_DTYPE, NEW_POINT_INFO_DTYPE
    P, S = 64, 384
    rng = np.random.default_rng(41)
    cases = [NC.natural_case(f"n{i}", 5000 + i, int(rng.integers(280, 321)), False, n_extra=20,
                             n_exist=30) for i in range(P)]
    b = NC.pack(cases, S)
    cap = int(b["base"][-1])

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d = {k: dev(b[k]) for k in ("keys", "u_right", "depth", "pose", "nkeys", "match12",
                                "kf1_slot", "kf2_slot", "median", "cursor_index")}
    pidx0, cur0, pts0 = dev(b["point_index"]), dev(b["cursor"]), dev(b["points"])
    pidx, cur, pts = pidx0.clone(), cur0.clone(), pts0.clone()
    status = torch.zeros(P * S, dtype=torch.uint8, device="cuda")
    x3d = torch.zeros(P * S * 3, dtype=torch.float32, device="cuda")
    pairs = torch.zeros(P * S * 2, dtype=torch.int32, device="cuda")
    info = torch.zeros(P * 64, dtype=torch.uint8, device="cuda")
    med = torch.zeros(P, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(P, dtype=torch.int32, device="cuda")
    m = orb.ORBmatcher(0.6, False)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def reset():
        with torch.cuda.stream(stream):
            pidx.copy_(pidx0)
            cur.copy_(cur0)
            pts.copy_(pts0)

    def create(n=P, p0=0):
        m.create_new_map_points_batch(
            n, d["kf1_slot"].data_ptr() + 4 * p0, d["kf2_slot"].data_ptr() + 4 * p0,
            d["keys"].data_ptr(), d["nkeys"].data_ptr(), pidx.data_ptr(), d["pose"].data_ptr(),
            d["u_right"].data_ptr(), d["depth"].data_ptr(), S, d["match12"].data_ptr() + 4 * S * p0,
            d["median"].data_ptr() + 4 * p0, NC.CAM_N, NC.CAM_N, NC.SCALE_FACTORS,
            NC.LEVEL_SIGMA2, False, pts.data_ptr(), cap, cur.data_ptr(),
            d["cursor_index"].data_ptr() + 4 * p0, status.data_ptr() + S * p0,
            x3d.data_ptr() + 12 * S * p0, pairs.data_ptr() + 8 * S * p0, info.data_ptr() + 64 * p0,
            sp)

    def median():
        m.scene_median_depth_batch(P, d["kf2_slot"].data_ptr(), d["nkeys"].data_ptr(),
                                   pidx0.data_ptr(), d["pose"].data_ptr(), S, pts0.data_ptr(),
                                   med.data_ptr(), cnt.data_ptr(), 2, sp)

    def events(prep, fn, reps=20):
        t = []
        for _ in range(reps):
            prep()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        t.sort()
        return {"median": t[len(t) // 2], "min": t[0], "max": t[-1]}

    for _ in range(3):
        reset()
        create()
        median()
    t_batch = events(reset, create)
    t_serial = events(reset, lambda: [create(1, p) for p in range(P)])
    t_median = events(lambda: None, median)
    reset()
    create()
    torch.cuda.synchronize()
    inf = info.cpu().numpy().view(NEW_POINT_INFO_DTYPE)
    st = status.cpu().numpy().reshape(P, S)
    xs = x3d.cpu().numpy().reshape(P, S, 3)
    pt = pts.cpu().numpy().view(MAP_POINT_DTYPE)
    exact = True
    for p in (0, 1, P // 2, P - 1):
        ref = cases[p].ref()
        n1k = len(cases[p].match12)
        lo, hi = int(b["base"][p]), int(b["base"][p + 1])
        got = inf[p].copy()
        got["first_point"] -= lo
        exact &= got.tobytes() == ref["info"].tobytes()
        exact &= st[p, :n1k].tobytes() == ref["status"].tobytes()
        has = np.isin(ref["status"], (2, 5, 6, 7, 8, 9, 10))
        exact &= xs[p, :n1k][has].tobytes() == ref["x3d"][has].tobytes()
        exact &= pt[lo:hi].tobytes() == ref["points"].tobytes()
    n_match = [int((c.match12 >= 0).sum()) for c in cases]
    return {"config": "N1", "library": str(orb.LIB_PATH),
            "workload": f"CreateNewMapPoints, {P} keyframe pairs x {int(np.mean(n_match))} matches "
                        f"on average ({min(n_match)}-{max(n_match)}), {S} keypoint slots, stereo "
                        f"keyframes (60 % stereo keypoints), 12 % gross outliers",
            "create_ms": t_batch, "create_serial_ms": t_serial,
            "create_serial_over_batch": t_serial["median"] / t_batch["median"],
            "median_depth_ms": t_median, "n_new_mean": float(inf["n_new"].mean()),
            "n_new_total": int(inf["n_new"].sum()), "gated": int(inf["gated"].sum()),
            "status_counts": inf["counts"].sum(0).tolist(),
            "max_stride": orb.ORBmatcher.create_new_map_points_max_stride(),
            "kernel_resources": "k_new_points: 167 VGPRs, 106 SGPRs, no scratch, occupancy 3 "
                                "waves/SIMD (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)",
            "exact_vs_restatement": bool(exact)}


def g1(args, orb, oracle, torch):
    import scenarios as S
    import tri_batch_ref as T
    P = 64
    probs = []
    for i in range(P):
        k0, k1 = S.keyframe_pair(oracle, 3 + i, rng_seed=1 + i, baseline=(0.5, 0.0, 0.1))
        rng = np.random.default_rng(16 + i)
        frac = 0.5 if i % 2 else 0.0       # a fresh keyframe, and one half covered with points
        pidx = [np.where(rng.random(len(k["keys"])) < frac, np.arange(len(k["keys"])), -1)
                .astype(np.int32) for k in (k0, k1)]
        probs.append(T.from_keyframes(oracle, k0, k1, *pidx))
        host = (S.camera(), k1["scale"], k1["sigma2"])
    sides = [s for q in probs for s in q[:2]]
    f12 = np.stack([q[2] for q in probs]).astype(np.float32)
    stride = max(len(s["desc"]) for s in sides)
    arr = T.pack_slots(sides, stride)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d = {k: dev(v) for k, v in arr.items()}
    s1, s2 = dev(np.arange(0, 2 * P, 2, dtype=np.int32)), dev(np.arange(1, 2 * P, 2, dtype=np.int32))
    d_f12 = dev(f12)
    m12 = torch.full((P * stride,), -7, dtype=torch.int32, device="cuda")
    info = torch.zeros(P * 6, dtype=torch.int32, device="cuda")
    m = orb.ORBmatcher(0.6, True)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def batch(n=P):
        m.search_for_triangulation_batch(
            n, s1.data_ptr(), s2.data_ptr(), d["keys"].data_ptr(), d["desc"].data_ptr(),
            d["nkeys"].data_ptr(), d["pidx"].data_ptr(), d["fv_nodes"].data_ptr(),
            d["fv_offs"].data_ptr(), d["fv_feats"].data_ptr(), d["n_fv_nodes"].data_ptr(),
            d["u_right"].data_ptr(), d["pose"].data_ptr(), stride, d_f12.data_ptr(), host[0],
            host[1], host[2], False, m12.data_ptr(), info.data_ptr(), sp)

    def events(fn, reps=20):
        t = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        t.sort()
        return {"median": t[len(t) // 2], "min": t[0], "max": t[-1]}

    frames = [(orb.Frame(a["keys"], a["desc"], host[1], 1241, 376, u_right=a["u_right"]),
               (a["pidx"] >= 0).astype(np.uint8),
               orb.Frame(b["keys"], b["desc"], host[1], 1241, 376, u_right=b["u_right"]),
               (b["pidx"] >= 0).astype(np.uint8), a, b, f) for a, b, f in probs]

    def one(p):
        fa, ha, fb, hb, a, b, f = frames[p]
        return m.SearchForTriangulation(fa, ha, fb, hb, host[2], f, host[0], a["pose"]["ow"],
                                        b["pose"]["rcw"], b["pose"]["tcw"], a["fv"], b["fv"], False)

    def serial(reps=20):
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p in range(P):
                one(p)
            t.append((time.perf_counter() - t0) * 1e3)   # every call ends in a synchronise
        t.sort()
        return {"median": t[len(t) // 2], "min": t[0], "max": t[-1]}

    for _ in range(3):
        batch()
        one(0)
    torch.cuda.synchronize()
    t_batch = {n: events(lambda n=n: batch(n)) for n in (P, 16, 1)}
    t_serial = serial()
    batch()
    torch.cuda.synchronize()
    rows = m12.cpu().numpy().reshape(P, stride)
    inf = info.cpu().numpy().view(T.INFO_DTYPE)
    exact = True
    for p in (0, 1, P // 2, P - 1):
        row, want = T.expected(oracle, *probs[p], *host, False, True)
        exact &= np.array_equal(rows[p, :len(row)], row) and tuple(inf[p]) == want
        n, r1 = one(p)
        exact &= n == want[0] and np.array_equal(r1, row)
    nk = [len(s["desc"]) for s in sides]
    return {"config": "G1", "library": str(orb.LIB_PATH),
            "workload": f"SearchForTriangulation, {P} keyframe pairs of {min(nk)}-{max(nk)} "
                        f"keypoints ({stride} slots), natural FeatureVectors "
                        f"({int(np.mean([len(s['fv'][0]) for s in sides]))} nodes on average), "
                        f"has_mp 0 % / 50 % alternating, orientation on",
            "batch_ms": t_batch[P], "batch16_ms": t_batch[16], "batch1_ms": t_batch[1],
            "one_per_call_ms": t_serial,
            "one_per_call_over_batch": t_serial["median"] / t_batch[P]["median"],
            "timing": "batch: device events around the one launch, median of 20; one per call: "
                      "host clock around 64 blocking orb_search_for_triangulation calls (14 "
                      "uploads and 2 downloads each), median of 20; the has_mp downloads and the "
                      "match12 upload of the integrator's loop are not in it",
            "n_matches_mean": float(inf["n_matches"].mean()),
            "n_matches_range": [int(inf["n_matches"].min()), int(inf["n_matches"].max())],
            "n_tried_mean": float(inf["n_tried"].mean()),
            "n_shared2_mean": float(inf["n_shared2"].mean()),
            "max_stride": orb.ORBmatcher.search_for_triangulation_batch_max_stride(),
            "kernel_resources": "k_tri_batch: 48 VGPRs, 96 SGPRs, no spill, ScratchSize 0, "
                                "occupancy 8 waves/SIMD, 544 B static LDS (hipcc "
                                "-Rpass-analysis=kernel-resource-usage, gfx950)",
            "exact_vs_oracle_and_one_problem_entry": bool(exact)}


def l1(args, orb, oracle, torch):
    """ComputeSim3's matchers as device batches: 64 loop candidates against one
    current keyframe.  With ORB_AMD_LIB naming a build without the batches only
    the one-problem entries are timed (the baseline side of the comparison)."""
    import sim3_chain_ref as R
    import scenarios as S
    import tri_batch_ref as T
    P = 64
    (s1, base2), pts0, md0, host, _ = R.loop_scene(oracle, nf=1000)
    n = len(base2["desc"])
    sides, points, mp_desc = [s1], [pts0[:n]], [md0[:n]]
    for i in range(P):      # the candidate's view of the scene: its own descriptors and points
        rng = np.random.default_rng(100 + i)
        bits = np.unpackbits(base2["desc"], axis=1) ^ (rng.random((n, 256)) < 0.02)
        desc = np.packbits(bits.astype(np.uint8), axis=1)
        pidx = np.where(base2["pidx"] >= 0, base2["pidx"] + n * i, -1).astype(np.int32)
        s = dict(base2, desc=desc, pidx=pidx, fv=tuple(oracle.feature_vector(S.vocab_nodes(desc))))
        sides.append(s)
        points.append(pts0[n:])
        mp_desc.append(md0[n:])
    points, mp_desc = np.concatenate(points), np.concatenate(mp_desc)
    stride = n
    arr = T.pack_slots(sides, stride, with_u_right=False)
    m = orb.ORBmatcher(0.75, True)
    cam, bounds = host["cam"], (0.0, float(host["width"]), 0.0, float(host["height"]))

    def serial(fn, reps=20):
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p in range(P):
                fn(p)
            t.append((time.perf_counter() - t0) * 1e3)   # every call ends in a synchronise
        t.sort()
        return {"median": t[len(t) // 2], "min": t[0], "max": t[-1]}

    bad = [R._bad_of(s["pidx"], points) for s in sides]
    rows = [R.bow_kf_expected(oracle, s1, sides[1 + p], points, 0.75, True, 20) for p in range(P)]
    exact_rec = R.sim3_record(s=1.1)
    kfs = []
    for p in range(P):
        a1, a2 = R.already_masks(rows[p][0], rows[p][1], n)
        k1 = R.kf_dict(s1, points, mp_desc, a1, host)
        k2 = R.kf_dict(sides[1 + p], points, mp_desc, a2, host)
        fr = lambda k: orb.Frame(k["keys"], k["desc"], k["scale"], k["width"], k["height"])
        kfs.append((fr(k1), fr(k2), k1, k2))

    def one_bow(p):
        s2 = sides[1 + p]
        return m.SearchByBoWKF(s1["desc"], s1["angle"], s1["pidx"], bad[0], s1["fv"], s2["desc"],
                               s2["angle"], s2["pidx"], bad[1 + p], s2["fv"])

    def one_sim3(p):
        f1, f2, k1, k2 = kfs[p]
        return m.SearchBySim3(f1, f2, float(host["log_scale"]), cam, k1["Rw"], k1["tw"], k2["Rw"],
                              k2["tw"], k1["mps"], k1["valid"], k1["already"], k1["mp_desc"],
                              k2["mps"], k2["valid"], k2["already"], k2["mp_desc"], 1.1,
                              exact_rec["R"].reshape(3, 3), exact_rec["t"], 7.5)

    for _ in range(3):
        one_bow(0), one_sim3(0)
    lib_path = Path(orb.LIB_PATH).resolve()
    out = {"config": "L1",
           "library": str(lib_path.relative_to(ROOT)) if ROOT in lib_path.parents else lib_path.name,
           "workload": f"ComputeSim3's matchers, {P} loop candidates against one current keyframe, "
                       f"{n} keypoints per slot, natural FeatureVectors (scenarios.vocab_nodes), "
                       f"scale drift 1.1, th 7.5",
           "bow_kf_one_per_call_ms": serial(one_bow), "search_by_sim3_one_per_call_ms": serial(one_sim3),
           "timing": "one per call: host clock around 64 blocking orb_match_bow_kf / "
                     "orb_search_by_sim3 calls, median of 20; batches: device events around each "
                     "launch, median of 20"}
    def write(key):
        """profiles/sim3chain_L1.json holds both runs: this build's and, from a run
        with ORB_AMD_LIB naming a build without the batches, the baseline's."""
        path = ROOT / "profiles" / "sim3chain_L1.json"
        both = json.loads(path.read_text()) if path.exists() else {}
        both[key] = out
        path.parent.mkdir(exist_ok=True)
        path.write_text(json.dumps({k: both[k] for k in ("this_build", "parent_build")
                                    if k in both}, indent=1) + "\n")
        return out

    if not hasattr(orb.lib(), "orb_match_bow_kf_batch"):
        return write("parent_build")

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d = {k: dev(v) for k, v in arr.items() if v is not None}
    p_ = lambda t: t.data_ptr()
    k1s, k2s = dev(np.zeros(P, np.int32)), dev(np.arange(1, P + 1, dtype=np.int32))
    dpts, ddesc = dev(points), dev(mp_desc)
    draws = dev(np.random.default_rng(1).integers(0, 2147483648, (P, 900)).astype(np.uint32))
    zeros = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    m12, ix2, new12 = zeros(P * stride * 4), zeros(P * stride * 4), zeros(P * stride * 4)
    binfo, sinfo = zeros(P * 20), zeros(P * 20)
    state, corr = zeros(P * orb.SIM3_STATE_DTYPE.itemsize), zeros(P * stride * orb.SIM3_CORR_DTYPE.itemsize)
    res, inl = zeros(P * orb.SIM3_RESULT_DTYPE.itemsize), zeros(P * stride)
    opt = zeros(P * orb.SIM3_OPT_RESULT_DTYPE.itemsize)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def bow(k=P):
        m.search_by_bow_kf_batch(k, p_(k1s), p_(k2s), p_(d["keys"]), p_(d["desc"]), p_(d["nkeys"]),
                                 p_(d["pidx"]), p_(d["fv_nodes"]), p_(d["fv_offs"]), p_(d["fv_feats"]),
                                 p_(d["n_fv_nodes"]), stride, p_(dpts), 20, p_(m12), p_(ix2),
                                 p_(binfo), stream=sp)

    def setup():
        m.sim3_solver_setup_batch(P, p_(k1s), p_(k2s), p_(d["keys"]), p_(d["nkeys"]), p_(d["pidx"]),
                                  p_(d["pose"]), stride, p_(dpts), p_(m12), 0, p_(ix2), host["sigma2"],
                                  cam, cam, False, p_(state), p_(corr), stream=sp)

    def iterate():
        m.sim3_solver_iterate_batch(P, stride, p_(state), p_(corr), p_(draws), 900, 5, p_(inl),
                                    p_(res), stream=sp)

    def search(k=P):
        m.search_by_sim3_batch(k, p_(k1s), p_(k2s), p_(d["keys"]), p_(d["desc"]), p_(d["nkeys"]),
                               p_(d["pidx"]), p_(d["pose"]), stride, p_(dpts), p_(ddesc), p_(m12),
                               p_(ix2), p_(inl), p_(res), cam, bounds, host["scale"],
                               float(host["log_scale"]), p_(sinfo), th=7.5, d_new12=p_(new12),
                               stream=sp)

    def optimise():
        m.optimize_sim3_batch(P, p_(k1s), p_(k2s), p_(d["keys"]), p_(d["nkeys"]), p_(d["pidx"]),
                              p_(d["pose"]), stride, p_(dpts), p_(m12), p_(ix2), p_(res),
                              host["inv_sigma2"], cam, cam, p_(opt), th2=10.0, fix_scale=False,
                              stream=sp)

    def prep():             # the state a round starts from: BoW rows, a fresh solver, one iterate
        bow(), setup(), iterate()

    def events(before, fn, reps=20):
        t = []
        for _ in range(reps):
            before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        t.sort()
        return {"median": t[len(t) // 2], "min": t[0], "max": t[-1]}

    for _ in range(3):
        prep(), search(), optimise()
    torch.cuda.synchronize()
    for k in (P, 16, 1):
        tag = "" if k == P else str(k)
        out[f"bow_kf_batch{tag}_ms"] = events(lambda: None, lambda k=k: bow(k))
        out[f"search_by_sim3_batch{tag}_ms"] = events(prep, lambda k=k: search(k))
    out["round_ms"] = events(lambda: (bow(), setup()), lambda: (iterate(), search(), optimise()))
    out["bow_kf_one_per_call_over_batch"] = \
        out["bow_kf_one_per_call_ms"]["median"] / out["bow_kf_batch_ms"]["median"]
    out["search_by_sim3_one_per_call_over_batch"] = \
        out["search_by_sim3_one_per_call_ms"]["median"] / out["search_by_sim3_batch_ms"]["median"]
    # exact check of four problems: the BoW rows, then the search on the device's own Sim3
    prep()
    torch.cuda.synchronize()
    host_of = lambda t, dt: t.cpu().numpy().view(dt)
    g12, gx2 = (host_of(t, np.int32).reshape(P, stride).copy() for t in (m12, ix2))
    gres = host_of(res, R.SIM3_RESULT_DTYPE).copy()
    ginl = host_of(inl, np.uint8).reshape(P, stride).copy()
    search()
    torch.cuda.synchronize()
    a12, ax2 = (host_of(t, np.int32).reshape(P, stride) for t in (m12, ix2))
    gs = host_of(sinfo, R.SEARCH_INFO_DTYPE)
    gb = host_of(binfo, R.B.INFO_DTYPE)
    exact = True
    for p in (0, 1, P // 2, P - 1):
        exact &= np.array_equal(g12[p], rows[p][0]) and np.array_equal(gx2[p], rows[p][1])
        exact &= tuple(int(v) for v in gb[p]) == rows[p][2]
        if gres[p]["has_sim3"]:
            want = R.sim3_expected(oracle, s1, sides[1 + p], points, mp_desc, g12[p], gx2[p],
                                   ginl[p], gres[p], host)
            exact &= np.array_equal(a12[p], want[0]) and np.array_equal(ax2[p], want[1])
            exact &= tuple(int(v) for v in gs[p]) == want[3]
    out.update(n_bow_matches_mean=float(gb["n_matches"].mean()),
               n_with_sim3=int(gres["has_sim3"].sum()),
               n_found_mean=float(gs["n_found"][gres["has_sim3"] != 0].mean()),
               max_stride_bow_kf=orb.match_bow_kf_batch_max_stride(),
               max_stride_search_by_sim3=orb.search_by_sim3_batch_max_stride(),
               kernel_resources="k_bow_kf_batch: 46 VGPRs, 96 SGPRs, ScratchSize 16 B/lane, "
                                "occupancy 8 waves/SIMD, 416 B static LDS; k_sim3_search_batch: "
                                "59 VGPRs, 106 SGPRs, ScratchSize 0, occupancy 7 waves/SIMD, 640 B "
                                "static LDS (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)",
               exact_vs_oracle=bool(exact))
    return write("this_build")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1,C2,C3,C5")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--cpu-seconds", type=float, default=6.0)
    args = ap.parse_args()
    import torch
    import oracle

    orb = bench.load_package()
    for c in args.configs.split(","):
        if c == "C1":
            r = c1(args, orb, oracle)
        elif c == "C2":
            r = c2(args, orb, oracle, torch)
        elif c == "C3":
            r = c3(args, orb, oracle, torch)
        elif c == "C5":
            r = c5(args, orb, oracle, torch)
        elif c == "C4M":
            r = c4m(args, orb, oracle, torch)
        elif c == "F1":
            r = f1(args, orb, oracle, torch)
        elif c == "F2":
            r = f2(args, orb, oracle, torch)
        elif c == "F3":
            r = f3(args, orb, oracle, torch)
        elif c == "P1":
            r = p1(args, orb, oracle, torch)
        elif c == "R1":
            r = r1(args, orb, oracle, torch)
        elif c == "T1":
            r = t1(args, orb, oracle, torch)
        elif c == "M1":
            r = m1(args, orb, oracle, torch)
        elif c == "B1":
            r = b1(args, orb, oracle, torch)
        elif c == "S1":
            r = s1(args, orb, oracle, torch)
        elif c == "O1":
            r = o1(args, orb, oracle, torch)
        elif c == "N1":
            r = n1(args, orb, oracle, torch)
        elif c == "G1":
            r = g1(args, orb, oracle, torch)
        elif c == "L1":
            r = l1(args, orb, oracle, torch)
        else:
            raise SystemExit(f"unknown config {c}")
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
