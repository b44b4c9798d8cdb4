#!/usr/bin/env python3
"""Rounds of the prefix resolve (k_proj_resolve<NW>) per problem, on the CPU.

The kernel's schedule is replayed over the candidate lists of a problem: a
window of W = 64 * NW points is evaluated against the committed locks, every
locking accept claims its keypoint, a point is in conflict when an earlier
point of the window claims a keypoint among the top-K entries it looked at,
the longest conflict-free prefix is committed, and a point whose top-K ran dry
is re-scanned alone once it is first in its window.  The replay's assignment
is checked against the oracle's, so the count belongs to the exact schedule.

As a script it prints, for the bench's own frames and maps (1241x376, 1000
features, 5,000 points), the rounds, the input-ring slides (one per W points)
and the commit sizes:

    python tools/attribution/resolve_rounds.py [--frames 8] [--nw 1]
"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
TOPK, TH_HIGH = 4, 100


def candidate_lists(o, keys, desc, scale, width, height, mps, mpd, th, locked=None):
    """Per map point the candidates of k_proj_candidates in scan order
    (keypoint, distance, octave), or None for a point that is not searched."""
    cs, idx = o.grid(keys, width, height)
    rank = np.full(len(keys), len(keys), np.int64)
    rank[idx] = np.arange(len(idx))
    bits = np.unpackbits(np.ascontiguousarray(desc, np.uint8), axis=1).astype(np.int16)
    mbits = np.unpackbits(np.ascontiguousarray(mpd, np.uint8), axis=1).astype(np.int16)
    free = np.ones(len(keys), bool) if locked is None else np.asarray(locked) == 0
    free &= rank < len(keys)
    kx, ky, ko = keys["x"], keys["y"], keys["octave"]
    out = []
    for i, mp in enumerate(mps):
        if not mp["in_view"] or mp["bad"]:
            out.append(None)
            continue
        lvl = int(mp["level"])
        r = np.float32(2.5) if float(mp["view_cos"]) > 0.998 else np.float32(4.0)
        if th != 1.0:
            r = r * np.float32(th)
        rs = np.float32(r * np.float32(scale[lvl]))
        c = np.nonzero(free & (ko >= lvl - 1) & (ko <= lvl) & (np.abs(kx - mp["proj_x"]) < rs) &
                       (np.abs(ky - mp["proj_y"]) < rs))[0]
        c = c[np.argsort(rank[c], kind="stable")]
        dist = np.abs(bits[c] - mbits[i][None, :]).sum(1)
        out.append([(int(k), int(dd), int(ko[k])) for k, dd in zip(c, dist) if dd < 256])
    return out


def _decide(entries, taken, nnratio, limit):
    """The first two untaken of entries[:limit] in order: (keypoint or -1,
    entries looked at, untaken found)."""
    best = second = None
    looked = 0
    for e in entries[:limit]:
        if best is not None and second is not None:
            break
        looked += 1
        if taken[e[0]]:
            continue
        if best is None:
            best = e
        else:
            second = e
    found = (best is not None) + (second is not None)
    ok = best is not None and best[1] <= TH_HIGH and not (
        second is not None and best[2] == second[2] and
        np.float32(best[1]) > np.float32(nnratio) * np.float32(second[1]))
    return (best[0] if ok else -1), looked, found


def replay(cands, has_obs, nkeys, nnratio, nw=1):
    """-> (kp_match, nmatches, rounds, slow re-scans, commit sizes)."""
    W = 64 * nw
    M = len(cands)
    taken = np.zeros(nkeys, bool)
    km = np.full(nkeys, -1, np.int64)
    top = [None if c is None else sorted(c, key=lambda e: e[1])[:TOPK] for c in cands]  # stable
    nmatches = rounds = slows = 0
    commits = []
    start = 0
    while start < M:
        rounds += 1
        res = []
        claim = {}
        for m in range(start, min(start + W, M)):
            if not cands[m]:
                res.append((-1, 0, False))
                continue
            k, looked, found = _decide(top[m], taken, nnratio, TOPK)
            slow = len(cands[m]) > TOPK and found < 2
            if slow:
                k = -1
            res.append((k, looked, slow))
            if k >= 0 and has_obs[m]:
                claim.setdefault(k, m)
        if res[0][2]:  # exact re-scan of the window's first point
            slows += 1
            c = sorted(cands[start], key=lambda e: e[1])
            k, _, _ = _decide(c, taken, nnratio, len(c))
            if k >= 0:
                km[k] = max(km[k], start)
                taken[k] |= bool(has_obs[start])
                nmatches += 1
            commits.append(1)
            start += 1
            continue
        commit = len(res)
        for j, (k, looked, slow) in enumerate(res):
            m = start + j
            if slow or any(claim.get(e[0], M) < m for e in (top[m] or [])[:looked]):
                commit = j
                break
        for j in range(commit):
            k = res[j][0]
            if k >= 0:
                km[k] = max(km[k], start + j)
                taken[k] |= bool(has_obs[start + j])
                nmatches += 1
        commits.append(commit)
        start += commit
    return km, nmatches, rounds, slows, commits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--nw", type=int, default=1)
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle as o
    o.lib()
    w, h, nf, M, seed = 1241, 376, 1000, 5000, 0x4B495454  # bench.py
    scale = o.params(nf)["scale"]
    rows = []
    for f in range(a.frames):
        k, d, _ = o.extract(o.synth_image(seed, f, w, h), nf, 1.2, 8, 20, 7)
        mps, mpd, lk = o.synth_local_map(seed + f, k, d, M, w, h)
        n_ref, km_ref = o.match_projection_local(k, d, scale, w, h, mps, mpd, 1.0, 0.8, lk)
        cands = candidate_lists(o, k, d, scale, w, h, mps, mpd, 1.0, lk)
        km, n, rounds, slows, commits = replay(cands, mps["has_obs"], len(k), 0.8, a.nw)
        assert n == n_ref and np.array_equal(km, km_ref), f
        W = 64 * a.nw
        c = np.array(commits)
        rows.append((rounds, slows))
        print(f"frame {f}: keypoints {len(k)} matches {n} rounds {rounds} (full windows "
              f"{(c == W).sum()}, slow re-scans {slows}) slides {-(-M // W)} "
              f"mean commit {c.mean():.1f} median {np.median(c):.0f} min {c.min()}")
    r = np.array(rows)
    print(f"NW={a.nw}: rounds per problem mean {r[:, 0].mean():.1f} min {r[:, 0].min()} "
          f"max {r[:, 0].max()}; lower bound {-(-M // (64 * a.nw))}")


if __name__ == "__main__":
    main()
