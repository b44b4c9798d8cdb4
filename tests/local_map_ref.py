"""Tracking::UpdateLocalMap restated in Python, literally: UpdateLocalKeyFrames
(src/Tracking.cc:1437-1558), UpdateLocalPoints (:1407-1434) and the first loop
of SearchLocalPoints (:1333-1354), over the arrays orb_map_view_t holds, plus
the two tails of TrackLocalMap (merge, finish :1109-1135).

std::map<KeyFrame*, int> and std::set<KeyFrame*> iterate in pointer order:
here, in `rank` order.  A map is a dict

    rank, bad, parent           per keyframe (int arrays)
    cov, child, kf_mp           per keyframe a list (best-first covisibles,
                                children in any order, map point per keypoint)
    obs                         per map point the keyframes observing it
    points, desc                MAP_POINT_DTYPE records and n_mp x 32 bytes

`rules` switches ONE reference rule to a wrong neighbour (RULES); the directed
inputs of tests/local_map_cases.py are built so that each switch changes a
named input's answer.
"""
from collections import Counter

import numpy as np

MAP_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"),
                            ("max_distance", "<f4"), ("bad", "u1"), ("seen", "u1"),
                            ("has_obs", "u1"), ("_pad", "u1")])
INFO_DTYPE = np.dtype([("n_local_kf", "<i4"), ("n_voted", "<i4"), ("n_added", "<i4"),
                       ("ref_kf", "<i4"), ("max_votes", "<i4"), ("n_local_points", "<i4"),
                       ("n_nulled", "<i4"), ("kept", "<i4")])

RULES = ("index_order", "max_ge", "neigh11", "limit_ge80", "no_parent_break", "parent_bad_check",
         "neigh_continue", "child_list_order", "clear_on_empty", "last_occurrence",
         "seen_from_map")


def update_local_keyframes(m, kp_match, local_kf, rules=(), ev=None):
    """:1437-1558.  kp_match (modified in place) and local_kf (a list, the
    previous frame's) -> (local_kf, info dict)."""
    ev = ev if ev is not None else Counter()
    rank, bad, parent = m["rank"], m["bad"], m["parent"]
    pts = m["points"]
    info = dict(n_voted=0, n_added=0, ref_kf=-1, max_votes=0, n_nulled=0, kept=0)
    # Each map point votes for the keyframes in which it has been observed (:1440-1460)
    counter = {}
    for i in range(len(kp_match)):
        pi = int(kp_match[i])
        if pi >= 0:                                   # :1444 (any negative value is NULL)
            if not pts["bad"][pi]:                    # :1447
                if not pts["has_obs"][pi]:
                    ev["matched_no_obs"] += 1
                for kf in m["obs"][pi]:               # :1450-1453
                    counter[int(kf)] = counter.get(int(kf), 0) + 1
            else:
                kp_match[i] = -1                      # :1457
                info["n_nulled"] += 1
        elif pi < -1:
            ev["minus2"] += 1
    info["n_voted"] = len(counter)
    if not counter:                                   # :1462
        if "clear_on_empty" in rules:
            return [], info
        info["kept"] = 1
        if len(local_kf):
            ev["stale_list_kept"] += 1
        return list(local_kf), info

    mx, kfmax = 0, -1                                 # :1465-1466
    local_kf = []                                     # :1468
    included = set()                                  # mnTrackReferenceForFrame == mnId
    order = sorted(counter) if "index_order" in rules else sorted(counter, key=lambda k: rank[k])
    for kf in order:                                  # :1472
        if bad[kf]:                                   # :1477
            continue
        c = counter[kf]
        if (c >= mx) if "max_ge" in rules else (c > mx):   # :1480
            mx, kfmax = c, kf
        local_kf.append(kf)                           # :1486
        included.add(kf)                              # :1488
    if not local_kf:
        ev["all_voted_bad"] += 1
    else:
        top = [k for k in local_kf if counter[k] == max(counter[k] for k in local_kf)]
        if len(top) > 1 and min(top) != min(top, key=lambda k: rank[k]):
            ev["max_tie_rank_vs_index"] += 1
    ev["n_voted_good"] = len(local_kf)

    # Include also some not-already-included keyframes that are neighbours (:1494-1550)
    n_voted_good = len(local_kf)                      # itEndKF is taken before any push
    n_neigh = 11 if "neigh11" in rules else 10
    added_now = set()
    for j in range(n_voted_good):
        if (len(local_kf) >= 80) if "limit_ge80" in rules else (len(local_kf) > 80):  # :1498
            ev["over80_break"] += 1
            break
        kf = local_kf[j]
        neighs = m["cov"][kf][:n_neigh]               # GetBestCovisibilityKeyFrames(10) (:1503)
        for q, nb in enumerate(neighs):               # :1505
            nb = int(nb)
            if not bad[nb]:                           # :1508
                if nb not in included:                # :1511
                    local_kf.append(nb)               # :1514
                    included.add(nb)
                    added_now.add(nb)
                    if "neigh_continue" in rules:
                        continue
                    break                             # :1517
                elif nb in added_now:
                    ev["neigh_already_added"] += 1
            else:
                ev["neigh_bad_skipped"] += 1
        else:
            cov = m["cov"][kf]
            if len(cov) > 10 and any(not bad[int(x)] and int(x) not in included for x in cov[10:11]):
                ev["neigh_11th_only"] += 1
        childs = list(m["child"][kf])                 # std::set<KeyFrame*> (:1522)
        if "child_list_order" not in rules:
            childs = sorted(childs, key=lambda k: rank[k])
        ok = [int(c) for c in m["child"][kf] if not bad[int(c)] and int(c) not in included]
        if len(ok) > 1 and ok[0] != min(ok, key=lambda k: rank[k]):
            ev["child_multi"] += 1
        if len(m["child"][kf]) > 16:
            ev["children_over_16"] += 1
        for ch in childs:                             # :1523
            ch = int(ch)
            if not bad[ch]:                           # :1526
                if ch not in included:                # :1528
                    local_kf.append(ch)               # :1531
                    included.add(ch)
                    added_now.add(ch)
                    break                             # :1533
        par = int(parent[kf])                         # :1538
        if par >= 0:                                  # :1539
            if par not in included:                   # :1541
                if "parent_bad_check" in rules and bad[par]:
                    continue
                if bad[par]:
                    ev["parent_bad_added"] += 1
                local_kf.append(par)                  # :1544
                included.add(par)
                added_now.add(par)
                if "no_parent_break" in rules:
                    continue
                if j + 1 < n_voted_good:
                    ev["parent_break_unvisited"] += 1
                break                                 # :1546 leaves the outer loop
            else:
                ev["parent_included_nobreak"] += 1
    info["n_added"] = len(local_kf) - n_voted_good
    info["ref_kf"] = kfmax                            # :1552-1557
    info["max_votes"] = mx
    return local_kf, info


def update_local_points(m, local_kf, rules=(), ev=None):
    """:1407-1434: the indices of mvpLocalMapPoints in order."""
    ev = ev if ev is not None else Counter()
    pts = m["points"]
    slots = []
    for kf in local_kf:                               # :1412
        mps = m["kf_mp"][kf]                          # :1416
        if len(mps) == 0:
            ev["kf_no_points"] += 1
        slots.extend(int(x) for x in mps)
        ids = [int(x) for x in mps if x >= 0]
        if len(set(ids)) < len(ids):
            ev["dup_within"] += 1
    if "last_occurrence" in rules:
        slots = slots[::-1]
    out, taken = [], set()
    for pi in slots:                                  # :1418
        if pi < 0:                                    # :1421
            ev["neg_slots"] += 1
            continue
        if pi in taken:                               # :1424
            ev["dup"] += 1
            continue
        if not pts["bad"][pi]:                        # :1426
            out.append(pi)                            # :1428
            taken.add(pi)                             # :1430
        else:
            ev["bad_points_skipped"] += 1
    if "last_occurrence" in rules:
        out = out[::-1]
    ev["distinct_ids"] = len({s for s in slots if s >= 0})
    ev["slot_total"] = len(slots)
    return out


def update_local_map(m, kp_match, local_kf, mp_stride, rules=(), ev=None):
    """The entry's outputs for one problem, as a dict of numpy arrays: kp_match
    (after the nulling), local_kf, local_index / mps / desc (the first
    min(count, mp_stride) local points), locked and info."""
    ev = ev if ev is not None else Counter()
    km = np.array(kp_match, np.int32)
    kfs, info = update_local_keyframes(m, km, [int(k) for k in local_kf], rules, ev)
    idx = update_local_points(m, kfs, rules, ev)
    pts = m["points"]
    held = {int(pi) for pi in km if pi >= 0}          # :1333-1354 after the nulling
    n = min(len(idx), mp_stride)
    if len(idx) > mp_stride:
        ev["over_mp_stride"] += 1
    sel = np.array(idx[:n], np.int64)
    mps = pts[sel].copy() if n else np.zeros(0, MAP_POINT_DTYPE)
    if "seen_from_map" not in rules and n:
        mps["seen"] = [1 if int(pi) in held else 0 for pi in sel]
    ev["seen_local"] = int(sum(1 for pi in idx if pi in held))
    ev["map_seen_differs"] = int(sum(1 for pi in idx if bool(pts["seen"][pi]) != (pi in held)))
    desc = m["desc"][sel] if n else np.zeros((0, 32), np.uint8)
    locked = np.array([1 if pi >= 0 and pts["has_obs"][pi] else 0 for pi in km], np.uint8)
    rec = np.zeros((), INFO_DTYPE)
    rec["n_local_kf"] = len(kfs)
    rec["n_local_points"] = len(idx)
    for k, v in info.items():
        rec[k] = v
    ev["n_local_points"] = len(idx)
    ev["matched_bad_nulled"] = int(info["n_nulled"])
    return dict(kp_match=km, local_kf=np.array(kfs, np.int32), local_index=sel.astype(np.int32),
                mps=mps, desc=np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), locked=locked,
                info=rec, n_local_points=len(idx))


def census(inp, mp_stride=1 << 30):
    """Counts of the conditions an input exercises (a Counter)."""
    ev = Counter()
    update_local_map(inp["map"], inp["kp_match"], inp["local_kf"], mp_stride, (), ev)
    return ev


def merge(kp_match, km_local, local_index):
    """F.mvpMapPoints[bestIdx] = pMP of the local matcher, as global indices."""
    out = np.array(kp_match, np.int32)
    for i, l in enumerate(km_local):
        if l >= 0:
            out[i] = local_index[l]
    return out


def finish(kp_match, outlier, points, only_tracking, null_outliers):
    """src/Tracking.cc:1109-1135 -> (mnMatchesInliers, kp_match)."""
    out = np.array(kp_match, np.int32)
    inliers = 0
    for i in range(len(out)):                         # :1112
        if out[i] >= 0:                               # :1114
            if not outlier[i]:                        # :1116
                if not only_tracking:                 # :1120
                    if points["has_obs"][out[i]]:     # :1123
                        inliers += 1
                else:
                    inliers += 1                      # :1129
            elif null_outliers:                       # :1131
                out[i] = -1
    return inliers, out
