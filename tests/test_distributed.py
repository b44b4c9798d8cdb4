"""bench.py's multi-GPU plumbing (frame sharding, keypoint-count all-gather,
max-over-ranks timing) on world_size 2 with the gloo backend on CPU."""
import os
import socket

import pytest

torch = pytest.importorskip("torch")
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    import bench

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    B = 4
    frames = bench.shard_frames(rank, B)
    counts = torch.tensor([1000 + f for f in frames], dtype=torch.int32)
    out = torch.zeros(world * B, dtype=torch.int32)
    bench.gather_counts(dist, counts, out)
    t = bench.max_over_ranks(dist, 1.0 + rank, "cpu")
    q.put((rank, frames, out.tolist(), t))
    dist.destroy_process_group()


def test_bench_distributed_plumbing_gloo():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    all_frames = res[0][1] + res[1][1]
    assert sorted(all_frames) == list(range(8))  # disjoint, complete shards
    for _, _, gathered, t in res:
        assert gathered == [1000 + f for f in range(8)]
        assert t == 2.0  # slowest rank's time


def test_bench_gpus_flag_world_resolution():
    """`--gpus` against the launcher's env: a mismatch with WORLD_SIZE fails
    loudly; --gpus > 1 from a plain shell asks for child ranks."""
    import bench

    assert bench.resolve_world(None, {}) == (1, False)
    assert bench.resolve_world(1, {}) == (1, False)
    assert bench.resolve_world(8, {}) == (8, True)
    assert bench.resolve_world(None, {"WORLD_SIZE": "4"}) == (4, False)
    assert bench.resolve_world(4, {"WORLD_SIZE": "4"}) == (4, False)
    with pytest.raises(SystemExit):
        bench.resolve_world(8, {"WORLD_SIZE": "1"})
    with pytest.raises(SystemExit):
        bench.resolve_world(0, {})


def test_bench_gpus_mismatch_exits_nonzero():
    """A rank whose WORLD_SIZE differs from --gpus exits non-zero before it
    touches a device (it never measures one GPU under an N-GPU label)."""
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "2"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr


def test_bench_dump_outputs_sample(tmp_path, orb):
    """--dump-outputs: float32 arrays of the last step's resident launches, the
    same fixed sample on every call, rows past a frame's count blanked."""
    import numpy as np

    import bench

    B, cap, NS, NB = 96, 37, 4, 8
    rng = np.random.default_rng(1)
    sets = []
    for _ in range(NS):
        k = np.zeros((B, cap), orb.KEYPOINT_DTYPE)
        k["x"], k["octave"], k["class_id"] = rng.random((B, cap)), rng.integers(0, 8, (B, cap)), -1
        sets.append(dict(kps=torch.from_numpy(k.view(np.int32).reshape(B, cap, 7)),
                         desc=torch.from_numpy(rng.integers(1, 256, (B, cap, 32), dtype=np.uint8)),
                         cnt=torch.from_numpy(rng.integers(0, cap + 1, B).astype(np.int32)),
                         match=torch.from_numpy(rng.integers(0, 5000, (B, cap)).astype(np.int32)),
                         nmatch=torch.from_numpy(rng.integers(0, cap, B).astype(np.int32))))
    counts = torch.arange(B * NB, dtype=torch.int32)
    g_end = 3 * NB  # three steps of NB launches: launches 20..23 are resident (batches 4..7)
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, sets, counts, g_end, NS, NB, B, orb, torch, 0, 7)
    a = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert set(a) == {"keypoint_counts", "sample_frames", "keypoints", "descriptors", "kp_match",
                      "nmatches"}
    for name, arr in a.items():
        assert arr.dtype == np.float32 and np.array_equal(arr, np.load(tmp_path / "b" / f"{name}.npy"))
    assert sum(arr.nbytes for arr in a.values()) <= 64 << 20
    n = min(bench.DUMP_FRAMES, NS * B)
    assert a["keypoint_counts"].tolist() == list(range(B * NB))
    assert a["keypoints"].shape == (n, cap, 7) and a["descriptors"].shape == (n, cap, 32)
    assert a["kp_match"].shape == (n, cap) and a["nmatches"].shape == (n,)
    f = a["sample_frames"].astype(int)
    assert len(set(f)) == n and f.min() >= 4 * B and f.max() < 8 * B
    for row, fr in enumerate(f):  # each row is that frame's buffer row, cut at its count
        st, i = sets[(fr // B) % NS], fr % B
        c = int(st["cnt"][i])
        assert a["nmatches"][row] == int(st["nmatch"][i])
        assert np.array_equal(a["descriptors"][row, :c], st["desc"][i, :c].numpy().astype(np.float32))
        assert np.array_equal(a["kp_match"][row, :c], st["match"][i, :c].numpy().astype(np.float32))
        k = st["kps"][i].numpy().view(orb.KEYPOINT_DTYPE)[:, 0]
        assert np.array_equal(a["keypoints"][row, :c, 0], k["x"][:c])
        assert np.array_equal(a["keypoints"][row, :c, 5], k["octave"][:c].astype(np.float32))
        assert not a["descriptors"][row, c:].any() and not a["keypoints"][row, c:].any()
        assert (a["kp_match"][row, c:] == -1).all()
