"""Frame::ComputeStereoMatches on the GPU (k_stereo_rows, k_stereo_match2<16>,
k_stereo_prune) on the directed inputs of stereo_edge_cases.py, against the CPU
oracle: u_right and depth bit for bit, and on the batch entry point d_sad too.

Single pairs go through ORBmatcher.ComputeStereoMatches on one matcher shared
by the whole module: every input runs once, again after calls of other sizes
(the capacity input and a one-keypoint one), then once more, so that the row
lists, the SAD array and the staged pyramids meet stale contents.
test_stereo_edge_cases.py shows on the CPU that these inputs reach the kernels'
branches (census) and separate the reference's rules from their wrong
neighbours."""
import functools

import numpy as np
import pytest

import stereo_edge_cases as E

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(name):
    return E.CASES[name][0]()


@functools.lru_cache(maxsize=None)
def reference(name):
    import oracle as o
    o.lib()
    return E.run_oracle(o, case(name))


@pytest.fixture(scope="module")
def matcher(gpu):
    return gpu.ORBmatcher()


def _check(got, ref, what):
    for label, a, b in zip(("u_right", "depth"), got, ref):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), \
            (what, label, np.nonzero(a != b)[0][:10], a[a != b][:10], b[a != b][:10])


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_directed_input(gpu, matcher, name):
    c, ref = case(name), reference(name)
    E.check_expect(c, ref)
    _check(E.run_gpu(gpu, matcher, c), ref, name)
    for other in ("capacity", "tiny"):
        _check(E.run_gpu(gpu, matcher, case(other)), reference(other), other + " (in between)")
    _check(E.run_gpu(gpu, matcher, c), ref, name + " (after other sizes)")
    _check(E.run_gpu(gpu, matcher, c), ref, name + " (repeated)")


# ------------------------------------------------------------------ batch path
W, H, STRIDE = 380, 230, 40
BF, FX = E.KITTI


def _keys(rows):
    k = np.zeros(len(rows), E.KEYPOINT_DTYPE)
    for i, (x, y, octv) in enumerate(rows):
        k[i]["x"], k[i]["y"], k[i]["octave"] = x, y, octv
    k["size"] = 31.0
    return k


def _batch_pairs():
    """(left image, right image, left keys, left desc, right keys, right desc)
    per pair: directed level-0 images, directed keypoints.  Counts 1, 17, 0
    left, 0 right, the stride, 17; the empty ones in the middle."""
    rng = np.random.default_rng(5)
    x = np.arange(W)
    stripes = np.tile(((x & 1) * 255).astype(np.uint8), (H, 1))
    tri = np.tile((np.abs(((x - 100) % 32) - 16) * 8).astype(np.uint8), (H, 1))
    blocks = rng.integers(0, 256, (H // 2 + 1, W // 2 + 16), dtype=np.uint8)
    tex = np.kron(blocks, np.ones((2, 2), np.uint8))[:H]
    left_tex = tex[:, 12:12 + W].copy()
    right_tex = tex[:, 12 + 7:12 + 7 + W].astype(np.int16) + rng.integers(-3, 4, (H, W))
    right_tex = np.clip(right_tex, 0, 255).astype(np.uint8)     # left moved 7 columns, plus noise

    def descs(n, hd):
        dl = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        return dl, np.array([E.flip_bits(d, hd) for d in dl], np.uint8).reshape(n, 32)

    def textured(n):
        # levels 0..2 in turn; the right keypoint 7 columns to the left
        lk, rk = [], []
        for i in range(n):
            lvl = i % 3
            xs, ys = 40 + 13 * (i % 17), 16 + 9 * (i // 3)
            xl, yl = E.level0(lvl, xs), E.level0(lvl, ys)
            lk.append((xl, yl, lvl))
            rk.append((E.f32(xl - E.f32(7.0)), yl, lvl))
        dl, dr = descs(n, 11)
        return _keys(lk), dl, _keys(rk), dr

    pairs = []
    # stripes, left = right: five shifts tie at SAD 0, -4 wins; median 0 resets it
    dl, dr = descs(1, 7)
    pairs.append((stripes, stripes, _keys([(100.0, 30.0, 0)]), dl, _keys([(90.0, 30.0, 0)]), dr))
    # triangle wave, left = right, 17 keypoints on crests with the right one at
    # the same x: disparity 0 -> 0.01f.  One pixel of the centre column, off the
    # centre row, keeps the SADs symmetric in the shift and positive
    right = tri.copy()
    lk = []
    for j in range(17):
        cx, cy = 36 + 32 * (j % 10), 12 + 12 * j
        lk.append((float(cx), float(cy), 0))
        right[cy - 3, cx] += 20 + j
    dl, dr = descs(17, 9)
    pairs.append((tri, right, _keys(lk), dl, _keys(lk), dr))
    k = textured(12)
    pairs.append((left_tex, right_tex, k[0][:0], k[1][:0], k[2], k[3]))          # 0 left
    pairs.append((left_tex, right_tex, k[0], k[1], k[2][:0], k[3][:0]))          # 0 right
    pairs.append((left_tex, right_tex) + textured(STRIDE))                       # the stride
    pairs.append((left_tex, right_tex) + textured(17))
    return pairs


def test_batch_directed(gpu, oracle):
    """orb_stereo_match_batch with directed keypoints on the pyramids of two
    extractors' batches: u_right, depth and d_sad per pair against the oracle,
    and nothing written past a pair's count.  d_sad is the SAD of every match
    found, pruned ones included, and -1 where none (include/orb_abi.h)."""
    torch = pytest.importorskip("torch")
    pairs = _batch_pairs()
    P = len(pairs)
    p = oracle.params(1000)
    assert np.array_equal(p["scale"], E.SCALE) and np.array_equal(p["inv_scale"], E.INV)
    refs, n_reset = [], 0
    for (li, ri, lk, ld, rk, rd) in pairs:
        lp, rp = oracle.pyramid(li), oracle.pyramid(ri)
        c = dict(name="batch", lk=lk, ld=ld, rk=rk, rd=rd, lpyr=lp, rpyr=rp, bf=BF, fx=FX)
        E.check_domain(c)
        ref = oracle.stereo_match(lk, ld, E.SCALE, rk, rd, lp, rp, E.INV, BF, FX, W, H,
                                  with_sad=True)
        n_reset += int(((ref[2] >= 0) & (ref[0] < 0)).sum())
        refs.append(ref)
    # the inputs show both sides of the d_sad contract
    assert n_reset >= 1 and sum(int((r[0] >= 0).sum()) for r in refs) >= 20
    dev = "cuda"
    Lx, Rx = gpu.ORBextractor(1000, 1.2, 8, 20, 7), gpu.ORBextractor(1000, 1.2, 8, 20, 7)
    cap = Lx.capacity(W, H)
    d_imgs = []
    for ext, side in ((Lx, 0), (Rx, 1)):
        d = torch.from_numpy(np.stack([pr[side] for pr in pairs])).to(dev)
        k = torch.zeros((P, cap, 7), dtype=torch.int32, device=dev)
        de = torch.zeros((P, cap, 32), dtype=torch.uint8, device=dev)
        n = torch.zeros(P, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ext.extract_batch(d.data_ptr(), P, W, H, W, W * H, k.data_ptr(), de.data_ptr(), cap,
                          n.data_ptr())
        torch.cuda.synchronize()
        d_imgs.append(d)   # level 0 of the batch pyramids is this memory

    def staged(side_k, side_d):
        keys = np.zeros((P, STRIDE, 7), np.int32)
        desc = np.zeros((P, STRIDE, 32), np.uint8)
        cnt = np.zeros(P, np.int32)
        for i, pr in enumerate(pairs):
            n = len(pr[side_k])
            assert n <= STRIDE
            keys[i, :n] = np.ascontiguousarray(pr[side_k]).view(np.int32).reshape(n, 7)
            desc[i, :n] = pr[side_d]
            cnt[i] = n
        return [torch.from_numpy(a).to(dev) for a in (keys, desc, cnt)], cnt
    (kl, dl, nl), cl = staged(2, 3)
    (kr, dr, nr), cr = staged(4, 5)
    assert list(cl) == [1, 17, 0, 12, STRIDE, 17] and list(cr) == [1, 17, 12, 0, STRIDE, 17]
    m = gpu.ORBmatcher()
    for round_ in range(2):   # the second call meets the first one's scratch
        ur = torch.full((P, STRIDE), -7777.0, dtype=torch.float32, device=dev)
        dp = torch.full((P, STRIDE), -7777.0, dtype=torch.float32, device=dev)
        sad = torch.full((P, STRIDE), -7777, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        m.stereo_match_batch(P, Lx, Rx, kl.data_ptr(), dl.data_ptr(), nl.data_ptr(), kr.data_ptr(),
                             dr.data_ptr(), nr.data_ptr(), STRIDE, BF, FX, ur.data_ptr(),
                             dp.data_ptr(), sad.data_ptr())
        torch.cuda.synchronize()
        ur_h, dp_h, sad_h = ur.cpu().numpy(), dp.cpu().numpy(), sad.cpu().numpy()
        for i, ref in enumerate(refs):
            n = int(cl[i])
            for label, got, want in zip(("u_right", "depth", "d_sad"), (ur_h, dp_h, sad_h), ref):
                assert got[i, :n].tobytes() == want.tobytes(), \
                    (round_, i, label, got[i, :n][got[i, :n] != want][:8], want[got[i, :n] != want][:8])
                assert (got[i, n:] == -7777).all(), (round_, i, label, "written past the count")
