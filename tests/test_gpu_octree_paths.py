"""k_octree's paths, each against the CPU oracle byte for byte (keypoints as
28-byte records in order, descriptors), at 320x240 and 640x480.

Every case runs three ways, which select different instantiations of the
kernel: a single frame (register-resident keys), a batch of 4 (cell FAST,
register-resident keys) and a batch of 17, the smallest call that takes the
batch instantiation (keys in LDS or in global scratch, four per thread)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OCTREE_LDS_KB = 52  # orb_plan.h ORB_OCTREE_LDS_KB


def _run_batch(gpu, ext, frames):
    """extract_batch over a list of equally sized frames -> [(keys, desc), ...]"""
    import torch
    h, w = frames[0].shape
    n = len(frames)
    cap = ext.capacity(w, h)
    imgs = torch.from_numpy(np.stack(frames)).cuda()
    kb = torch.zeros((n, cap, 7), dtype=torch.int32, device="cuda")
    db = torch.zeros((n, cap, 32), dtype=torch.uint8, device="cuda")
    nb = torch.zeros(n, dtype=torch.int32, device="cuda")
    ext.extract_batch(imgs.data_ptr(), n, w, h, w, w * h, kb.data_ptr(), db.data_ptr(), cap,
                      nb.data_ptr())
    torch.cuda.synchronize()
    kk = kb.cpu().numpy().view(gpu.KEYPOINT_DTYPE).reshape(n, cap)
    dd, nn = db.cpu().numpy(), nb.cpu().numpy()
    assert (nn >= 0).all(), nn
    return [(kk[i, :nn[i]], dd[i, :nn[i]]) for i in range(n)]


def _same(got, ref, what):
    (k, d), (kr, dr) = got, ref
    assert len(k) == len(kr), (what, len(k), len(kr))
    assert k.tobytes() == kr.tobytes(), what
    assert d.tobytes() == dr.tobytes(), what


def _three_ways(gpu, oracle, frames, nf, lead=0):
    """frames: up to 17 frames cycled to fill a batch; the oracle runs once per
    distinct frame.  `lead` is the frame the single-frame call takes."""
    ext = gpu.ORBextractor(nf, 1.2, 8, 20, 7)
    refs = {}
    for f in frames:
        if id(f) not in refs:
            kr, dr, _ = oracle.extract(f, nf)
            refs[id(f)] = (kr, dr)
    _same(ext(frames[lead]), refs[id(frames[lead])], "single frame")
    for nb in (4, 17):
        batch = [frames[(lead + i) % len(frames)] for i in range(nb)]
        for i, got in enumerate(_run_batch(gpu, ext, batch)):
            _same(got, refs[id(batch[i])], f"batch of {nb}, frame {i}")
    return refs


def _cell_grid(w, h):
    """Level 0's FAST cell grid (src/ORBextractor.cc:797-805): nCols, nRows, wCell, hCell."""
    W, H = w - 32, h - 32
    nc, nr = int(W / 30.0), int(H / 30.0)
    return nc, nr, -(-W // nc), -(-H // nr)


def _level0_cell_counts(oracle, img, nf=1000):
    """Candidates per level-0 cell.  oracle.candidates gives border-relative
    coordinates; a cell's FAST window keeps x in [3, wCell + 3) of its own."""
    k, per = oracle.candidates(img, nf)
    k = k[k["octave"] == 0]
    h, w = img.shape
    nc, nr, wc, hc = _cell_grid(w, h)
    j = ((k["x"] - 3) // wc).astype(int)
    i = ((k["y"] - 3) // hc).astype(int)
    cnt = np.zeros((nr, nc), int)
    np.add.at(cnt, (i, j), 1)
    return cnt, per, k


def _lds_key_cap(oracle, w, h, nf):
    """The extractor has no accessor for the octree's LDS key capacity: this is
    runtime.cpp's computation (orb_build_plan, "octree LDS") from the plan's
    constants: node tables for the largest nodeCap, one cellBase entry per cell
    of the largest level, the rest of ORB_OCTREE_LDS_KB at 6 bytes per key."""
    quota = oracle.params(nf)["quota"]
    node_cap, max_cells = 1, 1
    for l, (lw, lh) in enumerate(oracle.level_sizes(w, h)):
        W, H = lw - 32, lh - 32
        ncol, nrow = int(W / 30.0), int(H / 30.0)
        wc, hc = -(-W // ncol), -(-H // nrow)
        cells = 0
        for i in range(nrow):
            if 16 + i * hc >= lh - 16 - 3:
                continue
            cells += sum(1 for j in range(ncol) if 16 + j * wc < lw - 16 - 6)
        max_cells = max(max_cells, cells)
        n_ini = max(int(np.floor(np.float32(W) / np.float32(H) + np.float32(0.5))), 1)
        node_cap = max(node_cap, (max(int(quota[l]) + 4, 4 * n_ini + 4) + 1) & ~1)
    n2 = 1
    while n2 < node_cap:
        n2 <<= 1
    node_bytes = n2 * 8 + 2 * node_cap * 16 + node_cap * 16 + 4 * node_cap * 4 + ((max_cells + 3) & ~3) * 4
    budget = OCTREE_LDS_KB * 1024
    lds_nodes = 0 if node_bytes > 128 * 1024 else node_bytes
    return ((budget - lds_nodes) // 6) & ~7 if lds_nodes < budget else 0


@pytest.fixture(scope="module")
def noise480():
    return np.random.default_rng(3).integers(0, 256, (480, 640), dtype=np.uint8)


@pytest.fixture(scope="module")
def sparse480(gpu):
    return [gpu.synth_image(5, f, 640, 480) for f in (0, 1)]


def test_cell_count_residues(gpu, oracle):
    """Level-0 cells holding 0, 1, 2, 3, 4, 5, 7, 8 and 9 candidates (isolated
    bright pixels on a flat background: one FAST corner each) and one cell as
    dense as uniform noise makes it: list tails of every residue mod 4, empty
    cells between full ones, and a list longer than 64 keys."""
    w, h = 320, 240
    nc, nr, wc, hc = _cell_grid(w, h)
    img = np.full((h, w), 100, np.uint8)
    wanted = [1, 2, 3, 4, 5, 7, 8, 9]
    spots = [(a, b) for b in range(3) for a in range(3)]
    for idx, m in enumerate(wanted):
        i, j = (0, idx) if idx < nc - 1 else (2, idx - (nc - 1))
        x0, y0 = 19 + j * wc, 19 + i * hc
        for s, (a, b) in enumerate(spots[:m]):
            img[y0 + 4 + 8 * b, x0 + 4 + 8 * a] = 160 + 7 * s + idx
    # noise over cell (4, 4) and a margin (its neighbours get partial lists)
    rng = np.random.default_rng(21)
    y0, x0 = 19 + 4 * hc - 6, 19 + 4 * wc - 6
    img[y0:y0 + hc + 12, x0:x0 + wc + 12] = rng.integers(0, 256, (hc + 12, wc + 12), dtype=np.uint8)
    cnt, _, _ = _level0_cell_counts(oracle, img)
    have = set(cnt.ravel().tolist())
    assert {0, 1, 2, 3, 4, 5, 7, 8, 9} <= have, sorted(have)
    assert {c % 4 for c in have if c > 0} == {0, 1, 2, 3}
    assert cnt.max() > 64, cnt.max()
    _three_ways(gpu, oracle, [img], 1000)


def test_lds_and_global_keys_in_one_launch(gpu, oracle, noise480, sparse480):
    """A 17-frame batch whose two noise frames keep level 0's keys in global
    scratch while the sparse frames' fit the LDS: both key homes of the batch
    instantiation in one launch."""
    cap = _lds_key_cap(oracle, 640, 480, 1000)
    assert 1000 < cap < 8192, cap
    noise2 = np.random.default_rng(33).integers(0, 256, (480, 640), dtype=np.uint8)
    for f in (noise480, noise2):
        assert oracle.candidates(f)[1][0] > cap
    for f in sparse480:
        assert 0 < oracle.candidates(f)[1].max() <= cap
    s0, s1 = sparse480
    frames = [s0, s1, s0, noise480, s1, s0, s1, s0, s1, s0, s1, noise2, s0, s1, s0, s1, s0]
    assert len(frames) == 17
    _three_ways(gpu, oracle, frames, 1000, lead=3)  # single frame and batch of 4 start at the noise frame


def test_response_ties(gpu, oracle):
    """One identical stamp tiled over the frame: the candidates of a node share
    their response, so the key index alone decides which one a node retains."""
    w, h = 320, 240
    img = np.full((h, w), 90, np.uint8)
    img[20:h - 16:8, 20:w - 16:8] = 200
    k, per = oracle.candidates(img)
    for l in (0, 1):
        r = k[k["octave"] == l]["response"]
        assert len(r) > 100 and len(np.unique(r)) < len(r) // 4, (l, len(r), len(np.unique(r)))
    _three_ways(gpu, oracle, [img], 1000)
    _three_ways(gpu, oracle, [img], 200)


def test_stop_full_list_at_once(gpu, oracle, noise480):
    """nfeatures = 50 on noise: the final phase is reached after the first
    pass and jstop cuts the sorted candidates."""
    refs = _three_ways(gpu, oracle, [noise480], 50)
    (kr, _), = refs.values()
    assert 40 <= len(kr) <= 50 + 3 * 8  # a level's last division may overshoot its quota by 3


def test_stop_no_growth(gpu, oracle):
    """nfeatures = 5000 on a sparse 320x240 frame: fewer keys than the quota,
    every node ends with one key, the loop stops on alive == prev."""
    img = gpu.synth_image(7, 0, 320, 240)
    k, per = oracle.candidates(img, 5000)
    quota = oracle.params(5000)["quota"]
    assert per[0] > 0 and (per < quota).all(), (per, quota)
    _three_ways(gpu, oracle, [img], 5000)


def test_single_corner_and_flat_frames(gpu, oracle):
    """A frame with exactly one level-0 corner, and a flat frame (no key on
    any level) between frames that have keys."""
    w, h = 320, 240
    one = np.full((h, w), 100, np.uint8)
    one[117, 161] = 220
    k, per = oracle.candidates(one)
    assert per[0] == 1
    flat = np.full((h, w), 100, np.uint8)
    assert oracle.candidates(flat)[1].sum() == 0
    busy = gpu.synth_image(7, 0, w, h)
    _three_ways(gpu, oracle, [one], 1000)
    _three_ways(gpu, oracle, [busy, flat, one, busy, flat], 1000, lead=1)


def test_global_node_tables_batch17(gpu, oracle, noise480):
    """12,000 features put the node tables in global memory; 17 copies of one
    noise frame take the batch instantiation with them."""
    refs = _three_ways(gpu, oracle, [noise480], 12000)
    (kr, _), = refs.values()
    assert len(kr) > 8000
