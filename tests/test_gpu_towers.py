"""sn_tower_proposals on the device against the numpy oracle of its definition (tests/towers_cases.py) and against
constructions whose answer is known in closed form.  Every comparison is exact integer equality."""
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import towers_cases as tc

pytestmark = pytest.mark.gpu


def _run(positive, eps, min_points, voxel_size=None, max_towers=64, device=None):
    """bool grid(s) [B, n0, n1, n2] (numpy) as a bool tensor -> (labels, n_towers, stats) on the host"""
    g = torch.from_numpy(np.ascontiguousarray(positive)).to(device)
    p = sna.tower_proposals(g, eps=eps, min_points=min_points, voxel_size=voxel_size, max_towers=max_towers)
    return p.labels.cpu().numpy(), p.n_towers.cpu().numpy(), p.stats.cpu().numpy()


def _check_against_oracle(positive, eps, min_points, device, voxel_size=None, max_towers=64, what=""):
    got = _run(positive, eps, min_points, voxel_size, max_towers, device)
    want = tc.dbscan_batch(positive, eps, min_points, voxel_size, max_towers)
    assert np.array_equal(got[1], want[1]), f"n_towers {what}"
    assert np.array_equal(got[0], want[0]), f"labels {what}"
    for c, name in enumerate(tc.STAT_NAMES):
        assert np.array_equal(got[2][..., c], want[2][..., c]), f"stats column {name} {what}"
    return got


@pytest.mark.parametrize("shape", tc.SMALL_SHAPES)
def test_small_grids_against_the_oracle(hip_device, shape):
    positive = np.stack([tc.small_grid(shape, seed) for seed in (1, 2)])
    seen = set()
    for eps in (1.0, 3.0, 3.5):
        for min_points in (1, 4, 18, 10_000):
            lab, k, st = _check_against_oracle(positive, eps, min_points, hip_device, what=f"{shape} {eps} {min_points}")
            if min_points == 1:
                assert np.array_equal(lab >= 0, positive) and np.array_equal(st[..., 0], st[..., 1]), "all are core"
            if min_points == 10_000:
                assert k.sum() == 0
            seen.add(int(k.max()))
    assert len(seen) > 2, "the cases differ in their cluster counts"


def test_faces_corners_and_tile_boundaries(hip_device):
    # blobs in all eight corners and flush against every face: a row, plane or tile must not wrap into its neighbour
    g = tc.corner_blobs((12, 12, 70), 3)
    _, k, _ = _check_against_oracle(g[None], 2.0, 4, hip_device, what="corner blobs")
    assert k.tolist() == [14]
    g = tc.corner_blobs((13, 13, 130), 3)
    _, k, _ = _check_against_oracle(g[None], 2.0, 4, hip_device, what="corner blobs, three words per row")
    assert k.tolist() == [14]
    # the last plane of one tile and the first of the next stay two clusters in two tiles
    t = np.zeros((3, 8, 8, 8), dtype=bool)
    t[0, 7, 2:6, 2:6] = True
    t[1, 0, 2:6, 2:6] = True
    t[2, 0, 2:6, 2:6] = True
    t[2, 7, 2:6, 2:6] = True
    lab, k, st = _check_against_oracle(t, 1.0, 3, hip_device, what="tile boundary")
    assert k.tolist() == [1, 1, 2] and st[:, 0, 0].tolist() == [16, 16, 16]
    # an all-zero tile in the middle
    t[1] = False
    lab, k, st = _check_against_oracle(t, 1.0, 3, hip_device, what="empty tile")
    assert k.tolist() == [1, 0, 2] and np.all(lab[1] == -1) and not st[1].any()


def test_merge_boundary(hip_device):
    def blocks(gap):
        g = np.zeros((1, 7, 7, 20), dtype=bool)
        g[0, 2:5, 2:5, 2:5] = True
        g[0, 2:5, 2:5, 4 + gap:7 + gap] = True     # nearest faces `gap` apart
        return g
    lab, k, st = _check_against_oracle(blocks(3), 3.0, 4, hip_device, what="gap 3")
    assert k.tolist() == [1] and st[0, 0, 0] == 54
    lab, k, st = _check_against_oracle(blocks(4), 3.0, 4, hip_device, what="gap 4")
    assert k.tolist() == [2] and st[0, :2, 0].tolist() == [27, 27]


@pytest.mark.parametrize("axis", [0, 2])
def test_border_tie_takes_the_smaller_id(hip_device, axis):
    # two crosses two voxels apart along `axis`: each centre is core at min_points 4, the voxel between them is within
    # eps of both centres and is no core itself (3 positives in its stencil)
    g = np.zeros((1, 7, 7, 7), dtype=bool)
    arms = [a for a in range(3) if a != axis]
    c0, c1 = [3, 3, 3], [3, 3, 3]
    c0[axis], c1[axis] = 2, 4
    for c in (c0, c1):
        g[(0, *c)] = True
        for a, d in ((arms[0], -1), (arms[0], 1), (arms[1], -1)):
            v = list(c)
            v[a] += d
            g[(0, *v)] = True
    between = (0, 3, 3, 3)
    g[between] = True
    lab, k, st = _check_against_oracle(g, 1.0, 4, hip_device, what="border tie")
    assert k.tolist() == [2]
    assert lab[(0, *c0)] == 0 and lab[(0, *c1)] == 1 and lab[between] == 0
    assert st[0, :2, 0].tolist() == [5, 4] and st[0, :2, 1].tolist() == [1, 1]


def _touching(a, b):
    """6-adjacent or overlapping anywhere (no wrap-around)"""
    if (a & b).any():
        return True
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        if (a[tuple(lo)] & b[tuple(hi)]).any() or (a[tuple(hi)] & b[tuple(lo)]).any():
            return True
    return False


def test_depth_one_long_chain_and_two_interleaved(hip_device):
    """Expected values come from the construction: what a propagation scheme with a fixed trip count, or a union without
    a proper flatten, gets wrong."""
    n = 64
    g, count = tc.serpentine(n)
    assert count == int(g.sum()) and count > 60_000
    lab, k, st = _run(g[None], 1.0, 2, device=hip_device)
    assert k.tolist() == [1]
    assert np.array_equal(lab[0] == 0, g) and np.all(lab[0][~g] == -1)
    assert st[0, 0].tolist() == [count, count, *np.argwhere(g).sum(axis=0), 0, 0, 0, n - 2, n - 2, n - 1, 0]
    assert not st[0, 1:].any()
    a, b, na, nb = tc.two_serpentines(n)
    assert na == int(a.sum()) and nb == int(b.sum()) and not _touching(a, b)
    lab, k, st = _run((a | b)[None], 1.0, 2, device=hip_device)
    assert k.tolist() == [2]
    assert np.array_equal(lab[0] == 0, a) and np.array_equal(lab[0] == 1, b)
    assert st[0, :2, 0].tolist() == [na, nb] and st[0, :2, 1].tolist() == [na, nb]
    assert st[0, :2, 11].tolist() == [0, (2 * n + 0) * n + 2]


def test_dense_worst_case(hip_device):
    n = 16
    lab, k, st = _run(np.ones((1, n, n, n), dtype=bool), 3.5, 18, device=hip_device)
    assert k.tolist() == [1] and np.all(lab == 0)
    s = n * n * n * (n - 1) // 2
    assert st[0, 0].tolist() == [n ** 3, n ** 3, s, s, s, 0, 0, 0, n - 1, n - 1, n - 1, 0]
    n = 64
    lab, k, st = _run(np.ones((2, n, n, n), dtype=bool), 1.0, 2, device=hip_device)
    s = n * n * n * (n - 1) // 2
    assert k.tolist() == [1, 1] and np.all(lab == 0)
    for b in range(2):
        assert st[b, 0].tolist() == [n ** 3, n ** 3, s, s, s, 0, 0, 0, n - 1, n - 1, n - 1, 0]


def test_more_clusters_than_rows(hip_device):
    g = tc.isolated_voxels(64, 8, 100)
    grid = torch.from_numpy(g[None]).to(hip_device)
    max_towers, guard = 64, 4096
    ws = torch.empty(_hip.towers_ws_bytes(1, 64, 64, 64) // 8, dtype=torch.int64, device=hip_device)
    labels = torch.empty((1, 64, 64, 64), dtype=torch.int32, device=hip_device)
    n_towers = torch.empty(1, dtype=torch.int32, device=hip_device)
    room = torch.full((max_towers * tc.NSTAT + guard,), -12345, dtype=torch.int64, device=hip_device)
    _hip.tower_proposals(grid, 0.5, 3.5, 1, max_towers, ws, labels, n_towers, room[:max_towers * tc.NSTAT])
    assert n_towers.tolist() == [100]
    lab = labels.cpu().numpy()[0]
    assert lab[g].tolist() == list(range(100)) and np.all(lab[~g] == -1)
    room = room.cpu().numpy()
    assert np.all(room[max_towers * tc.NSTAT:] == -12345), "nothing is written past the rows"
    pts = np.argwhere(g)[:max_towers]
    want = np.concatenate([np.ones((max_towers, 2), dtype=np.int64), pts, pts, pts,
                           ((pts[:, 0] * 64 + pts[:, 1]) * 64 + pts[:, 2])[:, None]], axis=1)
    assert np.array_equal(room[:max_towers * tc.NSTAT].reshape(max_towers, tc.NSTAT), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_threshold_in_the_grids_dtype(hip_device, dtype):
    tau = 0.65
    at = torch.tensor(tau, dtype=torch.float64).to(dtype)                       # tau as torch rounds it to the dtype
    if dtype == torch.bfloat16:
        assert float(at) == 0.6484375
    ints = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}[dtype]
    below = (at.view(ints) - 1).view(dtype)                # one ulp below
    assert float(below) < float(at)
    shape = (2, 9, 10, 70)
    positive = np.stack([tc.small_grid(shape[1:], seed) for seed in (5, 6)])
    rng = np.random.default_rng(9)
    vals = torch.where(torch.from_numpy(rng.random(shape) < 0.5), below, torch.zeros((), dtype=dtype))
    vals = torch.where(torch.from_numpy(rng.random(shape) < 0.2), torch.full((), float("nan"), dtype=dtype), vals)
    high = torch.where(torch.from_numpy(rng.random(shape) < 0.5), at, torch.ones((), dtype=dtype))
    grid = torch.where(torch.from_numpy(positive), high, vals).to(hip_device)
    assert torch.isnan(grid).any() and (grid == at.to(hip_device)).any() and (grid == below.to(hip_device)).any()
    p = sna.tower_proposals(grid[:, None], tau=tau, eps=3.0, min_points=4)
    want = tc.dbscan_batch(positive, 3.0, 4)
    assert np.array_equal(p.labels.cpu().numpy(), want[0])
    assert np.array_equal(p.n_towers.cpu().numpy(), want[1])
    assert np.array_equal(p.stats.cpu().numpy(), want[2])


def test_byte_and_bool_grids(hip_device):
    positive = np.stack([tc.small_grid((9, 10, 70), seed) for seed in (5, 6)])
    ref = sna.tower_proposals(torch.from_numpy(positive.astype(np.float32)).to(hip_device), tau=0.65, eps=3.0, min_points=4)
    assert int(ref.n_towers.sum()) > 0
    bytes_ = np.where(positive, np.random.default_rng(1).integers(1, 256, positive.shape), 0).astype(np.uint8)
    for grid in (torch.from_numpy(bytes_), torch.from_numpy(positive)):
        for tau in (None, 0.9):                            # ignored for these dtypes
            p = sna.tower_proposals(grid.to(hip_device), tau=tau, eps=3.0, min_points=4)
            assert torch.equal(p.labels, ref.labels) and torch.equal(p.n_towers, ref.n_towers)
            assert torch.equal(p.stats, ref.stats)
    with pytest.raises(ValueError, match="tau"):
        sna.tower_proposals(torch.zeros((1, 4, 4, 4), device=hip_device))
    with pytest.raises(sna.HipLibraryError):
        sna.tower_proposals(torch.zeros((1, 4, 4, 4), dtype=torch.int32, device=hip_device), tau=0.5)


def test_anisotropic_voxels(hip_device):
    g = tc.random_grid((9, 20, 33), 0.2)
    _, k, _ = _check_against_oracle(g[None], 1.6, 5, hip_device, voxel_size=(1.3, 0.5, 0.5), what="anisotropic")
    assert k[0] > 0


def test_large_tile_takes_the_workspace_path_with_the_same_results(hip_device):
    """128^3: the tile's bitmap (256 KiB) does not fit LDS and is read from the workspace."""
    n = 128
    rng = np.random.default_rng(4)
    g = np.zeros((n, n, n), dtype=bool)
    for c in ((20, 30, 40), (100, 90, 66), (64, 64, 120)):           # three blobs, one across a word boundary
        box = tuple(slice(v - 5, v + 6) for v in c)
        g[box] = rng.random((11, 11, 11)) < 0.6
    noise = rng.integers(0, n, (300, 3))
    g[noise[:, 0], noise[:, 1], noise[:, 2]] = True
    _, k, _ = _check_against_oracle(g[None], 3.5, 18, hip_device, what="128^3")
    assert k[0] >= 3
    # the same content in a 64^3 box: once inside a 128^3 call (workspace path), once as a 64^3 call (LDS path)
    box = np.zeros((64, 64, 64), dtype=bool)
    box[:, :, :] = g[64:, 64:, 64:]
    box[3:14, 40:51, 10:21] = rng.random((11, 11, 11)) < 0.6
    big = np.zeros((n, n, n), dtype=bool)
    big[64:, 64:, 64:] = box
    lab_big, k_big, st_big = _run(big[None], 3.5, 18, device=hip_device)
    lab_box, k_box, st_box = _run(box[None], 3.5, 18, device=hip_device)
    assert k_big.tolist() == k_box.tolist() and k_box[0] >= 2
    assert np.array_equal(lab_big[0, 64:, 64:, 64:], lab_box[0])
    assert np.all(lab_big[0, :64] == -1) and np.all(lab_big[0, :, :64] == -1) and np.all(lab_big[0, :, :, :64] == -1)
    assert np.array_equal(st_big[..., :2], st_box[..., :2])
    assert np.array_equal(st_big[..., 5:11] - 64 * (st_big[..., 0:1] > 0), st_box[..., 5:11])


def test_capture_and_replay_on_refilled_grid(hip_device):
    first = np.stack([tc.small_grid((16, 16, 70), seed) for seed in (1, 2)])
    second = np.stack([tc.small_grid((16, 16, 70), seed) for seed in (3, 4)])
    second[1] = False
    buf = torch.from_numpy(first.astype(np.float32)).to(hip_device)
    eager = [sna.tower_proposals(torch.from_numpy(c.astype(np.float32)).to(hip_device), tau=0.65, eps=3.0, min_points=4)
             for c in (first, second)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        p = sna.tower_proposals(buf, tau=0.65, eps=3.0, min_points=4)
    for content, want in ((first, eager[0]), (second, eager[1]), (first, eager[0])):
        buf.copy_(torch.from_numpy(content.astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(p.labels, want.labels) and torch.equal(p.n_towers, want.n_towers)
        assert torch.equal(p.stats, want.stats)
    assert eager[0].n_towers.tolist() != eager[1].n_towers.tolist()


def test_python_layer(hip_device):
    positive = np.stack([tc.small_grid((9, 10, 70), 5), np.zeros((9, 10, 70), dtype=bool), tc.small_grid((9, 10, 70), 6)])
    p = sna.tower_proposals(torch.from_numpy(positive).to(hip_device), eps=3.0, min_points=4, max_towers=8)
    st = p.stats.cpu().numpy()
    k = p.n_towers.cpu().numpy()
    assert 0 < k.max() <= 8 and k[1] == 0
    present = st[..., 0] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        want_c = np.where(present[..., None], st[..., 2:5].astype(np.float64) / st[..., 0:1].astype(np.float64), np.nan)
    want_lo = np.where(present[..., None], st[..., 5:8].astype(np.float64), np.nan)
    want_hi = np.where(present[..., None], st[..., 8:11].astype(np.float64), np.nan)
    cents = p.centroids()
    lo, hi = p.boxes()
    assert cents.is_cuda and cents.dtype == torch.float64 and cents.shape == (3, 8, 3)
    assert np.array_equal(cents.cpu().numpy(), want_c, equal_nan=True)
    assert np.array_equal(lo.cpu().numpy(), want_lo, equal_nan=True)
    assert np.array_equal(hi.cpu().numpy(), want_hi, equal_nan=True)
    # to_world: origin + index * voxel_size, the product formed and then added, per tile
    origin = np.array([[0.1, -3.7, 1e6 / 3], [5.0, 6.0, 7.0], [-2.5, 0.3, 11.0 / 7]])
    size = np.array([[0.3, 0.7, 1.1 / 3], [1.0, 1.0, 1.0], [0.25, 0.2, 0.1]])
    world = p.to_world(torch.from_numpy(origin).to(hip_device), torch.from_numpy(size).to(hip_device))
    prod = want_c * size[:, None, :]
    assert np.array_equal(world.cpu().numpy(), origin[:, None, :] + prod, equal_nan=True)
    world = p.to_world((0.1, -3.7, 2.0 / 3), (0.3, 0.7, 1.1 / 3), index=hi)
    assert np.array_equal(world.cpu().numpy(), np.array([0.1, -3.7, 2.0 / 3]) + want_hi * np.array([0.3, 0.7, 1.1 / 3]),
                          equal_nan=True)
    # towers(b): the reference's return shape
    lab = p.labels.cpu().numpy()
    for b in (0, 2):
        towers, centroids = p.towers(b)
        assert isinstance(towers, list) and len(towers) == k[b] and centroids.shape == (k[b], 3)
        for i, t in enumerate(towers):
            assert t.dtype == np.float64 and np.array_equal(t, np.argwhere(lab[b] == i).astype(np.float64))
        assert np.array_equal(centroids, want_c[b, :k[b]])
    assert p.towers(1) == ([], [])
    kept, kc = sna.filter_towers(*p.towers(0), threshold=50.0, center=p.grid_center())
    assert len(kept) == len(kc) <= k[0]


def test_pipeline_tower_proposals_on_the_golden_tile(hip_device, golden_dir):
    torch.manual_seed(575)
    a = np.load(os.path.join(golden_dir, "ts40k_sample575_full.npz"))["tile"]
    model = sna.SceneNet({"cy": 2, "cone": 1, "neg": 1}, (9, 9, 9)).to(hip_device)
    pipe = sna.ScenePipeline(model, (64, 64, 64), keep_labels=[15], tau=0.65)
    batch = sna.PointBatch.from_tiles([a[:, :3]], [a[:, 3]], device=hip_device)
    pred, grids = pipe(batch, want_gt=True)
    got = pipe.tower_proposals(pred, grids)
    want = sna.tower_proposals(pred, tau=pipe.tau)
    assert got.grids is grids
    assert torch.equal(got.labels, want.labels) and torch.equal(got.n_towers, want.n_towers)
    assert torch.equal(got.stats, want.stats)
    positive = (pred[:, 0] >= 0.65).cpu().numpy()
    lab, k, st = tc.dbscan_batch(positive, 3.5, 18)
    assert np.array_equal(got.labels.cpu().numpy(), lab) and np.array_equal(got.n_towers.cpu().numpy(), k)
    assert np.array_equal(got.stats.cpu().numpy(), st)
    # and the ground truth's towers (the occupancy of the tower label): bool grid, tau not needed
    gt = sna.tower_proposals(grids.gt_occ, eps=3.5, min_points=18)
    lab, k, st = tc.dbscan_batch(grids.gt_occ[:, 0].cpu().numpy() != 0, 3.5, 18)
    assert np.array_equal(gt.labels.cpu().numpy(), lab) and np.array_equal(gt.n_towers.cpu().numpy(), k)
