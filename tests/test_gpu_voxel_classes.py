"""K18 on the GPU: sn_voxel_classes, sn_class_census / sn_class_paint and the layers above them against the oracles of
tests/voxel_classes_cases.py.  Every comparison is exact: integers as they are, fp64 as int64 views.  Seams of the two
chunks, batches with an odd start offset and a one-point tile, buffers offset by one element, sentinel-filled outputs with
guard rows, special labels, one crowded voxel, K1's binning of foreign points, the golden colours of the reference,
capture, and a file written with the colours."""
import os

import numpy as np
import pytest
import torch

import binning_cases as bc
import voxel_classes_cases as kc
import scene_net_amd as sna
from scene_net_amd import _hip

pytestmark = pytest.mark.gpu

GUARD = 5                      # sentinel rows / cells behind every output
SENT_F = -7.25e300             # what an untouched fp64 slot holds
SENT_I = -99
SENT_U16 = 4242


def shifted(arr, dev, shift):
    """The array on the device, `shift` elements into a larger buffer (8-byte aligned, not 16)."""
    flat = torch.from_numpy(np.ascontiguousarray(arr)).reshape(-1)
    buf = torch.empty(flat.numel() + shift, dtype=flat.dtype, device=dev)
    view = buf[shift:]
    view.copy_(flat)
    return view.reshape(arr.shape)


def sentinel(n, value, dtype, dev, shift):
    return torch.full((n + GUARD + shift,), value, dtype=dtype, device=dev)[shift:]


# ================================================================ the class grid
def run_grid(dev, tiles, labels, dims, desc, shift=0, skip=True):
    """One sn_voxel_classes through the ctypes layer with sentinel-filled outputs; numpy copies of everything."""
    sizes = [len(t) for t in tiles]
    B, V = len(tiles), dims[0] * dims[1] * dims[2]
    pts = shifted(np.concatenate(tiles).astype(np.float64), dev, shift)
    lab = shifted(np.concatenate(labels).astype(np.float64), dev, shift)
    offsets = shifted(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), dev, shift)
    d = shifted(np.asarray(desc, dtype=np.float64), dev, shift)
    grid = sentinel(B * V, SENT_F, torch.float64, dev, shift)
    unb = sentinel(B, SENT_I, torch.int64, dev, shift)
    nans = sentinel(B, SENT_I, torch.int64, dev, shift)
    _hip.voxel_classes(pts, lab, offsets, d, dims, grid[:B * V], unb[:B], nans[:B], skip=skip)
    torch.cuda.synchronize()
    g, u, n = grid.cpu().numpy(), unb.cpu().numpy(), nans.cpu().numpy()
    assert np.all(g[B * V:] == SENT_F) and np.all(u[B:] == SENT_I) and np.all(n[B:] == SENT_I), "guard slots were touched"
    return g[:B * V].reshape(B, dims[2], dims[0], dims[1]), u[:B], n[:B]


def check_grid(out, exp):
    assert np.array_equal(kc.bits(out[0]), kc.bits(exp[0]))
    assert np.array_equal(out[1], exp[1]) and np.array_equal(out[2], exp[2])


@pytest.mark.parametrize("dims", [(5, 7, 3), (8, 12, 4), (64, 64, 64)])
def test_grid_of_a_foreign_batch(hip_device, dims):
    assert dims in bc.DIMS
    desc, _ = bc.host_desc("own", dims, 3)
    tiles, _ = bc.foreign_batch(desc, dims)
    assert len(tiles) == 3 and len(tiles[0]) == 1001 and len(tiles[1]) == 1          # an odd start offset, a one-point tile
    rng = np.random.default_rng(180)
    labels = [kc.special_labels(len(t), rng) for t in tiles]
    exp = kc.expected_grid(desc, dims, tiles, labels)
    assert exp[1].sum() > 100 and exp[1][1] == 1 and exp[2].sum() > 100              # unbinned rows, NaN labels
    g = exp[0]
    assert np.isinf(g).any()
    if dims == (64, 64, 64):       # sparse enough that single rows decide voxels: every kind of label comes out
        assert np.isnan(g).any() and (g == -np.inf).any() and (g < 0).any() and (g == 1e300).any() and (g == 0).any()
        assert (g == 5e-324).any()
    first = None
    for shift in (0, 1):
        out = run_grid(hip_device, tiles, labels, dims, desc, shift=shift)
        check_grid(out, exp)
        first = out if first is None else first
        assert np.array_equal(kc.bits(out[0]), kc.bits(first[0]))                    # two runs: bit-identical
    check_grid(run_grid(hip_device, tiles, labels, dims, desc, skip=False), exp)      # every atomic sent: the same grid


def test_grid_with_a_size_mode_descriptor(hip_device):
    dims = bc.CAPACITY
    desc, own = bc.host_desc("sized", dims, 3)
    assert (own < np.array(dims)).any()                                              # padded tables
    tiles, _ = bc.foreign_batch(desc, dims, own)
    rng = np.random.default_rng(181)
    labels = [kc.special_labels(len(t), rng) for t in tiles]
    exp = kc.expected_grid(desc, dims, tiles, labels)
    # the padded table is used as it stands: rows above a tile's own last edge land in the padding cell and are binned
    inside_own = sum(int((bc.expected_flat(desc[b], dims, t, own[b]) >= 0).sum()) for b, t in enumerate(tiles))
    assert sum(len(t) for t in tiles) - exp[1].sum() > inside_own
    for shift in (0, 1):
        check_grid(run_grid(hip_device, tiles, labels, dims, desc, shift=shift), exp)


def test_grid_tile_sizes_on_the_chunk_seams(hip_device):
    c = _hip.voxel_classes_chunk_points()
    dims = (5, 7, 3)
    rng = np.random.default_rng(182)
    for total in (1, c - 1, c, c + 1, 2 * c + 3):
        tile = kc.cube_tile(total, 7 + total)
        desc = kc.own_desc(tile, dims)[None]
        lab = kc.special_labels(total, rng)
        exp = kc.expected_grid(desc, dims, [tile], [lab])
        assert exp[1][0] == 0
        for shift in (0, 1):
            check_grid(run_grid(hip_device, [tile], [lab], dims, desc, shift=shift), exp)
    # tiles that end one row before, on and one row behind a chunk seam, in one batch
    sizes = [c - 1, 1, 1, c + 2, 3]
    tiles = [kc.cube_tile(n, 90 + k) for k, n in enumerate(sizes)]
    desc = np.stack([kc.own_desc(t, dims) for t in tiles])
    labels = [kc.special_labels(n, rng) for n in sizes]
    check_grid(run_grid(hip_device, tiles, labels, dims, desc), kc.expected_grid(desc, dims, tiles, labels))


def test_one_crowded_voxel_and_a_voxel_of_nan_labels(hip_device):
    dims = (5, 7, 3)
    base = kc.cube_tile(600, 31)
    desc = kc.own_desc(base, dims)[None]
    lo, hi = desc[0, :3], desc[0, 3:6]
    step = (hi - lo) / np.array(dims)
    rng = np.random.default_rng(183)
    crowd = lo + step * np.array([2.5, 3.5, 1.5]) + (rng.random((6000, 3)) - 0.5) * 0.2 * step       # one voxel, 6000 rows
    quiet = lo + step * np.array([0.5, 0.5, 0.5]) + (rng.random((40, 3)) - 0.5) * 0.2 * step         # one voxel, NaN labels only
    keep = np.ones(len(base), dtype=bool)
    f_base = bc.expected_flat(desc[0], dims, base)
    f_crowd, f_quiet = (int(bc.expected_flat(desc[0], dims, p)[0]) for p in (crowd, quiet))
    keep &= (f_base != f_quiet) & (f_base != f_crowd)
    tile = np.concatenate([base[keep], crowd, quiet])
    lab = np.concatenate([kc.special_labels(int(keep.sum()), rng), rng.integers(0, 5000, 6000).astype(np.float64),
                          np.full(40, np.nan)])
    lab[len(tile) - 40 - 6000 + np.arange(0, 6000, 7)] = np.nan                  # NaN mixed into the crowd
    order = rng.permutation(len(tile))
    tile, lab = tile[order], lab[order]
    flat = bc.expected_flat(desc[0], dims, tile)
    assert (flat == f_crowd).sum() == 6000 and (flat == f_quiet).sum() == 40
    exp = kc.expected_grid(desc, dims, [tile], [lab])
    g = exp[0].reshape(-1)
    assert np.isnan(g[f_quiet]) and g[f_crowd] >= 4990
    for skip in (True, False):
        check_grid(run_grid(hip_device, [tile], [lab], dims, desc, skip=skip), exp)
    # ascending labels: every row of the crowd raises the cell (the skip never applies); descending: only the first does
    for direction in (1, -1):
        lab2 = np.arange(len(tile), dtype=np.float64)[::direction].copy()
        check_grid(run_grid(hip_device, [tile], [lab2], dims, desc), kc.expected_grid(desc, dims, [tile], [lab2]))


def test_voxel_classes_layer_own_and_given_descriptor(hip_device):
    dims = (8, 12, 4)
    rng = np.random.default_rng(184)
    tiles = [kc.cube_tile(1301, 41), kc.cube_tile(5, 42), kc.cube_tile(700, 43, extent=31.0)]
    labels = [kc.special_labels(len(t), rng) for t in tiles]
    batch = sna.PointBatch.from_tiles(tiles, labels, device=hip_device)
    vc = sna.voxel_classes(batch, dims)
    assert tuple(vc.grid.shape) == (3, 1, 4, 8, 12) and vc.grid.dtype == torch.float64 and vc.dims is None
    host = np.stack([kc.own_desc(t, dims) for t in tiles])
    assert np.array_equal(kc.bits(vc.desc.cpu().numpy()), kc.bits(host))         # the grid both sides bin with
    exp = kc.expected_grid(host, dims, tiles, labels)
    check_grid((vc.grid[:, 0].cpu().numpy(), vc.unbinned.cpu().numpy(), vc.nan_labels.cpu().numpy()), exp)
    # foreign points through a given descriptor: a crop's labels in the grid of the tile it came from
    fdesc, _ = bc.host_desc("own", dims, 3)
    ftiles, _ = bc.foreign_batch(fdesc, dims)
    flabels = [kc.special_labels(len(t), rng) for t in ftiles]
    fbatch = sna.PointBatch.from_tiles(ftiles, flabels, device=hip_device)
    fvc = sna.voxel_classes(fbatch, dims, desc=torch.from_numpy(fdesc).to(hip_device))
    fexp = kc.expected_grid(fdesc, dims, ftiles, flabels)
    assert fexp[1].sum() > 100
    check_grid((fvc.grid[:, 0].cpu().numpy(), fvc.unbinned.cpu().numpy(), fvc.nan_labels.cpu().numpy()), fexp)
    # size mode: the descriptor voxelize_batch builds for the same arguments
    svc = sna.voxel_classes(batch, bc.CAPACITY, voxel_dims=bc.VOXEL_SIZE)
    ref = sna.voxelize_batch(batch, bc.CAPACITY, voxel_dims=bc.VOXEL_SIZE, want_density=True, want_occ=False)
    assert torch.equal(svc.desc.view(torch.int64), ref.desc.view(torch.int64)) and torch.equal(svc.dims, ref.dims)
    sexp = kc.expected_grid(svc.desc.cpu().numpy(), bc.CAPACITY, tiles, labels)
    check_grid((svc.grid[:, 0].cpu().numpy(), svc.unbinned.cpu().numpy(), svc.nan_labels.cpu().numpy()), sexp)
    with pytest.raises(sna.HipLibraryError):
        sna.voxel_classes(sna.PointBatch(torch.zeros((4, 3), dtype=torch.float64), torch.zeros(4, dtype=torch.float64),
                                         torch.tensor([0, 4]), (4,)))


def test_classes_on_voxel_on_the_ts40k_sample(hip_device, golden_dir):
    a = np.load(os.path.join(golden_dir, "ts40k_sample575_subset.npy"))
    xyz, lab = a[:, :3], a[:, 3]
    dims = (64, 64, 64)
    got = sna.classes_on_voxel(xyz, lab)
    assert isinstance(got, np.ndarray) and got.shape == (64, 64, 64) and got.dtype == np.float64
    exp = kc.expected_grid(kc.own_desc(xyz, dims)[None], dims, [xyz], [lab])
    assert exp[1][0] == 0 and len(np.unique(exp[0])) >= 8                         # zero and most of the sample's classes
    assert np.array_equal(kc.bits(got), kc.bits(exp[0][0]))
    assert np.array_equal(kc.bits(sna.classes_on_voxel(xyz, lab, voxel_dims=(8, 12, 4))),
                          kc.bits(kc.expected_grid(kc.own_desc(xyz, (8, 12, 4))[None], (8, 12, 4), [xyz], [lab])[0][0]))


def test_round_trip_through_gather_points(hip_device):
    dims = (8, 12, 4)
    rng = np.random.default_rng(185)
    tiles = [kc.cube_tile(1500, 51), kc.cube_tile(800, 52)]
    labels = [np.where(rng.random(len(t)) < 0.1, np.nan, rng.integers(-3, 20, len(t)).astype(np.float64)) for t in tiles]
    batch = sna.PointBatch.from_tiles(tiles, labels, device=hip_device)
    vc = sna.voxel_classes(batch, dims)
    back = _hip.gather_points(vc.grid, batch.pts, batch.offsets, vc.desc, fill=-1e9).cpu().numpy()[0]
    own = np.concatenate(labels)
    known = ~np.isnan(own)
    assert known.sum() > 1800 and (back[known] >= own[known]).all() and (back[known] > own[known]).any()
    flat = np.concatenate([bc.expected_flat(vc.desc[b].cpu().numpy(), dims, t) + b * 8 * 12 * 4 for b, t in enumerate(tiles)])
    assert np.array_equal(kc.bits(back), kc.bits(vc.grid.cpu().numpy().reshape(-1)[flat]))


# ================================================================ class colours
def run_paint(dev, class_tiles, table, shift=0, want_colors=True, want_rgb=True, U_max=None, beyond=3):
    """census + paint through the ctypes layer, `beyond` rows behind offsets[B] inside `total`; numpy copies of everything."""
    sizes = [len(t) for t in class_tiles]
    B, n = len(sizes), int(sum(sizes))
    total = n + beyond
    packed = np.concatenate(list(class_tiles) + [np.full(beyond, 3.0)]).astype(np.float64)
    cls = shifted(packed, dev, shift)
    offsets = shifted(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), dev, shift)
    tab = shifted(np.asarray(table, dtype=np.float64), dev, shift)
    U = len(table) + 2 if U_max is None else U_max
    present = torch.full((B * _hip.SN_CLASS_WORDS + shift,), -1, dtype=torch.int32, device=dev)[shift:]
    bad = sentinel(B, SENT_I, torch.int64, dev, shift)
    n_unique = sentinel(B, SENT_I, torch.int64, dev, shift)
    short = sentinel(B, SENT_I, torch.int64, dev, shift)
    unique = torch.full((B * U + shift,), SENT_F, dtype=torch.float64, device=dev)[shift:].reshape(B, U)
    colors = sentinel(total * 3, SENT_F, torch.float64, dev, shift) if want_colors else None
    rgb = sentinel(total * 3, SENT_U16, torch.int16, dev, shift) if want_rgb else None
    _hip.class_census(cls, offsets, present, bad[:B])
    _hip.class_paint(cls, offsets, present, tab, colors, rgb, unique, n_unique[:B], short[:B])
    torch.cuda.synchronize()
    get = lambda x: None if x is None else x.cpu().numpy()   # noqa: E731
    out = dict(bad=get(bad), n_unique=get(n_unique), short=get(short), unique=get(unique), colors=get(colors),
               rgb=None if rgb is None else get(rgb).view(np.uint16), present=get(present).view(np.uint32).reshape(B, -1), n=n)
    for name in ("bad", "n_unique", "short"):
        assert np.all(out[name][B:] == SENT_I), name
    return out


def check_paint(out, class_tiles, table):
    n, start = out["n"], 0
    for b, c in enumerate(class_tiles):
        colors, unique, bad, short = kc.expected_colors(c, table)
        sl = slice(start, start + len(c))
        if out["colors"] is not None:
            assert np.array_equal(kc.bits(out["colors"][:3 * n].reshape(n, 3)[sl]), kc.bits(colors)), b
        if out["rgb"] is not None:
            assert np.array_equal(out["rgb"][:3 * n].reshape(n, 3)[sl], kc.rgb16(colors)), b
        assert out["bad"][b] == bad and out["short"][b] == short and out["n_unique"][b] == len(unique), b
        U = out["unique"].shape[1]
        k = min(U, len(unique))
        assert np.array_equal(kc.bits(out["unique"][b, :k]), kc.bits(unique[:k])) and np.all(out["unique"][b, k:] == SENT_F)
        want = np.zeros(_hip.SN_CLASS_WORDS, dtype=np.uint32)
        np.bitwise_or.at(want, unique.astype(np.int64) >> 5, np.uint32(1) << (unique.astype(np.int64) & 31).astype(np.uint32))
        assert np.array_equal(out["present"][b], want)
        start += len(c)
    if out["colors"] is not None:
        assert np.all(out["colors"][3 * n:] == SENT_F), "rows beyond offsets[B] were touched"
    if out["rgb"] is not None:
        assert np.all(out["rgb"][3 * n:] == SENT_U16), "rows beyond offsets[B] were touched"


def test_golden_colours(hip_device):
    gold = np.load(kc.GOLDEN)
    for name in gold["names"]:
        classes, table, want = gold[f"{name}_classes"], gold[f"{name}_table"], gold[f"{name}_colors"]
        cc = sna.class_colors(torch.from_numpy(classes).to(hip_device), table)
        assert cc.rgb is None and np.array_equal(kc.bits(cc.colors.cpu().numpy()), kc.bits(want)), name
        assert cc.bad.cpu().tolist() == [0] and cc.short_table.cpu().tolist() == [0]
        u = np.unique(classes)
        assert cc.n_unique.cpu().tolist() == [len(u)]
        assert np.array_equal(cc.unique.cpu().numpy()[0, :len(u)], u.astype(np.float64))
        assert np.isnan(cc.unique.cpu().numpy()[0, len(u):]).all()
        pcd = type("Cloud", (), {})()
        got = sna.color_pointcloud(pcd, classes, class_color=table)              # the reference's call, arrays in
        assert got.is_cuda and pcd.colors is got and np.array_equal(kc.bits(got.cpu().numpy()), kc.bits(want)), name
        out = run_paint(hip_device, [classes.astype(np.float64)], table, shift=1)
        check_paint(out, [classes.astype(np.float64)], table)
        assert np.array_equal(kc.bits(out["colors"][:3 * len(classes)].reshape(-1, 3)), kc.bits(want))


def test_class_vectors_on_the_chunk_seams(hip_device):
    c = _hip.class_chunk_points()
    rng = np.random.default_rng(186)
    table = rng.integers(0, 256, (40, 3)) / 255
    for total in (1, 255, 257, c - 1, c, c + 1, 2 * c + 3):
        classes = kc.KITTI_IDS[rng.integers(0, len(kc.KITTI_IDS), total)]
        for shift, colors, rgb in ((0, True, True), (1, True, False), (1, False, True)):
            check_paint(run_paint(hip_device, [classes], table, shift=shift, want_colors=colors, want_rgb=rgb), [classes], table)
    # tiles that end one row before, on and one row behind a seam; a class that only shows in the rows behind the seam
    sizes = [c - 1, 1, 1, c + 2, 3]
    tiles = [kc.LAS_CLASSES[rng.integers(0, 8, n)] for n in sizes]
    tiles[3][-2:] = 255.0
    check_paint(run_paint(hip_device, tiles, table), tiles, table)


def test_batch_with_other_classes_per_tile_invalid_rows_and_a_short_table(hip_device):
    rng = np.random.default_rng(187)
    a = kc.LAS_CLASSES[rng.integers(0, len(kc.LAS_CLASSES), 1001)]               # an odd start offset behind it
    b = np.array([65535.0])
    c = kc.KITTI_IDS[rng.integers(0, 12, 3000)]
    c[rng.integers(0, 3000, 40)] = np.nan
    c[[5, 77, 2999]] = [2.5, -1.0, 65536.0]
    c[[6, 78]] = [-0.5, 1e300]
    table = rng.integers(0, 256, (len(np.unique(a)), 3)) / 255                    # serves tile 0 exactly ...
    assert len(np.unique(a)) == 16
    tiles = [a, b, c]
    exp = [kc.expected_colors(t, table) for t in tiles]
    assert [e[2] for e in exp] == [0, 0, int(np.isnan(c).sum()) + 5] and [e[3] for e in exp] == [0, 0, 0]
    for shift in (0, 1):
        check_paint(run_paint(hip_device, tiles, table, shift=shift), tiles, table)
    short = table[:-1]                                                            # ... and one row too short
    exp = [kc.expected_colors(t, short) for t in tiles]
    assert exp[0][3] == int((a == 255.0).sum()) > 0 and exp[2][3] == 0 and np.isnan(exp[0][0]).any()
    out = run_paint(hip_device, tiles, short, U_max=4)                            # and fewer columns than classes
    check_paint(out, tiles, short)
    # the layer above: counted, not raised, by class_colors; raised by the reference's mirror
    packed = torch.from_numpy(np.concatenate(tiles)).to(hip_device)
    offsets = torch.tensor([0, 1001, 1002, 4002], dtype=torch.int64, device=hip_device)
    cc = sna.class_colors(packed, short, offsets=offsets, las=True)
    assert cc.colors is None and cc.rgb.dtype == torch.uint16 and tuple(cc.rgb.shape) == (4002, 3)
    assert cc.bad.cpu().tolist() == [e[2] for e in exp] and cc.short_table.cpu().tolist() == [e[3] for e in exp]
    assert np.array_equal(cc.rgb.cpu().view(torch.int16).numpy().view(np.uint16), kc.rgb16(np.concatenate([e[0] for e in exp])))
    for classes, tab in ((c, table), (a, short)):
        with pytest.raises(IndexError):
            sna.color_pointcloud(None, torch.from_numpy(classes).to(hip_device), class_color=tab)
    with pytest.raises(sna.HipLibraryError):
        sna.class_colors(torch.from_numpy(a), table)                              # a CPU tensor: there is no CPU path


def test_color_pointcloud_draws_the_seeded_table(hip_device, tmp_path):
    rng = np.random.default_rng(188)
    classes = kc.LAS_CLASSES[rng.integers(0, 9, 2500)]
    np.random.seed(77)
    table = np.random.choice(256, size=(len(np.unique(classes)), 3)) / 255
    np.random.seed(77)
    got = sna.color_pointcloud(None, torch.from_numpy(classes).to(hip_device))
    assert np.array_equal(kc.bits(got.cpu().numpy()), kc.bits(kc.colors_loop(classes, table)))
    import pickle
    path = str(tmp_path / "class_colors")
    with open(path, "wb") as f:
        pickle.dump(table, f)
    pcd = type("Cloud", (), {})()
    assert np.array_equal(sna.color_pointcloud(pcd, None, load=True, pck_name=path), table) and pcd.colors is not None


# ================================================================ capture, a file
def test_captured_grid_census_and_paint_give_the_eager_bits(hip_device):
    dev, dims = hip_device, (5, 7, 3)
    rng = np.random.default_rng(189)
    tiles = [kc.cube_tile(1500, 81), kc.cube_tile(900, 82)]
    total, B, V = 2400, 2, 105
    desc = torch.from_numpy(np.stack([kc.own_desc(t, dims) for t in tiles])).to(dev)
    pts = torch.from_numpy(np.concatenate(tiles)).to(dev)
    offsets = torch.tensor([0, 1500, 2400], dtype=torch.int64, device=dev)
    inputs = [(kc.special_labels(total, rng), kc.LAS_CLASSES[rng.integers(0, 4 + 6 * k, total)]) for k in range(2)]
    table = torch.from_numpy(rng.integers(0, 256, (12, 3)) / 255).to(dev)
    lab = torch.empty(total, dtype=torch.float64, device=dev)
    cls = torch.empty(total, dtype=torch.float64, device=dev)
    grid = torch.empty((B, V), dtype=torch.float64, device=dev)
    i64 = lambda: torch.empty(B, dtype=torch.int64, device=dev)   # noqa: E731
    unb, nans, bad, n_unique, short = i64(), i64(), i64(), i64(), i64()
    present = torch.empty((B, _hip.SN_CLASS_WORDS), dtype=torch.int32, device=dev)
    unique = torch.empty((B, 12), dtype=torch.float64, device=dev)
    colors = torch.empty((total, 3), dtype=torch.float64, device=dev)
    rgb = torch.empty((total, 3), dtype=torch.int16, device=dev)
    outs = (grid, unb, nans, bad, n_unique, short, present, unique, colors, rgb)
    names = ("grid", "unbinned", "nan_labels", "bad", "n_unique", "short_table", "present", "unique", "colors", "rgb")

    def launch():
        _hip.voxel_classes(pts, lab, offsets, desc, dims, grid, unb, nans)
        _hip.class_census(cls, offsets, present, bad)
        _hip.class_paint(cls, offsets, present, table, colors, rgb, unique, n_unique, short)

    def snapshot():
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in outs]

    def load(k):
        lab.copy_(torch.from_numpy(inputs[k][0]))
        cls.copy_(torch.from_numpy(inputs[k][1]))
        for t in outs:
            t.view(torch.uint8).fill_(0x5a)

    load(0)
    launch()                                                     # (eager first: the kernels are loaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    seen = []
    for k in (0, 1, 0):
        load(k)
        graph.replay()
        replayed = snapshot()
        load(k)
        launch()
        eager = snapshot()
        for name, a, b in zip(names, replayed, eager):
            assert a.tobytes() == b.tobytes(), (name, k, a.reshape(-1)[:4], b.reshape(-1)[:4])
        labels = [inputs[k][0][:1500], inputs[k][0][1500:]]
        exp = kc.expected_grid(desc.cpu().numpy(), dims, tiles, labels)
        assert np.array_equal(kc.bits(replayed[0].reshape(exp[0].shape)), kc.bits(exp[0]))
        want = np.concatenate([kc.expected_colors(c, table.cpu().numpy())[0] for c in (inputs[k][1][:1500], inputs[k][1][1500:])])
        assert np.array_equal(kc.bits(replayed[8]), kc.bits(want))
        seen.append(replayed[8].tobytes())
    assert seen[0] == seen[2] and seen[0] != seen[1]


def test_scan_written_with_its_class_colours_reads_back(hip_device, tmp_path):
    n = 2000
    rng = np.random.default_rng(190)
    xyz = np.round(rng.random((n, 3)) * 50.0, 3)
    classes = kc.LAS_CLASSES[rng.integers(0, 13, n)]                             # <= 18: the legacy formats hold them
    table = rng.integers(0, 256, (13, 3)) / 255
    d_xyz, d_cls = torch.from_numpy(xyz).to(hip_device), torch.from_numpy(classes).to(hip_device)
    cc = sna.class_colors(d_cls, table, las=True)
    path = str(tmp_path / "coloured.las")
    written = sna.write_las(path, d_xyz, classes=d_cls, rgb=cc.rgb, scale=(0.001, 0.001, 0.001), offset=(0.0, 0.0, 0.0))
    assert written.point_format == 2 and written.n_points == n
    scan = sna.read_las(path, device=hip_device)
    assert np.array_equal(scan.classes.cpu().numpy(), classes) and scan.xyz.shape == (n, 3)
    raw = np.fromfile(path, dtype=np.uint8)[written.data_offset:].reshape(n, written.record_length)
    rgb = np.ascontiguousarray(raw[:, 20:26]).view("<u2")
    want = kc.rgb16(kc.colors_loop(classes, table))
    assert np.array_equal(rgb, want) and len(np.unique(rgb, axis=0)) >= 10
