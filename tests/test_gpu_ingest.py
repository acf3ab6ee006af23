"""sn_tiles_unpack against numpy: every output bit-equal, `bad` equal to numpy's per-tile count, nothing written beyond
`total`.  Tile sizes put tile boundaries inside a vector, a wave and a workgroup; the last tile spans several workgroups."""
import numpy as np
import pytest
import torch

from scene_net_amd import _hip

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1025, 20011]
CANARY = -7.25


def _rows(cols, dtype, total, seed):
    """Raw rows at UTM magnitudes with the special values sprinkled through every column."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((total, cols))
    a[:, 0] += 5.44e5
    a[:, 1] += 4.634e6
    a[:, -1] = rng.integers(0, 20, total)
    a = a.astype(dtype)
    bits = a.view(np.uint64 if dtype == np.float64 else np.uint32).reshape(-1)
    if dtype == np.float64:
        special = [0x7ff8000000abc123, 0xfff4000000000001, 0x7ff0000000000000, 0xfff0000000000000, 0x8000000000000000,
                   0x0000000000000001, 0x800fffffffffffff]
    else:
        special = [0x7fc0a123, 0xffa00001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff, 0x00400000]
    where = rng.choice(bits.size, size=min(bits.size, 40 * len(special)), replace=False)
    for k, w in enumerate(where):
        bits[w] = special[k % len(special)]
    # the first and the last element carry one each (tile 0 of one point; the last point: the pair kernel's lone tail
    # point when `total` is odd, see test_unpack_odd_total_tail)
    bits[0] = special[0]
    bits[bits.size - 1] = special[2]
    return a


def _reference(a, offsets, with_labels):
    with np.errstate(invalid="ignore"):
        pts = np.ascontiguousarray(a[:, :3]).astype(np.float64)
        lab = a[:, -1].astype(np.float64) if with_labels else None
    read = pts if lab is None else np.concatenate([pts, lab[:, None]], axis=1)
    nf = ~np.isfinite(read).all(axis=1)
    bad = np.array([int(nf[offsets[b]:offsets[b + 1]].sum()) for b in range(len(offsets) - 1)], dtype=np.int32)
    return pts, lab, bad


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cols,with_labels", [(4, True), (5, True), (7, True), (3, False), (4, False)])
@pytest.mark.parametrize("misalign", [0, 1])
def test_unpack_bits_bad_and_canaries(hip_device, B, dtype, cols, with_labels, misalign):
    sizes = SIZES if B != 1 else [sum(SIZES)]
    sizes = (sizes * ((B + len(sizes) - 1) // len(sizes)))[:B] if B != 1 else sizes
    _check_unpack(hip_device, sizes, dtype, cols, with_labels, misalign)


@pytest.mark.parametrize("sizes", [[1], [3], SIZES + [7], [sum(SIZES) + 1]], ids=["1", "3", "22009-in-12", "22003-in-1"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("with_labels", [True, False])
def test_unpack_odd_total_tail(hip_device, sizes, dtype, with_labels):
    """cols == 4, aligned, an ODD total: the pair kernel moves its last point alone.  That point carries an infinity in
    its last column (counted in `bad` only when labels are read) and the canaries sit right behind it."""
    assert sum(sizes) % 2 == 1
    _check_unpack(hip_device, sizes, dtype, 4, with_labels, 0)


def _check_unpack(hip_device, sizes, dtype, cols, with_labels, misalign):
    B = len(sizes)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(offsets[-1])
    a = _rows(cols, dtype, total, seed=cols * 100 + B)
    pts_ref, lab_ref, bad_ref = _reference(a, offsets, with_labels)
    assert bad_ref.sum() > 0
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    # rows base 16-byte aligned (a fresh allocation) or moved on by one element
    store = torch.zeros(total * cols + 4, dtype=tdt, device=hip_device)
    assert store.data_ptr() % 16 == 0
    rows = store[misalign:misalign + total * cols].view(total, cols)
    rows.copy_(torch.from_numpy(a))
    assert rows.data_ptr() % 16 == (misalign * a.itemsize)
    pad = 64
    pts = torch.full(((total + pad) * 3,), CANARY, dtype=torch.float64, device=hip_device)
    labels = torch.full((total + pad,), CANARY, dtype=torch.float64, device=hip_device) if with_labels else None
    d_off = torch.from_numpy(offsets).to(hip_device)
    bad = torch.full((B,), 12345, dtype=torch.int32, device=hip_device)
    _hip.tiles_unpack(rows, pts, labels, d_off, bad)
    torch.cuda.synchronize()
    assert np.array_equal(_u64(pts[:total * 3]), pts_ref.reshape(-1).view(np.uint64))
    assert np.array_equal(_u64(pts[total * 3:]), np.full(pad * 3, CANARY).view(np.uint64))
    if with_labels:
        assert np.array_equal(_u64(labels[:total]), lab_ref.view(np.uint64))
        assert np.array_equal(_u64(labels[total:]), np.full(pad, CANARY).view(np.uint64))
    assert np.array_equal(bad.cpu().numpy(), bad_ref)
    _hip.tiles_unpack(rows, pts, labels, d_off, bad)      # a second call overwrites the counts
    torch.cuda.synchronize()
    assert np.array_equal(bad.cpu().numpy(), bad_ref)
    _hip.tiles_unpack(rows, pts, labels)                   # without offsets / bad
    torch.cuda.synchronize()
    assert np.array_equal(_u64(pts[:total * 3]), pts_ref.reshape(-1).view(np.uint64))


def test_unpack_f32_widening_of_every_exponent(hip_device):
    """All 256 exponent fields x both signs x a few mantissas, denormals and NaN payloads included: the widening is numpy's."""
    mant = np.array([0, 1, 2, 0x400000, 0x400001, 0x7fffff, 0x2aaaaa, 0x000100], dtype=np.uint32)
    e = np.arange(256, dtype=np.uint32)[:, None, None] << 23
    s = np.array([0, 1], dtype=np.uint32)[None, :, None] << 31
    bits = (e | s | mant[None, None, :]).reshape(-1)
    a = bits.view(np.float32).reshape(-1, 4).copy()
    with np.errstate(invalid="ignore"):
        ref = a.astype(np.float64)
    rows = torch.from_numpy(a).to(hip_device)
    pts = torch.zeros((a.shape[0], 3), dtype=torch.float64, device=hip_device)
    lab = torch.zeros((a.shape[0],), dtype=torch.float64, device=hip_device)
    _hip.tiles_unpack(rows, pts, lab)
    torch.cuda.synchronize()
    assert np.array_equal(_u64(pts), np.ascontiguousarray(ref[:, :3]).view(np.uint64))
    assert np.array_equal(_u64(lab), np.ascontiguousarray(ref[:, 3]).view(np.uint64))


def test_unpack_past_2_31_bytes(hip_device):
    """70,000,000 f64 rows of 4 columns: 2.24 GB of rows, byte offsets past 2^31."""
    free, _ = torch.cuda.mem_get_info()
    if free < 8 * 2**30:
        pytest.skip(f"needs 8 GB of free device memory for 2.24 GB of rows and their outputs ({free / 2**30:.1f} GB free)")
    total = 70_000_000
    raw = torch.rand((total, 4), dtype=torch.float64, device=hip_device)
    pts = torch.empty((total, 3), dtype=torch.float64, device=hip_device)
    lab = torch.empty((total,), dtype=torch.float64, device=hip_device)
    offsets = torch.tensor([0, 33_554_433, total], dtype=torch.int64, device=hip_device)
    bad = torch.full((2,), -1, dtype=torch.int32, device=hip_device)
    _hip.tiles_unpack(raw, pts, lab, offsets, bad)
    torch.cuda.synchronize()
    assert torch.equal(lab, raw[:, 3])
    del lab
    assert torch.equal(pts, raw[:, :3].contiguous())
    assert bad.tolist() == [0, 0]
