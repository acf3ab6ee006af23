"""SemanticKITTI decode (K14), host side: the numpy oracle against hand-written values, the scan listing against a
restatement of the reference's slice arithmetic, the reader's size checks, the lut rule, the module surface and the
argument checks of sn_kitti_decode.  No GPU."""
import ctypes
import math
import os

import numpy as np
import pytest

import scene_net_amd as sna
from scene_net_amd import kitti as sk

import kitti_cases as kc


# ---- the oracle against hand-written values ----------------------------------------------------------------------------
def test_oracle_edge_words_by_hand():
    w = kc.edge_words()
    assert w.tolist() == [0, 0xFFFF, 0x10000, 0xFFFF0050, 0xFFFFFFFF, 80 | 7 << 16]
    rows = np.zeros((6, 4), dtype="<f4")
    got = kc.decode_oracle(rows.tobytes(), w.astype("<u4").tobytes(), [6], None, 260)
    assert got["labels"].tolist() == [0.0, 65535.0, 0.0, 80.0, 65535.0, 80.0]
    assert got["instance"].tolist() == [0, 0, 1, 65535, 65535, 7] and got["instance"].dtype == np.int32
    want = np.zeros(260, dtype=np.int64)
    want[0], want[80] = 2, 2                                       # 65535 >= 260: not counted
    assert np.array_equal(got["hist"][0], want)
    assert got["unmapped"] is None and got["bad"].tolist() == [0]
    # a remap of 81 entries: 0 -> 5, 80 -> -7; 65535 is beyond it
    lut = np.full(81, -1, dtype=np.int32)
    lut[0], lut[80] = 5, -7
    got = kc.decode_oracle(rows.tobytes(), w.astype("<u4").tobytes(), [2, 0, 4], lut, 6)
    assert got["labels"].tolist() == [5.0, -1.0, 5.0, -7.0, -1.0, -7.0]
    assert got["unmapped"].tolist() == [1, 0, 1]
    assert got["hist"].tolist() == [[0, 0, 0, 0, 0, 1], [0] * 6, [0, 0, 0, 0, 0, 1]]


def test_oracle_edge_floats_by_hand():
    e = kc.edge_floats()
    want = {0x00000000: 0x0000000000000000, 0x80000000: 0x8000000000000000,
            0x00000001: 0x36A0000000000000,                       # 2^-149
            0x80000001: 0xB6A0000000000000,
            0x007FFFFF: 0x380FFFFFC0000000,                       # (2^23 - 1) * 2^-149
            0x00400000: 0x3800000000000000,                       # 2^-127
            0x7F800000: 0x7FF0000000000000, 0xFF800000: 0xFFF0000000000000,
            0x7FC00000: 0x7FF8000000000000, 0xFFC00000: 0xFFF8000000000000,
            0x7FC12345: 0x7FF82468A0000000,
            0x7F800001: 0x7FF8000020000000,                       # a signalling NaN: quietened, payload kept
            0xFF800001: 0xFFF8000020000000,
            0x7F7FFFFF: 0x47EFFFFFE0000000,                       # FLT_MAX
            0x00800000: 0x3810000000000000, 0x3F800000: 0x3FF0000000000000}
    assert set(want) <= set(e.tolist())
    rows = np.zeros((e.size, 4), dtype=np.uint32)
    rows[:, 1] = e
    got = kc.decode_oracle(rows.astype("<u4").tobytes(), None, [e.size])
    bits = got["pts"].view(np.uint64)
    for k, v in enumerate(e.tolist()):
        if v in want:
            assert int(bits[k, 1]) == want[v], hex(v)
    assert got["labels"] is None and got["instance"] is None and got["hist"] is None
    nonfinite = [(v & 0x7F800000) == 0x7F800000 for v in e.tolist()]
    assert got["bad"].tolist() == [sum(nonfinite)] and sum(nonfinite) == 9
    # the remission column is carried bit for bit and is no part of `bad`
    rows[:, 1], rows[:, 3] = 0, e
    got = kc.decode_oracle(rows.astype("<u4").tobytes(), None, [e.size])
    assert np.array_equal(got["remission"].view(np.uint32), e) and got["bad"].tolist() == [0]


def test_edge_scan_holds_every_edge_in_every_column():
    b, l, n = kc.edge_scan()
    rows = np.frombuffer(b, dtype="<u4").reshape(n, 4)
    for col in range(4):
        assert set(kc.edge_floats().tolist()) <= set(rows[:, col].tolist())
    assert set(np.frombuffer(l, dtype="<u4").tolist()) == set(kc.edge_words().tolist())


# ---- the listing -------------------------------------------------------------------------------------------------------
def _reference_lists(root, split):
    """semKITTI.py:332-381, restated"""
    scans, labels = [], []
    for seq in np.arange(0, 21):
        seq = "{0:02d}".format(seq)
        sp = os.path.join(root, "sequences", seq, "velodyne")
        if not os.path.isdir(sp):
            continue
        scans += [os.path.join(dp, f) for dp, dn, fn in os.walk(sp) for f in fn]
        lp = os.path.join(root, "sequences", seq, "labels")
        if not os.path.isdir(lp):
            continue
        labels += [os.path.join(dp, f) for dp, dn, fn in os.walk(lp) for f in fn]
    scans, labels = np.sort(np.array(scans)), np.sort(np.array(labels))
    assert len(scans) == len(labels)
    beg, end = {"samples": [0.0, 1.0], "train": [0.0, 0.2], "val": [0.2, 0.4], "test": [0.4, 1.0]}[split]
    return (scans[math.floor(beg * scans.size):math.floor(end * scans.size)].tolist(),
            labels[math.floor(beg * labels.size):math.floor(end * labels.size)].tolist())


def _tree(tmp_path, counts=(("00", 7), ("03", 1), ("11", 5))):
    root = str(tmp_path / "kitti")
    for seq, n in counts:
        kc.write_sequence(root, seq, [kc.random_scans([3], seed=k) for k in range(n)])
    return root


@pytest.mark.parametrize("split", ["samples", "train", "val", "test"])
def test_scan_lists_follow_the_references_slices(tmp_path, split):
    root = _tree(tmp_path)
    got = sna.kitti_scan_lists(root, split)
    assert got == _reference_lists(root, split)
    assert len(got[0]) == len(got[1]) == {"samples": 13, "train": 2, "val": 3, "test": 8}[split]
    assert all(a.endswith(".bin") and b.endswith(".label") and os.path.basename(a)[:6] == os.path.basename(b)[:6]
               for a, b in zip(*got))


def test_scan_lists_missing_labels_folder(tmp_path):
    root = _tree(tmp_path)
    kc.write_sequence(root, "05", [kc.random_scans([2], seed=9)], with_labels=False)
    with pytest.raises(ValueError, match="labels"):
        sna.kitti_scan_lists(root)
    scans, labels = sna.kitti_scan_lists(root, labels=False)
    assert len(scans) == 14 and labels == []
    with pytest.raises(ValueError, match="split"):
        sna.kitti_scan_lists(root, "fit")


# ---- the reader's size checks ------------------------------------------------------------------------------------------
def test_size_checks_name_the_file(tmp_path):
    root = str(tmp_path)
    bins, labels = kc.write_sequence(root, "00", [kc.random_scans([5], seed=1), kc.random_scans([4], seed=2)])
    assert sk.scan_sizes(bins, labels) == [5, 4] and sk.scan_sizes(bins) == [5, 4]
    with open(bins[1], "ab") as f:
        f.write(b"\0" * 8)
    with pytest.raises(ValueError, match=r"000001\.bin.*multiple of 16"):
        sk.scan_sizes(bins, labels)
    with open(bins[1], "ab") as f:
        f.write(b"\0" * 8)                           # five points now, four labels
    with pytest.raises(ValueError, match=r"000001\.label: 4 labels for the 5 points"):
        sk.scan_sizes(bins, labels)
    with open(labels[0], "ab") as f:
        f.write(b"\0" * 2)
    with pytest.raises(ValueError, match=r"000000\.label.*multiple of 4"):
        sk.scan_sizes(bins, labels)
    with pytest.raises(ValueError, match="label files"):
        sk.scan_sizes(bins, labels[:1])


def test_batch_plan_and_its_limit():
    sizes = [5, 4, 0, 7, 1]
    assert sk.plan_batches(sizes, 20, 64 << 20) == [(0, 5)]
    assert sk.plan_batches(sizes, 20, 180) == [(0, 3), (3, 5)]
    assert sk.plan_batches(sizes, 20, 140) == [(0, 1), (1, 3), (3, 4), (4, 5)]
    assert sk.plan_batches([], 20, 100) == []
    with pytest.raises(ValueError, match=r"c\.bin.*batch_bytes = 139"):
        sk.plan_batches(sizes, 20, 139, ["a.bin", "b.bin", "e.bin", "c.bin", "d.bin"])
    assert sk.plan_batches([0] * (sk.KITTI_MAX_BATCH_SCANS + 1), 20, 100) == [(0, sk.KITTI_MAX_BATCH_SCANS),
                                                                            (sk.KITTI_MAX_BATCH_SCANS, sk.KITTI_MAX_BATCH_SCANS + 1)]


# ---- the lut rule ------------------------------------------------------------------------------------------------------
def test_lut_dict_becomes_an_array_filled_with_minus_one():
    a = sna.lut_array({0: 0, 80: 18, 5: -3})
    assert a.dtype == np.int32 and a.shape == (81,) and a.flags.c_contiguous
    want = np.full(81, -1)
    want[0], want[80], want[5] = 0, 18, -3
    assert np.array_equal(a, want)
    assert np.array_equal(sna.lut_array(np.arange(7, dtype=np.int64)), np.arange(7)) and sna.lut_array(None) is None
    assert sna.lut_array({65535: 1}).shape == (65536,)
    for bad in ({}, {-1: 0}, {65536: 0}, np.zeros((2, 2), dtype=np.int32), np.zeros(3), np.zeros(0, dtype=np.int32),
                np.zeros(65537, dtype=np.int32), {1: 2**31}):
        with pytest.raises(ValueError):
            sna.lut_array(bad)


def test_module_surface():
    for name in ("KittiReader", "KittiScans", "read_kitti_scan", "kitti_scan_lists", "semKITTI", "build_pole_samples",
                 "build_pole_radius_samples", "lut_array"):
        assert hasattr(sna, name) and name in sna.__all__
    assert sk.KITTI_SPLITS == {"samples": (0.0, 1.0), "train": (0.0, 0.2), "val": (0.2, 0.4), "test": (0.4, 1.0)}
    fields = list(sna.KittiScans.__dataclass_fields__)
    assert fields == ["pts", "labels", "offsets", "sizes", "remission", "instance", "hist", "bad", "unmapped", "paths"]


# ---- the entry's argument checks ---------------------------------------------------------------------------------------
def test_entry_argument_checks_need_no_gpu():
    from scene_net_amd import _hip
    lib = _hip.load()
    buf = ctypes.create_string_buffer(512)
    base = ctypes.cast(buf, ctypes.c_void_p).value
    base += (-base) % 16
    p = ctypes.c_void_p(base)

    def call(scans=p, words=p, total=1, offsets=p, B=1, lut=None, n_lut=0, pts=p, labels=p, remission=None, instance=None,
             hist=None, n_hist=0, bad=None, unmapped=None):
        return lib.sn_kitti_decode(scans, words, total, offsets, B, lut, n_lut, pts, labels, remission, instance, hist,
                                   n_hist, bad, unmapped, None)

    INVALID, UNSUPPORTED = -1, -2
    assert call(scans=None) == INVALID and b"scans" in lib.sn_last_error()
    assert call(pts=None) == INVALID and b"pts" in lib.sn_last_error()
    assert call(offsets=None) == INVALID and b"offsets" in lib.sn_last_error()
    assert call(total=0) == INVALID and call(total=-3) == INVALID and b"total" in lib.sn_last_error()
    assert call(B=0) == INVALID and call(B=-1) == INVALID
    assert call(words=None) == INVALID and b"labels need label_words" in lib.sn_last_error()
    assert call(labels=None) == INVALID and b"label_words need labels" in lib.sn_last_error()
    assert call(words=None, labels=None, instance=p) == INVALID and b"instance" in lib.sn_last_error()
    assert call(words=None, labels=None, lut=p, n_lut=4) == INVALID and b"lut needs" in lib.sn_last_error()
    assert call(words=None, labels=None, hist=p, n_hist=4) == INVALID and b"hist needs" in lib.sn_last_error()
    for n_lut in (0, -1, 65537):
        assert call(lut=p, n_lut=n_lut) == INVALID and b"n_lut" in lib.sn_last_error()
    for n_hist in (0, -1, 1025):
        assert call(hist=p, n_hist=n_hist) == INVALID and b"n_hist" in lib.sn_last_error()
    assert call(unmapped=p) == INVALID and b"unmapped needs lut" in lib.sn_last_error()
    odd2, odd4 = ctypes.c_void_p(base + 2), ctypes.c_void_p(base + 4)
    for kw in ({"scans": odd2}, {"words": odd2}, {"lut": odd2, "n_lut": 4}, {"remission": odd2}, {"instance": odd2},
               {"bad": odd2}, {"lut": p, "n_lut": 4, "unmapped": odd2}, {"pts": odd4}, {"labels": odd4},
               {"hist": odd4, "n_hist": 4}, {"offsets": odd4}):
        assert call(**kw) == INVALID and b"aligned" in lib.sn_last_error(), kw
    assert call(total=2**36 + 1) == UNSUPPORTED and b"2^36" in lib.sn_last_error()
    assert call(B=2**20 + 1) == UNSUPPORTED and b"2^20" in lib.sn_last_error()
    assert _hip.kitti_chunk_points() == lib.sn_kitti_chunk_points() >= 64
