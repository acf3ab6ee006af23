"""SemanticKITTI decode on the device (K14: sn_kitti_decode, scene_net_amd.kitti) against the numpy oracle of kitti_cases
-- np.frombuffer, `& 0xFFFF`, `>> 16`, astype(float64), the remap, np.bincount per scan.  Every comparison is bit for bit:
fp64 as int64 views, fp32 as int32 views, counts as they are.  Every raw call reads inputs that lie at a chosen residue
mod 16 inside a larger buffer of junk bytes and writes sentinel-filled outputs with guard words on both sides."""
import io
import itertools
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import kitti_cases as kc

pytestmark = pytest.mark.gpu

SENTINEL64 = 0x5A5A5A5A5A5A5A5A
SENTINEL32 = 0x5A5A5A5A
GUARD = 64
GRID_CAP = 2048      # csrc/kitti.hip kMaxBlocks: more chunks than this and a workgroup takes several consecutive ones


def _place(dev, raw, residue):
    """`raw` (bytes) on the device at an address that is `residue` mod 16, junk bytes in front of and behind it"""
    raw = np.frombuffer(bytes(raw), dtype=np.uint8)
    junk = np.random.default_rng(raw.size + residue).integers(0, 256, raw.size + 160, dtype=np.uint8)
    big = torch.from_numpy(junk).to(dev)
    start = 64 + (residue - (big.data_ptr() + 64)) % 16
    big[start:start + raw.size] = torch.from_numpy(raw.copy()).to(dev)
    view = big[start:start + raw.size]
    assert view.data_ptr() % 16 == residue and view.is_contiguous()
    return big, view


def _guarded(n, dev, dtype, shift=0):
    """(whole buffer, the n elements inside it): GUARD sentinel elements on both sides, the inside sentinel too; `shift`
    elements move the inside off the buffer's 16-byte alignment"""
    buf = torch.full((n + 2 * GUARD + shift,), SENTINEL64 if dtype == torch.int64 else SENTINEL32, dtype=dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + shift:GUARD + shift + n]


def _guards_intact(name, buf, inside, shift):
    b = buf.cpu().numpy()
    s = SENTINEL64 if b.dtype == np.int64 else SENTINEL32
    lo = GUARD + shift
    assert np.all(b[:lo] == s) and np.all(b[lo + inside.numel():] == s), f"{name}: guard words were written"


class Run:
    """one sn_kitti_decode call and what it left"""

    def __init__(self, dev, bin_bytes, label_bytes, sizes, lut=None, n_hist=0, res_scans=0, res_words=0, shift64=0,
                 shift32=0, want_remission=True, want_instance=True, want_bad=True, want_unmapped=True, hist0=None):
        total, B = int(sum(sizes)), len(sizes)
        self.total, self.B = total, B
        big_s, scans = _place(dev, bin_bytes, res_scans)
        big_w, words = _place(dev, label_bytes, res_words) if label_bytes is not None else (None, None)
        before = (big_s.clone(), None if big_w is None else big_w.clone())
        offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
        lut_t = None if lut is None else torch.from_numpy(np.ascontiguousarray(lut, dtype=np.int32)).to(dev)
        has_labels = label_bytes is not None
        bufs = {"pts": _guarded(3 * total, dev, torch.int64, shift64)}
        if has_labels:
            bufs["labels"] = _guarded(total, dev, torch.int64, shift64)
        if want_remission:
            bufs["remission"] = _guarded(total, dev, torch.int32, shift32)
        if want_instance and has_labels:
            bufs["instance"] = _guarded(total, dev, torch.int32, shift32)
        if n_hist and has_labels:
            bufs["hist"] = _guarded(B * n_hist, dev, torch.int64, shift64)
            bufs["hist"][1].copy_(torch.zeros(B * n_hist, dtype=torch.int64) if hist0 is None
                                  else torch.from_numpy(np.asarray(hist0, dtype=np.int64).reshape(-1)))
        if want_bad:
            bufs["bad"] = _guarded(B, dev, torch.int32, shift32)            # (left at the sentinel: WRITTEN, not added to)
        if want_unmapped and lut is not None:
            bufs["unmapped"] = _guarded(B, dev, torch.int32, shift32)
        self.shift = {k: (shift64 if v[0].dtype == torch.int64 else shift32) for k, v in bufs.items()}
        get = lambda k: bufs[k][1] if k in bufs else None   # noqa: E731
        _hip.kitti_decode(scans, words, total, offsets, get("pts").view(torch.float64),
                          None if get("labels") is None else get("labels").view(torch.float64), lut_t,
                          None if get("remission") is None else get("remission").view(torch.float32), get("instance"),
                          None if get("hist") is None else get("hist").view(B, n_hist), get("bad"), get("unmapped"))
        torch.cuda.synchronize()
        for name, (buf, inside) in bufs.items():
            _guards_intact(name, buf, inside, self.shift[name])
        assert torch.equal(big_s, before[0]) and (big_w is None or torch.equal(big_w, before[1])), "an input was written"
        self.got = {k: v[1].cpu().numpy() for k, v in bufs.items()}
        if "hist" in self.got:
            self.got["hist"] = self.got["hist"].reshape(B, n_hist)

    def assert_oracle(self, want, hist0=None, what=""):
        g = self.got
        assert np.array_equal(g["pts"].reshape(-1, 3), want["pts"].view(np.int64)), f"{what}: pts"
        if "labels" in g:
            assert np.array_equal(g["labels"], want["labels"].view(np.int64)), f"{what}: labels"
        if "remission" in g:
            assert np.array_equal(g["remission"], want["remission"].view(np.int32)), f"{what}: remission"
        if "instance" in g:
            assert np.array_equal(g["instance"], want["instance"]), f"{what}: instance"
        if "hist" in g:
            assert np.array_equal(g["hist"], want["hist"] + (0 if hist0 is None else np.asarray(hist0))), f"{what}: hist"
        if "bad" in g:
            assert np.array_equal(g["bad"], want["bad"]), f"{what}: bad"
        if "unmapped" in g:
            assert np.array_equal(g["unmapped"], want["unmapped"]), f"{what}: unmapped"


def _check(dev, sizes, seed, lut=None, n_hist=260, classes=None, what="", **kw):
    b, l = kc.random_scans(sizes, seed, classes)
    run = Run(dev, b, l, sizes, lut, n_hist, **kw)
    want = kc.decode_oracle(b, l, sizes, lut, n_hist)
    run.assert_oracle(want, what=what or f"sizes {sizes}")
    return run, want


KITTI_CLASSES = [0, 1, 10, 11, 13, 15, 16, 18, 20, 30, 31, 32, 40, 44, 48, 49, 50, 51, 52, 60, 70, 71, 72, 80, 81, 99, 252,
                 253, 254, 255, 256, 257, 258, 259]


# ---- 1. one scan on the seams of the chunk -----------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(7))
def test_one_scan_on_the_seams(hip_device, which):
    C = _hip.kitti_chunk_points()
    n = [1, 2, 3, C - 1, C, C + 1, 2 * C + 1][which]
    for j, (rs, rw) in enumerate([(0, 0), (4, 12), (8, 4)]):
        _check(hip_device, [n], seed=10 * which + j, classes=KITTI_CLASSES, res_scans=rs, res_words=rw, shift64=(which + j) % 2,
               shift32=(which + 2 * j) % 4, what=f"n={n} residues {rs}, {rw}")


# ---- 2. scan boundaries ------------------------------------------------------------------------------------------------
def test_scan_boundaries_inside_and_between_chunks(hip_device):
    C = _hip.kitti_chunk_points()
    lut = np.arange(300, dtype=np.int32)
    lut[13] = -4
    for sizes in ([1, C + 3, 0, 2, 3 * C - 1, 0], [3] * 40, [0, 5, C], [0, 0, 1], [C, C, 0, 0, C]):
        _, want = _check(hip_device, sizes, seed=len(sizes), n_hist=260, classes=KITTI_CLASSES + [300, 7000],
                         lut=lut, what=f"sizes {sizes}")
        assert sum(sizes) < 100 or (want["hist"].sum(axis=1).max() > 0 and want["unmapped"].sum() > 0)
        # a non-finite point right at every scan's first and last place
        b, l = kc.random_scans(sizes, 5, KITTI_CLASSES)
        rows = np.frombuffer(b, dtype="<u4").reshape(-1, 4).copy()
        bounds = np.cumsum([0] + sizes)
        for s, n in enumerate(sizes):
            if n:
                rows[bounds[s], s % 3] = 0x7F800000
                rows[bounds[s + 1] - 1, (s + 1) % 3] = 0xFFC00001
        want = kc.decode_oracle(rows.tobytes(), l, sizes, None, 260)
        assert want["bad"].tolist() == [min(n, 2) for n in sizes]
        Run(hip_device, rows.tobytes(), l, sizes, None, 260, res_scans=4, shift64=1).assert_oracle(want, what=f"bad, {sizes}")


# ---- 3. every residue of the bases -------------------------------------------------------------------------------------
def test_every_residue_of_the_input_and_output_bases(hip_device):
    n = _hip.kitti_chunk_points() + 5
    b, l = kc.random_scans([n], 33, KITTI_CLASSES)
    want = kc.decode_oracle(b, l, [n], None, 260)
    for rs, rw in itertools.product((0, 4, 8, 12), repeat=2):
        for shift32 in (1, 2, 3):        # remission / instance at 4, 8 and 12 mod 16; pts / labels at 8 mod 16
            Run(hip_device, b, l, [n], None, 260, res_scans=rs, res_words=rw, shift64=1, shift32=shift32).assert_oracle(
                want, what=f"scans {rs} words {rw} shift32 {shift32}")


# ---- 4. edge values ----------------------------------------------------------------------------------------------------
def test_edge_floats_and_edge_words(hip_device):
    b, l, n = kc.edge_scan()
    e = kc.edge_floats()
    nonfinite = int(sum((int(v) & 0x7F800000) == 0x7F800000 for v in e))
    for sizes in ([n], [len(e), len(e), len(e), len(e), 1]):
        want = kc.decode_oracle(b, l, sizes, None, 1024)
        if len(sizes) == 5:   # one scan per column: the non-finite remissions of the fourth are not counted
            assert want["bad"].tolist() == [nonfinite, nonfinite, nonfinite, 0, 1]
        for rs in (0, 4):
            run = Run(hip_device, b, l, sizes, None, 1024, res_scans=rs, res_words=8)
            run.assert_oracle(want, what=f"edges, sizes {sizes}")
    # the signalling NaN of the issue, by hand
    k = e.tolist().index(0x7F800001)
    assert int(run.got["pts"].reshape(-1, 3)[k, 0]) == 0x7FF8000020000000
    assert run.got["instance"][:6].tolist() == [0, 0, 1, 65535, 65535, 7]
    assert run.got["labels"][:6].view(np.float64).tolist() == [0.0, 65535.0, 0.0, 80.0, 65535.0, 80.0]


# ---- 5. the remap and the census widths --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["identity", "negative", "one", "full"])
def test_lut(hip_device, case):
    C = _hip.kitti_chunk_points()
    sizes = [C + 7, 0, 2 * C - 3]
    rng = np.random.default_rng(3)
    lut = {"identity": np.arange(300, dtype=np.int32),
           "negative": rng.integers(-5, 40, 300).astype(np.int32),
           "one": np.array([7], dtype=np.int32),
           "full": rng.integers(-2**31, 2**31, 65536).astype(np.int32)}[case]
    if case == "full":
        lut[:300] = rng.integers(0, 1030, 300)
    classes = None if case == "full" else KITTI_CLASSES + [299, 300, 301, 65535]
    for n_hist in (1, 260, 1024):
        run, want = _check(hip_device, sizes, seed=n_hist, lut=lut, n_hist=n_hist, classes=classes, res_scans=8, res_words=4,
                           what=f"lut {case} n_hist {n_hist}")
        if case != "full":
            assert want["unmapped"].sum() > 0 and (want["labels"] == -1.0).sum() >= want["unmapped"].sum()
        else:
            assert want["unmapped"].sum() == 0


@pytest.mark.parametrize("n_hist", [1, 260, 1024])
def test_classes_at_the_edge_of_the_census(hip_device, n_hist):
    C = _hip.kitti_chunk_points()
    classes = [0, n_hist - 1, n_hist, n_hist + 1, 65535]
    run, want = _check(hip_device, [C + 1, 3], seed=n_hist, n_hist=n_hist, classes=classes)
    assert want["hist"][:, n_hist - 1].sum() > 0
    assert want["hist"].sum() < C + 4            # (the classes at n_hist and beyond were drawn and are not counted)


# ---- 6. optional outputs -----------------------------------------------------------------------------------------------
def test_every_combination_of_optional_outputs(hip_device):
    C = _hip.kitti_chunk_points()
    sizes = [C - 2, 9]
    b, l = kc.random_scans(sizes, 6, KITTI_CLASSES)
    lut = np.arange(256, dtype=np.int32)
    for rem, inst, hist, bad, unm, with_lut in itertools.product((False, True), repeat=6):
        if unm and not with_lut:
            continue
        n_hist = 260 if hist else 0
        run = Run(hip_device, b, l, sizes, lut if with_lut else None, n_hist, res_scans=4 * (rem + 2 * inst), want_remission=rem,
                  want_instance=inst, want_bad=bad, want_unmapped=unm)
        assert set(run.got) == ({"pts", "labels"} | ({"remission"} if rem else set()) | ({"instance"} if inst else set())
                                | ({"hist"} if hist else set()) | ({"bad"} if bad else set()) | ({"unmapped"} if unm else set()))
        run.assert_oracle(kc.decode_oracle(b, l, sizes, lut if with_lut else None, n_hist), what="optional outputs")
    # points only
    for rem, bad in itertools.product((False, True), repeat=2):
        run = Run(hip_device, b, None, sizes, None, 0, res_scans=12, shift64=1, want_remission=rem, want_bad=bad)
        assert "labels" not in run.got and "instance" not in run.got
        run.assert_oracle(kc.decode_oracle(b, None, sizes), what="points only")


# ---- 7. accumulated and written ----------------------------------------------------------------------------------------
def test_hist_accumulates_and_the_counters_do_not(hip_device):
    C = _hip.kitti_chunk_points()
    sizes = [C + 9, 4]
    lut = np.arange(100, dtype=np.int32)
    start = (np.arange(2 * 260, dtype=np.int64) * 1000 + 2**40).reshape(2, 260)
    b1, l1 = kc.random_scans(sizes, 1, KITTI_CLASSES)
    b2, l2 = kc.random_scans(sizes, 2, KITTI_CLASSES)
    first = Run(hip_device, b1, l1, sizes, lut, 260, hist0=start)
    w1 = kc.decode_oracle(b1, l1, sizes, lut, 260)
    first.assert_oracle(w1, hist0=start, what="first call")
    second = Run(hip_device, b2, l2, sizes, lut, 260, hist0=first.got["hist"])
    w2 = kc.decode_oracle(b2, l2, sizes, lut, 260)
    second.assert_oracle(w2, hist0=first.got["hist"], what="second call")       # (bad / unmapped: the second call's alone)
    assert np.array_equal(second.got["hist"] - start, w1["hist"] + w2["hist"]) and w2["unmapped"].sum() > 0


# ---- 8. a captured launch replayed on refilled buffers -----------------------------------------------------------------
def test_captured_replay_on_refilled_buffers(hip_device):
    dev = hip_device
    C = _hip.kitti_chunk_points()
    sizes = [C + 31, 0, 2 * C - 5]
    total, B = sum(sizes), len(sizes)
    lut_np = np.arange(200, dtype=np.int32)
    cases = [kc.random_scans(sizes, s, KITTI_CLASSES) for s in (61, 62)]
    _, scans = _place(dev, cases[0][0], 4)
    _, words = _place(dev, cases[0][1], 12)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
    lut = torch.from_numpy(lut_np).to(dev)
    pts = torch.empty((total, 3), dtype=torch.float64, device=dev)
    labels = torch.empty((total,), dtype=torch.float64, device=dev)
    rem = torch.empty((total,), dtype=torch.float32, device=dev)
    inst = torch.empty((total,), dtype=torch.int32, device=dev)
    hist = torch.zeros((B, 260), dtype=torch.int64, device=dev)
    bad = torch.empty((B,), dtype=torch.int32, device=dev)
    unm = torch.empty((B,), dtype=torch.int32, device=dev)
    call = lambda: _hip.kitti_decode(scans, words, total, offsets, pts, labels, lut, rem, inst, hist, bad, unm)   # noqa: E731
    call()                                                       # (eager first: the kernel is loaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hist.zero_()
        call()
    for b, l in (cases[1], cases[0], cases[1]):
        scans.copy_(torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()))
        words.copy_(torch.from_numpy(np.frombuffer(l, dtype=np.uint8).copy()))
        pts.fill_(float("nan"))
        bad.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        want = kc.decode_oracle(b, l, sizes, lut_np, 260)
        assert np.array_equal(pts.cpu().numpy().view(np.int64), want["pts"].view(np.int64))
        assert np.array_equal(labels.cpu().numpy().view(np.int64), want["labels"].view(np.int64))
        assert np.array_equal(rem.cpu().numpy().view(np.int32), want["remission"].view(np.int32))
        assert np.array_equal(inst.cpu().numpy(), want["instance"]) and np.array_equal(hist.cpu().numpy(), want["hist"])
        assert np.array_equal(bad.cpu().numpy(), want["bad"]) and np.array_equal(unm.cpu().numpy(), want["unmapped"])


# ---- 9. beyond the grid's cap: a workgroup takes consecutive chunks ----------------------------------------------------
def test_a_size_just_beyond_the_grid_cap(hip_device):
    C = _hip.kitti_chunk_points()
    total = GRID_CAP * C + C + 3
    assert total <= 2**22
    sizes = [100_001, 0, 3 * C + 1, total - 100_001 - 3 * C - 1 - 7, 7]
    lut = np.arange(259, dtype=np.int32)
    _check(hip_device, sizes, seed=9, lut=lut, n_hist=260, classes=KITTI_CLASSES, res_scans=4, res_words=4, shift64=1, shift32=3,
           what="beyond the cap")
    _check(hip_device, [total], seed=10, n_hist=260, classes=KITTI_CLASSES, what="beyond the cap, one scan")


# ---- 10. KittiReader ---------------------------------------------------------------------------------------------------
SCAN_SIZES = [700, 1, 300, 0, 513]


def _written(tmp_path, seq="00"):
    scans = [kc.random_scans([n], 100 + k, KITTI_CLASSES) for k, n in enumerate(SCAN_SIZES)]
    bins, labels = kc.write_sequence(str(tmp_path / "kitti"), seq, scans)
    return scans, bins, labels


def _scans_equal(got, scans, sizes, lut=None, n_hist=0, what=""):
    b, l = b"".join(s[0] for s in scans), b"".join(s[1] for s in scans)
    want = kc.decode_oracle(b, l, sizes, lut, n_hist)
    assert got.sizes == tuple(sizes) and got.offsets.cpu().tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    assert got.pts.shape == (sum(sizes), 3) and got.pts.dtype == torch.float64 and got.pts.is_cuda
    assert np.array_equal(got.pts.cpu().numpy().view(np.int64), want["pts"].view(np.int64)), f"{what}: pts"
    assert np.array_equal(got.labels.cpu().numpy().view(np.int64), want["labels"].view(np.int64)), f"{what}: labels"
    assert np.array_equal(got.bad.cpu().numpy(), want["bad"]), f"{what}: bad"
    if got.remission is not None:
        assert np.array_equal(got.remission.cpu().numpy().view(np.int32), want["remission"].view(np.int32)), f"{what}: remission"
    if got.instance is not None:
        assert np.array_equal(got.instance.cpu().numpy(), want["instance"]), f"{what}: instance"
    if n_hist:
        assert np.array_equal(got.hist.cpu().numpy(), want["hist"]), f"{what}: hist"
    if lut is not None:
        assert np.array_equal(got.unmapped.cpu().numpy(), want["unmapped"]), f"{what}: unmapped"


def test_reader_gives_the_same_tensors_at_every_batch_size(hip_device, tmp_path):
    scans, bins, labels = _written(tmp_path)
    lut = {c: k for k, c in enumerate(KITTI_CLASSES[:-3])}
    lut_np = sna.lut_array(lut)
    for batch_bytes, batches in ((700 * 20, 3), (1001 * 20, 2), (64 << 20, 1)):
        reader = sna.KittiReader(hip_device, batch_bytes=batch_bytes)
        from scene_net_amd.kitti import plan_batches
        assert len(plan_batches(SCAN_SIZES, 20, batch_bytes)) == batches
        got = reader.read(bins, labels, lut=lut, want_remission=True, want_instance=True, n_hist=260)
        torch.cuda.synchronize()
        _scans_equal(got, scans, SCAN_SIZES, lut_np, 260, what=f"batch_bytes {batch_bytes}")
        assert got.paths == tuple(bins)
        pb = got.point_batch()
        assert pb.pts.data_ptr() == got.pts.data_ptr() and pb.labels.data_ptr() == got.labels.data_ptr() and pb.sizes == got.sizes
        xyz, gt = got.scan(2)
        assert xyz.shape == (300, 3) and gt.shape == (300,) and xyz.data_ptr() == got.pts[701:].data_ptr()
    with pytest.raises(ValueError, match="batch_bytes"):
        sna.KittiReader(hip_device, batch_bytes=700 * 20 - 1).read(bins, labels)
    plain = reader.read(bins)
    torch.cuda.synchronize()
    assert plain.labels is None and plain.hist is None and plain.unmapped is None
    want = kc.decode_oracle(b"".join(s[0] for s in scans), None, SCAN_SIZES)
    assert np.array_equal(plain.pts.cpu().numpy().view(np.int64), want["pts"].view(np.int64))
    with pytest.raises(_hip.HipLibraryError):
        sna.KittiReader("cpu")


def test_one_reader_two_consecutive_batches_the_second_smaller(hip_device, tmp_path):
    scans, bins, labels = _written(tmp_path)
    reader = sna.KittiReader(hip_device, batch_bytes=1001 * 20)
    a = reader.read(bins[:3], labels[:3], n_hist=260)
    b = reader.read(bins[3:], labels[3:], n_hist=260)          # (no synchronisation in between: the events order the reuse)
    a2 = reader.read(bins[:3], labels[:3], n_hist=260)
    torch.cuda.synchronize()
    _scans_equal(a, scans[:3], SCAN_SIZES[:3], None, 260, what="first")
    _scans_equal(b, scans[3:], SCAN_SIZES[3:], None, 260, what="second, smaller")
    _scans_equal(a2, scans[:3], SCAN_SIZES[:3], None, 260, what="first again")
    one = sna.read_kitti_scan(bins[4], labels[4], device=hip_device, want_instance=True)
    torch.cuda.synchronize()
    _scans_equal(one, scans[4:], SCAN_SIZES[4:], what="read_kitti_scan")


def test_dataset_shapes_and_batches(hip_device, tmp_path):
    scans, bins, labels = _written(tmp_path, seq="07")
    with torch.cuda.device(hip_device):
        ds = sna.semKITTI(str(tmp_path / "kitti"), reader=sna.KittiReader(hip_device, batch_bytes=1 << 20))
        assert len(ds) == 5 and ds.scan_names == bins and ds.label_names == labels
        for idx in (0, 1, 3, torch.tensor(4)):
            xyz, gt = ds[idx]
            n = SCAN_SIZES[int(idx)]
            assert xyz.shape == (1, n, 3) and gt.shape == (1, n) and xyz.dtype == gt.dtype == torch.float64 and xyz.is_cuda
            want = kc.decode_oracle(*scans[int(idx)], [n])
            assert np.array_equal(xyz[0].cpu().numpy().view(np.int64), want["pts"].view(np.int64))
            assert np.array_equal(gt[0].cpu().numpy().view(np.int64), want["labels"].view(np.int64))
        ds.transform = lambda sample: (sample[0].shape, sample[1].shape)
        assert ds[2] == ((300, 3), (300,))
        ds.transform = None
        got = list(ds.batches(2, n_hist=260))
        assert [g.sizes for g in got] == [(700, 1), (300, 0), (513,)]
        for k, g in enumerate(got):
            _scans_equal(g, scans[2 * k:2 * k + 2], SCAN_SIZES[2 * k:2 * k + 2], None, 260, what=f"batch {k}")
        assert len(sna.semKITTI(str(tmp_path / "kitti"), split="train")) == 1


# ---- 11. the builders --------------------------------------------------------------------------------------------------
def _npy_bytes(t):
    f = io.BytesIO()
    np.save(f, t.cpu().numpy())
    return f.getvalue()


def test_builders_write_what_the_crops_of_the_oracle_arrays_give(hip_device, tmp_path):
    dev = hip_device
    scans = [kc.pole_scan(400, [], seed=1), kc.pole_scan(400, [(17.5, 15.0, 12)], seed=2),
             kc.pole_scan(400, [(32.5, 25.0, 4)], seed=3)]
    root = str(tmp_path / "kitti")
    kc.write_sequence(root, "00", scans)
    want_radius, want_slabs = [], []
    for b, l in scans:
        o = kc.decode_oracle(b, l, [400], None, 260)
        xyz, gt = torch.from_numpy(o["pts"]).to(dev), torch.from_numpy(o["labels"]).to(dev)
        want_radius.append(sna.pole_radius_samples(xyz, gt))
        want_slabs.append(sna.crop_pole_slabs(xyz, gt))
        assert o["hist"][0, 80] == int((o["labels"] == 80).sum())
    assert [len(w) for w in want_radius] == [0, 1, 0] and [len(w) for w in want_slabs] == [0, 1, 0]
    assert all(w.shape[1] == 4 and w.dtype == torch.float64 for w in want_radius[1] + want_slabs[1])
    assert int((want_radius[1][0][:, 3] == 80).sum()) == 12

    with torch.cuda.device(dev):
        reader = sna.KittiReader(dev, batch_bytes=1 << 20)
        for batch in (2, 32):
            out = tmp_path / f"radius{batch}"
            assert sna.build_pole_radius_samples(root, str(out), batch=batch, reader=reader) == 1
            assert sorted(os.listdir(out / "samples")) == ["sample_0.npy"]
            assert (out / "samples" / "sample_0.npy").read_bytes() == _npy_bytes(want_radius[1][0])
            out = tmp_path / f"slabs{batch}"
            assert sna.build_pole_samples(root, str(out), batch=batch, reader=reader) == 1
            assert sorted(os.listdir(out / "samples")) == ["sample_0.npy"]
            assert (out / "samples" / "sample_0.npy").read_bytes() == _npy_bytes(want_slabs[1][0])
        # the directory exists: None raises, False leaves it alone, True counts on behind its files
        out = tmp_path / "radius2"
        with pytest.raises(FileExistsError):
            sna.build_pole_radius_samples(root, str(out), reader=reader)
        assert sna.build_pole_radius_samples(root, str(out), overwrite=False, reader=reader) == 1
        assert sna.build_pole_radius_samples(root, str(out), overwrite=True, reader=reader) == 2
        assert sorted(os.listdir(out / "samples")) == ["sample_0.npy", "sample_1.npy"]
        assert (out / "samples" / "sample_1.npy").read_bytes() == _npy_bytes(want_radius[1][0])
