"""TileStream on the device: streamed batches and what the pipeline makes of them equal the resident loader's bit for bit,
slot reuse is ordered behind the consumer's stream, nothing is allocated after the constructor, shutdown is clean."""
import threading
import time

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd.synthetic import synthetic_tile

pytestmark = pytest.mark.gpu

N_FILES, BATCH = 32, 4


def _tile(rng, n):
    xyz, lab = synthetic_tile(int(rng.integers(1 << 30)), n)
    return np.concatenate([xyz, lab[:, None]], axis=1)


@pytest.fixture(scope="module")
def ragged(tmp_path_factory):
    """The 32 ragged files (N in 300..3000) of the host tests' shape, towers and ground included (synthetic_tile)."""
    root = tmp_path_factory.mktemp("stream")
    (root / "fit").mkdir()
    rng = np.random.default_rng(7)
    for k, n in enumerate(rng.integers(300, 3001, N_FILES)):
        np.save(root / "fit" / f"sample_{k:03d}.npy", _tile(rng, int(n)))
    return sna.TS40KTiles(str(root), "fit"), root


@pytest.fixture(scope="module")
def pipe(hip_device):
    torch.manual_seed(0)
    model = sna.SceneNet({"cy": 1, "cone": 1, "neg": 1}, (9, 9, 9)).to(hip_device)
    return sna.ScenePipeline(model, (64, 64, 64), keep_labels=[15], per_point=True)


def _run(pipe, batch):
    with torch.no_grad():
        out, grids, pp = pipe(batch, want_gt=True)
    return grids.occ, grids.gt_occ, out, pp


def _bytes(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


@pytest.fixture(scope="module")
def resident(ragged, pipe, hip_device):
    """Per batch, from the resident loader, computed once: the batch's arrays and the pipeline's four outputs, as bytes."""
    ds, _ = ragged
    ref = []
    for k in range(0, N_FILES, BATCH):
        batch = ds.load_batch(range(k, k + BATCH), device=hip_device)
        outs = _run(pipe, batch)
        torch.cuda.synchronize()
        ref.append(dict(pts=_bytes(batch.pts), labels=_bytes(batch.labels), offsets=_bytes(batch.offsets),
                        sizes=batch.sizes, outs=[_bytes(o) for o in outs]))
    return ref


def _check_batch(batch, ref):
    assert batch.sizes == ref["sizes"]
    assert batch.pts.shape == (sum(ref["sizes"]), 3) and batch.labels.shape == (sum(ref["sizes"]),)
    assert _bytes(batch.pts) == ref["pts"] and _bytes(batch.labels) == ref["labels"]
    assert batch.offsets.dtype == torch.int64 and _bytes(batch.offsets) == ref["offsets"]


@pytest.mark.parametrize("slots", [2, 3])
def test_streamed_batches_and_pipeline_outputs_equal_resident(ragged, pipe, resident, hip_device, slots):
    ds, _ = ragged
    with sna.TileStream(ds, BATCH, device=hip_device, slots=slots, timeout_s=20) as stream:
        assert len(stream) == 8
        n = 0
        for k, batch in enumerate(stream):
            outs = _run(pipe, batch)
            _check_batch(batch, resident[k])
            assert [_bytes(o) for o in outs] == resident[k]["outs"], f"pipeline outputs of batch {k}"
            assert stream.last_indices == tuple(range(k * BATCH, (k + 1) * BATCH))
            assert stream.last_bad.dtype == torch.int32 and stream.last_bad.tolist() == [0] * BATCH
            n += 1
        assert n == 8 and stream.skipped == []


@pytest.mark.parametrize("slots", [2, 3])
def test_slow_consumer_keeps_its_batch(ragged, pipe, resident, hip_device, slots):
    """A few milliseconds of device work sit between next() and the use of the batch; the results are fetched only after
    the NEXT batch was asked for, so a slot reused too early would show."""
    ds, _ = ragged
    a = torch.randn(2048, 2048, device=hip_device)
    held = []
    with sna.TileStream(ds, BATCH, device=hip_device, slots=slots, timeout_s=20) as stream:
        for k, batch in enumerate(stream):
            for _ in range(8):
                a = torch.tanh(a @ a) * 0.5            # device work ahead of the batch's use, same stream
            outs = _run(pipe, batch)
            held.append((outs, batch.pts.clone(), batch.labels.clone()))   # clones are enqueued work, ordered like it
    torch.cuda.synchronize()
    assert len(held) == 8
    for k, (outs, pts, labels) in enumerate(held):
        assert _bytes(pts) == resident[k]["pts"] and _bytes(labels) == resident[k]["labels"]
        assert [_bytes(o) for o in outs] == resident[k]["outs"], f"pipeline outputs of batch {k}"


def test_no_allocation_after_the_constructor(ragged, hip_device):
    ds, _ = ragged
    stream = sna.TileStream(ds, BATCH, device=hip_device, slots=3, timeout_s=20)
    try:
        spans = []
        for d in stream._dev:
            for t in d.values():
                spans.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()))
        inside = lambda t: any(lo <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= hi  # noqa: E731
                               for lo, hi in spans)
        host_ptrs = [s.rows.ctypes.data for s in stream.ring.slots] + [s.offsets.ctypes.data for s in stream.ring.slots]
        assert stream._host_rows.is_pinned() and stream._host_offsets.is_pinned()
        host_stats = getattr(torch.cuda, "host_memory_stats", None)
        snap = None
        for epoch in range(2):
            n = 0
            for batch in stream:
                assert inside(batch.pts) and inside(batch.labels) and inside(batch.offsets) and inside(stream.last_bad)
                n += 1
                if snap is None:   # after the first batch
                    torch.cuda.synchronize()
                    snap = (dict(host_stats()) if host_stats else {},
                            torch.cuda.memory_stats(hip_device)["allocation.all.allocated"])
            assert n == 8
        torch.cuda.synchronize()
        assert torch.cuda.memory_stats(hip_device)["allocation.all.allocated"] == snap[1]
        if host_stats:
            now = host_stats()
            for key in ("num_host_alloc", "allocated.allocated", "segment.allocated"):
                if key in snap[0]:
                    assert now[key] == snap[0][key], key
        assert [s.rows.ctypes.data for s in stream.ring.slots] + [s.offsets.ctypes.data for s in stream.ring.slots] \
            == host_ptrs
    finally:
        stream.close()


def test_last_bad_counts_injected_points(ragged, tmp_path, hip_device):
    ds, root = ragged
    d = tmp_path / "fit"
    d.mkdir()
    for k in range(4):
        a = np.load(root / "fit" / f"sample_{k:03d}.npy")
        if k == 2:
            a[5, 0] = np.nan
            a[17, 3] = np.nan
            a[len(a) - 1, 1:3] = np.nan      # two values of one point: one point
        np.save(d / f"sample_{k:03d}.npy", a)
    with sna.TileStream(sna.TS40KTiles(str(tmp_path), "fit"), BATCH, device=hip_device, timeout_s=20) as stream:
        batches = [(b.sizes, stream.last_bad.tolist()) for b in stream]
    assert len(batches) == 1 and batches[0][1] == [0, 0, 3, 0]


def test_skipped_files_and_complete_batches(ragged, tmp_path, hip_device):
    ds, root = ragged
    d = tmp_path / "fit"
    d.mkdir()
    for k in range(6):
        (d / f"sample_{k:03d}.npy").write_bytes((root / "fit" / f"sample_{k:03d}.npy").read_bytes())
    blob = (d / "sample_001.npy").read_bytes()
    (d / "sample_001.npy").write_bytes(blob[:len(blob) - 100])
    np.save(d / "sample_004.npy", np.zeros((40, 3)))
    ds2 = sna.TS40KTiles(str(tmp_path), "fit")
    with sna.TileStream(ds2, 3, device=hip_device, seed=2, timeout_s=20) as stream:
        got = []
        for batch in stream:
            ref = ds2.load_batch(stream.last_indices, device=hip_device)
            assert len(batch.sizes) == 3 and batch.sizes == ref.sizes
            assert _bytes(batch.pts) == _bytes(ref.pts) and _bytes(batch.labels) == _bytes(ref.labels)
            got.append(stream.last_indices)
        assert [(i, f) for i, f, _ in stream.skipped] == [(1, "sample_001.npy"), (4, "sample_004.npy")]
    # one child stream of default_rng(2) per (epoch, batch, scan-time), over the ok files the batch does not hold yet
    def draw(key, cands):
        return cands[int(np.random.default_rng(np.random.SeedSequence(2, spawn_key=key)).integers(len(cands)))]
    assert got == [(0, draw((0, 0, 0), [3, 5]), 2), (3, draw((0, 1, 0), [0, 2]), 5)]


def test_close_mid_epoch_is_clean(ragged, hip_device):
    ds, _ = ragged
    start = threading.active_count()
    stream = sna.TileStream(ds, BATCH, device=hip_device, slots=2, timeout_s=5)
    it = iter(stream)
    next(it)
    next(it)
    t0 = time.monotonic()
    stream.close()
    assert time.monotonic() - t0 < 5
    deadline = time.monotonic() + 5
    while threading.active_count() > start and time.monotonic() < deadline:
        time.sleep(0.005)
    assert threading.active_count() == start
    assert sum(1 for _ in stream) == 8      # and a new epoch runs
    stream.close()
