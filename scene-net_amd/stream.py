"""Streaming tile loader: TS40K files -> a pinned host ring -> HBM, de-interleaved on the device (sn_tiles_unpack).

The reference streams samples through 8 DataLoader workers (core/lit_modules/lit_data_wrappers.py:38, 62-72;
core/datasets/ts40k.py:192-225).  Here the host does straight byte copies only:

* `scan_tiles` reads every file's `.npy` HEADER: shape, dtype, order and payload offset.  Truncated, empty, `(N,3)` and
  non-npy files are known before an epoch starts, and every batch's CSR offsets before a byte of payload is read.
* `TileRing` is the host state machine: `slots` slots of `(capacity_points, 4)` f64 rows `x, y, z, label` plus
  `offsets [B+1]`, FREE -> FILLING -> FILLED -> IN_FLIGHT -> FREE, filled by reader threads that claim whole tiles (a C-order
  f64 `(N,4)` payload is read in place with `readinto`; any other readable layout goes through `np.load` and one
  assignment).  Pure host code over any numpy buffers.  Every wait takes a timeout and raises `TimeoutError` when it
  expires; an exception in a reader is re-raised in the consumer.
* `TileStream` owns the pinned ring, two device slots, one copy stream and the events, all allocated in its constructor,
  and yields `PointBatch` views bit-identical to `TS40KTiles.load_batch` of the same indices.  Every HIP call is made on
  the consumer's thread; readers touch files and host memory only.

Bad samples.  The reference replaces a sample that fails to load by `random.randint` over the whole list, with no bound on
retries (ts40k.py:200-223).  Here a file that is not ok at the scan, or whose read fails later, is replaced by a file
drawn with `np.random.default_rng(seed)` -- one child stream of that seed per (epoch, batch), so the draw depends on the
order alone -- from the ok files of the epoch's own index set only, preferring a file the batch does not hold yet; it is
recorded in `skipped` as `(index, file, reason)`, and a `RuntimeError` is raised when no ok file is left.  A replacement
caused by a late read failure changes the batch's offsets: that slot is rebuilt serially (a cold path), and the file
counts as not ok from the next epoch on.

Capacity.  A slot holds the sum of the `batch_size` largest `n_rows` among the ok files (with `indices`: among the files
named, each as often as it is named), which every batch of the plan fits; a batch that would not (a replacement that has
to repeat a file because no other is left) raises `ValueError` instead of being clipped.

Order.  `indices` (an explicit sequence) or all files, permuted by `default_rng(seed + epoch)` when `shuffle`; `drop_last`
as in a DataLoader.  The file in batch i, position j depends on the order alone, never on thread timing.
"""
from __future__ import annotations

import os
import threading
import time
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .tiles import TS40KTiles

FREE, FILLING, FILLED, IN_FLIGHT = 0, 1, 2, 3
MAX_READERS = 8
# what a read of a bad sample raises: the tile is replaced; anything else is a bug and surfaces in the consumer
_BAD_SAMPLE = (OSError, ValueError, EOFError)


class TileInfo(NamedTuple):
    n_rows: int
    cols: int
    dtype: Optional[np.dtype]
    fortran: bool
    payload_offset: int
    ok: bool
    reason: str


def _scan_one(path: str) -> TileInfo:
    try:
        with open(path, "rb") as f:
            version = np.lib.format.read_magic(f)
            if version == (1, 0):
                shape, fortran, dtype = np.lib.format.read_array_header_1_0(f)
            elif version == (2, 0):
                shape, fortran, dtype = np.lib.format.read_array_header_2_0(f)
            else:
                return TileInfo(0, 0, None, False, 0, False, f"npy version {version} is not read")
            offset = f.tell()
            size = os.fstat(f.fileno()).st_size
    except Exception as e:   # noqa: BLE001 -- whatever the parser raises on a file that is no npy file
        return TileInfo(0, 0, None, False, 0, False, f"header: {e}")
    if len(shape) != 2:
        return TileInfo(0, 0, dtype, bool(fortran), offset, False, f"ndim {len(shape)} (a tile is (N, 4))")
    n, c = int(shape[0]), int(shape[1])
    info = TileInfo(n, c, dtype, bool(fortran), offset, False, "")
    if dtype.hasobject or dtype.kind not in "fiu":
        return info._replace(reason=f"dtype {dtype} is not numeric")
    if c < 4:
        return info._replace(reason=f"{c} columns (a tile is x, y, z, label)")
    if n < 1:
        return info._replace(reason="no rows")
    want = offset + n * c * dtype.itemsize
    if size != want:
        return info._replace(reason=f"file size {size} != {want} (truncated or trailing bytes)")
    return info._replace(ok=True)


def scan_tiles(ds: TS40KTiles) -> List[TileInfo]:
    """Per file of `ds`, from the `.npy` header alone: (n_rows, cols, dtype, fortran, payload_offset, ok, reason)."""
    return [_scan_one(os.path.join(ds.dataset_path, str(f))) for f in ds.npy_files]


def capacity_points(infos: Sequence[TileInfo], batch_size: int, indices: Optional[Sequence[int]] = None) -> int:
    """Rows one slot must hold: the sum of the `batch_size` largest n_rows among the ok files -- among the files that
    `indices` names when given, each counted as often as it is named (a batch may then hold a file twice)."""
    chosen = infos if indices is None else [infos[int(i)] for i in indices]
    rows = sorted((i.n_rows for i in chosen if i.ok), reverse=True)
    return int(sum(rows[:batch_size]))


def _direct(info: TileInfo) -> bool:
    return info.cols == 4 and not info.fortran and info.dtype == np.dtype("<f8") and info.dtype.isnative


def _read_tile(path: str, info: TileInfo, out: np.ndarray) -> None:
    """Fills out [n_rows, 4] f64 (a C-contiguous slice of a slot) with the tile's x, y, z, label."""
    if _direct(info):
        with open(path, "rb", buffering=0) as f:
            want = info.payload_offset + info.n_rows * 32
            if os.fstat(f.fileno()).st_size != want:
                raise ValueError("file size changed since the scan")
            f.seek(info.payload_offset)
            mv = memoryview(out).cast("B")
            got = 0
            while got < len(mv):
                n = f.readinto(mv[got:])
                if not n:
                    raise EOFError(f"payload ends after {got} of {len(mv)} bytes")
                got += n
        return
    a = np.load(path)
    if a.shape != (info.n_rows, info.cols):
        raise ValueError(f"shape {a.shape} differs from the scanned header")
    out[:, :3] = a[:, :3]
    out[:, 3] = a[:, -1]


class Slot:
    """One slot of the ring: rows [capacity, 4] f64, offsets [batch_size + 1] i64 and what the current batch put there."""

    def __init__(self, index: int, rows: np.ndarray, offsets: np.ndarray) -> None:
        self.index, self.rows, self.offsets = index, rows, offsets
        self.state = FREE
        self.batch_no = -1
        self.files: List[int] = []
        self.next_tile = self.done = 0
        self.failed: List[Tuple[int, str]] = []

    @property
    def n_tiles(self) -> int:
        return len(self.files)

    @property
    def total(self) -> int:
        return int(self.offsets[len(self.files)])

    @property
    def sizes(self) -> Tuple[int, ...]:
        return tuple(int(v) for v in np.diff(self.offsets[:len(self.files) + 1]))


class TileRing:
    """`slots` host slots filled in batch order by up to 8 reader threads and handed to one consumer in the same order.

    start(epoch) plans the epoch and starts the readers; next() returns the next FILLED slot as IN_FLIGHT (None after the
    last batch); release(slot) frees it; close() stops and joins the readers.  Batch k always uses slot k % slots.
    `rows` / `offsets`: one preallocated buffer per slot ([capacity, 4] f64 / [batch_size + 1] i64), e.g. views of pinned
    memory; allocated here from ordinary memory when not given.  Never reallocated."""

    def __init__(self, ds: TS40KTiles, batch_size: int, slots: int = 3, readers: int = 4, shuffle: bool = False,
                 seed: int = 0, indices: Optional[Sequence[int]] = None, drop_last: bool = False,
                 timeout_s: float = 30.0, infos: Optional[Sequence[TileInfo]] = None,
                 rows: Optional[Sequence[np.ndarray]] = None, offsets: Optional[Sequence[np.ndarray]] = None) -> None:
        if batch_size < 1 or slots < 2:
            raise ValueError("batch_size >= 1 and slots >= 2")
        if not 1 <= readers <= MAX_READERS:
            raise ValueError(f"readers must lie in 1..{MAX_READERS}")
        self.ds, self.batch_size, self.n_slots, self.readers = ds, int(batch_size), int(slots), int(readers)
        self.shuffle, self.seed, self.drop_last, self.timeout_s = bool(shuffle), int(seed), bool(drop_last), float(timeout_s)
        self.infos = list(infos) if infos is not None else scan_tiles(ds)
        self.indices = None if indices is None else [int(i) for i in indices]
        base = range(len(ds)) if self.indices is None else self.indices
        self._pool = self._ok_pool()   # replacements are drawn from here; fixed for the length of an epoch
        self.capacity_points = capacity_points(self.infos, self.batch_size, self.indices)
        if rows is None:
            rows = [np.empty((self.capacity_points, 4), dtype=np.float64) for _ in range(self.n_slots)]
        if offsets is None:
            offsets = [np.zeros(self.batch_size + 1, dtype=np.int64) for _ in range(self.n_slots)]
        for r, o in zip(rows, offsets):
            if r.shape != (self.capacity_points, 4) or r.dtype != np.float64 or not r.flags.c_contiguous:
                raise ValueError("a slot's rows are C-contiguous [capacity_points, 4] float64")
            if o.shape != (self.batch_size + 1,) or o.dtype != np.int64:
                raise ValueError("a slot's offsets are [batch_size + 1] int64")
        self.slots = [Slot(i, r, o) for i, (r, o) in enumerate(zip(rows, offsets))]
        if len(self.slots) != self.n_slots:
            raise ValueError("one rows / offsets buffer per slot")
        self._planned_skips: List[Tuple[int, str, str]] = []
        self._late_skips: List[Tuple[int, int, Tuple[int, str, str]]] = []   # (batch, position, entry)
        self._late_bad: dict = {}     # file -> reason: read failures of this epoch; not ok from the next plan on
        self._epoch_no = 0
        self._cond = threading.Condition()
        self._threads: List[threading.Thread] = []
        self._plan: List[List[int]] = []
        self._opened = self._consumed = 0
        self._stop = False
        self._error: Optional[BaseException] = None

    # ---- plan ----
    def _path(self, i: int) -> str:
        return os.path.join(self.ds.dataset_path, str(self.ds.npy_files[i]))

    @property
    def skipped(self) -> List[Tuple[int, str, str]]:
        """(index, file, reason) of every file replaced in the current epoch: those known from the scan in batch order,
        then the late read failures in batch order."""
        with self._cond:
            return list(self._planned_skips) + [e for _, _, e in sorted(self._late_skips)]

    def _ok_pool(self) -> List[int]:
        base = range(len(self.ds)) if self.indices is None else self.indices
        pool = sorted({int(i) for i in base if self.infos[int(i)].ok})
        if not pool:
            raise RuntimeError("no readable tile: " + "; ".join(
                f"{self.ds.npy_files[i]}: {self.infos[i].reason}" for i in list(base)[:8]))
        return pool

    def _replace_rng(self, batch_no: int, late: bool) -> np.random.Generator:
        """The replacement draws of one batch: a child stream of `default_rng(seed)` named by (epoch, batch, scan | late
        failure), so a draw depends on the order alone -- not on earlier epochs' draws, not on which slot rebuilds first."""
        return np.random.default_rng(np.random.SeedSequence(self.seed, spawn_key=(self._epoch_no, batch_no, int(late))))

    def _draw(self, rng: np.random.Generator, batch: Sequence[int], failed: Sequence[int], what: str) -> int:
        """Another ok file for `batch`: one the batch does not hold yet while there is one (a batch of distinct files
        always fits a slot), never one of `failed`."""
        cands = [p for p in self._pool if p not in batch and p not in failed] or [p for p in self._pool if p not in failed]
        if not cands:
            raise RuntimeError(f"no readable tile is left to replace {what}")
        return cands[int(rng.integers(len(cands)))]

    def _check_fits(self, files: Sequence[int], batch_no: int) -> None:
        need = sum(self.infos[i].n_rows for i in files)
        if need > self.capacity_points:
            raise ValueError(f"batch {batch_no} holds {need} rows, a slot {self.capacity_points} (files "
                             f"{[str(self.ds.npy_files[i]) for i in files]})")

    def plan_epoch(self, epoch: int = 0) -> List[List[int]]:
        """The epoch's batches as lists of file indices, bad files already replaced (resets `skipped`).  Files whose
        read failed in an earlier epoch count as not ok from here on."""
        for i, reason in sorted(self._late_bad.items()):
            self.infos[i] = self.infos[i]._replace(ok=False, reason=reason)
        self._late_bad = {}
        self._epoch_no = int(epoch)
        self._pool = self._ok_pool()
        order = np.arange(len(self.ds)) if self.indices is None else np.asarray(self.indices, dtype=np.int64)
        if self.shuffle:
            order = np.random.default_rng(self.seed + int(epoch)).permutation(order)
        self._planned_skips, self._late_skips = [], []
        bs = self.batch_size
        plan = [[int(i) for i in order[k:k + bs]] for k in range(0, len(order), bs)]
        if self.drop_last and plan and len(plan[-1]) < bs:
            plan.pop()
        for k, files in enumerate(plan):
            rng = None
            for pos, i in enumerate(files):
                if self.infos[i].ok:
                    continue
                rng = rng or self._replace_rng(k, late=False)
                self._planned_skips.append((i, str(self.ds.npy_files[i]), self.infos[i].reason))
                files[pos] = self._draw(rng, [f for f in files if self.infos[f].ok], (),
                                        f"{self.ds.npy_files[i]} ({self.infos[i].reason})")
            self._check_fits(files, k)
        return plan

    # ---- consumer side ----
    def start(self, epoch: int = 0) -> int:
        """Plans epoch `epoch`, frees every slot and starts the readers; returns the number of batches."""
        self.close()
        self._plan = self.plan_epoch(epoch)
        for s in self.slots:
            s.state, s.batch_no = FREE, -1
        self._opened = self._consumed = 0
        self._stop, self._error = False, None
        n = min(self.readers, max(1, sum(len(b) for b in self._plan)))
        self._threads = [threading.Thread(target=self._reader, name=f"tile-reader-{k}", daemon=True) for k in range(n)]
        for t in self._threads:
            t.start()
        return len(self._plan)

    def next(self, on_idle: Optional[Callable[[], None]] = None) -> Optional[Slot]:
        """The slot of the next batch, IN_FLIGHT; None when the epoch is exhausted (the readers are joined then).
        `on_idle` is called before every wait, with the lock held (re-entrant): the place to release() slots whose
        use has ended, so that the readers are never starved by the consumer that waits for them."""
        with self._cond:
            if self._consumed < len(self._plan):
                slot = self.slots[self._consumed % self.n_slots]
                deadline = time.monotonic() + self.timeout_s
                while True:
                    if self._error is not None:
                        break
                    if slot.state == FILLED and slot.batch_no == self._consumed:
                        slot.state = IN_FLIGHT
                        self._consumed += 1
                        return slot
                    if on_idle is not None:
                        on_idle()
                    remaining = deadline - time.monotonic()
                    if remaining <= 0:
                        self._error = TimeoutError(f"no FILLED slot for batch {self._consumed} within {self.timeout_s} s")
                        break
                    self._cond.wait(min(remaining, 0.002) if on_idle is not None else remaining)
        err = self._error
        try:
            self.close()
        except TimeoutError:
            if err is None:   # (otherwise the first error is the one to report; a reader stuck in a read stays a daemon)
                raise
        if err is not None:
            raise err
        return None

    def release(self, slot: Slot) -> None:
        with self._cond:
            if slot.state != IN_FLIGHT:
                raise RuntimeError(f"slot {slot.index} is not IN_FLIGHT")
            slot.state = FREE
            self._cond.notify_all()

    def close(self) -> None:
        """Stops the readers and joins them within `timeout_s` (TimeoutError otherwise).  The buffers stay."""
        with self._cond:
            self._stop = True
            self._cond.notify_all()
        deadline = time.monotonic() + self.timeout_s
        for t in self._threads:
            t.join(max(0.0, deadline - time.monotonic()))
        alive = [t.name for t in self._threads if t.is_alive()]
        if alive:
            raise TimeoutError(f"reader threads {alive} did not stop within {self.timeout_s} s")
        self._threads = []

    def epoch(self, epoch: int = 0):
        """Host-only iteration: yields each slot, releasing it when the consumer comes back for the next."""
        self.start(epoch)
        try:
            while True:
                slot = self.next()
                if slot is None:
                    return
                yield slot
                self.release(slot)
        finally:
            self.close()

    # ---- reader side: files and host memory only ----
    def _open(self, slot: Slot) -> None:
        files = list(self._plan[self._opened])
        self._check_fits(files, self._opened)   # (plan_epoch checked it; a slice past the slot's end would clip silently)
        slot.state, slot.batch_no, slot.files = FILLING, self._opened, files
        slot.next_tile = slot.done = 0
        slot.failed = []
        slot.offsets[0] = 0
        np.cumsum([self.infos[i].n_rows for i in files], out=slot.offsets[1:len(files) + 1])
        self._opened += 1

    def _claim(self) -> Optional[Tuple[Slot, int]]:
        with self._cond:
            deadline = None
            while True:
                if self._stop or self._error is not None:
                    return None
                lo = max(0, self._opened - self.n_slots)
                for k in range(lo, self._opened):   # FILLING slots, oldest batch first
                    s = self.slots[k % self.n_slots]
                    if s.state == FILLING and s.batch_no == k and s.next_tile < s.n_tiles:
                        s.next_tile += 1
                        return s, s.next_tile - 1
                if self._opened >= len(self._plan):
                    return None
                s = self.slots[self._opened % self.n_slots]
                if s.state == FREE:
                    self._open(s)
                    deadline = None
                    continue
                if deadline is None:
                    deadline = time.monotonic() + self.timeout_s
                remaining = deadline - time.monotonic()
                if remaining <= 0:
                    raise TimeoutError(f"reader waited {self.timeout_s} s for slot {s.index} to become FREE")
                self._cond.wait(remaining)

    def _finish(self, slot: Slot, pos: int, err: Optional[BaseException]) -> None:
        with self._cond:
            if err is not None:
                slot.failed.append((pos, f"read: {err}"))
            slot.done += 1
            if slot.done < slot.n_tiles:
                return
            failed = sorted(slot.failed)
        if failed:   # every tile of the slot is claimed and finished: this thread owns it until it says FILLED
            self._rebuild(slot, failed)
        with self._cond:
            slot.state = FILLED
            self._cond.notify_all()

    def _rebuild(self, slot: Slot, failed: List[Tuple[int, str]]) -> None:
        """Cold path: replaces the tiles whose read failed and fills the whole slot again, serially."""
        rng = self._replace_rng(slot.batch_no, late=True)
        gone: List[int] = []   # files this slot has seen fail
        while failed:
            with self._cond:
                for pos, reason in failed:
                    i = slot.files[pos]
                    if i not in gone:
                        gone.append(i)
                        self._late_skips.append((slot.batch_no, pos, (i, str(self.ds.npy_files[i]), reason)))
                        self._late_bad.setdefault(i, reason)
                for pos, reason in failed:
                    rest = [f for p, f in enumerate(slot.files) if p != pos and f not in gone]
                    slot.files[pos] = self._draw(rng, rest, gone, f"{self.ds.npy_files[slot.files[pos]]} ({reason})")
                self._check_fits(slot.files, slot.batch_no)
                np.cumsum([self.infos[i].n_rows for i in slot.files], out=slot.offsets[1:slot.n_tiles + 1])
            failed = []
            for pos, i in enumerate(slot.files):
                try:
                    _read_tile(self._path(i), self.infos[i], slot.rows[slot.offsets[pos]:slot.offsets[pos + 1]])
                except _BAD_SAMPLE as e:
                    failed.append((pos, f"read: {e}"))

    def _reader(self) -> None:
        try:
            while True:
                task = self._claim()
                if task is None:
                    return
                slot, pos = task
                i = slot.files[pos]
                err = None
                try:
                    _read_tile(self._path(i), self.infos[i], slot.rows[slot.offsets[pos]:slot.offsets[pos + 1]])
                except _BAD_SAMPLE as e:
                    err = e
                self._finish(slot, pos, err)
        except BaseException as e:   # noqa: BLE001 -- handed to the consumer, which re-raises it at its next next()
            with self._cond:
                if self._error is None:
                    self._error = e
                self._cond.notify_all()


class TileStream:
    """Iterable of `PointBatch` streamed from disk; a context manager with close().

    The constructor allocates everything, once: the pinned host ring (`slots` slots), two device slots (raw rows, pts,
    labels, offsets, bad [B]), one copy stream and the events.  Per batch, on the caller's thread: the copy stream waits
    for the device slot's "consumed" event, copies the slot's raw rows and offsets host-to-device, runs sn_tiles_unpack
    and records "ready"; the caller's current stream waits on it.  The copy of batch i+1 is enqueued before batch i is
    handed out, which is what overlaps transfer with compute.

    Validity: a yielded batch is a VIEW into a device slot, valid until the next batch is asked for.  Work enqueued on the
    current stream before that is ordered ahead of the slot's reuse (the "consumed" event is recorded on the current
    stream at that moment); work enqueued later, or on another stream, must clone what it needs.
    `last_bad` is the device [B] i32 of the batch (points with a non-finite value, per tile), `last_indices` its files.
    One epoch per iteration; epoch e is ordered by `default_rng(seed + e)`."""

    def __init__(self, ds: TS40KTiles, batch_size: int, device=None, slots: int = 3, readers: int = 4,
                 shuffle: bool = False, seed: int = 0, indices: Optional[Sequence[int]] = None, drop_last: bool = False,
                 timeout_s: float = 30.0) -> None:
        import torch
        from . import _hip
        self._torch, self._hip = torch, _hip
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise _hip.HipLibraryError("TileStream feeds HBM: device must be a HIP device")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        infos = scan_tiles(ds)
        cap = max(1, capacity_points(infos, batch_size, indices))
        B = int(batch_size)
        self._host_rows = torch.empty((slots, cap, 4), dtype=torch.float64).pin_memory()
        self._host_offsets = torch.zeros((slots, B + 1), dtype=torch.int64).pin_memory()
        rows_np, off_np = self._host_rows.numpy(), self._host_offsets.numpy()
        self.ring = TileRing(ds, batch_size, slots, readers, shuffle, seed, indices, drop_last, timeout_s, infos,
                             [rows_np[s] for s in range(slots)], [off_np[s] for s in range(slots)])
        self.timeout_s = float(timeout_s)
        with torch.cuda.device(device):
            self._dev = [dict(rows=torch.empty((cap, 4), dtype=torch.float64, device=device),
                              pts=torch.empty((cap, 3), dtype=torch.float64, device=device),
                              labels=torch.empty((cap,), dtype=torch.float64, device=device),
                              offsets=torch.zeros((B + 1,), dtype=torch.int64, device=device),
                              bad=torch.zeros((B,), dtype=torch.int32, device=device)) for _ in range(2)]
            self._copy = torch.cuda.Stream(device=device)
            self._ready = [torch.cuda.Event() for _ in range(2)]
            self._consumed = [torch.cuda.Event() for _ in range(2)]
            self._copied = [torch.cuda.Event() for _ in range(slots)]
        self._consumed_recorded = [False, False]
        self._inflight: List[Slot] = []     # host slots whose host-to-device copy may still be running
        self._queued: dict = {}             # batch number -> what its enqueue left (sizes, files, tile count)
        self._epoch = 0
        self._n_batches = self._k = 0
        self._handed: Optional[int] = None  # device slot of the batch the caller holds
        self._active = False
        self.last_bad = None
        self.last_indices: Tuple[int, ...] = ()

    @property
    def skipped(self):
        return self.ring.skipped

    def __len__(self) -> int:
        n, bs = len(self.ring.indices) if self.ring.indices is not None else len(self.ring.ds), self.ring.batch_size
        return n // bs if self.ring.drop_last else -(-n // bs)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # ---- slot bookkeeping (caller's thread) ----
    def _reap(self) -> None:
        """Releases the host slots whose copy has finished (never blocks)."""
        while self._inflight and self._copied[self._inflight[0].index].query():
            self.ring.release(self._inflight.pop(0))

    def _drain(self) -> None:
        """Waits, bounded, for the copies still reading host slots, then releases them."""
        deadline = time.monotonic() + self.timeout_s
        while self._inflight:
            self._reap()
            if self._inflight:
                if time.monotonic() > deadline:
                    raise TimeoutError(f"a host-to-device copy did not finish within {self.timeout_s} s")
                time.sleep(0.0002)

    def _enqueue(self, k: int) -> None:
        torch = self._torch
        slot = self.ring.next(on_idle=self._reap)
        d, s = k % 2, slot.index
        dev, total, nb = self._dev[d], slot.total, slot.n_tiles
        with torch.cuda.device(self.device), torch.cuda.stream(self._copy):
            if self._consumed_recorded[d]:
                self._copy.wait_event(self._consumed[d])
            dev["rows"][:total].copy_(self._host_rows[s, :total], non_blocking=True)
            dev["offsets"][:nb + 1].copy_(self._host_offsets[s, :nb + 1], non_blocking=True)
            self._copied[s].record(self._copy)
            self._hip.tiles_unpack(dev["rows"][:total], dev["pts"], dev["labels"], dev["offsets"][:nb + 1],
                                   dev["bad"][:nb])
            self._ready[d].record(self._copy)
        self._inflight.append(slot)
        self._queued[k] = (slot.sizes, tuple(slot.files), total, nb)

    def _mark_consumed(self) -> None:
        if self._handed is not None:
            self._consumed[self._handed].record(self._torch.cuda.current_stream(self.device))
            self._consumed_recorded[self._handed] = True
            self._handed = None

    def _next(self):
        from .voxelization import PointBatch
        self._mark_consumed()
        k = self._k
        if k >= self._n_batches:
            return None
        if k not in self._queued:
            self._enqueue(k)
        if k + 1 < self._n_batches:
            self._enqueue(k + 1)
        d = k % 2
        self._torch.cuda.current_stream(self.device).wait_event(self._ready[d])
        sizes, files, total, nb = self._queued.pop(k)
        dev = self._dev[d]
        self._k, self._handed = k + 1, d
        self.last_bad, self.last_indices = dev["bad"][:nb], files
        return PointBatch(dev["pts"][:total], dev["labels"][:total], dev["offsets"][:nb + 1], sizes)

    def _end_epoch(self) -> None:
        if not self._active:
            return
        self._active = False
        try:
            self._mark_consumed()
            self._drain()
        finally:
            self._queued.clear()
            self._inflight = []
            self.ring.close()

    def __iter__(self):
        self._end_epoch()
        self._n_batches = self.ring.start(self._epoch)
        self._epoch += 1
        self._k, self._active = 0, True
        mine = self._epoch
        try:
            while True:
                batch = self._next()
                if batch is None:
                    return
                yield batch
        finally:
            if self._epoch == mine:   # (an abandoned iterator that is collected late must not end a newer epoch)
                self._end_epoch()

    def close(self) -> None:
        """Ends the running epoch: waits (bounded) for copies that still read the ring and joins the readers."""
        self._end_epoch()
        self.ring.close()
