"""SemanticKITTI scans into HBM: the velodyne and label bytes of a batch of scans travel host-to-device as the files hold
them and are decoded there in one launch (K14: sn_kitti_decode, csrc/kitti.hip).

The reference opens a scan with SemLaserScan.open_scan / open_label (core/datasets/semKITTI.py:388-403): np.fromfile,
reshape((-1, 4)), `label & 0xFFFF`, one scan at a time on one host core, and only then can it be uploaded.  Here the host
lists files and moves bytes:

    scans = sna.KittiReader().read(bin_paths, label_paths, n_hist=260)    # KittiScans: pts [total,3] f64, labels [total] f64
    xyz, gt = scans.scan(0)                                               # views of one scan
    batch = scans.point_batch()                                           # the PointBatch K1 reads, no copy
    ds = sna.semKITTI(root, split="train"); xyz, gt = ds[0]               # the reference's dataset, shapes [1,N,3] / [1,N]
    sna.build_pole_radius_samples(root, save_path)                        # SemanticKITTI files in, pole samples out

`KittiReader` owns two pinned host buffers, two raw device buffers, one copy stream and its events, all allocated in the
constructor.  The files of one batch are `readinto` a pinned buffer -- every .bin first, then every .label, then the batch's
CSR, so the .bin region starts 16-byte aligned --, go to the device in ONE copy and are decoded by ONE launch; while batch k
is copied and decoded, the caller's thread reads batch k+1 into the other buffer.  There are no threads.

Definition (normative, include/scenenet_hip.h): .bin is little-endian float32 [n,4] (x, y, z, remission), .label is
little-endian uint32 [n]; xyz is the exact widening of the three floats, sem = w & 0xFFFF, instance = w >> 16, labels =
(double)sem, or (double)lut[sem] with a class remap (-1.0 and a count in `unmapped` where sem is beyond the map).
Unpinned: the reference imports SemKITTI_API.auxiliary.laserscan.SemLaserScan (semKITTI.py:26) and does not carry it, so
nothing here is pinned against the reference's own output; the layout is the published SemanticKITTI one and the oracle is
numpy on those definitions.  No yaml is parsed: a caller passes the `learning_map` dict of their semantic-kitti.yaml as lut.
There is no CPU path: a reader on a CPU device raises HipLibraryError.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np

POLE_LABEL = 80
KITTI_SPLITS = {"samples": (0.0, 1.0), "train": (0.0, 0.2), "val": (0.2, 0.4), "test": (0.4, 1.0)}
KITTI_MAX_BATCH_SCANS = 4096     # scans per launch: the batch's CSR travels behind the file bytes


@dataclass
class KittiScans:
    """B decoded scans on the device: pts [total,3] f64, labels [total] f64 | None, offsets [B+1] i64 (CSR), sizes (host),
    remission [total] f32 | None, instance [total] i32 | None, hist [B,n_hist] i64 | None, bad [B] i32 (points with a
    non-finite coordinate), unmapped [B] i32 | None (label words beyond the lut), and the files they came from."""
    pts: "torch.Tensor"
    labels: Optional["torch.Tensor"]
    offsets: "torch.Tensor"
    sizes: Tuple[int, ...]
    remission: Optional["torch.Tensor"]
    instance: Optional["torch.Tensor"]
    hist: Optional["torch.Tensor"]
    bad: "torch.Tensor"
    unmapped: Optional["torch.Tensor"]
    paths: Tuple[str, ...]

    def point_batch(self):
        """The PointBatch that K1 reads: the same tensors, no copy."""
        from .voxelization import PointBatch
        return PointBatch(self.pts, self.labels, self.offsets, self.sizes)

    def scan(self, b: int):
        """Views (xyz [n_b,3], labels [n_b] | None) of scan b."""
        b = range(len(self.sizes))[b]
        first = sum(self.sizes[:b])
        stop = first + self.sizes[b]
        return self.pts[first:stop], None if self.labels is None else self.labels[first:stop]


def lut_array(lut) -> Optional[np.ndarray]:
    """The class remap as a contiguous int32 array: a 1-D integer array as it is, a dict {raw: mapped} as an array of
    max(key) + 1 entries filled with -1 (host only).  1 to 65536 entries."""
    if lut is None:
        return None
    if isinstance(lut, dict):
        if not lut:
            raise ValueError("lut: the dict is empty")
        keys = [int(k) for k in lut]
        if min(keys) < 0:
            raise ValueError("lut: a raw class is negative")
        arr = np.full(max(keys) + 1, -1, dtype=np.int64)
        for k, v in lut.items():
            arr[int(k)] = int(v)
    else:
        arr = np.asarray(lut)
        if arr.ndim != 1 or not np.issubdtype(arr.dtype, np.integer):
            raise ValueError("lut must be a 1-D integer array or a dict {raw: mapped}")
        arr = arr.astype(np.int64)
    if not 1 <= arr.size <= 65536:
        raise ValueError(f"lut must hold 1..65536 entries (got {arr.size}): a raw class is 16 bits")
    if arr.size and (arr.min() < -2**31 or arr.max() >= 2**31):
        raise ValueError("lut: a mapped class does not fit int32")
    return np.ascontiguousarray(arr, dtype=np.int32)


def scan_sizes(bin_paths: Sequence[str], label_paths: Optional[Sequence[str]] = None) -> List[int]:
    """Points per scan from the files' sizes (host only).  ValueError naming the file for a .bin whose size is not a
    multiple of 16, a .label whose size is not a multiple of 4 and a label count that differs from the point count (the
    reference's `assert len(xyz) == len(gt)`, semKITTI.py:401)."""
    if label_paths is not None and len(label_paths) != len(bin_paths):
        raise ValueError(f"{len(bin_paths)} scans but {len(label_paths)} label files")
    sizes = []
    for k, p in enumerate(bin_paths):
        nb = os.stat(p).st_size
        if nb % 16:
            raise ValueError(f"{p}: {nb} bytes are not a multiple of 16 (float32 x, y, z, remission per point)")
        if label_paths is not None:
            nl = os.stat(label_paths[k]).st_size
            if nl % 4:
                raise ValueError(f"{label_paths[k]}: {nl} bytes are not a multiple of 4 (one uint32 per point)")
            if nl // 4 != nb // 16:
                raise ValueError(f"{label_paths[k]}: {nl // 4} labels for the {nb // 16} points of {p}")
        sizes.append(nb // 16)
    return sizes


def plan_batches(sizes: Sequence[int], bytes_per_point: int, batch_bytes: int, paths: Optional[Sequence[str]] = None
                 ) -> List[Tuple[int, int]]:
    """[first scan, stop scan) of every batch: consecutive scans while their file bytes fit batch_bytes (and at most
    KITTI_MAX_BATCH_SCANS of them).  ValueError naming the scan whose files alone are larger than batch_bytes.  Host only."""
    out, first, used = [], 0, 0
    for k, n in enumerate(sizes):
        need = int(n) * bytes_per_point
        if need > batch_bytes:
            name = paths[k] if paths is not None else f"scan {k}"
            raise ValueError(f"{name}: a batch of this one scan takes {need} bytes, more than batch_bytes = {batch_bytes}")
        if k > first and (used + need > batch_bytes or k - first >= KITTI_MAX_BATCH_SCANS):
            out.append((first, k))
            first, used = k, 0
        used += need
    if len(sizes) > first:
        out.append((first, len(sizes)))
    return out


class KittiReader:
    """Reads SemanticKITTI scans into HBM through buffers allocated once (module docstring).  `batch_bytes` sizes the two
    pinned and the two device buffers: the file bytes of one launch's scans (20 per point with labels, 16 without)."""

    def __init__(self, device=None, batch_bytes: int = 64 << 20) -> None:
        import torch
        from . import _hip
        self._torch, self._hip = torch, _hip
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise _hip.HipLibraryError("KittiReader feeds HBM: device must be a HIP device; there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if int(batch_bytes) < 1:
            raise ValueError("batch_bytes must be positive")
        self.device, self.batch_bytes = device, int(batch_bytes)
        cap = (self.batch_bytes + 15) // 16 * 16 + 8 * (KITTI_MAX_BATCH_SCANS + 1)   # file bytes, then the batch's CSR
        self._host = [torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._host_np = [h.numpy() for h in self._host]
        with torch.cuda.device(device):
            self._raw = [torch.empty(cap, dtype=torch.uint8, device=device) for _ in range(2)]
            self._copy = torch.cuda.Stream(device=device)
            self._copied = [torch.cuda.Event() for _ in range(2)]
            self._start, self._done = torch.cuda.Event(), torch.cuda.Event()
        self._copy_pending = [False, False]
        self._turn = 0
        self._lut_key, self._lut_dev = None, None

    def _lut(self, lut):
        """the remap on the device; uploaded again only when its content changes"""
        arr = lut_array(lut)
        if arr is None:
            return None
        key = arr.tobytes()
        if key != self._lut_key:
            self._lut_dev = self._torch.from_numpy(arr).to(self.device)
            self._lut_dev.record_stream(self._copy)   # (read on the copy stream; a later lut may replace it mid-flight)
            self._lut_key = key
        return self._lut_dev

    @staticmethod
    def _fill(path: str, mv: memoryview) -> None:
        with open(path, "rb", buffering=0) as f:
            got = 0
            while got < len(mv):
                r = f.readinto(mv[got:])
                if not r:
                    raise EOFError(f"{path}: the file ends after {got} of {len(mv)} bytes")
                got += r

    def read(self, bin_paths: Sequence[str], label_paths: Optional[Sequence[str]] = None, lut=None,
             want_remission: bool = False, want_instance: bool = False, n_hist: int = 0) -> KittiScans:
        """The scans of bin_paths (and their labels) on the device, in the order given.  The outputs are the only
        allocation; the caller's current stream waits for the last decode, so work enqueued on it afterwards sees every
        scan.  ValueError, before anything is copied: scan_sizes' and plan_batches' complaints."""
        torch, hip = self._torch, self._hip
        bin_paths = [os.fspath(p) for p in bin_paths]
        label_paths = None if label_paths is None else [os.fspath(p) for p in label_paths]
        with_labels = label_paths is not None
        if not with_labels and (lut is not None or want_instance or n_hist):
            raise ValueError("lut, want_instance and n_hist need label_paths")
        n_hist = int(n_hist)
        if n_hist < 0 or n_hist > hip.SN_KITTI_MAX_HIST:
            raise ValueError(f"n_hist must lie in 0..{hip.SN_KITTI_MAX_HIST}")
        sizes = scan_sizes(bin_paths, label_paths)
        plan = plan_batches(sizes, 20 if with_labels else 16, self.batch_bytes, bin_paths)
        B, total, dev = len(sizes), int(sum(sizes)), self.device
        starts = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.int64)
        with torch.cuda.device(dev):
            current = torch.cuda.current_stream(dev)
            lut_dev = self._lut(lut)
            pts = torch.empty((total, 3), dtype=torch.float64, device=dev)
            labels = torch.empty((total,), dtype=torch.float64, device=dev) if with_labels else None
            remission = torch.empty((total,), dtype=torch.float32, device=dev) if want_remission else None
            instance = torch.empty((total,), dtype=torch.int32, device=dev) if want_instance else None
            hist = torch.zeros((B, n_hist), dtype=torch.int64, device=dev) if n_hist else None
            bad = torch.zeros((B,), dtype=torch.int32, device=dev)
            unmapped = torch.zeros((B,), dtype=torch.int32, device=dev) if lut_dev is not None else None
            offsets = torch.from_numpy(starts).to(dev)
            self._start.record(current)            # the copy stream starts behind the allocations and the zeroing
            self._copy.wait_event(self._start)
            for s0, s1 in plan:
                n = int(starts[s1] - starts[s0])
                if n == 0:
                    continue                       # (only empty scans: nothing to decode, the counts stay zero)
                b = self._turn
                self._turn ^= 1
                if self._copy_pending[b]:
                    self._copied[b].synchronize()   # the copy that last read this pinned buffer has completed
                    self._copy_pending[b] = False
                mv = memoryview(self._host_np[b])
                at = 0
                for k in range(s0, s1):
                    self._fill(bin_paths[k], mv[at:at + 16 * sizes[k]])
                    at += 16 * sizes[k]
                if with_labels:
                    for k in range(s0, s1):
                        self._fill(label_paths[k], mv[at:at + 4 * sizes[k]])
                        at += 4 * sizes[k]
                csr, nb = (at + 15) // 16 * 16, s1 - s0   # the batch's CSR rides behind the file bytes: one copy
                self._host_np[b][csr:csr + 8 * (nb + 1)].view(np.int64)[:] = starts[s0:s1 + 1] - starts[s0]
                with torch.cuda.stream(self._copy):
                    raw = self._raw[b]
                    raw[:csr + 8 * (nb + 1)].copy_(self._host[b][:csr + 8 * (nb + 1)], non_blocking=True)
                    self._copied[b].record(self._copy)
                    self._copy_pending[b] = True
                    first = int(starts[s0])
                    hip.kitti_decode(raw[:16 * n], raw[16 * n:20 * n] if with_labels else None, n,
                                     raw[csr:csr + 8 * (nb + 1)].view(torch.int64), pts[first:],
                                     None if labels is None else labels[first:], lut_dev,
                                     None if remission is None else remission[first:],
                                     None if instance is None else instance[first:],
                                     None if hist is None else hist[s0:s1], bad[s0:s1],
                                     None if unmapped is None else unmapped[s0:s1])
            self._done.record(self._copy)
            current.wait_event(self._done)
            for t in (pts, labels, remission, instance, hist, bad, unmapped):   # (written on the copy stream)
                if t is not None:
                    t.record_stream(self._copy)
        return KittiScans(pts, labels, offsets, tuple(int(n) for n in sizes), remission, instance, hist, bad, unmapped,
                          tuple(bin_paths))


def read_kitti_scan(bin_path: str, label_path: Optional[str] = None, device=None, **kw) -> KittiScans:
    """One scan through a KittiReader made for it, sized for it (a loop over scans keeps one KittiReader instead)."""
    need = os.stat(bin_path).st_size // 16 * 20
    reader = KittiReader(device, batch_bytes=max(need, 16))
    return reader.read([bin_path], None if label_path is None else [label_path], **kw)


def kitti_scan_lists(dataset_path: str, split: str = "samples", labels: bool = True) -> Tuple[List[str], List[str]]:
    """(scan_names, label_names) as semKITTI.py:332-381 lists them: the sequences 00..20 that exist under
    dataset_path/sequences/<seq>/velodyne (and labels), every file under them by os.walk, each list sorted on its own, then
    names[floor(beg * size) : floor(end * size)] with the splits samples [0, 1], train [0, .2], val [.2, .4], test [.4, 1].
    A sequence with scans and no labels folder, or lists of different lengths, make the reference's assert fail: ValueError
    here -- unless labels is False, which lists the scans only and returns [] for the labels.  Host only."""
    if split not in KITTI_SPLITS:
        raise ValueError(f"split must be one of {sorted(KITTI_SPLITS)} (got {split!r})")
    scan_names: List[str] = []
    label_names: List[str] = []
    for seq in range(21):
        seq = "{0:02d}".format(seq)
        scan_paths = os.path.join(dataset_path, "sequences", seq, "velodyne")
        if not os.path.isdir(scan_paths):
            continue
        scan_names += [os.path.join(dp, f) for dp, dn, fn in os.walk(os.path.expanduser(scan_paths)) for f in fn]
        if not labels:
            continue
        label_paths = os.path.join(dataset_path, "sequences", seq, "labels")
        if not os.path.isdir(label_paths):
            raise ValueError(f"{label_paths}: sequence {seq} has scans and no labels folder")
        label_names += [os.path.join(dp, f) for dp, dn, fn in os.walk(os.path.expanduser(label_paths)) for f in fn]
    scan_names.sort()
    label_names.sort()
    if labels and len(scan_names) != len(label_names):
        raise ValueError(f"{dataset_path}: {len(scan_names)} scans but {len(label_names)} label files")
    beg, end = KITTI_SPLITS[split]
    cut = lambda names: names[math.floor(beg * len(names)):math.floor(end * len(names))]   # noqa: E731
    return cut(scan_names), cut(label_names)


class semKITTI:
    """core/datasets/semKITTI.py:294-420 on the device.  `ds[idx]` gives the reference's shapes, (xyz [1,N,3] f64, gt [1,N]
    f64) without a transform and transform((xyz [N,3], gt [N])) with one; `batches(B)` iterates KittiScans of B consecutive
    scans, one launch each: the fast path.  The labels are the raw semantic classes (w & 0xFFFF), as SemLaserScan.sem_label
    holds them.  Not mirrored: the "corrupted or empty" substitute of :411-418 -- a bad file raises."""

    def __init__(self, dataset_path: str, split: str = "samples", transform=None, reader: Optional[KittiReader] = None
                 ) -> None:
        self.dataset_path, self.transform = dataset_path, transform
        self.scan_names, self.label_names = kitti_scan_lists(dataset_path, split)
        self._reader = reader

    @property
    def reader(self) -> KittiReader:
        if self._reader is None:
            self._reader = KittiReader()
        return self._reader

    def __len__(self) -> int:
        return len(self.scan_names)

    def __getitem__(self, idx):
        if hasattr(idx, "tolist"):
            idx = idx.tolist()
        scans = self.reader.read([self.scan_names[idx]], [self.label_names[idx]])
        xyz, gt = scans.pts, scans.labels
        if self.transform:
            return self.transform((xyz, gt))
        return xyz[None], gt[None, :]

    def batches(self, B: int, **kw) -> Iterator[KittiScans]:
        B = int(B)
        if B < 1:
            raise ValueError("B must be positive")
        for first in range(0, len(self), B):
            yield self.reader.read(self.scan_names[first:first + B], self.label_names[first:first + B], **kw)


def _save(samples_path: str, counter: int, sample) -> None:
    with open(os.path.join(samples_path, f"sample_{counter}.npy"), "wb") as f:
        np.save(f, sample.cpu().numpy())   # x, y, z, label


def build_pole_samples(dataset_path: str, save_path: str, batch: int = 32, reader: Optional[KittiReader] = None) -> int:
    """semKITTI.py:37-88: every scan of the dataset is cut into slabs along its longest axis (crop_pole_slabs) and a slab
    with at least five pole points (class 80) is written as save_path/samples/sample_{counter}.npy, [m,4] f64, counted from
    0 as the reference counts.  `batch` scans are decoded per launch.  Returns the number of samples written."""
    from .census import crop_pole_slabs
    samples_path = os.path.join(save_path, "samples")
    os.makedirs(samples_path, exist_ok=True)
    kitti = semKITTI(dataset_path, transform=None, reader=reader)
    counter = 0
    for scans in kitti.batches(batch, n_hist=260):
        for b in range(len(scans.sizes)):
            xyz, gt = scans.scan(b)
            for sample in crop_pole_slabs(xyz, gt, POLE_LABEL):
                _save(samples_path, counter, sample)
                counter += 1
    return counter


def build_pole_radius_samples(dataset_path: str, save_path: str, batch: int = 32, overwrite: Optional[bool] = None,
                              reader: Optional[KittiReader] = None) -> int:
    """semKITTI.py:105-158: a scan with a pole point -- np.any(gt == 80), read off hist[:, 80] in one host read per batch --
    has its pole points clustered and a disc cut around every cluster (pole_radius_samples); a disc with at least five pole
    points is written as save_path/samples/sample_{counter}.npy, [m,4] f64.  The reference's interactive question when the
    directory exists is `overwrite`: None raises FileExistsError, False returns at once, True continues counting from
    len(os.listdir).  Returns the counter behind the last sample."""
    from .census import pole_radius_samples
    samples_path = os.path.join(save_path, "samples")
    if not os.path.exists(samples_path):
        os.makedirs(samples_path)
        counter = 0
    else:
        if overwrite is None:
            raise FileExistsError(f"{samples_path} exists: pass overwrite=True to continue counting behind its files")
        if not overwrite:
            return len(os.listdir(samples_path))
        counter = len(os.listdir(samples_path))
    kitti = semKITTI(dataset_path, transform=None, reader=reader)
    for scans in kitti.batches(batch, n_hist=260):
        has_pole = (scans.hist[:, POLE_LABEL] > 0).cpu().tolist()
        for b in range(len(scans.sizes)):
            if not has_pole[b]:
                continue
            xyz, gt = scans.scan(b)
            for sample in pole_radius_samples(xyz, gt, POLE_LABEL):
                _save(samples_path, counter, sample)
                counter += 1
    return counter
