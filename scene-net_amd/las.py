"""LAS scans into HBM: the file's point records travel host-to-device as they are and are decoded there (K13:
sn_las_decode, csrc/las.hip).

The reference opens a scan with `lp.read(filename)` and `las_to_numpy(las)` (core/datasets/ts40k.py:73-86,
utils/pcd_processing.py:99-120): laspy scales three int32 columns to fp64, `np.vstack(...).transpose()` copies them into
[n,3], the class byte is copied out, all on one host core, and only then can the scan be uploaded.  Here the host parses
the public header block (`read_las_header`, `struct` only: laspy is not needed) and moves bytes:

    scan = sna.read_las("tile.las")                    # LasScan: xyz [n,3] f64, classes [n] f64, hist [256] i64, on the device
    xyz, classes = sna.las_to_numpy(scan)              # the reference's call shape
    sna.build_data_samples([las_dir], save_dir)        # LAS files in, TS40K sample files out (ts40k.py:31-148)

`LasReader` owns two pinned host buffers, two raw device buffers, one copy stream and its events, all allocated in the
constructor.  A file is cut into chunks of whole records; the caller's thread `readinto`s chunk k+1 into the free pinned
buffer while chunk k is copied and decoded on the copy stream.  There are no threads: every HIP call is made on the
caller's thread.  A pinned buffer is refilled only after the event behind its previous copy has completed; a raw device
buffer is overwritten by a copy that is ordered, on the one copy stream, behind the decode that read it.

Definition (normative, include/scenenet_hip.h): xyz = X * scale + offset in fp64 with the product and the sum rounded once
each (numpy's arithmetic, which is laspy's scaled view); classes = byte 15 & 31 for the point formats 0..5 (the synthetic,
key-point and withheld bits are dropped, as `las.classification` drops them) and byte 16 for 6..10; hist = np.bincount of
the classes, minlength 256.  Served: LAS 1.0-1.4, point formats 0..10, uncompressed.  LAZ is refused by the header parser.
Unpinned: no LAS file written by another program and no laspy exist where this was built -- the layout is pinned against
the ASPRS LAS 1.4 specification and numpy's arithmetic, not against laspy's output.
There is no CPU path: a reader on a CPU device raises HipLibraryError.
"""
from __future__ import annotations

import math
import os
import pickle
import random
import shutil
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

LAS_STANDARD_LENGTH = (20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67)   # point formats 0..10
LAS_HEADER_SIZE = (227, 227, 227, 235, 375)                          # LAS 1.0 .. 1.4
LAS_MAX_RECORD_LENGTH = 65535
POWER_LINE_SUPPORT_TOWER = 15


@dataclass(frozen=True)
class LasHeader:
    """What read_las_header takes from the public header block.  bbox = (max x, min x, max y, min y, max z, min z) as the
    file states it: returned as read, not trusted and not used."""
    path: str
    version: Tuple[int, int]
    header_size: int
    data_offset: int
    point_format: int
    record_length: int
    n_points: int
    scale: Tuple[float, float, float]
    offset: Tuple[float, float, float]
    bbox: Tuple[float, float, float, float, float, float]
    file_size: int

    @property
    def payload_bytes(self) -> int:
        return self.n_points * self.record_length


def read_las_header(path: str) -> LasHeader:
    """Parses the public header block of a LAS 1.0-1.4 file (host only).  ValueError, with the reason, for a wrong
    signature, a version other than 1.0-1.4, a LAZ-compressed file (format bits 6 or 7), a point format above 10, a record
    length below the format's standard length, a header size too small for the version, point data that would start inside
    the header or end beyond the file, and a scale or offset that is not finite.  Bytes behind the last record (the
    extended variable length records of LAS 1.4) are legal and are not read."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        head = f.read(375)
        size = os.fstat(f.fileno()).st_size
    if len(head) < 227:
        raise ValueError(f"{path}: {len(head)} bytes are no LAS header (227 at least)")
    if head[:4] != b"LASF":
        raise ValueError(f"{path}: signature {head[:4]!r} is not b'LASF'")
    major, minor = head[24], head[25]
    if major != 1 or minor > 4:
        raise ValueError(f"{path}: LAS version {major}.{minor} is not read (1.0 to 1.4)")
    header_size, data_offset = struct.unpack_from("<HI", head, 94)
    fmt_byte, record_length, legacy_count = struct.unpack_from("<BHI", head, 104)
    if fmt_byte & 0xC0:
        raise ValueError(f"{path}: point format byte {fmt_byte:#04x} has a compression bit set (LAZ is not served)")
    if fmt_byte > 10:
        raise ValueError(f"{path}: point format {fmt_byte} is above 10")
    if record_length < LAS_STANDARD_LENGTH[fmt_byte]:
        raise ValueError(f"{path}: record length {record_length} is below the {LAS_STANDARD_LENGTH[fmt_byte]} bytes of "
                         f"point format {fmt_byte}")
    if header_size < LAS_HEADER_SIZE[minor]:
        raise ValueError(f"{path}: header size {header_size} is too small for LAS 1.{minor} ({LAS_HEADER_SIZE[minor]})")
    if len(head) < LAS_HEADER_SIZE[minor]:
        raise ValueError(f"{path}: the file ends inside its LAS 1.{minor} header")
    if data_offset < header_size:
        raise ValueError(f"{path}: point data at byte {data_offset} would start inside the {header_size}-byte header")
    scale = struct.unpack_from("<3d", head, 131)
    offset = struct.unpack_from("<3d", head, 155)
    bbox = struct.unpack_from("<6d", head, 179)
    if not all(math.isfinite(v) for v in scale + offset):
        raise ValueError(f"{path}: scale {scale} / offset {offset} is not finite")
    n = legacy_count
    if minor == 4 and (legacy_count == 0 or fmt_byte >= 6):
        n = struct.unpack_from("<Q", head, 247)[0]
    if data_offset + n * record_length > size:
        raise ValueError(f"{path}: {n} records of {record_length} bytes from byte {data_offset} end beyond the file's "
                         f"{size} bytes (truncated)")
    return LasHeader(path, (major, minor), header_size, data_offset, fmt_byte, record_length, int(n), tuple(scale),
                     tuple(offset), tuple(bbox), size)


def plan_chunks(n_points: int, record_length: int, chunk_bytes: int) -> List[Tuple[int, int]]:
    """(first record, record count) of every chunk of a file: whole records, max(1, chunk_bytes // record_length) of them,
    the last chunk short.  Host only."""
    n_points, record_length, chunk_bytes = int(n_points), int(record_length), int(chunk_bytes)
    if record_length < 1 or chunk_bytes < 1 or n_points < 0:
        raise ValueError("record_length and chunk_bytes must be positive, n_points not negative")
    per = max(1, chunk_bytes // record_length)
    return [(first, min(per, n_points - first)) for first in range(0, n_points, per)]


@dataclass
class LasScan:
    """One decoded file on the device: xyz [n,3] f64, classes [n] f64 | None, hist [256] i64 | None, and its header."""
    xyz: "torch.Tensor"
    classes: Optional["torch.Tensor"]
    hist: Optional["torch.Tensor"]
    header: LasHeader


class LasReader:
    """Reads LAS files into HBM through buffers allocated once (module docstring).  `chunk_bytes` sizes the two pinned
    and the two device buffers; they hold one record of the largest legal length (65535 bytes) at least."""

    def __init__(self, device=None, chunk_bytes: int = 64 << 20) -> None:
        import torch
        from . import _hip
        self._torch, self._hip = torch, _hip
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise _hip.HipLibraryError("LasReader feeds HBM: device must be a HIP device; there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if int(chunk_bytes) < 1:
            raise ValueError("chunk_bytes must be positive")
        self.device, self.chunk_bytes = device, int(chunk_bytes)
        cap = max(self.chunk_bytes, LAS_MAX_RECORD_LENGTH)
        self._host = [torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._host_np = [h.numpy() for h in self._host]
        with torch.cuda.device(device):
            self._raw = [torch.empty(cap, dtype=torch.uint8, device=device) for _ in range(2)]
            self._copy = torch.cuda.Stream(device=device)
            self._copied = [torch.cuda.Event() for _ in range(2)]
            self._start, self._done = torch.cuda.Event(), torch.cuda.Event()
        self._copy_pending = [False, False]

    def plan(self, header: LasHeader) -> List[Tuple[int, int]]:
        return plan_chunks(header.n_points, header.record_length, self.chunk_bytes)

    def read(self, path: str, want_classes: bool = True, want_hist: bool = True) -> LasScan:
        """The file's points on the device.  The outputs are the only allocation; the caller's current stream waits for
        the last decode, so work enqueued on it afterwards sees the whole scan."""
        torch, hip = self._torch, self._hip
        h = read_las_header(path)
        n, S, dev = h.n_points, h.record_length, self.device
        with torch.cuda.device(dev):
            current = torch.cuda.current_stream(dev)
            xyz = torch.empty((n, 3), dtype=torch.float64, device=dev)
            classes = torch.empty((n,), dtype=torch.float64, device=dev) if want_classes else None
            hist = torch.zeros((256,), dtype=torch.int64, device=dev) if want_hist else None
            if n == 0:
                return LasScan(xyz, classes, hist, h)
            self._start.record(current)            # the copy stream starts behind the allocation and the zeroing
            self._copy.wait_event(self._start)
            with open(h.path, "rb", buffering=0) as f:
                f.seek(h.data_offset)
                for k, (first, count) in enumerate(self.plan(h)):
                    b, nbytes = k % 2, count * S
                    if self._copy_pending[b]:
                        self._copied[b].synchronize()   # the copy that last read this pinned buffer has completed
                        self._copy_pending[b] = False
                    mv = memoryview(self._host_np[b])[:nbytes]
                    got = 0
                    while got < nbytes:
                        r = f.readinto(mv[got:])
                        if not r:
                            raise EOFError(f"{h.path}: point data ends after {first * S + got} of {h.payload_bytes} bytes")
                        got += r
                    with torch.cuda.stream(self._copy):
                        self._raw[b][:nbytes].copy_(self._host[b][:nbytes], non_blocking=True)
                        self._copied[b].record(self._copy)
                        self._copy_pending[b] = True
                        hip.las_decode(self._raw[b][:nbytes], count, h.point_format, S, h.scale, h.offset, xyz[first:],
                                       None if classes is None else classes[first:], hist)
            self._done.record(self._copy)
            current.wait_event(self._done)
            for t in (xyz, classes, hist):   # (written on the copy stream: the allocator must not hand them out early)
                if t is not None:
                    t.record_stream(self._copy)
        return LasScan(xyz, classes, hist, h)


def read_las(path: str, device=None, chunk_bytes: int = 64 << 20, want_classes: bool = True, want_hist: bool = True
             ) -> LasScan:
    """One file through a LasReader made for it (a loop over files keeps one LasReader instead)."""
    return LasReader(device, chunk_bytes).read(path, want_classes, want_hist)


def las_to_numpy(las: LasScan):
    """(xyz [n,3] f64, classes [n] f64) of a LasScan, both on the device -- utils/pcd_processing.py:99-120's call shape."""
    if not isinstance(las, LasScan):
        raise TypeError("las_to_numpy takes the LasScan that read_las / LasReader.read return")
    if las.classes is None:
        raise ValueError("this LasScan was read without classes")
    return las.xyz, las.classes


def split_slices(sample_size: int, data_split: Dict[str, float]) -> Dict[str, Tuple[int, int]]:
    """The [start, stop) slice of the shuffled sample list that build_data_samples moves into every folder other than
    'fit', with the reference's arithmetic (ts40k.py:130-144): int(split_sum * size) .. math.ceil((split_sum + split) *
    size), split_sum running over the folders in the dictionary's order, 'fit' included."""
    out, split_sum = {}, 0
    for folder, split in data_split.items():
        if folder != "fit":
            out[folder] = (int(split_sum * sample_size), math.ceil((split_sum + split) * sample_size))
        split_sum += split
    return out


def build_data_samples(data_dirs: Sequence[str], save_dir: Optional[str] = None, tower_radius: bool = True,
                       data_split={"fit": .6, "test": .4}, seed: Optional[int] = None, reader: Optional[LasReader] = None
                       ) -> None:
    """core/datasets/ts40k.py:31-148 with the same file layout: every `.las` file of data_dirs is decoded on the device,
    skipped when it holds no point of class 15 (hist[15] == 0: one host read per file, the only one in front of the
    crops), cut into tower samples (crop_tower_samples, or crop_two_towers_samples with tower_radius False), each written
    as save_dir/fit/sample_{counter}.npy, (N,4) f64 through np.save; save_dir/read_files.pickle lists the files that are
    done, so a run resumes; then the samples are shuffled (the sorted list by random.Random(seed) with a seed,
    random.shuffle of os.listdir's order without) and the
    slices of split_slices are moved into their folders.  data_split == 0: no split.
    Deviations: the working directory is not changed (a file is named realpath(dir) + "/" + name, what the reference's
    os.getcwd() gives after its chdir); a file without a tower is recorded in read_files.pickle too, so that a resumed run
    does not decode it again (the reference leaves it out and reads it on every run)."""
    import torch
    from .clusters import crop_two_towers_samples
    from .crops import crop_tower_samples
    save_dir = os.getcwd() if save_dir is None else save_dir
    folders = list(data_split.keys()) if data_split != 0 else []
    for folder in folders + ["fit"]:
        os.makedirs(os.path.join(save_dir, folder), exist_ok=True)
    fit_path = os.path.join(save_dir, "fit")
    counter = len(os.listdir(fit_path))
    read_files: List[str] = []
    pik_path = os.path.join(save_dir, "read_files.pickle")
    if os.path.exists(pik_path):
        with open(pik_path, "rb") as f:
            read_files = pickle.load(f)
    for d in data_dirs:
        base = os.path.realpath(d)
        for las_file in os.listdir(base):
            filename = base + "/" + las_file
            if ".las" not in filename or filename in read_files:
                continue
            if reader is None:
                reader = LasReader()
            scan = reader.read(filename)
            samples: List[torch.Tensor] = []
            if int(scan.hist[POWER_LINE_SUPPORT_TOWER]) != 0:
                xyz, classes = las_to_numpy(scan)
                samples = crop_tower_samples(xyz, classes) if tower_radius else crop_two_towers_samples(xyz, classes)
            for sample in samples:
                with open(f"{fit_path}/sample_{counter}.npy", "wb") as f:
                    np.save(f, sample.cpu().numpy())   # x, y, z, class
                counter += 1
            del scan, samples
            read_files.append(filename)
            with open(pik_path, "wb") as f:
                pickle.dump(read_files, f)
    if data_split == 0:
        return
    samples = os.listdir(fit_path)
    if seed is not None:
        samples.sort()   # (os.listdir's order is the file system's: a seeded shuffle starts from a definite one)
    if seed is None:
        random.shuffle(samples)
    else:
        random.Random(seed).shuffle(samples)
    assert sum(list(data_split.values())) <= 1, "data splits should not surpass 1"
    for folder, (start, stop) in split_slices(len(samples), data_split).items():
        dst = os.path.join(save_dir, folder)
        os.makedirs(dst, exist_ok=True)
        for sample in samples[start:stop]:
            shutil.move(os.path.join(fit_path, sample), dst)
