"""Scans out of HBM into LAS files: xyz and classes are quantised and packed into point records on the device and the
record bytes travel device-to-host as the file will hold them (K15: sn_las_encode, csrc/las_write.hip).  The mirror image of
las.py (K13).

    scan = sna.read_las("tile.las")
    pred = ...                                                   # [n] f64 classes, on the device
    sna.write_las("tile_pred.las", scan.xyz, pred, like=scan.header)     # same format, same grid: the same X, Y, Z integers
    sna.reclassify_las("tile.las", "tile_pred.las", pred)        # or: keep every other byte of the file, patch the class

With laspy one would copy xyz and classes to the host (32 B per point), assign them to the scaled dimensions --
np.rint((x - offset) / scale) per column -- and pack the unaligned records on one host core.  `LasWriter` owns two raw device
buffers, two pinned host buffers, one copy stream and its events, all allocated in the constructor.  A scan is cut into
chunks of whole records; chunk k is encoded into a device buffer and copied to a pinned buffer on the copy stream while
the caller's thread writes chunk k - 1 to the file.  There are no threads: every HIP call is made on the caller's thread.
The file is written as `path + ".part"` and renamed onto `path` after the header -- count, bounding box -- has been
rewritten from what the device counted.

Definition (normative, include/scenenet_hip.h): X = rint((x - offset) / scale) in fp64, the difference and the true
quotient rounded once each, half to even (numpy's arithmetic, which is laspy's assignment to a scaled dimension), saturated
to int32; the class byte is written when the class is an integer the format can hold (0..31 for the point formats 0..3,
0..255 for 6..8) and 0 otherwise; both events are counted (`bad`), and `strict` refuses the file.  Every record is "return
1 of 1"; scan angle, user data, point source id, the flag bits and NIR are 0.  Served: the point formats 0, 1, 2, 3
(written as LAS 1.2) and 6, 7, 8 (LAS 1.4), uncompressed.  No variable length record is written, hence NO coordinate
reference system: a LAS 1.4 file of the formats 6..8 sets the WKT bit of the global encoding as the specification
demands, and carries no WKT record.  LAZ is not written.
There is no CPU path: a writer on a CPU device, or CPU tensors, raise HipLibraryError.
"""
from __future__ import annotations

import math
import os
import struct
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .las import LAS_HEADER_SIZE, LAS_STANDARD_LENGTH, LasHeader, plan_chunks, read_las_header

LAS_WRITE_FORMATS = (0, 1, 2, 3, 6, 7, 8)
LAS_WRITE_MAX_RECORD_LENGTH = 80
_GPS_FORMATS, _RGB_FORMATS = (1, 3, 6, 7, 8), (2, 3, 7, 8)
_INT32_MAX, _INT32_MIN = 2**31 - 1, -2**31
_EMPTY_BOX = (_INT32_MAX, _INT32_MIN) * 3
SYSTEM_IDENTIFIER = b"scene_net_amd"
GENERATING_SOFTWARE = b"scene_net_amd LasWriter (K15)"


@dataclass(frozen=True)
class LasWritten(LasHeader):
    """The header of a file LasWriter.write has made, as read_las_header parses it, and what the device counted on the
    way: box = (min X, max X, min Y, max Y, min Z, max Z) of the integers written, hist = the 256 class counts, bad =
    (points with a coordinate that did not fit int32, classes the format cannot hold -- written as 0)."""
    box: Tuple[int, ...] = _EMPTY_BOX
    hist: Tuple[int, ...] = (0,) * 256
    bad: Tuple[int, int] = (0, 0)


def box_to_bbox(box_xyz: Sequence[int], scale: Sequence[float], offset: Sequence[float]
                ) -> Tuple[float, float, float, float, float, float]:
    """(max x, min x, max y, min y, max z, min z), the header's order, of the integers (min X, max X, min Y, max Y, min
    Z, max Z): integer * scale + offset in numpy's arithmetic, the value a reader computes for those records.  An empty
    box (a minimum above its maximum) gives zeros."""
    out = []
    for a in range(3):
        lo, hi = int(box_xyz[2 * a]), int(box_xyz[2 * a + 1])
        if lo > hi:
            out += [0.0, 0.0]
            continue
        s, o = np.float64(scale[a]), np.float64(offset[a])
        v = np.array([lo, hi], dtype=np.int32) * s + o
        out += [float(v.max()), float(v.min())]   # (a negative scale swaps them)
    return tuple(out)


def las_header_bytes(point_format: int, record_length: int, n: int, scale: Sequence[float], offset: Sequence[float],
                     box_xyz: Sequence[int], version: Optional[Tuple[int, int]] = None, creation: Tuple[int, int] = (0, 0)
                     ) -> bytes:
    """The public header block of a file of `n` records (host only): LAS 1.2 (227 bytes) for the point formats 0..3, LAS 1.4
    (375 bytes, global-encoding bit 4 set) for 6..8; version=(1, 4) writes a 1.4 header for 0..3 too.  No variable length
    records -- so no coordinate reference system --: the data offset equals the header size.  Every point is the single
    return of its pulse: points-by-return[0] = n.  Formats 0..3 fill the legacy 32-bit count and refuse n >= 2^32; LAS
    1.4 fills the 64-bit count and the 15 x u64 points-by-return (and leaves the legacy fields 0 for the formats 6..8, as
    the specification demands).  The bounding box is box_to_bbox(box_xyz, scale, offset).  System identifier and generating
    software name this package; creation = (day of year, year) defaults to zeros, so equal inputs give equal files."""
    fmt, S, n = int(point_format), int(record_length), int(n)
    if fmt not in LAS_WRITE_FORMATS:
        raise ValueError(f"point format {fmt} is not written (served: {LAS_WRITE_FORMATS})")
    if not LAS_STANDARD_LENGTH[fmt] <= S <= 65535:
        raise ValueError(f"record length {S} is outside {LAS_STANDARD_LENGTH[fmt]}..65535 for point format {fmt}")
    if version is None:
        version = (1, 4) if fmt >= 6 else (1, 2)
    version = (int(version[0]), int(version[1]))
    if version not in ((1, 2), (1, 4)):
        raise ValueError(f"LAS {version[0]}.{version[1]} is not written (1.2 or 1.4)")
    if fmt >= 6 and version != (1, 4):
        raise ValueError(f"point format {fmt} needs LAS 1.4")
    if n < 0 or (fmt <= 5 and n >= 2**32):
        raise ValueError(f"{n} points do not fit the 32-bit count of point format {fmt}")
    if len(scale) != 3 or len(offset) != 3 or len(box_xyz) != 6:
        raise ValueError("scale and offset have 3 entries each, box_xyz has 6")
    if not all(math.isfinite(float(v)) for v in tuple(scale) + tuple(offset)):
        raise ValueError(f"scale {tuple(scale)} / offset {tuple(offset)} is not finite")
    minor = version[1]
    size = LAS_HEADER_SIZE[minor]
    h = bytearray(size)
    h[0:4] = b"LASF"
    struct.pack_into("<HH", h, 4, 0, 0x10 if minor == 4 else 0)      # file source id, global encoding (bit 4: WKT)
    h[24], h[25] = 1, minor
    h[26:26 + len(SYSTEM_IDENTIFIER)] = SYSTEM_IDENTIFIER           # char[32] each, zero padded
    h[58:58 + len(GENERATING_SOFTWARE)] = GENERATING_SOFTWARE
    struct.pack_into("<HH", h, 90, int(creation[0]), int(creation[1]))
    struct.pack_into("<HII", h, 94, size, size, 0)                   # header size, offset to point data, number of VLRs
    legacy = n if fmt <= 5 else 0
    struct.pack_into("<BHI5I", h, 104, fmt, S, legacy, legacy, 0, 0, 0, 0)
    struct.pack_into("<3d", h, 131, *[float(v) for v in scale])
    struct.pack_into("<3d", h, 155, *[float(v) for v in offset])
    struct.pack_into("<6d", h, 179, *box_to_bbox(box_xyz, scale, offset))
    if minor == 4:
        struct.pack_into("<QQI", h, 227, 0, 0, 0)                    # waveform data start, first EVLR, number of EVLRs
        struct.pack_into("<Q15Q", h, 247, n, n, *([0] * 14))
    return bytes(h)


def class_byte_offset(point_format: int) -> int:
    return 15 if point_format <= 5 else 16


def patch_class_bytes(rows: np.ndarray, point_format: int, classes_u8: np.ndarray) -> None:
    """In place, on the host: writes the classes into the records `rows` [m, record_length] uint8.  Formats 0..5: byte 15
    = (old & 0xE0) | c, the synthetic, key-point and withheld bits are kept; formats 6..10: byte 16 = c."""
    c = np.asarray(classes_u8, dtype=np.uint8)
    if rows.ndim != 2 or c.shape != (rows.shape[0],):
        raise ValueError("rows is [m, record_length] and classes holds m entries")
    if point_format <= 5:
        rows[:, 15] = (rows[:, 15] & 0xE0) | c
    else:
        rows[:, 16] = c


class LasWriter:
    """Writes LAS files from HBM through buffers allocated once (module docstring).  `chunk_bytes` sizes the two device
    and the two pinned buffers; they hold one record of the largest served length (80 bytes) at least."""

    def __init__(self, device=None, chunk_bytes: int = 64 << 20) -> None:
        import torch
        from . import _hip
        self._torch, self._hip = torch, _hip
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise _hip.HipLibraryError("LasWriter drains HBM: device must be a HIP device; there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if int(chunk_bytes) < 1:
            raise ValueError("chunk_bytes must be positive")
        self.device, self.chunk_bytes = device, int(chunk_bytes)
        cap = max(self.chunk_bytes, LAS_WRITE_MAX_RECORD_LENGTH)
        self._host = [torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._host_np = [h.numpy() for h in self._host]
        with torch.cuda.device(device):
            self._raw = [torch.empty(cap, dtype=torch.uint8, device=device) for _ in range(2)]   # (16-byte aligned and more)
            self._copy = torch.cuda.Stream(device=device)
            self._copied = [torch.cuda.Event() for _ in range(2)]
            self._start, self._done = torch.cuda.Event(), torch.cuda.Event()

    def plan(self, n_points: int, record_length: int) -> List[Tuple[int, int]]:
        return plan_chunks(n_points, record_length, self.chunk_bytes)

    def _check_inputs(self, xyz, classes, intensity, gps_time, rgb) -> int:
        torch, hip = self._torch, self._hip
        for name, t in (("xyz", xyz), ("classes", classes), ("intensity", intensity), ("gps_time", gps_time), ("rgb", rgb)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise hip.HipLibraryError(f"{name} must be a tensor on a HIP device; there is no CPU path")
            if t.device != self.device:
                raise hip.HipLibraryError(f"{name} lives on {t.device}, this writer on {self.device}")
            if not t.is_contiguous():
                raise hip.HipLibraryError(f"{name} must be contiguous")
        if xyz.dtype != torch.float64 or xyz.dim() != 2 or xyz.shape[1] != 3:
            raise hip.HipLibraryError("xyz must be [n,3] float64")
        n = int(xyz.shape[0])
        for name, t, dtypes, shape in (("classes", classes, (torch.float64,), (n,)),
                                       ("intensity", intensity, (torch.uint16, torch.int16), (n,)),
                                       ("gps_time", gps_time, (torch.float64,), (n,)),
                                       ("rgb", rgb, (torch.uint16, torch.int16), (n, 3))):
            if t is not None and (t.dtype not in dtypes or tuple(t.shape) != shape):
                raise hip.HipLibraryError(f"{name} must be {list(shape)} {dtypes[0]} (got {list(t.shape)} {t.dtype})")
        return n

    def write(self, path: str, xyz, classes=None, intensity=None, gps_time=None, rgb=None, *,
              point_format: Optional[int] = None, scale: Optional[Sequence[float]] = None,
              offset: Optional[Sequence[float]] = None, like: Optional[LasHeader] = None, extra_bytes: int = 0,
              strict: bool = True) -> LasWritten:
        """xyz [n,3] f64, classes [n] f64, intensity [n] u16, gps_time [n] f64, rgb [n,3] u16 (all but xyz optional, all
        on this writer's device) -> the file `path`.  `like` (a LasHeader, e.g. scan.header) supplies point format, scale
        and offset wherever they are not given: a scan goes back out on the grid it came in on.  Otherwise the format is 0,
        plus 1 with gps_time, plus 2 with rgb, and 6 (7 with rgb) if any class exceeds 31 (one device reduction); the scale
        is 0.001 and the offset floor(min xyz) over the finite coordinates (one more).  Records are the format's standard
        length plus `extra_bytes` zero bytes.  With `strict`, a coordinate that does not fit int32 at this scale and offset
        (NaN, inf) or a class the format cannot hold removes the part file and raises ValueError; without, the file is
        written with the saturated integers and class 0 and the returned header's `bad` says how many.  Synchronises."""
        torch, hip = self._torch, self._hip
        path = os.fspath(path)
        n = self._check_inputs(xyz, classes, intensity, gps_time, rgb)
        dev = self.device
        with torch.cuda.device(dev):
            if point_format is None and like is not None:
                point_format = like.point_format
            if point_format is None:
                point_format = (1 if gps_time is not None else 0) + (2 if rgb is not None else 0)
                if classes is not None and n and bool((classes > 31).any()):
                    point_format = 7 if rgb is not None else 6
            fmt = int(point_format)
            if fmt not in LAS_WRITE_FORMATS:
                raise hip.HipLibraryError(f"point format {fmt} is not written (served: {LAS_WRITE_FORMATS})")
            if gps_time is not None and fmt not in _GPS_FORMATS:
                raise hip.HipLibraryError(f"point format {fmt} holds no gps_time")
            if rgb is not None and fmt not in _RGB_FORMATS:
                raise hip.HipLibraryError(f"point format {fmt} holds no rgb")
            S = LAS_STANDARD_LENGTH[fmt] + int(extra_bytes)
            if extra_bytes < 0 or S > LAS_WRITE_MAX_RECORD_LENGTH:
                raise hip.HipLibraryError(f"record length {S} is outside {LAS_STANDARD_LENGTH[fmt]}.."
                                          f"{LAS_WRITE_MAX_RECORD_LENGTH} for point format {fmt}")
            if fmt <= 5 and n >= 2**32:
                raise ValueError(f"{n} points do not fit the 32-bit count of point format {fmt}")
            if scale is None:
                scale = like.scale if like is not None else (0.001, 0.001, 0.001)
            if offset is None:
                if like is not None:
                    offset = like.offset
                elif n:
                    lo = torch.where(torch.isfinite(xyz), xyz, torch.full_like(xyz, math.inf)).amin(dim=0).floor().tolist()
                    offset = tuple(v if math.isfinite(v) else 0.0 for v in lo)
                else:
                    offset = (0.0, 0.0, 0.0)
            scale, offset = tuple(float(v) for v in scale), tuple(float(v) for v in offset)
            if len(scale) != 3 or len(offset) != 3:
                raise ValueError("scale and offset have 3 entries each")
            if not all(math.isfinite(v) for v in scale + offset) or 0.0 in scale:
                raise ValueError(f"scale {scale} must be finite and not zero, offset {offset} finite")

            part = path + ".part"
            box, hist, bad = _EMPTY_BOX, (0,) * 256, (0, 0)
            try:
                with open(part, "wb", buffering=0) as f:
                    f.write(las_header_bytes(fmt, S, n, scale, offset, _EMPTY_BOX))   # (room: rewritten below)
                    if n:
                        box, hist, bad = self._stream_out(f, xyz, classes, intensity, gps_time, rgb, n, fmt, S, scale, offset)
                        f.seek(0)
                        f.write(las_header_bytes(fmt, S, n, scale, offset, box))
                if strict and (bad[0] or bad[1]):
                    raise ValueError(f"{path}: {bad[0]} points have a coordinate that is NaN or does not fit int32 at scale "
                                     f"{scale} and offset {offset}, {bad[1]} classes are no integer of 0.."
                                     f"{31 if fmt <= 5 else 255} (strict: nothing is written)")
                os.replace(part, path)
            except BaseException:
                self._copy.synchronize()   # (no copy may still be landing in a pinned buffer)
                if os.path.exists(part):
                    os.remove(part)
                raise
        h = read_las_header(path)
        return LasWritten(h.path, h.version, h.header_size, h.data_offset, h.point_format, h.record_length, h.n_points,
                          h.scale, h.offset, h.bbox, h.file_size, box, hist, bad)

    def _stream_out(self, f, xyz, classes, intensity, gps_time, rgb, n, fmt, S, scale, offset):
        """encodes and writes the n records behind the file's current position; returns (box, hist, bad) as tuples"""
        torch, hip = self._torch, self._hip
        dev = self.device
        current = torch.cuda.current_stream(dev)
        box_t = torch.tensor(_EMPTY_BOX, dtype=torch.int32, device=dev)
        counts = torch.zeros(256 + 2, dtype=torch.int64, device=dev)   # hist, bad
        self._start.record(current)   # the copy stream starts behind whatever made the inputs, and behind the two above
        self._copy.wait_event(self._start)
        plan = self.plan(n, S)
        for k, (first, count) in enumerate(plan):
            b, nbytes = k % 2, count * S
            # raw[b] and host[b] are free: chunk k - 2 was written to the file in the previous round
            with torch.cuda.stream(self._copy):
                hip.las_encode(xyz[first:], count, fmt, S, scale, offset, self._raw[b],
                               None if classes is None else classes[first:],
                               None if intensity is None else intensity[first:],
                               None if gps_time is None else gps_time[first:],
                               None if rgb is None else rgb[first:], box_t, counts[:256], counts[256:])
                self._host[b][:nbytes].copy_(self._raw[b][:nbytes], non_blocking=True)
                self._copied[b].record(self._copy)
            if k:   # chunk k - 1 goes to the file while chunk k is encoded and copied
                self._copied[1 - b].synchronize()
                f.write(memoryview(self._host_np[1 - b])[:plan[k - 1][1] * S])
        b = (len(plan) - 1) % 2
        self._copied[b].synchronize()
        f.write(memoryview(self._host_np[b])[:plan[-1][1] * S])
        with torch.cuda.stream(self._copy):
            box = tuple(int(v) for v in box_t.cpu().tolist())
            c = counts.cpu().tolist()
        self._done.record(self._copy)
        current.wait_event(self._done)
        for t in (xyz, classes, intensity, gps_time, rgb, box_t, counts):   # (read on the copy stream: the allocator must
            if t is not None:                                               # not hand their memory out before it is done)
                t.record_stream(self._copy)
        return box, tuple(int(v) for v in c[:256]), (int(c[256]), int(c[257]))


def write_las(path: str, xyz, classes=None, intensity=None, gps_time=None, rgb=None, *, device=None,
              chunk_bytes: int = 64 << 20, **options) -> LasWritten:
    """One file through a LasWriter made for it (a loop over files keeps one LasWriter instead).  `options`: the keyword
    arguments of LasWriter.write."""
    import torch
    if device is None and isinstance(xyz, torch.Tensor) and xyz.is_cuda:
        device = xyz.device
    if device is None or torch.device(device).type != "cuda":
        from . import _hip
        raise _hip.HipLibraryError("write_las drains HBM: xyz must live on a HIP device; there is no CPU path")
    return LasWriter(device, chunk_bytes).write(path, xyz, classes, intensity, gps_time, rgb, **options)


def reclassify_las(src: str, dst: str, classes, device=None, chunk_bytes: int = 64 << 20) -> LasHeader:
    """Copies the LAS file `src` to `dst` with the class of every point replaced by `classes` ([n] on a HIP device, any
    real dtype; cast to bytes there, so one byte per point comes device-to-host).  Every other byte is kept: intensity, GPS
    time, RGB, the variable length records in front of the points and whatever follows them; the point formats 0..5 keep
    the three flag bits of byte 15.  All point formats 0..10 are served -- nothing but the class byte is interpreted.  The
    length of `classes` and that every class is an integer the format holds (0..31 for the formats 0..5, 0..255 above) are
    checked on the device before `dst` is touched (ValueError); src == dst is refused.  No kernel of its own: sending the
    records up and down to patch one byte in 20..67 would move 60 times the bytes.  Returns dst's header."""
    import torch
    from . import _hip
    src, dst = os.fspath(src), os.fspath(dst)
    if not isinstance(classes, torch.Tensor) or not classes.is_cuda:
        raise _hip.HipLibraryError("classes must be a tensor on a HIP device; there is no CPU path")
    if device is not None and torch.device(device).type != "cuda":
        raise _hip.HipLibraryError("reclassify_las casts the classes on a HIP device; there is no CPU path")
    if os.path.realpath(src) == os.path.realpath(dst) or (os.path.exists(dst) and os.path.samefile(src, dst)):
        raise ValueError(f"{src}: source and destination are the same file")
    h = read_las_header(src)
    n, S, fmt = h.n_points, h.record_length, h.point_format
    if classes.dim() != 1 or classes.shape[0] != n:
        raise ValueError(f"{src} holds {n} points, classes has the shape {list(classes.shape)}")
    top = 31 if fmt <= 5 else 255
    if n:
        c = classes.to(torch.float64)
        ok = (c == c.floor()) & (c >= 0) & (c <= top)
        wrong = n - int(ok.sum())
        if wrong:
            raise ValueError(f"{wrong} classes are no integer of 0..{top}, what point format {fmt} holds")
        c8 = c.to(torch.uint8).cpu().numpy()
    else:
        c8 = np.zeros(0, dtype=np.uint8)
    part = dst + ".part"
    per = max(1, int(chunk_bytes) // S)
    try:
        with open(src, "rb") as fi, open(part, "wb") as fo:
            left = h.data_offset
            while left:                      # header and variable length records
                blob = fi.read(min(left, 1 << 20))
                if not blob:
                    raise EOFError(f"{src}: the file ends in front of its point data")
                fo.write(blob)
                left -= len(blob)
            for first in range(0, n, per):
                m = min(per, n - first)
                blob = bytearray(m * S)
                if fi.readinto(blob) != m * S:
                    raise EOFError(f"{src}: point data ends inside record {first}..{first + m}")
                patch_class_bytes(np.frombuffer(blob, dtype=np.uint8).reshape(m, S), fmt, c8[first:first + m])
                fo.write(blob)
            while True:                      # whatever follows the points
                blob = fi.read(1 << 20)
                if not blob:
                    break
                fo.write(blob)
        os.replace(part, dst)
    except BaseException:
        if os.path.exists(part):
            os.remove(part)
        raise
    return read_las_header(dst)
