"""SemanticKITTI decode (K14): the numpy oracle -- np.frombuffer, reshape, `& 0xFFFF`, `>> 16`, astype(float64), the class
remap, np.bincount per scan -- and the builders its host and GPU tests share.  The layout is the published SemanticKITTI
one: .bin little-endian float32 [n,4] (x, y, z, remission), .label little-endian uint32 [n], semantic class in the low 16
bits, instance id in the high 16.  Everything is compared exactly."""
import os

import numpy as np

FLT_MAX_BITS = 0x7F7FFFFF


def decode_oracle(bin_bytes, label_bytes, sizes, lut=None, n_hist=0):
    """dict of what sn_kitti_decode is to give for the concatenated .bin bytes (and .label bytes | None) of scans of
    `sizes` points: pts [total,3] f64, remission [total] f32, labels [total] f64, instance [total] i32, hist [B,n_hist]
    i64, bad [B] i32, unmapped [B] i32 (labels .. unmapped None where they do not apply)."""
    total = int(sum(sizes))
    rows = np.frombuffer(bytes(bin_bytes), dtype="<f4").reshape(-1, 4)
    assert rows.shape[0] == total
    with np.errstate(invalid="ignore"):
        pts = rows[:, :3].astype(np.float64)          # numpy's widening: a signalling NaN is quietened, payload kept
    out = {"pts": pts, "remission": rows[:, 3].copy(), "labels": None, "instance": None, "hist": None, "unmapped": None}
    bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    finite = np.isfinite(rows[:, :3]).all(axis=1)
    out["bad"] = np.array([int((~finite[a:b]).sum()) for a, b in zip(bounds[:-1], bounds[1:])], dtype=np.int32)
    if label_bytes is None:
        return out
    w = np.frombuffer(bytes(label_bytes), dtype="<u4")
    assert w.shape[0] == total
    sem = (w & 0xFFFF).astype(np.int64)
    out["instance"] = (w >> 16).astype(np.int32)
    if lut is None:
        cls = sem
    else:
        lut = np.asarray(lut, dtype=np.int64)
        inside = sem < lut.size
        cls = np.where(inside, lut[np.minimum(sem, lut.size - 1)], -1)
        out["unmapped"] = np.array([int((~inside[a:b]).sum()) for a, b in zip(bounds[:-1], bounds[1:])], dtype=np.int32)
    out["labels"] = cls.astype(np.float64)
    if n_hist:
        hist = np.zeros((len(sizes), n_hist), dtype=np.int64)
        for s, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            c = cls[a:b]
            c = c[(c >= 0) & (c < n_hist)]
            hist[s] = np.bincount(c, minlength=n_hist)
        out["hist"] = hist
    return out


def random_scans(sizes, seed, classes=None):
    """(bin bytes, label bytes) of scans of `sizes` points: coordinates of a lidar's range, every class of the 16 bits or
    (with `classes`) a draw from that list, random instance ids"""
    rng = np.random.default_rng(seed)
    total = int(sum(sizes))
    rows = (rng.standard_normal((total, 4)) * [30.0, 30.0, 2.0, 0.3]).astype("<f4")
    sem = rng.integers(0, 65536, total, dtype=np.uint32) if classes is None else rng.choice(np.asarray(classes, dtype=np.uint32), total)
    words = (sem | (rng.integers(0, 65536, total, dtype=np.uint32) << 16)).astype("<u4")
    return rows.tobytes(), words.tobytes()


def edge_floats():
    """f32 bit patterns (uint32): +-0, denormals, +-inf, quiet and signalling NaNs with payloads, FLT_MAX, and ordinary values"""
    return np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00400000, 0x00000100, 0x807FFFFF,
                     0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FC12345, 0x7F800001, 0xFF800001, 0x7FBFFFFF,
                     0xFFA5A5A5, FLT_MAX_BITS, 0xFF7FFFFF, 0x00800000, 0x3F800000, 0xC2F6E979], dtype=np.uint32)


def edge_words():
    return np.array([0, 0xFFFF, 0x10000, 0xFFFF0050, 0xFFFFFFFF, 80 | 7 << 16], dtype=np.uint32)


def edge_scan():
    """(bin bytes, label bytes, n): every edge float in every column against ordinary values in the others, the edge words
    cycled over the points"""
    e = edge_floats()
    rows = []
    for col in range(4):
        for v in e:
            r = [0x3F800000, 0x40000000, 0x40400000, 0x3E800000]
            r[col] = int(v)
            rows.append(r)
    rows.append([int(e[13]), int(e[8]), int(e[10]), int(e[9])])        # everything non-finite at once
    rows = np.array(rows, dtype=np.uint32)
    w = np.resize(edge_words(), rows.shape[0]).astype("<u4")
    return rows.astype("<u4").tobytes(), w.tobytes(), rows.shape[0]


def write_sequence(root, seq, scans, with_labels=True):
    """writes scans = [(bin bytes, label bytes), ...] as root/sequences/<seq>/velodyne/%06d.bin and labels/%06d.label;
    returns (bin paths, label paths)"""
    vel = os.path.join(root, "sequences", seq, "velodyne")
    lab = os.path.join(root, "sequences", seq, "labels")
    os.makedirs(vel, exist_ok=True)
    if with_labels:
        os.makedirs(lab, exist_ok=True)
    bins, labels = [], []
    for k, (b, l) in enumerate(scans):
        bins.append(os.path.join(vel, f"{k:06d}.bin"))
        with open(bins[-1], "wb") as f:
            f.write(b)
        if with_labels:
            labels.append(os.path.join(lab, f"{k:06d}.label"))
            with open(labels[-1], "wb") as f:
                f.write(l)
    return bins, labels


def pole_scan(n, poles, seed):
    """(bin bytes, label bytes) of a 60 m x 40 m x 3 m patch of n ground points (class 40) with `poles` = [(x, y, count)]:
    `count` pole points (class 80) within 0.2 m of a vertical line at (x, y)"""
    rng = np.random.default_rng(seed)
    rows = np.empty((n, 4), dtype=np.float32)
    rows[:, 0] = rng.uniform(0, 60, n)
    rows[:, 1] = rng.uniform(0, 40, n)
    rows[:, 2] = rng.uniform(0, 0.3, n)
    rows[:, 3] = rng.uniform(0, 1, n)
    sem = np.full(n, 40, dtype=np.uint32)
    at = 0
    for x, y, count in poles:
        rows[at:at + count, 0] = x + rng.uniform(-0.2, 0.2, count)
        rows[at:at + count, 1] = y + rng.uniform(-0.2, 0.2, count)
        rows[at:at + count, 2] = rng.uniform(0, 3, count)
        sem[at:at + count] = 80
        at += count
    words = (sem | (rng.integers(0, 9, n, dtype=np.uint32) << 16)).astype("<u4")
    return rows.astype("<f4").tobytes(), words.tobytes()
