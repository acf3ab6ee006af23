"""What the thinning tests share (tests/test_thin_host.py, tests/test_gpu_thin.py): the reference's two downsampling loops
(utils/pcd_processing.py:375-420 and :423-474) restated literally in numpy over the project's own binning oracle
(tests/binning_cases.py::expected_flat -- pyntcloud is not installed, so its binning is not pinned here, as for K1), the
plain scan-order oracle, the Philox4x32-10 restatement and the case builders.  No test lives here."""
import numpy as np

from scene_net_amd.thin import philox4x32, philox_uniforms   # noqa: F401  (the restatement the device is compared with)

import binning_cases as bc

# philox4x32-10 known answers (Random123, kat_vectors): counter, key, output
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

SEED = 0x9E3779B97F4A7C15          # both 32-bit halves non-zero
BIG_TILE_ID = 2 ** 32 + 7          # the counter's fourth word is not zero
NONE, Z, VOXEL = 0, 1, 2           # SN_THIN_GROUP_*


def groups_of(kind, dims, flat):
    """The group of every point from its flat [z][x][y] index (-1: unbinned stays -1)."""
    nx, ny, _ = dims
    flat = np.asarray(flat, dtype=np.int64)
    if kind == NONE:
        return np.zeros_like(flat)
    if kind == Z:
        return np.where(flat < 0, -1, flat // (nx * ny))
    return flat


def n_groups(kind, dims):
    nx, ny, nz = dims
    return {NONE: 1, Z: nz, VOXEL: nx * ny * nz}[kind]


def keep_mask(group, u, thr):
    """keep iff binned and u <= thr[group], literally (NaN on either side: False)."""
    group = np.asarray(group)
    binned = group >= 0
    with np.errstate(invalid="ignore"):
        return binned & (np.asarray(u) <= np.asarray(thr)[np.maximum(group, 0)])


def scan_order(group, u, thr):
    """The plain oracle: the kept points in scan order."""
    return np.flatnonzero(keep_mask(group, u, thr))


def reference_order(group, u, thr):
    """The reference's loops, literally: a dict of lists in insertion order, then per group `idx[u[idx] <= thr]`; u is
    indexed by scan index.  A point without a group (the reference has none: its grid is built from the cloud) is left out,
    the project's rule.  Returns the indices in the order the reference returns them."""
    u = np.asarray(u)
    voxels = dict()
    for i in range(len(group)):
        idx = int(group[i])
        if idx < 0:
            continue
        vox = voxels.get(idx, list())
        vox.append(int(i))
        voxels[idx] = vox
    sampling = np.zeros(len(group))
    counter = 0
    for vox in voxels:
        npvox = np.array(voxels[vox])
        selected = u[npvox]
        with np.errstate(invalid="ignore"):
            sample = npvox[selected <= thr[vox]]
        end = counter + len(sample)
        sampling[counter:end] = sample
        counter = end
    return sampling[:counter].astype(int)


def first_appearance(group, G):
    """[G] int64: the smallest index of any point of each group, -1 (all ones) for an empty group."""
    first = np.full(G, -1, dtype=np.int64)
    for i in range(len(group) - 1, -1, -1):
        if group[i] >= 0:
            first[group[i]] = i
    return first


def expected_batch(tiles, kind, dims, desc, thr, us):
    """The whole batch's expectation: tiles (list of [n_b,3]), desc [B, desc_len] | None, thr [B, G], us (list of [n_b]) ->
    dict(src: packed indices kept in scan order, key, offsets [B+1], unbinned [B], first [B, G], groups: list)."""
    G = n_groups(kind, dims)
    src, key, sizes, unb, first, groups = [], [], [], [], [], []
    start = 0
    for b, t in enumerate(tiles):
        flat = bc.expected_flat(desc[b], dims, t) if kind != NONE else np.zeros(len(t), dtype=np.int64)
        g = groups_of(kind, dims, flat)
        kept = scan_order(g, us[b], thr[b])
        src.append(kept + start)
        key.append(g[kept])
        sizes.append(len(kept))
        unb.append(int((g < 0).sum()))
        first.append(first_appearance(g, G))
        groups.append(g)
        start += len(t)
    return dict(src=np.concatenate(src).astype(np.int64), key=np.concatenate(key).astype(np.int64),
                offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), unbinned=np.array(unb, dtype=np.int64),
                first=np.stack(first), groups=groups)


def cube_cloud(n, seed, shuffle=True):
    """n points uniform in a 20 m cube at UTM scale: every z slab of a regular 64^3 grid is populated from a few thousand
    points on.  Not shuffled: sorted by z, so that z slabs are visited in ascending first appearance."""
    rng = np.random.default_rng(seed)
    pts = bc.UTM + rng.random((n, 3)) * 20.0
    if not shuffle:
        pts = pts[np.argsort(pts[:, 2], kind="stable")]
    return pts


def own_desc(pts, dims):
    """The n-mode descriptor sn_voxel_prepare(regular=1) builds for one tile, with the oracle's arithmetic."""
    from oracle import voxel_oracle as vo
    g = vo.voxelgrid_compute(pts, n_xyz=dims)
    return np.concatenate([g["xyzmin"], g["xyzmax"]] + [vo.linspace_edges(g["xyzmin"][a], g["xyzmax"][a], dims[a])
                                                        for a in range(3)])
