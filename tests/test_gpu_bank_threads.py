"""The bank builder's body is a function of (tid, nthreads): its hosts run it with 1024 threads (the rider of the one-pass
voxelisation kernel at 64^3) and with 256 (the stand-alone kernels, the rider of the bounding-box kernel at 128^3).  Whatever
the workgroup, the same bits: the bank and every field of the preparation blob a kernel reads are byte-equal across

    stand-alone K2 (sn_geneo_bank) + stand-alone preparation (sn_conv_bank_prep)
    K2 with the preparation as its tail (sn_geneo_bank_prep)
    the 64^3 rider  (sn_voxel_occupancy_fused_bank, one-pass kernel)
    the 128^3 rider (sn_voxel_occupancy_fused_bank, bounding-box kernel)

for G = 16, 4 (twelve pad entries) and 20 (two groups), and for a bank with a poisoned (NaN) kernel and an all-zero one.
The kernel sizes other than 9 x 9 x 9 have no preparation: there the two stand-alone builders (sn_geneo_bank,
sn_geneo_bank_lambdas) must agree byte for byte, and with the golden kernels within test_gpu_bank's 2e-6.

Every kernel a GENEO's parameters can give is symmetric in x and y, so those hosts only ever see the symmetry verdict 1; the
verdict 0 is reached through the one host that takes weights (sn_conv_bank_prep), tap by tap.

The give-up counter is cumulative per process and device, without a reset: it is checked as the difference of two readings."""
import json
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip
from scene_net_amd.geneos import KIND_OF_CLASS, pack_params
from scene_net_amd.synthetic import apply_bank_spec, synthetic_bank_spec, synthetic_tile

pytestmark = pytest.mark.gpu
TOL = 2e-6   # tests/test_gpu_bank.py: fp32 closed form vs the reference's op order

# (name, first byte, one past the last) -- conv_prep.h's blob layout: what the contraction kernels and their callers read
FIELDS = [("digit table", 0, 12288), ("scales", 12288, 12352), ("bounds", 12352, 12480), ("symmetry", 12480, 12544),
          ("fit", 12544, 12608), ("magic", 12608, 12612), ("route", 12672, 12676), ("zero block", 12800, 12816)]


def _packed(hip_device, geneo_num):
    specs, names, lambdas, last = synthetic_bank_spec(geneo_num)
    model = sna.SceneNet(geneo_num, (9, 9, 9))
    apply_bank_spec(model, specs, names, lambdas, last)
    params, kinds = model.to(hip_device).packed_params(hip_device)
    return params.clone(), kinds.clone()


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _four_forms(params, kinds, hip_device):
    """{form: (bank bytes, blob bytes)}"""
    G = params.shape[0]
    nblob = _hip.SN_CONV_PREP_BYTES * ((G + 15) // 16)
    out = {}
    bank = _hip.geneo_bank(params, kinds, (9, 9, 9))
    out["K2 + preparation, stand-alone"] = (_bytes(bank), _bytes(_hip.conv_bank_prep(bank)))
    bank_p, _, prep_p = _hip.geneo_bank_prep(params, kinds)
    out["K2 with the preparation as its tail"] = (_bytes(bank_p), _bytes(prep_p))
    tiles = [synthetic_tile(i, 20_000 + 1000 * i)[0] for i in range(3)]
    batch = sna.PointBatch.from_tiles(tiles, device=hip_device)
    for name, n in (("64^3 rider", 64), ("128^3 rider", 128)):
        b = torch.full((G, 9, 9, 9), float("nan"), dtype=torch.float32, device=hip_device)
        p = torch.zeros(nblob, dtype=torch.uint8, device=hip_device)
        _hip.voxel_occupancy_fused(batch.pts, None, batch.offsets, (n, n, n), out_dtype=torch.bool,
                                   bank_rider=(params, kinds, b, p))
        out[name] = (_bytes(b), _bytes(p))
    return out


def _assert_same(forms, G):
    names = list(forms)
    bank0, blob0 = forms[names[0]]
    for name in names[1:]:
        bank, blob = forms[name]
        assert np.array_equal(bank, bank0), (name, "bank")
        for grp in range((G + 15) // 16):
            o = grp * _hip.SN_CONV_PREP_BYTES
            for field, lo, hi in FIELDS:
                if field in ("magic", "route", "zero block") and grp > 0:
                    continue   # written once per preparation, by kernel 0 of the first group
                assert np.array_equal(blob[o + lo:o + hi], blob0[o + lo:o + hi]), (name, grp, field)
    return bank0, blob0


@pytest.mark.parametrize("geneo_num", [{"cy": 6, "cone": 5, "neg": 5}, {"cy": 2, "cone": 1, "neg": 1},
                                       {"cy": 7, "cone": 6, "neg": 7}])
def test_every_host_of_the_bank_body_writes_the_same_bytes(hip_device, geneo_num):
    params, kinds = _packed(hip_device, geneo_num)
    G = params.shape[0]
    assert G in (16, 4, 20)
    _, blob = _assert_same(_four_forms(params, kinds, hip_device), G)
    assert blob[12608:12612].view(np.int32)[0] == 0x5a57414c
    assert blob[12672:12676].view(np.int32)[0] == -1 and not blob[12800:12816].any()
    for grp in range((G + 15) // 16):
        o = grp * _hip.SN_CONV_PREP_BYTES
        assert blob[o + 12480:o + 12544].view(np.int32).tolist() == [1] * 16   # every family is symmetric; pads too
        scales = blob[o + 12288:o + 12352].view(np.float32)
        live = min(16, G - 16 * grp)
        assert (scales[:live] > 0).all() and not scales[live:].any()


def test_a_poisoned_and_an_all_zero_kernel(hip_device):
    params, kinds = _packed(hip_device, {"cy": 6, "cone": 5, "neg": 5})
    assert int(kinds[3]) == _hip.SN_GENEO_CY and int(kinds[5]) == _hip.SN_GENEO_CY
    params[3, _hip.SN_P_SIGMA] = float("nan")   # sigma x exp(.): every tap NaN
    params[5, _hip.SN_P_SIGMA] = 0.0            # every tap 0, so is every mean
    bank, blob = _assert_same(_four_forms(params, kinds, hip_device), 16)
    w = bank.view(np.float32).reshape(16, 729)
    assert np.isnan(w[3]).all() and not w[5].any() and np.isfinite(np.delete(w, 3, 0)).all()
    scales = blob[12288:12352].view(np.float32)
    assert np.isnan(scales[3]) and scales[5] == 0.0 and (np.delete(scales, [3, 5]) > 0).all()
    # Q = 0 for both: their lanes of the digit table (lane = 16 qq + g of every uint4 row) are zero
    wd = blob[:12288].reshape(12, 64, 16)
    for g in (3, 5):
        assert not wd[:, [g, 16 + g, 32 + g, 48 + g], :].any()
    assert wd[:, [0, 16, 32, 48], :].any()


def test_the_symmetry_verdict_tap_by_tap(hip_device):
    """One tap of an otherwise symmetric kernel moved by one ulp: the verdict is 0 unless the tap is its own mirror in x and
    in y (dx = dy = 4) -- for taps in every part of the kernel, the corners and the centre planes among them."""
    params, kinds = _packed(hip_device, {"cy": 6, "cone": 5, "neg": 5})
    bank = _hip.geneo_bank(params, kinds, (9, 9, 9)).cpu().numpy().copy()
    taps = [(0, 0, 0), (8, 8, 8), (4, 4, 4), (3, 4, 4), (2, 4, 1), (6, 7, 4), (0, 8, 0), (5, 0, 8), (8, 3, 5), (1, 4, 8),
            (7, 1, 4), (4, 5, 5), (2, 2, 2), (3, 6, 0), (6, 4, 3), (0, 4, 4)]   # kernel g gets tap (dz, dx, dy)
    expect = []
    for g, (dz, dx, dy) in enumerate(taps):
        bank[g, dz, dx, dy] = np.nextafter(bank[g, dz, dx, dy], np.float32(np.inf))
        bits = bank[g].view(np.uint32)
        expect.append(int(np.array_equal(bits, bits[:, ::-1, :]) and np.array_equal(bits, bits[:, :, ::-1])))
        assert expect[-1] == int(dx == 4 and dy == 4)
    assert 0 in expect and 1 in expect
    blob = _bytes(_hip.conv_bank_prep(torch.from_numpy(bank).to(hip_device)))
    assert blob[12480:12544].view(np.int32).tolist() == expect


def test_other_kernel_sizes_through_both_standalone_builders(hip_device, golden_dir):
    K = np.load(os.path.join(golden_dir, "geneo_kernels.npz"))
    with open(os.path.join(golden_dir, "geneo_kernels_meta.json")) as f:
        cases = json.load(f)
    sizes = sorted({tuple(m["kernel_size"]) for m in cases})
    assert (9, 9, 9) in sizes and len(sizes) > 1
    for ks in sizes:
        mine = [m for m in cases if tuple(m["kernel_size"]) == ks]
        params = torch.stack([pack_params(KIND_OF_CLASS[m["kind"]], m["params"], hip_device) for m in mine]).contiguous()
        kinds = torch.tensor([KIND_OF_CLASS[m["kind"]] for m in mine], dtype=torch.int32, device=hip_device)
        G = len(mine)
        bank = _hip.geneo_bank(params, kinds, ks)
        lam = torch.full((G,), 1.0 / G, dtype=torch.float32, device=hip_device)
        order = torch.arange(G, dtype=torch.int32, device=hip_device)
        bank_l, _ = _hip.geneo_bank_lambdas(params, kinds, ks, lam, order, G - 1)
        assert np.array_equal(_bytes(bank), _bytes(bank_l)), ks
        got = bank.cpu().numpy()
        for i, m in enumerate(mine):
            err = np.abs(got[i] - K[m["key"]]).max()
            assert err < TOL, (m["key"], err)


def test_exchange_giveups_are_counted(hip_device):
    """The one-pass kernel counts the workgroups that gave up the box exchange: none in a normal run; with the wait switched
    off, every workgroup that does not find all its siblings' tags at its first look -- some, and at most the launch's 8
    workgroups per tile (one that looks last may still see them all) -- with the same grids either way."""
    tiles = [synthetic_tile(i, 30_000)[0] for i in range(4)]
    batch = sna.PointBatch.from_tiles(tiles, device=hip_device)
    c0 = _hip.voxel_onepass_giveups()
    plain = sna.voxelize_batch(batch, (64, 64, 64), occ_dtype=torch.bool)
    assert _hip.voxel_onepass_giveups() == c0
    with _hip.options(voxel_onepass_spin=0):
        alone = sna.voxelize_batch(batch, (64, 64, 64), occ_dtype=torch.bool)
        c1 = _hip.voxel_onepass_giveups()
    assert 0 < c1 - c0 <= 8 * len(tiles)
    assert torch.equal(alone.occ, plain.occ) and torch.equal(alone.desc, plain.desc)
