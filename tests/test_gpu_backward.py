"""Backward on the MI355X: sn_conv_corr + sn_geneo_bank_bwd behind torch.autograd, against autograd
through the oracle (which is the reference's own op sequence).  Tolerance: 2e-3 relative + 2e-4 absolute
(fp32 reductions over up to 10^5 terms vs the fp64 oracle)."""
import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip
from scene_net_amd.geneos import KIND_OF_CLASS, pack_params
from oracle import geneo_oracle as go

pytestmark = pytest.mark.gpu


def _close(a, b, rtol=2e-3, atol=2e-4):
    a, b = float(a), float(b)
    return abs(a - b) <= atol + rtol * max(abs(a), abs(b))


PARAMS = {
    "cy": dict(radius=2.3, sigma=1.4), "cone": dict(radius=1.7, sigma=1.2, apex=3.0, cone_radius=2.5, cone_inc=0.21),
    "neg": dict(radius=2.6, sigma=0.8, neg_factor=0.3),
    "cy_v1": dict(radius=2.1, sigma=1.6), "cone_v1": dict(radius=1.9, sigma=1.5, apex=3.0, cone_radius=2.2, cone_inc=0.6),
    "neg_v1": dict(radius=2.4, sigma=2.5, neg_factor=0.25),
}


@pytest.mark.parametrize("kind", list(PARAMS))
@pytest.mark.parametrize("ks", [(9, 9, 9), (9, 5, 5), (6, 5, 6)])
def test_generator_jacobians(hip_device, kind, ks):
    torch.manual_seed(3)
    dW = torch.randn(ks)
    leaf = {k: torch.tensor(v, dtype=torch.float32, requires_grad=(k != "apex")) for k, v in PARAMS[kind].items()}
    (go.geneo_kernel(kind, ks, leaf).double() * dW.double()).sum().backward()
    p = pack_params(KIND_OF_CLASS[kind], PARAMS[kind], hip_device).unsqueeze(0).contiguous()
    kinds = torch.tensor([KIND_OF_CLASS[kind]], dtype=torch.int32, device=hip_device)
    got = _hip.geneo_bank_bwd(p, kinds, ks, dW.unsqueeze(0).to(hip_device).contiguous())[0].cpu()
    slot = {"radius": _hip.SN_P_RADIUS, "sigma": _hip.SN_P_SIGMA, "cone_radius": _hip.SN_P_CONE_RADIUS,
            "cone_inc": _hip.SN_P_CONE_INC, "neg_factor": _hip.SN_P_NEG_FACTOR}
    for name, s in slot.items():
        if name in leaf:
            assert _close(got[s], leaf[name].grad), (kind, ks, name, float(got[s]), float(leaf[name].grad))
    assert got[_hip.SN_P_APEX].item() == 0.0


@pytest.mark.parametrize("ks", [(9, 9, 9), (9, 5, 5)])
def test_fused_parameter_backward_equals_its_parts(hip_device, ks):
    """sn_geneo_backward == sn_geneo_bank_bwd on dW_g = lambda_g C (bit for bit) and <K_g, C> - <K_last, C>."""
    torch.manual_seed(8)
    kinds_l = ["cy", "cone", "neg", "cy", "neg"]
    G, last = len(kinds_l), 3
    P = torch.stack([pack_params(KIND_OF_CLASS[k], {n: v * (1 + 0.07 * i) if n != "apex" else v
                                                    for n, v in PARAMS[k].items()}, hip_device)
                     for i, k in enumerate(kinds_l)]).contiguous()
    kinds = torch.tensor([KIND_OF_CLASS[k] for k in kinds_l], dtype=torch.int32, device=hip_device)
    bank = _hip.geneo_bank(P, kinds, ks)
    lam = (torch.rand(G, device=hip_device) - 0.3).contiguous()
    C = torch.randn(ks, device=hip_device).contiguous()
    out = torch.full((G * _hip.SN_NPARAM + G,), float("nan"), device=hip_device)
    _hip.geneo_backward(P, kinds, ks, bank, lam, C, last, out)
    dW = (lam.reshape(G, 1) * C.reshape(1, -1)).reshape(bank.shape).contiguous()
    parts = _hip.geneo_bank_bwd(P, kinds, ks, dW)
    assert torch.equal(out[: G * _hip.SN_NPARAM].view(G, _hip.SN_NPARAM), parts)
    dlam = (bank.reshape(G, -1).double() @ C.reshape(-1).double())
    want = (dlam - dlam[last]).float()
    got = out[G * _hip.SN_NPARAM:]
    assert got[last].item() == 0.0
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-4 * float(dlam.abs().max()))


def test_correlation_kernel(hip_device):
    """C[t] = sum delta * shifted x  ==  the weight gradient of a 1-kernel conv3d."""
    torch.manual_seed(5)
    for shape, ks in [((2, 1, 12, 10, 20), (5, 5, 5)), ((1, 1, 9, 17, 70), (9, 9, 9)), ((3, 1, 8, 8, 8), (6, 5, 6))]:
        x = (torch.rand(shape) < 0.3).double()
        g = torch.randn(shape).double() * (torch.rand(shape) < 0.4)
        w = torch.zeros((1, 1) + ks, dtype=torch.float64, requires_grad=True)
        (torch.nn.functional.conv3d(x, w, padding="same") * g).sum().backward()
        for xin in (x.bool(), x.float(), x):
            C = _hip.conv_corr(xin.to(hip_device), g.float().to(hip_device).contiguous(), None, ks)
            assert (C.cpu().double() - w.grad[0, 0]).abs().max().item() < 1e-3 * max(1.0, w.grad.abs().max().item())
        C1 = _hip.conv_corr(x.bool().to(hip_device), g.float().to(hip_device).contiguous(), None, ks)
        C2 = _hip.conv_corr(x.bool().to(hip_device), g.float().to(hip_device).contiguous(), None, ks)
        assert torch.equal(C1, C2)  # fixed-order reduction


@pytest.mark.parametrize("shape,ks", [((2, 1, 12, 10, 20), (5, 5, 5)), ((1, 1, 9, 17, 70), (9, 9, 9)),
                                      ((3, 1, 8, 8, 8), (6, 5, 6)), ((2, 1, 20, 33, 48), (9, 7, 9)),
                                      ((1, 1, 5, 3, 7), (3, 3, 3)), ((2, 1, 11, 40, 64), (9, 9, 9)),
                                      ((1, 1, 4, 6, 300), (3, 5, 17))])
@pytest.mark.parametrize("density", [0.0, 0.03, 0.6, 1.0])
def test_sparse_correlation_against_conv3d_weight_gradient(hip_device, shape, ks, density):
    """K4s -- binary occupancy: the gather over the set voxels -- == the weight gradient of a one-kernel conv3d (fp64, CPU),
    with and without the fused relu(tanh) derivative; == the GEMM form (K4) within fp32 summation error; every tile size of
    the gather gives the same numbers up to that error; two runs give the same bits (ragged extents, Y not a multiple of
    16, kernels of every parity, empty and full grids)."""
    torch.manual_seed(hash((shape, ks)) % 1000)
    x = torch.rand(shape) < density
    g = torch.randn(shape)
    o = torch.tanh(torch.randn(shape)).clamp_min(0.0)   # a forward output: relu(tanh(.)), zero on half the voxels
    xd, gd, od = x.to(hip_device), g.to(hip_device).contiguous(), o.to(hip_device).contiguous()
    for out_cpu, out_dev in ((None, None), (o, od)):
        delta = g.double() if out_cpu is None else g.double() * (out_cpu.double() > 0) * (1 - out_cpu.double() ** 2)
        w = torch.zeros((1, 1) + ks, dtype=torch.float64, requires_grad=True)
        (torch.nn.functional.conv3d(x.double(), w, padding="same") * delta).sum().backward()
        want = w.grad[0, 0]
        tol = 2e-4 * max(1.0, want.abs().max().item())
        got = {}
        for tile_bytes in (0, 1024, 256):
            with _hip.options(corr_dense=0, corr_sparse_tile_bytes=tile_bytes):
                got[tile_bytes] = _hip.conv_corr(xd, gd, out_dev, ks)
                again = _hip.conv_corr(xd, gd, out_dev, ks)
            assert torch.equal(got[tile_bytes], again), (shape, ks, tile_bytes)
            assert (got[tile_bytes].cpu().double() - want).abs().max().item() < tol, (shape, ks, density, tile_bytes)
        with _hip.options(corr_dense=1):   # the GEMM form (K4)
            dense = _hip.conv_corr(xd, gd, out_dev, ks)
        assert (dense.cpu().double() - want).abs().max().item() < tol
        if density == 0.0:
            assert not got[0].any()


def test_sparse_correlation_c2_shape_and_bf16(hip_device):
    """the training shape (64^3 tiles, 9^3 kernel, LiDAR-like density): K4s == K4 within fp32 summation error, for fp32 and
    bf16 gradient storage; bf16 inputs give the same bits as the same values widened (sums and products are fp32)."""
    torch.manual_seed(3)
    shape = (4, 1, 64, 64, 64)
    x = (torch.rand(shape, device=hip_device) < 0.035)
    x[:, :, 20:23] |= torch.rand((4, 1, 3, 64, 64), device=hip_device) < 0.25    # "ground" planes
    g = torch.randn(shape, device=hip_device)
    o = torch.tanh(torch.randn(shape, device=hip_device)).clamp_min(0.0)
    with _hip.options(corr_dense=0):
        sparse = _hip.conv_corr(x, g, o, (9, 9, 9))
        sparse16 = _hip.conv_corr(x, g.bfloat16(), o.bfloat16(), (9, 9, 9))
        sparse16w = _hip.conv_corr(x, g.bfloat16().float(), o.bfloat16().float(), (9, 9, 9))
    with _hip.options(corr_dense=1):
        dense = _hip.conv_corr(x, g, o, (9, 9, 9))
    scale = dense.abs().max().item()
    assert (sparse - dense).abs().max().item() < 2e-5 * scale
    assert torch.equal(sparse16, sparse16w)


@pytest.mark.parametrize("cls,geneo_num,ks", [(sna.SceneNet, {"cy": 2, "cone": 2, "neg": 1}, (9, 7, 7)),
                                              (sna.SCENE_Net, {"cy": 1, "cone": 1, "neg": 1}, (9, 5, 5)),
                                              (sna.SceneNet, {"cy": 6, "cone": 5, "neg": 5}, (9, 9, 9))])
def test_module_gradients_match_reference_autograd(hip_device, cls, geneo_num, ks):
    torch.manual_seed(11)
    model = cls(geneo_num, ks).to(hip_device)
    v1 = cls is sna.SCENE_Net
    with torch.no_grad():  # keep tanh out of saturation so the gradients are informative
        for n in model.geneos:
            model.lambdas_dict[f"lambda_{n}"].mul_(0.05)
    x = (torch.rand(2, 1, 20, 16, 24) < 0.1)
    wgt = torch.randn(2, 1, 20, 16, 24)
    names = list(model.geneos.keys())
    # oracle graph: leaves are clones of the module's scalars
    leaf = {n: {k: p.detach().cpu().clone().requires_grad_(k != "apex") for k, p in model.geneos[n].geneo_params.items()}
            for n in names}
    lam_leaf = [model.lambdas_dict[f"lambda_{n}"].detach().cpu().clone().requires_grad_(True) for n in names]
    last = names.index(model.last_lambda.replace("lambda_", ""))
    specs = [(n.split("_")[0] + ("_v1" if v1 else ""), leaf[n]) for n in names]
    ref = go.scenenet_forward(x.double(), specs, ks, lam_leaf, last, names=names)
    (ref * wgt.double()).sum().backward()

    for inp in (x.to(hip_device), x.double().to(hip_device)):  # int8 forward and fp32 forward
        model.zero_grad(set_to_none=True)
        out = model(inp)
        assert out.requires_grad
        assert (out.detach().double().cpu() - ref.detach()).abs().max().item() < 1e-4
        (out * wgt.to(hip_device).to(out.dtype)).sum().backward()
        for n in names:
            for k, p in model.geneos[n].geneo_params.items():
                if k == "apex":
                    assert p.grad is None
                    continue
                assert p.grad is not None and _close(p.grad, leaf[n][k].grad), (n, k, float(p.grad), float(leaf[n][k].grad))
        for i, n in enumerate(names):
            p = model.lambdas_dict[f"lambda_{n}"]
            if i == last:
                assert not p.requires_grad
            else:
                assert _close(p.grad, lam_leaf[i].grad), (n, float(p.grad), float(lam_leaf[i].grad))


def test_one_sgd_step_moves_the_loss(hip_device):
    torch.manual_seed(2)
    model = sna.SceneNet({"cy": 1, "cone": 1, "neg": 1}, (9, 5, 5)).to(hip_device)
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-2)
    x = (torch.rand(4, 1, 16, 16, 32, device=hip_device) < 0.15)
    y = (torch.rand(4, 1, 16, 16, 32, device=hip_device) < 0.05).float()
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = ((model(x) - y) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0]
    with torch.no_grad():
        model(x)  # like the reference, the frozen last coefficient is refreshed by the next forward
    assert abs(sum(float(p.detach()) for p in model.lambdas_dict.values()) - 1.0) < 1e-5  # convexity is maintained


def test_round3_entry_points_refuse_bad_arguments(hip_device):
    """sn_conv_corr_ws with a workspace too small for even the partial rows, sn_voxel_occupancy_fused_bank with a bank that
    is not 9 x 9 x 9 or a misaligned blob, sn_conv_fused_v without a verdict word: an error code and a message, no launch."""
    import ctypes
    lib = _hip.load()
    x = (torch.rand(1, 1, 8, 8, 16, device=hip_device) < 0.2)
    g = torch.randn(1, 1, 8, 8, 16, device=hip_device)
    C = torch.empty(27, device=hip_device)
    need = int(lib.sn_conv_corr_ws_bytes(_hip.SN_OCC8, 1, 8, 8, 16, 3, 3, 3))
    assert need >= int(lib.sn_conv_corr_blocks(1, 8, 8, 16)) * 27 * 4
    small = torch.empty(64, dtype=torch.uint8, device=hip_device)
    rc = lib.sn_conv_corr_ws(x.data_ptr(), _hip.SN_OCC8, g.data_ptr(), None, _hip.SN_F32, 1, 8, 8, 16, 3, 3, 3,
                             small.data_ptr(), 64, C.data_ptr(), None)
    assert rc != 0 and b"workspace" in lib.sn_last_error()
    # a workspace with room for the partial rows only: served by the GEMM form, same numbers as the gather up to fp32 order
    rows_only = int(lib.sn_conv_corr_blocks(1, 8, 8, 16)) * 27 * 4
    ws = torch.empty(rows_only, dtype=torch.uint8, device=hip_device)
    rc = lib.sn_conv_corr_ws(x.data_ptr(), _hip.SN_OCC8, g.data_ptr(), None, _hip.SN_F32, 1, 8, 8, 16, 3, 3, 3,
                             ws.data_ptr(), rows_only, C.data_ptr(), None)
    assert rc == 0
    ref = _hip.conv_corr(x, g, None, (3, 3, 3)).reshape(-1)
    assert (C - ref).abs().max().item() <= 1e-4 * max(1.0, ref.abs().max().item())
    # the rider entry: a 9 x 5 x 5 bank is refused before anything is launched
    model = sna.SceneNet({"cy": 1, "cone": 1, "neg": 1}, (9, 5, 5)).to(hip_device)
    with pytest.raises(sna.HipLibraryError):
        model.bank_rider(hip_device)
    pts = torch.rand(100, 3, dtype=torch.float64, device=hip_device)
    off = torch.tensor([0, 100], dtype=torch.int64, device=hip_device)
    params, kinds = model.packed_params(hip_device)
    bank = torch.empty((3, 9, 9, 9), device=hip_device)
    prep = torch.empty(_hip.SN_CONV_PREP_BYTES + 16, dtype=torch.uint8, device=hip_device)
    with pytest.raises(sna.HipLibraryError, match="16-byte"):
        _hip.voxel_occupancy_fused(pts, None, off, (32, 32, 32), out_dtype=torch.bool,
                                   bank_rider=(params, kinds, bank, prep[4:4 + _hip.SN_CONV_PREP_BYTES]))
    out = torch.empty(x.shape, device=hip_device)
    rc = lib.sn_conv_fused_v(x.data_ptr(), _hip.SN_OCC8, bank.data_ptr(), params.data_ptr(), 1, 8, 8, 16, 3, 9, 9, 9,
                             out.data_ptr(), _hip.SN_F32, None, 0, None)
    assert rc != 0 and b"null" in lib.sn_last_error()
