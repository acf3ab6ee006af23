"""K6 training metrics on the device (sn_binary_stats / BinarySegmentationMetrics) against a torch-on-CPU oracle:
`(pred >= tau)` on pred's own dtype and `target.to(torch.int) == 1`, the reading of torchmetrics 0.9 that metrics.py
documents.  Counts must match bit for bit."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import scene_net_amd as sna
from scene_net_amd import _hip
from scene_net_amd import metrics as snm

pytestmark = pytest.mark.gpu

PRED_DT = [torch.float32, torch.bfloat16, torch.float64]
TGT_DT = [torch.float32, torch.float64, torch.bfloat16, torch.uint8, torch.bool, torch.int32]
C2 = 32 * 64 ** 3
SIZES = [1, 63, 64, 1000 + 3, 2 ** 20 + 5, C2]


def oracle_counts(pred, target, tau):
    """(tp, fp, fn, tn, bad_pred, bad_target) on the CPU with torch's own semantics."""
    p, t = pred.detach().cpu().reshape(-1), target.detach().cpu().reshape(-1)
    pp = p >= tau
    ti = t.to(torch.int)
    tt = ti == 1
    pf = p.float() if p.dtype == torch.bfloat16 else p
    bad_p = int(((pf < 0) | (pf > 1)).sum())
    bad_t = int(((ti != 0) & (ti != 1)).sum())
    if t.dtype.is_floating_point:   # NaN / Inf truncate to whatever the CPU makes of them: bad either way
        bad_t = int((~torch.isfinite(t.float()) | ((ti != 0) & (ti != 1))).sum())
    tp = int((pp & tt).sum())
    return (tp, int((pp & ~tt).sum()), int((~pp & tt).sum()), int((~pp & ~tt).sum()), bad_p, bad_t)


def device_counts(pred, target, tau=0.65, beta=0.5):
    ws = torch.empty(_hip.SN_METRIC_WS_BYTES // 8, dtype=torch.int64, device=pred.device)
    state = torch.zeros(6, dtype=torch.int64, device=pred.device)
    batch = torch.full((6,), -7, dtype=torch.int64, device=pred.device)
    _hip.binary_stats(pred, target, tau, beta, ws, state, batch=batch)
    b = tuple(int(v) for v in batch.cpu())
    assert tuple(int(v) for v in state.cpu()) == b
    return b


def _data(n, pdt, tdt, gen):
    p = torch.rand(n, generator=gen, dtype=torch.float64)
    p[torch.rand(n, generator=gen) < 0.05] = 0.65   # the threshold itself, as the dtype rounds it
    p = p.to(pdt)
    if tdt == torch.bool:
        t = torch.rand(n, generator=gen) < 0.3
    elif tdt.is_floating_point:
        vals = torch.tensor([0.0, 1.0, 0.999, 1.7, 0.3, 1.0], dtype=torch.float64)
        t = vals[torch.randint(0, len(vals), (n,), generator=gen)].to(tdt)
    else:
        t = torch.randint(0, 2, (n,), generator=gen).to(tdt)
    return p, t


@pytest.mark.parametrize("pdt", PRED_DT, ids=str)
@pytest.mark.parametrize("tdt", TGT_DT, ids=str)
def test_counts_match_the_cpu_oracle(hip_device, pdt, tdt):
    gen = torch.Generator().manual_seed(11)
    for n in SIZES:
        p, t = _data(n + 2, pdt, tdt, gen)
        pd, td = p.to(hip_device), t.to(hip_device)
        for lo_p, lo_t in ((0, 0), (1, 1), (1, 0), (2, 1)):   # aligned, both at offset 1, misaligned against each other
            want = oracle_counts(p[lo_p:lo_p + n], t[lo_t:lo_t + n], 0.65)
            got = device_counts(pd[lo_p:lo_p + n], td[lo_t:lo_t + n])
            assert got == want, (n, lo_p, lo_t, got, want)


def _neighbours(x):
    """x rounded to its dtype, and its two neighbours one ulp away (x > 0)."""
    bits = {torch.float32: torch.int32, torch.bfloat16: torch.int16}[x.dtype]
    i = x.view(bits)
    return (i - 1).view(x.dtype), x, (i + 1).view(x.dtype)


@pytest.mark.parametrize("pdt", [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize("tau", [0.65, 0.5, 0.1, 1 / 3])
def test_threshold_boundary(hip_device, pdt, tau):
    x = torch.tensor([tau], dtype=pdt)
    below, at, above = _neighbours(x)
    p = torch.cat([below, at, above])
    t = torch.ones(3, dtype=torch.bool)
    pp = p >= tau
    assert pp.tolist() == [False, True, True]   # the CPU oracle: tau is rounded to pred's dtype
    got = device_counts(p.to(hip_device), t.to(hip_device), tau=tau)
    assert got == oracle_counts(p, t, tau) == (2, 0, 1, 0, 0, 0)


def test_fp32_tau_rounding_counts_0p65_as_positive(hip_device):
    p = torch.tensor([0.65, 0.6484375, 0.65], dtype=torch.float32)
    t = torch.tensor([1, 1, 0], dtype=torch.int32)
    assert device_counts(p.to(hip_device), t.to(hip_device)) == (1, 1, 1, 0, 0, 0)
    pb = p.to(torch.bfloat16)   # bf16: 0.65 -> 0.6484375, so all three are positive
    assert device_counts(pb.to(hip_device), t.to(hip_device)) == (2, 1, 0, 0, 0, 0)


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64, torch.bfloat16], ids=str)
def test_target_truncation_and_bad_values(hip_device, tdt):
    vals = [0.999 if tdt != torch.bfloat16 else 0.99,   # (bf16 rounds 0.999 to 1.0)
            1.0, 1.7, -0.5, 0.0, 2.0, -1.0, float("nan"), float("inf"), float("-inf"), 5.5]
    t = torch.tensor(vals, dtype=tdt)
    p = torch.full((len(vals),), 0.9, dtype=torch.float32)
    got = device_counts(p.to(hip_device), t.to(hip_device))
    # positives: 1.0 and 1.7; bad: 2.0, -1.0, nan, inf, -inf, 5.5
    assert got == (2, len(vals) - 2, 0, 0, 0, 6)
    assert got[:4] == oracle_counts(p, t, 0.65)[:4]
    m = sna.init_metrics().to(hip_device)
    m.update(p.to(hip_device), t.to(hip_device))
    with pytest.raises(ValueError, match="target"):
        m.compute()
    m.reset()
    assert m.state_counts()["bad_target"] == 0 and sum(m.state.tolist()) == 0


@pytest.mark.parametrize("tdt,vals,bad", [(torch.uint8, [0, 1, 2, 255], 2), (torch.int32, [0, 1, 2, -1], 2),
                                          (torch.bool, [False, True], 0)], ids=["u8", "i32", "bool"])
def test_integer_targets(hip_device, tdt, vals, bad):
    t = torch.tensor(vals, dtype=tdt)
    p = torch.full((len(vals),), 0.9, dtype=torch.float32)
    got = device_counts(p.to(hip_device), t.to(hip_device))
    assert got == oracle_counts(p, t, 0.65) and got[5] == bad and got[0] == 1


def test_nan_and_out_of_range_preds(hip_device):
    p = torch.tensor([float("nan"), 0.9, 0.1, float("nan")], dtype=torch.float32)
    t = torch.tensor([1, 1, 0, 0], dtype=torch.bool)
    assert device_counts(p.to(hip_device), t.to(hip_device)) == (1, 0, 1, 2, 0, 0)   # NaN: negative, not an error
    m = sna.init_metrics().to(hip_device)
    m.update(p.to(hip_device), t.to(hip_device))
    m.compute()
    m.update(torch.tensor([-0.1, 1.1, 0.5], device=hip_device), torch.ones(3, dtype=torch.bool, device=hip_device))
    assert m.state_counts()["bad_pred"] == 2
    with pytest.raises(ValueError, match=r"should be probabilities, but values were detected outside of \[0,1\] range"):
        m.compute()
    m.reset()
    assert m.state.tolist() == [0] * 6
    with pytest.warns(UserWarning, match="before any update"):
        z = m.compute()
    assert tuple(z) == snm.METRIC_NAMES and all(float(v) == 0.0 for v in z.values())


def test_accumulation_and_batch_values(hip_device):
    gen = torch.Generator().manual_seed(5)
    sizes = [17, 4096, 100_003, 63, 1 << 18]
    parts = [_data(n, torch.float32, torch.bool, gen) for n in sizes]
    m = sna.init_metrics().to(hip_device)
    returned = []
    for p, t in parts:
        out = m(p.to(hip_device), t.to(hip_device))
        assert tuple(out) == snm.METRIC_NAMES and all(v.dim() == 0 and v.dtype == torch.float32 for v in out.values())
        returned.append(({k: v for k, v in out.items()}, {k: float(v) for k, v in out.items()}))
        alone = sna.init_metrics().to(hip_device)
        alone.update(p.to(hip_device), t.to(hip_device))
        ref = alone.compute()
        assert {k: float(v) for k, v in out.items()} == {k: float(v) for k, v in ref.items()}
        c = alone.state_counts()
        assert {k: float(v) for k, v in out.items()} == snm.binary_metric_values(c["tp"], c["fp"], c["fn"], c["tn"])
    for tensors, floats in returned:   # later calls wrote fresh buffers: earlier results are unchanged
        assert {k: float(v) for k, v in tensors.items()} == floats
    whole = sna.init_metrics().to(hip_device)
    whole.update(torch.cat([p for p, _ in parts]).to(hip_device), torch.cat([t for _, t in parts]).to(hip_device))
    assert m.state.tolist() == whole.state.tolist()
    want = oracle_counts(torch.cat([p for p, _ in parts]), torch.cat([t for _, t in parts]), 0.65)
    assert tuple(m.state.tolist()) == want
    a, b = m.compute(), whole.compute()
    assert {k: float(v) for k, v in a.items()} == {k: float(v) for k, v in b.items()}
    assert {k: float(v) for k, v in a.items()} == snm.binary_metric_values(*want[:4])


def _count_periodic(n, period, pos_idx):
    q, r = divmod(n, period)
    return q * len(pos_idx) + sum(1 for i in pos_idx if i < r)


def test_counts_above_32_bits(hip_device):
    """n = 2^31 + 17 elements, pattern of period 15 built on the device: pred positive at i % 15 == 0, target positive at
    i % 15 in {0, 1}.  Three updates push tn past 2^32."""
    n = 2 ** 31 + 17
    base_p = torch.full((15,), 0.2, dtype=torch.bfloat16, device=hip_device)
    base_p[0] = 0.9
    base_t = torch.zeros(15, dtype=torch.bool, device=hip_device)
    base_t[:2] = True
    reps = (n + 14) // 15
    p = base_p.repeat(reps)[:n]
    t = base_t.repeat(reps)[:n]
    npred = _count_periodic(n, 15, [0])
    ntgt = _count_periodic(n, 15, [0, 1])
    tp = npred
    one = (tp, npred - tp, ntgt - tp, n - npred - ntgt + tp, 0, 0)
    m = sna.init_metrics().to(hip_device)
    for _ in range(3):
        m.update(p, t)
    got = tuple(m.state.tolist())
    assert got == tuple(3 * v for v in one)
    assert got[3] > 2 ** 32
    del p, t
    torch.cuda.empty_cache()


def test_update_replays_from_a_captured_graph(hip_device):
    gen = torch.Generator().manual_seed(9)
    p, t = _data(300_001, torch.float32, torch.float32, gen)
    pd, td = p.to(hip_device), t.to(hip_device)
    m = sna.init_metrics().to(hip_device)
    m.update(pd, td)   # warm-up outside the capture
    one = tuple(m.state.tolist())
    assert one == oracle_counts(p, t, 0.65)
    m.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.update(pd, td)
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    assert tuple(m.state.tolist()) == tuple(10 * v for v in one)


def _training_parts(dev, seed=21):
    from scene_net_amd.synthetic import synthetic_tile
    tiles, labels = zip(*[synthetic_tile(t, 20_000) for t in range(2)])
    torch.manual_seed(seed)
    model = sna.SceneNet({"cy": 2, "cone": 1, "neg": 1}, (9, 5, 5)).to(dev)
    with torch.no_grad():
        for n in model.geneos:
            model.lambdas_dict[f"lambda_{n}"].mul_(0.1)
    batch = sna.PointBatch.from_tiles(tiles, labels, device=dev)
    pipe = sna.ScenePipeline(model, (32, 32, 32), keep_labels=[15.0])
    gt = pipe.voxelize(batch, want_gt=True).gt_occ
    crit = sna.GENEO_Tversky_Loss(targets=gt.float(), weighting_scheme_path=None, save_weighting_scheme=False)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-2, capturable=True)
    return pipe, crit, opt, batch


def test_captured_training_step_counts_each_replay(hip_device):
    m = sna.init_metrics().to(hip_device)
    pipe, crit, opt, batch = _training_parts(hip_device)
    step = sna.CapturedTrainingStep(pipe, crit, opt, batch, warmup=2, metrics=m)
    assert m.state.tolist() == [0] * 6          # warm-up and capture are not counted
    total = np.zeros(6, dtype=np.int64)
    losses = []
    for _ in range(6):
        losses.append(step.replay().item())
        total += np.array(oracle_counts(step.pred, step.target, 0.65))
    assert step.target.dtype == torch.bool and step.pred.shape == step.target.shape
    assert m.state.tolist() == total.tolist()
    assert total[:4].sum() == 6 * step.pred.numel()
    # the metrics do not perturb training: the same trajectory without them, with the keyword and without it
    for kw in ({}, {"metrics": None}):
        pipe2, crit2, opt2, batch2 = _training_parts(hip_device)
        step2 = sna.CapturedTrainingStep(pipe2, crit2, opt2, batch2, warmup=2, **kw)
        assert [step2.replay().item() for _ in range(6)] == losses


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _pg_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import scene_net_amd as sna_w
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    gen = torch.Generator().manual_seed(123)   # the same global data on both ranks; each takes its half
    n = 1_000_001
    p = torch.rand(n, generator=gen)
    t = torch.rand(n, generator=gen) < 0.2
    half = sna_w.shard_range(n, rank, world)
    m = sna_w.init_metrics().to(dev)
    m.update(p[half[0]:half[1]].to(dev), t[half[0]:half[1]].to(dev))
    synced = {k: float(v) for k, v in m.compute().items()}
    local = sna_w.BinarySegmentationMetrics(sync_on_compute=False).to(dev)
    local.update(p[half[0]:half[1]].to(dev), t[half[0]:half[1]].to(dev))
    whole = sna_w.BinarySegmentationMetrics(sync_on_compute=False).to(dev)
    whole.update(p.to(dev), t.to(dev))
    q.put((rank, synced, {k: float(v) for k, v in local.compute().items()},
           {k: float(v) for k, v in whole.compute().items()}, m.state.tolist()))
    dist.destroy_process_group()


def test_compute_all_reduces_over_the_process_group():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_pg_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, s0, l0, w0, st0), (_, s1, l1, w1, st1) = res
    assert s0 == s1 == w0 == w1
    assert l0 != l1          # each rank counted a different half; compute() left the local state as it was
    assert st0 != st1
