"""The threshold sweep on the device (sn_binary_curve / BinarySegmentationCurve) against a torch-on-CPU oracle in the
direct form: `pred >= tau` per threshold on pred's own dtype and `target.to(torch.int) == 1`, never the code under test.
Counts must match bit for bit, and column k must equal what sn_binary_stats gives at tau = thresholds[k]."""
import os
import socket

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
OFFSETS = ((0, 0), (1, 1), (1, 0), (2, 1))   # aligned, both at offset 1, misaligned against each other
LIN20 = torch.linspace(0.5, 0.95, 20).tolist()
CAP = _hip.SN_CURVE_MAX_THRESHOLDS
# 0.6484375 and its bf16 neighbours (one ulp = 2^-8 in [0.5, 1)), and two values that bf16 rounds onto 0.6484375:
# distinct columns in fp32 / fp64, equal columns in bf16
BF16_ULP = [0.64453125, 0.6484375, 0.6485, 0.649, 0.65234375, 0.65625]
SWEEPS = {"lin20": LIN20, "one": [0.65], "cap": torch.linspace(0.004, 0.996, CAP, dtype=torch.float64).tolist(),
          "bf16_ulp": BF16_ULP}


def oracle_curve(pred, target, thresholds):
    """([(tp, fp, fn, tn)] per threshold, bad_pred, bad_target) on the CPU with torch's own semantics."""
    p, t = pred.detach().cpu().reshape(-1), target.detach().cpu().reshape(-1)
    ti = t.to(torch.int)
    tt = ti == 1
    pf = p.float() if p.dtype == torch.bfloat16 else p
    bad_p = int(((pf < 0) | (pf > 1)).sum())
    bad_t = int(((ti != 0) & (ti != 1)).sum())
    if t.dtype.is_floating_point:   # NaN / Inf truncate to whatever the CPU makes of them: bad either way
        bad_t = int((~torch.isfinite(t.float()) | ((ti != 0) & (ti != 1))).sum())
    n, ntgt = p.numel(), int(tt.sum())
    p_pos = p[tt]
    rows = []
    for tau in thresholds:
        npred = int(torch.count_nonzero(p >= tau))          # tau is rounded to p's dtype by the comparison
        tp = int(torch.count_nonzero(p_pos >= tau))
        rows.append((tp, npred - tp, ntgt - tp, n - npred - ntgt + tp))
    return rows, bad_p, bad_t


def rows_of(hist):
    """[(tp, fp, fn, tn)] per threshold from a histogram [2, T + 1] given as nested lists: positive = bin > k."""
    neg, pos = hist
    return [(sum(pos[k + 1:]), sum(neg[k + 1:]), sum(pos[:k + 1]), sum(neg[:k + 1])) for k in range(len(neg) - 1)]


def device_records(pred, target, thresholds, segments=1, poison_ws=False):
    """One sn_binary_curve call from a zeroed state: the records [segments, 2 * (T + 1) + 2] as nested lists."""
    T = len(thresholds)
    need = _hip.curve_ws_bytes(pred.numel() // segments, segments, T)
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=pred.device)
    if poison_ws:
        ws.fill_(-7)
    state = torch.zeros((segments, _hip.curve_record(T)), dtype=torch.int64, device=pred.device)
    batch = torch.full_like(state, -7)
    _hip.binary_curve(pred, target, thresholds, ws, state, segments=segments, batch=batch)
    assert torch.equal(state, batch)
    return batch.cpu().tolist()


def device_curve(pred, target, thresholds, **kw):
    (rec,) = device_records(pred, target, thresholds, **kw)
    T = len(thresholds)
    return rows_of([rec[:T + 1], rec[T + 1:2 * (T + 1)]]), rec[-2], rec[-1]


def _data(n, pdt, tdt, gen, thresholds):
    p = torch.rand(n, generator=gen, dtype=torch.float64)
    on = torch.rand(n, generator=gen) < 0.1                  # the thresholds themselves, as the dtype rounds them
    thr = torch.tensor(thresholds, dtype=torch.float64)
    p[on] = thr[torch.randint(0, len(thresholds), (n,), generator=gen)][on]
    p = p.to(pdt)
    if tdt == torch.bool:
        t = torch.rand(n, generator=gen) < 0.3
    elif tdt.is_floating_point:
        vals = torch.tensor([0.0, 1.0, 0.999, 1.7, 0.3, 1.0], dtype=torch.float64)
        t = vals[torch.randint(0, len(vals), (n,), generator=gen)].to(tdt)
    else:
        t = torch.randint(0, 2, (n,), generator=gen).to(tdt)
    return p, t


@pytest.mark.parametrize("sweep", list(SWEEPS))
@pytest.mark.parametrize("pdt", PRED_DT, ids=str)
@pytest.mark.parametrize("tdt", TGT_DT, ids=str)
def test_counts_match_the_cpu_oracle(hip_device, pdt, tdt, sweep):
    thr = SWEEPS[sweep]
    gen = torch.Generator().manual_seed(11)
    for n in SIZES:
        p, t = _data(n + 2, pdt, tdt, gen, thr)
        pd, td = p.to(hip_device), t.to(hip_device)
        for lo_p, lo_t in OFFSETS:
            want = oracle_curve(p[lo_p:lo_p + n], t[lo_t:lo_t + n], thr)
            got = device_curve(pd[lo_p:lo_p + n], td[lo_t:lo_t + n], thr)
            assert got == want, (n, lo_p, lo_t, sweep)
        if sweep == "bf16_ulp" and n >= 1003:
            rows = want[0]
            if pdt == torch.bfloat16:   # three thresholds round to one bf16 value: equal columns
                assert rows[1] == rows[2] == rows[3] and rows[0] != rows[1] != rows[4]
            else:
                assert len(set(rows)) == len(rows)


def _neighbours(x):
    """x rounded to its dtype, and its two neighbours one ulp away (x > 0)."""
    bits = {torch.float32: torch.int32, torch.bfloat16: torch.int16}[x.dtype]
    i = x.view(bits)
    return (i - 1).view(x.dtype), x, (i + 1).view(x.dtype)


def stats_counts(pred, target, tau):
    """sn_binary_stats, the kernel the curve's semantics are defined by: (tp, fp, fn, tn, bad_pred, bad_target)."""
    ws = torch.empty(_hip.SN_METRIC_WS_BYTES // 8, dtype=torch.int64, device=pred.device)
    state = torch.zeros(6, dtype=torch.int64, device=pred.device)
    _hip.binary_stats(pred, target, tau, 0.5, ws, state)
    return tuple(state.tolist())


def assert_columns_equal_single_threshold_kernel(pd, td, thr):
    rows, bad_p, bad_t = device_curve(pd, td, thr)
    for k, tau in enumerate(thr):
        assert rows[k] + (bad_p, bad_t) == stats_counts(pd, td, tau), (k, tau)
    return rows, bad_p, bad_t


@pytest.mark.parametrize("pdt", [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize("sweep", ["lin20", "bf16_ulp", "one"])
def test_boundary_triplets_against_the_single_threshold_kernel(hip_device, pdt, sweep):
    thr = SWEEPS[sweep]
    p = torch.cat([torch.cat(_neighbours(torch.tensor([tau], dtype=pdt))) for tau in thr])
    p = torch.cat([p, p])
    t = torch.cat([torch.ones(p.numel() // 2), torch.zeros(p.numel() // 2)]).to(torch.bool)
    rows, bad_p, bad_t = assert_columns_equal_single_threshold_kernel(p.to(hip_device), t.to(hip_device), thr)
    assert (rows, bad_p, bad_t) == oracle_curve(p, t, thr) and bad_p == bad_t == 0
    for k, tau in enumerate(thr):   # below / at / above threshold k itself: negative, positive, positive
        assert (p[3 * k:3 * k + 3] >= tau).tolist() == [False, True, True]


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64, torch.bfloat16], ids=str)
def test_target_edge_values_against_the_single_threshold_kernel(hip_device, tdt):
    vals = [0.999 if tdt != torch.bfloat16 else 0.99,   # (bf16 rounds 0.999 to 1.0)
            1.0, 1.7, -0.5, 0.0, 2.0, -1.0, float("nan"), float("inf"), float("-inf"), 5.5]
    t = torch.tensor(vals, dtype=tdt)
    p = torch.tensor([0.9, 0.7, 0.2, 0.6, 0.97, 0.55, 0.9, 0.1, 0.8, 0.52, float("nan")], dtype=torch.float32)
    pd, td = p.to(hip_device), t.to(hip_device)
    rows, bad_p, bad_t = assert_columns_equal_single_threshold_kernel(pd, td, LIN20)
    assert bad_t == 6 and bad_p == 0                    # bad: 2.0, -1.0, nan, inf, -inf, 5.5
    assert all(r[0] + r[2] == 2 for r in rows)          # positives: 1.0 and 1.7, at every threshold
    assert rows == oracle_curve(p, t, LIN20)[0]
    c = sna.BinarySegmentationCurve().to(hip_device)
    m = sna.init_metrics().to(hip_device)
    c.update(pd, td)
    m.update(pd, td)
    with pytest.raises(ValueError) as e_m:
        m.compute()
    with pytest.raises(ValueError) as e_c:
        c.compute()
    assert str(e_c.value) == str(e_m.value) and "target" in str(e_c.value)
    c.reset()
    c.update(torch.tensor([-0.1, 1.1, 0.5, float("nan")], device=hip_device),
             torch.ones(4, dtype=torch.bool, device=hip_device))
    with pytest.raises(ValueError, match=r"should be probabilities, but values were detected outside of \[0,1\] range"):
        c.compute()
    assert c.state[0, -2:].tolist() == [2, 0]           # NaN is no bad pred, and clears no threshold
    assert int(c.histogram()[1, 0]) == 2 and int(c.histogram()[1, 20]) == 1 and int(c.histogram()[1, 1]) == 1


def head_like(n, pdt, seed=11):
    """What the model's head gives on a real batch: relu(tanh(score)), 3 % towers, most predictions exactly 0."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.rand(n, generator=gen) < 0.03
    s = torch.where(t, 0.9 + 0.9 * torch.randn(n, generator=gen, dtype=torch.float64),
                    -0.6 + 0.8 * torch.randn(n, generator=gen, dtype=torch.float64))
    return torch.relu(torch.tanh(s)).to(pdt), t


@pytest.mark.parametrize("pdt", PRED_DT, ids=str)
def test_realistic_input_values_ap_and_best_threshold(hip_device, pdt):
    n = 2 ** 20 + 5
    p, t = head_like(n, pdt)
    assert 0.70 < float((p == 0).double().mean()) < 0.80
    thr = LIN20
    rows, bad_p, bad_t = oracle_curve(p, t, thr)
    assert all(tp > 0 and fp > 0 and fn > 0 for tp, fp, fn, _ in rows) and bad_p == bad_t == 0   # not degenerate
    c = sna.BinarySegmentationCurve(thresholds=thr, beta=0.5).to(hip_device)
    c.update(p.to(hip_device), t.to(hip_device))
    res = {k: v.cpu() for k, v in c.compute().items()}
    assert res["thresholds"].tolist() == thr
    for i, name in enumerate(("tp", "fp", "fn", "tn")):
        assert res[name].tolist() == [r[i] for r in rows], name
    for k, r in enumerate(rows):
        col = snm.binary_metric_values(*r, beta=0.5)
        for name in snm.METRIC_NAMES:
            assert float(res[name][k]) == col[name], (name, k)
    want_ap = snm.binned_average_precision([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    assert float(res["AveragePrecision"]) == want_ap and 0.0 < want_ap < 1.0
    f1 = [snm.binary_metric_values(*r)["F1Score"] for r in rows]
    k = snm.best_index(f1)
    assert c.best_threshold("F1Score") == (thr[k], f1[k])
    at = c.at(thr[k])
    assert (int(at["tp"]), int(at["fp"]), int(at["fn"]), int(at["tn"])) == rows[k]
    print(f"{pdt}: best F1 at k = {k} (tau = {thr[k]:.4f}): {f1[k]:.4f}; AP = {want_ap:.4f}")


@pytest.mark.parametrize("shape", [(5, 24, 24, 24), (5, 1003)], ids=["24cubed", "odd"])
@pytest.mark.parametrize("pdt,tdt", [(torch.float32, torch.bool), (torch.bfloat16, torch.float32),
                                     (torch.float64, torch.uint8)], ids=["f32-bool", "bf16-f32", "f64-u8"])
def test_per_tile_histograms(hip_device, shape, pdt, tdt):
    gen = torch.Generator().manual_seed(3)
    n = 1
    for s in shape:
        n *= s
    p, t = _data(n, pdt, tdt, gen, LIN20)
    pd, td = p.to(hip_device).reshape(shape), t.to(hip_device).reshape(shape)
    S, per = shape[0], n // shape[0]
    tiles = device_records(pd.reshape(-1), td.reshape(-1), LIN20, segments=S)
    whole = device_records(pd.reshape(-1), td.reshape(-1), LIN20)[0]
    for i in range(S):
        one = device_records(pd.reshape(S, per)[i], td.reshape(S, per)[i], LIN20)[0]
        assert tiles[i] == one, i
        want, bad_p, bad_t = oracle_curve(p.reshape(S, per)[i], t.reshape(S, per)[i], LIN20)
        assert rows_of([one[:21], one[21:42]]) == want and one[-2:] == [bad_p, bad_t]
    assert [sum(col) for col in zip(*tiles)] == whole
    c = sna.BinarySegmentationCurve(per_tile=True).to(hip_device)
    c.update(pd, td)
    c.update(pd, td)
    assert c.state.cpu().tolist() == [[2 * v for v in row] for row in tiles]
    res = c.compute()
    assert tuple(res["tp"].shape) == (S, 20) and tuple(res["AveragePrecision"].shape) == (S,)
    assert tuple(res["F1Score"].shape) == (S, 20) and res["thresholds"].dim() == 1
    taus, vals = c.best_threshold()
    assert tuple(taus.shape) == tuple(vals.shape) == (S,)
    with pytest.raises(ValueError, match="tiles"):
        c.update(pd[:3], td[:3])
    c.reset()
    assert tuple(c.state.shape) == (S, 44) and int(c.state.abs().sum()) == 0


def test_accumulation_reset_and_determinism(hip_device):
    gen = torch.Generator().manual_seed(5)
    parts = [_data(n, torch.float32, torch.bool, gen, LIN20) for n in (17, 100_003, 1 << 18)]
    c = sna.BinarySegmentationCurve().to(hip_device)
    for p, t in parts:
        c.update(p.to(hip_device), t.to(hip_device))
    allp, allt = torch.cat([p for p, _ in parts]), torch.cat([t for _, t in parts])
    rows, bad_p, bad_t = oracle_curve(allp, allt, LIN20)
    res = c.compute()
    assert [tuple(int(res[n][k]) for n in ("tp", "fp", "fn", "tn")) for k in range(20)] == rows
    assert rows_of(c.histogram().tolist()) == rows
    c.reset()
    assert c.state.cpu().tolist() == [[0] * 44]
    # the same update twice from a zeroed state: identical bytes; a poisoned workspace changes nothing
    pd, td = allp.to(hip_device), allt.to(hip_device)
    a = device_records(pd, td, LIN20)
    b = device_records(pd, td, LIN20)
    poisoned = device_records(pd, td, LIN20, poison_ws=True)
    assert a == b == poisoned and rows_of([a[0][:21], a[0][21:42]]) == rows
    tiles_a = device_records(pd[:5 * 70_000], td[:5 * 70_000], LIN20, segments=5)
    tiles_b = device_records(pd[:5 * 70_000], td[:5 * 70_000], LIN20, segments=5, poison_ws=True)
    assert tiles_a == tiles_b


def test_update_replays_from_a_captured_graph(hip_device):
    gen = torch.Generator().manual_seed(9)
    p, t = _data(300_001, torch.float32, torch.float32, gen, LIN20)
    pd, td = p.to(hip_device), t.to(hip_device)
    c = sna.BinarySegmentationCurve().to(hip_device)
    c.update(pd, td)   # warm-up outside the capture (it sizes the workspace)
    one = c.state.cpu().tolist()[0]
    assert rows_of([one[:21], one[21:42]]) == oracle_curve(p, t, LIN20)[0]
    c.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.update(pd, td)
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    assert c.state.cpu().tolist()[0] == [10 * v for v in one]


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


@pytest.mark.parametrize("per_tile", [False, True])
def test_captured_training_step_counts_each_replay(hip_device, per_tile):
    thr = torch.linspace(0.05, 0.95, 19).tolist()
    c = sna.BinarySegmentationCurve(thresholds=thr, per_tile=per_tile).to(hip_device)
    pipe, crit, opt, batch = _training_parts(hip_device)
    step = sna.CapturedTrainingStep(pipe, crit, opt, batch, warmup=2, metrics=c)
    assert int(c.state.abs().sum()) == 0          # warm-up and capture are not counted
    total = None
    losses = []
    for _ in range(6):
        losses.append(step.replay().item())
        rows, bad_p, bad_t = oracle_curve(step.pred, step.target, thr)
        assert bad_p == bad_t == 0
        total = rows if total is None else [tuple(a + b for a, b in zip(r, s)) for r, s in zip(total, rows)]
    res = c.compute()
    got = torch.stack([res[n] for n in ("tp", "fp", "fn", "tn")], -1).cpu()
    if per_tile:
        assert tuple(got.shape) == (step.pred.shape[0], 19, 4)
        got = got.sum(0)
    assert [tuple(r) for r in got.tolist()] == total
    assert all(sum(r) == 6 * step.pred.numel() for r in total)
    # the curve does not perturb training: the same trajectory without it
    pipe2, crit2, opt2, batch2 = _training_parts(hip_device)
    step2 = sna.CapturedTrainingStep(pipe2, crit2, opt2, batch2, warmup=2)
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
    flat = lambda res: {k: v.cpu().tolist() for k, v in res.items()}   # noqa: E731
    c = sna_w.BinarySegmentationCurve().to(dev)
    c.update(p[half[0]:half[1]].to(dev), t[half[0]:half[1]].to(dev))
    synced = flat(c.compute())
    local = sna_w.BinarySegmentationCurve(sync_on_compute=False).to(dev)
    local.update(p[half[0]:half[1]].to(dev), t[half[0]:half[1]].to(dev))
    whole = sna_w.BinarySegmentationCurve(sync_on_compute=False).to(dev)
    whole.update(p.to(dev), t.to(dev))
    q.put((rank, synced, flat(local.compute()), flat(whole.compute()), c.state.cpu().tolist()))
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
    assert s0 == s1 == w0 == w1          # the curve of the union, on both ranks
    assert l0 != l1                      # each rank counted a different half; compute() left the local state as it was
    assert st0 != st1
