#!/usr/bin/env python3
"""K6 training metrics at BASELINE C2 (32 x 64^3 = 8.4 M voxels per batch): sn_binary_stats (BinarySegmentationMetrics
.update, two launches) timed by HIP events, hot (one batch, Infinity-Cache resident) and rotating over >= 7 distinct
batches (> 256 MB in all: HBM), beside the torch composite it replaces; then CapturedTrainingStep ms/step with and
without `metrics`.  Writes one JSON file.   python tools/metrics_bench.py --out metrics_bench.json [--iters 200]
--curve adds the threshold sweep (sn_binary_curve, BinarySegmentationCurve.update) at T = 1, 20, 100, 255 on uniform
and on head-like predictions, each beside (a) one sn_binary_stats update and (b) T of them on the same batches, and the
captured training step with the curve as `metrics`."""
import argparse
import gc
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scene_net_amd as sna  # noqa: E402
from scene_net_amd.synthetic import apply_bank_spec, synthetic_bank_spec, synthetic_tile  # noqa: E402

HBM_COPY_TBPS = 6.29   # measured device-to-device copy rate of the MI355X (MI355X_MICROARCH.md)
C2 = 32 * 64 ** 3
TAU = 0.65


def timed(fn, iters, spin_ms=150.0):
    """ms per call by events over `iters` calls, after ~150 ms of the same work (clocks settle) and a synchronise."""
    gc.collect()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < spin_ms:
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def rotating(fn, batches):
    it = [0]

    def call():
        p, t = batches[it[0] % len(batches)]
        it[0] += 1
        fn(p, t)
    return call


def torch_composite(pred, target):
    """What the reference's loop costs without the kernel: flatten, .to(int), >=, the logical ops and four sums."""
    pp = torch.flatten(pred) >= TAU
    tt = torch.flatten(target).to(torch.int) == 1
    return ((pp & tt).sum(), (pp & ~tt).sum(), (~pp & tt).sum(), (~pp & ~tt).sum())


def update_case(name, pdt, tdt, dev, iters, nbatch):
    gen = torch.Generator(device=dev).manual_seed(1)
    batches = []
    for _ in range(nbatch):
        p = torch.rand(C2, generator=gen, device=dev).to(pdt)
        t = torch.rand(C2, generator=gen, device=dev) < 0.05
        batches.append((p, t.to(tdt)))
    nbytes = C2 * (batches[0][0].element_size() + batches[0][1].element_size())
    m = sna.init_metrics().to(dev)
    hot = timed(lambda: m.update(*batches[0]), iters)
    rot = timed(rotating(m.update, batches), iters)
    comp_hot = timed(lambda: torch_composite(*batches[0]), max(10, iters // 10))
    comp_rot = timed(rotating(torch_composite, batches), max(10, iters // 10))
    # the counts of the last batch against the composite (the bench also checks what it times)
    ref = sna.init_metrics().to(dev)
    ref.update(*batches[-1])
    want = [int(v) for v in torch_composite(*batches[-1])]
    assert ref.state.tolist()[:4] == want, (ref.state.tolist(), want)
    us = lambda ms: round(ms * 1e3, 2)   # noqa: E731
    frac = lambda ms: round(nbytes / (ms * 1e-3) / (HBM_COPY_TBPS * 1e12), 3)   # noqa: E731
    return {"case": name, "n": C2, "pred": str(pdt), "target": str(tdt), "bytes_per_update": nbytes,
            "rotating_batches": nbatch, "rotating_bytes": nbytes * nbatch,
            "update_us_hot": us(hot), "update_us_rotating": us(rot),
            "hbm_fraction_hot": frac(hot), "hbm_fraction_rotating": frac(rot),
            "bytes_floor_us": round(nbytes / (HBM_COPY_TBPS * 1e12) * 1e6, 2),
            "torch_composite_us_hot": us(comp_hot), "torch_composite_us_rotating": us(comp_rot),
            "speedup_rotating": round(comp_rot / rot, 1)}


def head_like(gen, dev):
    """relu(tanh(score)) of a 3 % tower batch: ~75 % of the predictions are exactly 0 (the input of the GPU tests)."""
    t = torch.rand(C2, generator=gen, device=dev) < 0.03
    z = torch.randn(C2, generator=gen, device=dev, dtype=torch.float64)
    s = torch.where(t, 0.9 + 0.9 * z, -0.6 + 0.8 * z)
    return torch.relu(torch.tanh(s)), t


def curve_thresholds(T):
    return [0.65] if T == 1 else torch.linspace(0.5, 0.95, T, dtype=torch.float64).tolist()


def curve_case(name, pdt, tdt, kind, dev, iters, nbatch, sweeps=(1, 20, 100, 255)):
    gen = torch.Generator(device=dev).manual_seed(1)
    batches = []
    for _ in range(nbatch):
        if kind == "uniform":
            p = torch.rand(C2, generator=gen, device=dev)
            t = torch.rand(C2, generator=gen, device=dev) < 0.05
        else:
            p, t = head_like(gen, dev)
        batches.append((p.to(pdt), t.to(tdt)))
    nbytes = C2 * (batches[0][0].element_size() + batches[0][1].element_size())
    us = lambda ms: round(ms * 1e3, 2)   # noqa: E731
    frac = lambda ms: round(nbytes / (ms * 1e-3) / (HBM_COPY_TBPS * 1e12), 3)   # noqa: E731
    m = sna.init_metrics().to(dev)
    one_hot = timed(lambda: m.update(*batches[0]), iters)
    one_rot = timed(rotating(m.update, batches), iters)
    out = {"case": name, "input": kind, "n": C2, "pred": str(pdt), "target": str(tdt), "bytes_per_update": nbytes,
           "zero_fraction": round(float((batches[0][0] == 0).float().mean()), 4),
           "rotating_batches": nbatch, "rotating_bytes": nbytes * nbatch,
           "bytes_floor_us": round(nbytes / (HBM_COPY_TBPS * 1e12) * 1e6, 2),
           "stats_update_us_hot": us(one_hot), "stats_update_us_rotating": us(one_rot), "sweeps": []}
    for T in sweeps:
        thr = curve_thresholds(T)
        curve = sna.BinarySegmentationCurve(thresholds=thr).to(dev)
        hot = timed(lambda: curve.update(*batches[0]), iters)
        rot = timed(rotating(curve.update, batches), iters)
        singles = [sna.BinarySegmentationMetrics(tau=tau).to(dev) for tau in thr]

        def sweep(p, t):
            for s in singles:
                s.update(p, t)
        it_b = max(3, iters // T)
        b_hot = timed(lambda: sweep(*batches[0]), it_b)
        b_rot = timed(rotating(sweep, batches), it_b)
        # the bench checks what it times: every column of the curve against the single-threshold kernel
        curve.reset()
        curve.update(*batches[-1])
        res = curve.compute()
        for k, s in enumerate(singles):
            s.reset()
            s.update(*batches[-1])
            want = s.state.tolist()[:4]
            got = [int(res[n][k]) for n in ("tp", "fp", "fn", "tn")]
            assert got == want, (T, k, got, want)
        out["sweeps"].append({"T": T, "curve_us_hot": us(hot), "curve_us_rotating": us(rot),
                              "hbm_fraction_hot": frac(hot), "hbm_fraction_rotating": frac(rot),
                              "ratio_to_one_stats_update_hot": round(hot / one_hot, 2),
                              "ratio_to_one_stats_update_rotating": round(rot / one_rot, 2),
                              "T_stats_updates_us_hot": us(b_hot), "T_stats_updates_us_rotating": us(b_rot),
                              "speedup_over_T_updates_hot": round(b_hot / hot, 1),
                              "speedup_over_T_updates_rotating": round(b_rot / rot, 1)})
        del singles, curve
    return out


def training_step(dev, iters, with_metrics):
    geneo_num = {"cy": 6, "cone": 5, "neg": 5}
    specs, names, lambdas, last = synthetic_bank_spec(geneo_num)
    torch.manual_seed(0)
    model = sna.SceneNet(geneo_num, (9, 9, 9))
    apply_bank_spec(model, specs, names, lambdas, last)
    model = model.to(dev)
    tiles, labels = zip(*[synthetic_tile(i, 100_000) for i in range(32)])
    batch = sna.PointBatch.from_tiles(tiles, labels, device=dev)
    pipe = sna.ScenePipeline(model, (64, 64, 64), keep_labels=[15.0])
    gt = pipe.voxelize(batch, want_gt=True).gt_occ
    crit = sna.GENEO_Tversky_Loss(targets=gt.float().cpu(), weighting_scheme_path=None, save_weighting_scheme=False)
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    if with_metrics == "curve":
        m = sna.BinarySegmentationCurve().to(dev)
    else:
        m = sna.init_metrics().to(dev) if with_metrics else None
    step = sna.CapturedTrainingStep(pipe, crit, opt, batch, warmup=3, metrics=m)
    ms = timed(step.replay, iters)
    out = {"ms_per_step": round(ms, 4)}
    if with_metrics == "curve":
        res = m.compute()
        out["counted_elements"] = int(res["tp"][0] + res["fp"][0] + res["fn"][0] + res["tn"][0])
        out["average_precision"] = float(res["AveragePrecision"])
        out["best_f1_threshold"] = list(m.best_threshold("F1Score"))
    elif m is not None:
        c = m.state_counts()
        out["counted_elements"] = c["tp"] + c["fp"] + c["fn"] + c["tn"]
        out["values"] = {k: float(v) for k, v in m.compute().items()}
    del step
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="metrics_bench.json")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batches", type=int, default=8, help="distinct batches of the rotating timing (>= 7: > 256 MB)")
    ap.add_argument("--no-train", action="store_true", help="skip the CapturedTrainingStep comparison")
    ap.add_argument("--curve", action="store_true", help="add the threshold sweep (sn_binary_curve) to the measurements")
    ap.add_argument("--skip-base", action="store_true", help="with --curve: leave the single-threshold section out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("metrics_bench needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "hbm_copy_tbps": HBM_COPY_TBPS, "updates": []}
    if not (args.curve and args.skip_base):
        res["updates"].append(update_case("f32 pred + bool target", torch.float32, torch.bool, dev, args.iters,
                                          args.batches))
        res["updates"].append(update_case("bf16 pred + f32 target", torch.bfloat16, torch.float32, dev, args.iters,
                                          args.batches))
    for u in res["updates"]:
        print(f"{u['case']:26s} hot {u['update_us_hot']:7.2f} us  rotating {u['update_us_rotating']:7.2f} us "
              f"({u['hbm_fraction_rotating']:.2f} of {HBM_COPY_TBPS} TB/s; floor {u['bytes_floor_us']} us)   "
              f"torch composite {u['torch_composite_us_rotating']:8.2f} us")
    if args.curve:
        res["curve"] = []
        for kind in ("uniform", "head-like"):
            for name, pdt, tdt in (("f32 pred + bool target", torch.float32, torch.bool),
                                   ("bf16 pred + f32 target", torch.bfloat16, torch.float32)):
                torch.cuda.empty_cache()
                c = curve_case(name, pdt, tdt, kind, dev, args.iters, args.batches)
                res["curve"].append(c)
                print(f"curve, {kind:9s} {name:24s} one stats update {c['stats_update_us_rotating']:7.2f} us rotating")
                for w in c["sweeps"]:
                    print(f"    T = {w['T']:3d}: hot {w['curve_us_hot']:7.2f} us  rotating {w['curve_us_rotating']:7.2f} us "
                          f"({w['hbm_fraction_rotating']:.2f} of {HBM_COPY_TBPS} TB/s, "
                          f"{w['ratio_to_one_stats_update_rotating']:.2f} x one stats update); T stats updates "
                          f"{w['T_stats_updates_us_rotating']:9.2f} us ({w['speedup_over_T_updates_rotating']:.1f} x)")
    torch.cuda.empty_cache()
    if args.curve and not args.no_train:
        plain, curv = [], []
        for _ in range(2):
            plain.append(training_step(dev, max(50, args.iters // 2), False))
            curv.append(training_step(dev, max(50, args.iters // 2), "curve"))
        res["training_step_curve"] = {"without_metrics_ms": [r["ms_per_step"] for r in plain],
                                      "with_curve_ms": [r["ms_per_step"] for r in curv],
                                      "overhead_us": round((min(r["ms_per_step"] for r in curv)
                                                            - min(r["ms_per_step"] for r in plain)) * 1e3, 2),
                                      "thresholds": 20, "counted_elements": curv[-1]["counted_elements"],
                                      "average_precision": curv[-1]["average_precision"],
                                      "best_f1_threshold": curv[-1]["best_f1_threshold"]}
        print(f"captured training step: {res['training_step_curve']['without_metrics_ms']} ms without metrics, "
              f"{res['training_step_curve']['with_curve_ms']} ms with the curve "
              f"(overhead {res['training_step_curve']['overhead_us']} us)")
    if not args.no_train and not (args.curve and args.skip_base):
        # alternate the two builds so that drift of the shared host does not favour either
        plain, metr = [], []
        for _ in range(2):
            plain.append(training_step(dev, max(50, args.iters // 2), False))
            metr.append(training_step(dev, max(50, args.iters // 2), True))
        res["training_step"] = {"without_metrics_ms": [r["ms_per_step"] for r in plain],
                                "with_metrics_ms": [r["ms_per_step"] for r in metr],
                                "overhead_us": round((min(r["ms_per_step"] for r in metr)
                                                      - min(r["ms_per_step"] for r in plain)) * 1e3, 2),
                                "counted_elements": metr[-1]["counted_elements"], "values": metr[-1]["values"]}
        print(f"captured training step: {res['training_step']['without_metrics_ms']} ms without metrics, "
              f"{res['training_step']['with_metrics_ms']} ms with (overhead {res['training_step']['overhead_us']} us)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
