#!/usr/bin/env python3
"""K20 (csrc/quantile.hip), the weighted pinball loss of the quantile ensemble, at BASELINE C2 (B = 32, Q = 3, 64^3) and at
B = 4, 128^3; float32 predictions, bool and float32 targets.  Per case, all in the same run:

  * the forward pair of launches and the backward launch alone, and forward + backward together, each as a replayed
    hipGraph of `--reps` calls rotating over `--batches` distinct batches (no host time between the launches; the batches
    together exceed the 256 MB Infinity Cache), timed by events around the replays;
  * the yardstick: K5's sn_loss_forward (weighted-MSE term) and sn_loss_backward on a [B Q, n_per] problem of the same
    dtypes, measured the same way and scaled by the byte ratios (Q sp + sg) / (Q (sp + sg)) forward and
    (2 Q sp + sg) / (Q (2 sp + sg)) backward; the mark is 1.25 x the scaled yardstick -- INSIDE or OUTSIDE, gating nothing;
  * the reference's expression in torch ops on the device, per sample (weights by the argmin binning, the Q pinball terms,
    cat, sum, mean; autograd backward), eager between events.

The bench checks what it times: the kernel's loss against the torch expression on the last batch.
    python tools/quantile_loss_bench.py --out profiles/quantile_loss_bench.json"""
import argparse
import gc
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scene_net_amd as sna  # noqa: E402
from scene_net_amd import _hip  # noqa: E402

HBM_COPY_TBPS = 6.29   # measured device-to-device copy rate of the MI355X (MI355X_MICROARCH.md)
QS = [0.1, 0.5, 0.9]
MARGIN = 1.25
FREQS = [3_000_000, 1200, 800, 700, 650, 400, 300, 310, 150, 9000]


def timed(fn, iters, spin_ms=150.0):
    """ms per call by events over `iters` calls, after ~150 ms of the same work (clocks settle) and a synchronise."""
    gc.collect()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < spin_ms:
        fn()
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def graphed(calls, reps, iters):
    """ms per call of `calls[k % len(calls)]()` captured `reps` times into one graph and replayed."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for c in calls:
            c()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    keep = []
    with torch.cuda.graph(g):
        for k in range(reps):
            keep.append(calls[k % len(calls)]())
    ms = timed(g.replay, iters) / reps
    del g, keep
    return ms


def make_batches(B, Q, n, gdt, nbatch, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    out = []
    for _ in range(nbatch):
        u = torch.rand((B, n), generator=gen, device=dev)
        if gdt == torch.bool:
            gt = u < 0.05
        else:   # reg_on_voxel-like: mostly 0, some 1, some ratios
            gt = torch.where(u < 0.9, torch.zeros_like(u), torch.where(u < 0.95, torch.ones_like(u), (u - 0.95) * 20))
        # relu(tanh(.))-like predictions: exactly 0 on most empty voxels (ties), in (0, 1) elsewhere
        pred = torch.rand((B, Q, n), generator=gen, device=dev)
        pred = torch.where(torch.rand((B, Q, n), generator=gen, device=dev) < 0.6, torch.zeros_like(pred), pred)
        out.append((pred.contiguous(), gt.contiguous()))
    return out


def case(name, B, side_len, gdt, dev, args):
    Q, n = len(QS), side_len ** 3
    sp, sg = 4, (1 if gdt == torch.bool else 4)
    batches = make_batches(B, Q, n, gdt, args.batches, dev)
    crit = sna.QuantileLoss(targets=torch.zeros(4), qs=torch.tensor(QS), hist_path=None, alpha=1.5, epsilon=0.05,
                            save_weighting_scheme=False)
    crit.freqs = torch.as_tensor(FREQS).to(dev)
    ranges, bin_w = crit._device_tables(dev)
    qs = crit._qs_host
    up = torch.ones(1, dtype=torch.float32, device=dev)
    coefs = [_hip.quantile_forward(p, t, qs, ranges, bin_w)[3] for p, t in batches]

    fwd = graphed([lambda p=p, t=t: _hip.quantile_forward(p, t, qs, ranges, bin_w) for p, t in batches], args.reps, args.iters)
    bwd = graphed([lambda p=p, t=t, c=c: _hip.quantile_backward(p, t, qs, ranges, c, up)
                   for (p, t), c in zip(batches, coefs)], args.reps, args.iters)

    def both(p, t):
        loss, _, _, c = _hip.quantile_forward(p, t, qs, ranges, bin_w)
        return loss, _hip.quantile_backward(p, t, qs, ranges, c, up)
    fb = graphed([lambda p=p, t=t: both(p, t) for p, t in batches], args.reps, args.iters)

    # the yardstick: K5 on [B Q, n] of the same dtypes
    yb = [(p.reshape(B * Q, n), t.unsqueeze(1).expand(B, Q, n).reshape(B * Q, n).contiguous()) for p, t in batches]
    ycoef = [_hip.loss_forward(p, t, ranges, bin_w, _hip.SN_LOSS_WMSE)[2] for p, t in yb]
    up64 = torch.ones(1, dtype=torch.float64, device=dev)
    yf = graphed([lambda p=p, t=t: _hip.loss_forward(p, t, ranges, bin_w, _hip.SN_LOSS_WMSE) for p, t in yb], args.reps,
                 args.iters)
    ybw = graphed([lambda p=p, t=t, c=c: _hip.loss_backward(p, t, ranges, c, up64) for (p, t), c in zip(yb, ycoef)],
                  args.reps, args.iters)
    del yb, ycoef
    torch.cuda.empty_cache()
    rf = (Q * sp + sg) / (Q * (sp + sg))
    rb = (2 * Q * sp + sg) / (Q * (2 * sp + sg))

    # the reference's expression in torch ops, per sample
    def torch_expr(p, t):
        tf = t if t.dtype.is_floating_point else t.to(p.dtype)
        w = crit.get_weight_target(tf)
        return torch.mean(w * crit.quantile_loss(p, tf))

    def torch_step(p, t):
        pr = p.detach().requires_grad_(True)
        torch_expr(pr, t).backward()
        return pr.grad
    it_t = max(5, args.iters // 10)
    with torch.no_grad():
        t_fwd = timed(lambda: torch_expr(*batches[0]), it_t)
    t_fb = timed(lambda: torch_step(*batches[0]), it_t)

    # the bench checks what it times
    p, t = batches[-1]
    mine = _hip.quantile_forward(p, t, qs, ranges, bin_w)[0][0].item()
    with torch.no_grad():
        want = torch_expr(p, t).item()
    assert abs(mine - want) <= 1e-4 * abs(want), (mine, want)
    g_mine = _hip.quantile_backward(p, t, qs, ranges, coefs[-1], up)
    g_want = torch_step(p, t)
    gerr = ((g_mine - g_want).abs().max() / g_want.abs().max()).item()
    assert gerr <= 1e-4, gerr

    bytes_f = B * n * (Q * sp + sg)
    bytes_b = B * n * (2 * Q * sp + sg)
    us = lambda ms: round(ms * 1e3, 2)   # noqa: E731
    tbps = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / 1e12, 3)   # noqa: E731
    verdict = lambda ms, mark: "INSIDE" if ms <= mark else "OUTSIDE"   # noqa: E731
    mark_f, mark_b = MARGIN * yf * rf, MARGIN * ybw * rb
    res = {"case": name, "B": B, "Q": Q, "n_per": n, "pred": "float32", "gt": str(gdt).replace("torch.", ""),
           "rotating_batches": len(batches), "rotating_bytes_forward": bytes_f * len(batches),
           "forward": {"us": us(fwd), "bytes": bytes_f, "tb_per_s": tbps(bytes_f, fwd),
                       "bytes_floor_us": round(bytes_f / (HBM_COPY_TBPS * 1e12) * 1e6, 2),
                       "yardstick_us": us(yf), "byte_ratio": round(rf, 4), "yardstick_scaled_us": us(yf * rf),
                       "mark_us": us(mark_f), "verdict": verdict(fwd, mark_f)},
           "backward": {"us": us(bwd), "bytes": bytes_b, "tb_per_s": tbps(bytes_b, bwd),
                        "bytes_floor_us": round(bytes_b / (HBM_COPY_TBPS * 1e12) * 1e6, 2),
                        "yardstick_us": us(ybw), "byte_ratio": round(rb, 4), "yardstick_scaled_us": us(ybw * rb),
                        "mark_us": us(mark_b), "verdict": verdict(bwd, mark_b)},
           "forward_backward_graph_us": us(fb),
           "torch_expression": {"forward_us": us(t_fwd), "forward_backward_us": us(t_fb),
                                "speedup_forward": round(t_fwd / fwd, 1), "speedup_forward_backward": round(t_fb / fb, 1)},
           "checked": {"loss": mine, "torch_loss": want, "grad_rel_err": gerr}}
    print(f"{name:34s} fwd {res['forward']['us']:8.2f} us ({res['forward']['tb_per_s']} TB/s; mark "
          f"{res['forward']['mark_us']} us: {res['forward']['verdict']})  bwd {res['backward']['us']:8.2f} us "
          f"({res['backward']['tb_per_s']} TB/s; mark {res['backward']['mark_us']} us: {res['backward']['verdict']})  "
          f"fwd+bwd {res['forward_backward_graph_us']} us; torch ops {res['torch_expression']['forward_backward_us']} us")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="quantile_loss_bench.json")
    ap.add_argument("--iters", type=int, default=300, help="timed graph replays per measurement")
    ap.add_argument("--reps", type=int, default=12, help="calls captured in one graph")
    ap.add_argument("--batches", type=int, default=3, help="distinct batches the calls rotate over")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("quantile_loss_bench needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "hbm_copy_tbps": HBM_COPY_TBPS, "margin": MARGIN, "qs": QS,
           "reps_per_graph": args.reps, "replays": args.iters, "cases": []}
    for name, B, side_len, gdt in (("C2 32 x 3 x 64^3, f32 / bool", 32, 64, torch.bool),
                                   ("C2 32 x 3 x 64^3, f32 / f32", 32, 64, torch.float32),
                                   ("4 x 3 x 128^3, f32 / bool", 4, 128, torch.bool),
                                   ("4 x 3 x 128^3, f32 / f32", 4, 128, torch.float32)):
        torch.cuda.empty_cache()
        res["cases"].append(case(name, B, side_len, gdt, dev, args))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
