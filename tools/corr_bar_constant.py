"""The constants A of tests/test_gpu_corr_plans.py's elementwise bar, measured on a CPU (no device, no library).

    |C - want|[t] <= A * sqrt(N_t) * 2^-24 * S_t

The backward correlation C[t] = sum delta[b,v] x[b, v+t-p] is emulated in fp32 the way the kernels are organised -- delta
formed in fp32 (gout * (1 - out * out) where out > 0, each operation rounded, as the kernels and torch's own tanh backward
form it), one fp32 accumulator per partial row (here: per (b, z) delta plane, its terms added in memory order), the rows
then added one after the other in fp32 -- and compared with the same sum in fp64, for every grid, kernel size and density
the test compares with its reference (tests/corr_plan_cases.py: bar_cases), on 8 seeds.  Printed: the largest ratio
|emu - ref| / (sqrt(N_t) 2^-24 S_t) over all taps and seeds, without and with the derivative.
    python tools/corr_bar_constant.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from corr_plan_cases import bar_cases  # noqa: E402

SEEDS = 8


def occupancy(rng, shape, density):
    if density == "layered":
        x = np.zeros(shape, dtype=bool)
        for z in (shape[1] // 3, shape[1] - 2):
            x[:, z] = rng.random((shape[0],) + shape[2:]) < 0.5
        return x
    return rng.random(shape) < density


def shifted(x, t, ks):
    """x[b, v + t - p], zero outside the grid"""
    out = np.zeros_like(x)
    src, dst = [slice(None)], [slice(None)]
    for n, k, tt in zip(x.shape[1:], ks, t):
        s = tt - (k - 1) // 2
        lo, hi = max(0, -s), min(n, n - s)
        if hi <= lo:
            return out
        dst.append(slice(lo, hi))
        src.append(slice(lo + s, hi + s))
    out[tuple(dst)] = x[tuple(src)]
    return out


def worst_ratio(shape, ks, density, seed, with_out):
    rng = np.random.default_rng(seed)
    x = occupancy(rng, shape, density).astype(np.float32)
    g = rng.standard_normal(shape).astype(np.float32)
    if with_out:
        o = np.maximum(np.tanh(rng.standard_normal(shape)), 0).astype(np.float32)
        d32 = np.where(o > 0, g * (np.float32(1) - o * o), np.float32(0)).astype(np.float32)
        d64 = np.where(o > 0, g.astype(np.float64) * (1 - o.astype(np.float64) ** 2), 0.0)
    else:
        d32, d64 = g, g.astype(np.float64)
    B, Z = shape[:2]
    worst = 0.0
    for t in np.ndindex(*ks):
        xs = shifted(x, t, ks)
        N = np.count_nonzero((xs != 0) & (d64 != 0))
        if N == 0:
            continue
        ref = (d64 * xs).sum()
        S = (np.abs(d64) * xs).sum()
        rows = np.cumsum((d32 * xs).reshape(B * Z, -1), axis=1, dtype=np.float32)[:, -1]   # sequential fp32, per row
        emu = np.cumsum(rows, dtype=np.float32)[-1]
        worst = max(worst, abs(float(emu) - ref) / (np.sqrt(N) * 2.0 ** -24 * S))
    return worst


if __name__ == "__main__":
    top = {False: 0.0, True: 0.0}
    for shape5, ks, densities in bar_cases():
        shape = (shape5[0],) + tuple(shape5[2:])
        for density in densities:
            w = {wo: max(worst_ratio(shape, ks, density, seed, wo) for seed in range(SEEDS)) for wo in (False, True)}
            print(f"{'x'.join(map(str, shape)):14s} {str(ks):12s} density {str(density):8s} plain {w[False]:7.3f}   "
                  f"derivative {w[True]:7.3f}", flush=True)
            for wo in w:
                top[wo] = max(top[wo], w[wo])
    print(f"largest: plain {top[False]:.3f}, derivative {top[True]:.3f};  "
          f"A = 4 x largest: plain {4 * top[False]:.3f}, derivative {4 * top[True]:.3f}")
