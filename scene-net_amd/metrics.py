"""Training metrics of the reference's loop on the device: JaccardIndex, Precision, Recall, F1Score and FBetaScore of a
binary prediction at threshold tau, as the MetricCollection of `init_metrics(tau=0.65)` (utils/scripts_utils.py:80-91)
that LitSceneNet.{training,validation,test}_step call on every batch and that scripts/main.py monitors for its
checkpoints and early stopping.

Every update is ONE call of sn_binary_stats (csrc/metrics.hip, two launches): it counts the batch's (tp, fp, fn, tn) and
adds them to a device-resident state of int64 counters.  Nothing synchronises until compute(), so an update can sit
inside a captured training step (CapturedTrainingStep(metrics=...)).

Semantics -- our reading of torchmetrics 0.9.0 (the version of the reference's requirements.txt).  torchmetrics is not a
dependency of this package and was not available to check against, so the reading is unpinned:
  - predicted positive: `pred >= tau` in pred's own dtype, tau rounded to it the way torch rounds a Python scalar
    (fp32: 0.65 -> 0.64999998, so an fp32 0.65 is positive; bf16: 0.65 -> 0.6484375; fp64 exact); NaN is negative;
  - target positive: `int(target) == 1` under C truncation, as `.to(torch.int)` does (0.999 -> 0, 1.7 -> 1); a target
    whose truncation is neither 0 nor 1 (>= 2, <= -1, NaN, +-Inf, bytes > 1) is a bad target;
  - a pred outside [0, 1] is a bad pred (torchmetrics 0.9 refuses non-probabilities);
  - state: tp, fp, fn, tn summed over every update since reset() (micro sums, as torchmetrics' metric states);
  - values in fp64 from the counts, returned as fp32, 0/0 -> 0 (torchmetrics' zero_division / absent_score default):
    P = tp/(tp+fp), R = tp/(tp+fn), F1 = 2PR/(P+R), Fbeta = (1+b^2)PR/(b^2 P+R),
    JaccardIndex = (tp/(tp+fp+fn) + tn/(tn+fp+fn)) / 2 -- the macro mean over both classes (num_classes=2 counts the
    background too).
Unlike torchmetrics, a bad pred or target does not raise in update(): the kernel counts them and compute() raises
ValueError (an update must not synchronise).  There is no CPU path: CPU tensors raise HipLibraryError.

BinarySegmentationCurve (below) is the same collection at T thresholds from ONE pass (sn_binary_curve): the
precision-recall curve, the binned average precision and the best threshold.
"""
from __future__ import annotations

import ctypes
import warnings
from typing import Dict, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _hip
from ._hip import HipLibraryError

METRIC_NAMES = ("JaccardIndex", "Precision", "Recall", "F1Score", "FBetaScore")
_COUNT_NAMES = ("tp", "fp", "fn", "tn", "bad_pred", "bad_target")
PRED_RANGE_ERROR = "The `preds` should be probabilities, but values were detected outside of [0,1] range."
TARGET_RANGE_ERROR = ("The `target` should hold binary labels (0 or 1 after truncation to int), but other values were "
                      "detected.")


def _ratio(a: float, b: float) -> float:
    return 0.0 if b == 0.0 else a / b


def f_beta(precision: float, recall: float, beta: float) -> float:
    """(1 + beta^2) P R / (beta^2 P + R) in fp64, 0/0 -> 0 (beta = 1: F1Score)."""
    b2 = beta * beta
    return _ratio((1.0 + b2) * precision * recall, b2 * precision + recall)


def binary_metric_values(tp: int, fp: int, fn: int, tn: int, beta: float = 0.5) -> Dict[str, float]:
    """The five values from the confusion counts: fp64, 0/0 -> 0, each rounded once to fp32.  The same operations in
    the same order as the combine kernel of csrc/metrics.hip, so the device's values equal these bit for bit."""
    tp, fp, fn, tn = float(tp), float(fp), float(fn), float(tn)
    P = _ratio(tp, tp + fp)
    R = _ratio(tp, tp + fn)
    F1 = _ratio(2.0 * P * R, P + R)
    FB = f_beta(P, R, beta)
    J = 0.5 * (_ratio(tp, tp + fp + fn) + _ratio(tn, tn + fp + fn))
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))   # noqa: E731
    return dict(zip(METRIC_NAMES, (f32(J), f32(P), f32(R), f32(F1), f32(FB))))


class BinarySegmentationMetrics(nn.Module):
    """The reference's MetricCollection([JaccardIndex(num_classes=2, threshold=tau), Precision(threshold=tau),
    Recall(threshold=tau), F1Score(threshold=tau), FBetaScore(beta=beta, threshold=tau)]) on the device.

    m(pred, target) updates the state and returns this batch's values {name: 0-d fp32 device tensor};
    m.update(pred, target) only updates; m.compute() gives the accumulated values (one synchronisation; all-reduced over
    `process_group` first when it has more than one rank and sync_on_compute is set); m.reset() zeroes the state.
    Keys, iteration and items() follow the reference's order (scripts/main.py names its checkpoints after them).
    The state moves with .to(device) and adds no state-dict keys."""

    def __init__(self, tau: float = 0.65, beta: float = 0.5, sync_on_compute: bool = True, process_group=None):
        super().__init__()
        if not 0.0 < float(tau) < 1.0:
            raise ValueError(f"tau must lie in (0, 1) (got {tau})")
        if not float(beta) > 0.0:
            raise ValueError(f"beta must be positive (got {beta})")
        self.tau, self.beta = float(tau), float(beta)
        self.sync_on_compute, self.process_group = bool(sync_on_compute), process_group
        self.register_buffer("state", torch.zeros(_hip.SN_METRIC_NCOUNT, dtype=torch.int64), persistent=False)
        self.register_buffer("_ws", torch.zeros(_hip.SN_METRIC_WS_BYTES // 8, dtype=torch.int64), persistent=False)

    # -- the MetricCollection's mapping face
    def keys(self):
        return list(METRIC_NAMES)

    def __iter__(self):
        return iter(METRIC_NAMES)

    def __len__(self):
        return len(METRIC_NAMES)

    def items(self):
        return [(n, _MetricView(self, n)) for n in METRIC_NAMES]

    def values(self):
        return [_MetricView(self, n) for n in METRIC_NAMES]

    def __getitem__(self, name: str) -> "_MetricView":
        if name not in METRIC_NAMES:
            raise KeyError(name)
        return _MetricView(self, name)

    def _launch(self, pred: torch.Tensor, target: torch.Tensor, values: Optional[torch.Tensor]) -> None:
        if pred.numel() != target.numel():
            raise ValueError(f"pred ({pred.numel()} elements) and target ({target.numel()} elements) must have the same "
                             "number of elements")
        if pred.is_cuda and self.state.device != pred.device:
            raise HipLibraryError(f"the metric state lives on {self.state.device}: move the module with "
                                  f".to({pred.device}) first")
        _hip.binary_stats(pred.reshape(-1), target.reshape(-1), self.tau, self.beta, self._ws, self.state,
                          values=values)

    @torch.no_grad()
    def update(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        self._launch(pred, target, None)

    @torch.no_grad()
    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> Dict[str, torch.Tensor]:
        values = torch.empty(2 * _hip.SN_METRIC_NVALUE, dtype=torch.float32, device=pred.device)
        self._launch(pred, target, values)
        return {n: values[i] for i, n in enumerate(METRIC_NAMES)}

    def state_counts(self) -> Dict[str, int]:
        """The accumulated counters of THIS process (tp, fp, fn, tn, bad_pred, bad_target); synchronises."""
        return dict(zip(_COUNT_NAMES, (int(v) for v in self.state.tolist())))

    def _synced_counts(self) -> torch.Tensor:
        counts = self.state.clone()
        if self.sync_on_compute:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.process_group) > 1:
                dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=self.process_group)
        return counts

    def compute(self) -> Dict[str, torch.Tensor]:
        tp, fp, fn, tn, bad_pred, bad_target = (int(v) for v in self._synced_counts().tolist())
        if bad_pred:
            raise ValueError(PRED_RANGE_ERROR)
        if bad_target:
            raise ValueError(TARGET_RANGE_ERROR)
        dev = self.state.device
        if tp + fp + fn + tn == 0:
            warnings.warn("BinarySegmentationMetrics.compute() was called before any update(); returning zeros",
                          UserWarning)
            return {n: torch.zeros((), dtype=torch.float32, device=dev) for n in METRIC_NAMES}
        vals = binary_metric_values(tp, fp, fn, tn, self.beta)
        out = torch.tensor([vals[n] for n in METRIC_NAMES], dtype=torch.float32, device=dev)
        return {n: out[i] for i, n in enumerate(METRIC_NAMES)}

    @torch.no_grad()
    def reset(self) -> None:
        self.state.zero_()

    def extra_repr(self) -> str:
        return f"tau={self.tau}, beta={self.beta}, metrics={list(METRIC_NAMES)}"


class _MetricView:
    """One entry of the collection (what MetricCollection.items() pairs with a name): compute() gives its value."""

    def __init__(self, owner: BinarySegmentationMetrics, name: str):
        self.owner, self.name = owner, name

    def compute(self) -> torch.Tensor:
        return self.owner.compute()[self.name]

    def __repr__(self) -> str:
        return f"{self.name}(threshold={self.owner.tau})"


def init_metrics(tau: float = 0.65) -> BinarySegmentationMetrics:
    """utils/scripts_utils.py:init_metrics: the drop-in `metric_initializer` of LitSceneNet."""
    return BinarySegmentationMetrics(tau=tau, beta=0.5)


# --------------------------------------------------------------------------- #
# The threshold sweep: the counts of T thresholds from one pass (sn_binary_curve).
CURVE_COUNT_NAMES = ("tp", "fp", "fn", "tn")


def _check_thresholds(thresholds) -> Tuple[float, ...]:
    """The C entry's own rules: 1 <= T <= SN_CURVE_MAX_THRESHOLDS, strictly increasing, inside (0, 1)."""
    thr = tuple(float(v) for v in (thresholds.tolist() if isinstance(thresholds, torch.Tensor) else thresholds))
    if not 1 <= len(thr) <= _hip.SN_CURVE_MAX_THRESHOLDS:
        raise ValueError(f"between 1 and {_hip.SN_CURVE_MAX_THRESHOLDS} thresholds are served (got {len(thr)})")
    for k, v in enumerate(thr):
        if not 0.0 < v < 1.0:
            raise ValueError(f"thresholds must lie in (0, 1) (entry {k} is {v})")
        if k and not v > thr[k - 1]:
            raise ValueError(f"thresholds must be strictly increasing (entry {k}: {v} after {thr[k - 1]})")
    return thr


def curve_counts(hist: torch.Tensor) -> Dict[str, torch.Tensor]:
    """hist [..., 2, T + 1] int64 (bin = number of thresholds a prediction clears; target negative, then positive) ->
    {"tp", "fp", "fn", "tn"} int64 [..., T]: at threshold k the predicted positives are the bins above k."""
    hist = hist.to(torch.int64)
    above = hist.flip(-1).cumsum(-1).flip(-1)[..., 1:]      # [..., 2, T]: sum over bins b > k
    total = hist.sum(-1, keepdim=True)
    fp, tp = above[..., 0, :], above[..., 1, :]
    return {"tp": tp, "fp": fp, "fn": total[..., 1, :] - tp, "tn": total[..., 0, :] - fp}


def curve_values(tp, fp, fn, tn, beta: float = 0.5) -> Dict[str, torch.Tensor]:
    """The five values per threshold, fp32 [..., T]: every entry is binary_metric_values of its column."""
    shape = tp.shape
    cols = [binary_metric_values(a, b, c, d, beta) for a, b, c, d in
            zip(tp.reshape(-1).tolist(), fp.reshape(-1).tolist(), fn.reshape(-1).tolist(), tn.reshape(-1).tolist())]
    return {n: torch.tensor([c[n] for c in cols], dtype=torch.float32).reshape(shape) for n in METRIC_NAMES}


def binned_average_precision(tp: Sequence[int], fp: Sequence[int], fn: Sequence[int]) -> float:
    """torchmetrics 0.9's BinnedAveragePrecision as we read it (unpinned: torchmetrics was not available to check
    against): with P_k, R_k the fp64 precision and recall at threshold k (0/0 -> 0) and (P, R) = (1, 0) appended after
    the last threshold, AP = -sum_k (R_{k+1} - R_k) P_k, summed in threshold order in fp64 and rounded once to fp32."""
    P = [_ratio(float(a), float(a) + float(b)) for a, b in zip(tp, fp)] + [1.0]
    R = [_ratio(float(a), float(a) + float(c)) for a, c in zip(tp, fn)] + [0.0]
    ap = 0.0
    for k in range(len(P) - 1):
        ap -= (R[k + 1] - R[k]) * P[k]
    return float(torch.tensor(ap, dtype=torch.float32))


def best_index(values: Sequence[float]) -> int:
    """Index of the largest value; ties go to the lowest index (the lowest threshold)."""
    best = 0
    for k, v in enumerate(values):
        if v > values[best]:
            best = k
    return best


def curve_from_hist(hist: torch.Tensor, thresholds: Sequence[float], beta: float = 0.5) -> Dict[str, torch.Tensor]:
    """Everything BinarySegmentationCurve.compute() returns, from a histogram [..., 2, T + 1] on the host."""
    counts = curve_counts(hist.cpu())
    out = {"thresholds": torch.tensor(list(thresholds), dtype=torch.float64)}
    out.update(counts)
    out.update(curve_values(counts["tp"], counts["fp"], counts["fn"], counts["tn"], beta))
    lead = counts["tp"].shape[:-1]
    T = counts["tp"].shape[-1]
    rows = [binned_average_precision(a, b, c) for a, b, c in
            zip(counts["tp"].reshape(-1, T).tolist(), counts["fp"].reshape(-1, T).tolist(),
                counts["fn"].reshape(-1, T).tolist())]
    out["AveragePrecision"] = torch.tensor(rows, dtype=torch.float32).reshape(lead)
    return out


class BinarySegmentationCurve(nn.Module):
    """The confusion counts of `thresholds` from ONE pass over the batch, and what follows from them: the
    precision-recall curve, the binned average precision the reference's MetricCollection carries commented out
    (`BinnedAveragePrecision(num_classes=1, thresholds=torch.linspace(0.5, 0.95, 20))`, utils/scripts_utils.py:90), and
    the threshold that maximises a metric.  Semantics are BinarySegmentationMetrics' own: column k of every result equals
    `BinarySegmentationMetrics(tau=thresholds[k], beta)` on the same updates, bit for bit (each threshold rounded to
    pred's dtype, `>=`, NaN negative, targets truncated, bad preds / targets counted and raised by compute()).

    update(pred, target) is one sn_binary_curve call (two launches, no synchronisation: it sits inside a captured
    training step, CapturedTrainingStep(metrics=curve)); with per_tile=True the leading dimension of `pred` is the tile
    count and every tile keeps a histogram of its own, in a state sized at the first update.  compute() synchronises
    once (all-reduced over `process_group` first when it has more than one rank and sync_on_compute is set) and returns
    {"thresholds" fp64 [T]; "tp", "fp", "fn", "tn" int64 [T]; "JaccardIndex", "Precision", "Recall", "F1Score",
    "FBetaScore" fp32 [T]; "AveragePrecision" fp32 scalar}, with a leading [tiles] dimension on everything but the
    thresholds when per_tile is set.  The average precision is our reading of torchmetrics 0.9's binned rule
    (binned_average_precision); torchmetrics was not available to check against, so that reading is unpinned.
    The state moves with .to(device) and adds no state-dict keys.  There is no CPU path."""

    def __init__(self, thresholds=None, beta: float = 0.5, per_tile: bool = False, sync_on_compute: bool = True,
                 process_group=None):
        super().__init__()
        if thresholds is None:
            thresholds = torch.linspace(0.5, 0.95, 20)
        self.thresholds = _check_thresholds(thresholds)
        if not float(beta) > 0.0:
            raise ValueError(f"beta must be positive (got {beta})")
        self.beta, self.per_tile = float(beta), bool(per_tile)
        self.sync_on_compute, self.process_group = bool(sync_on_compute), process_group
        self._thr_c = None   # the ctypes table of the thresholds, built at the first update (never copied or pickled)
        self._record = _hip.curve_record(len(self.thresholds))
        # per tile: no rows until the first update has shown how many tiles a batch holds
        self.register_buffer("state", torch.zeros((0 if self.per_tile else 1, self._record), dtype=torch.int64),
                             persistent=False)
        self.register_buffer("_ws", torch.zeros(0, dtype=torch.int64), persistent=False)

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_thr_c"] = None
        return state

    @torch.no_grad()
    def update(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        if pred.numel() != target.numel():
            raise ValueError(f"pred ({pred.numel()} elements) and target ({target.numel()} elements) must have the same "
                             "number of elements")
        if pred.is_cuda and self.state.device != pred.device:
            raise HipLibraryError(f"the curve state lives on {self.state.device}: move the module with "
                                  f".to({pred.device}) first")
        segments = 1
        if self.per_tile:
            if pred.dim() < 2:
                raise ValueError("per_tile=True takes pred [tiles, ...]")
            segments = int(pred.shape[0])
            if self.state.shape[0] == 0:
                self.state = torch.zeros((segments, self._record), dtype=torch.int64, device=self.state.device)
            elif self.state.shape[0] != segments:
                raise ValueError(f"the state holds {self.state.shape[0]} tiles; this batch has {segments} "
                                 "(reset() keeps the tile count; build a new curve for another)")
        T = len(self.thresholds)
        if self._thr_c is None:
            self._thr_c = (ctypes.c_double * T)(*self.thresholds)
        need = _hip.curve_ws_bytes(pred.numel() // max(segments, 1), segments, T) if pred.numel() else 0
        if self._ws.numel() * 8 < need:
            self._ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=self.state.device)
        _hip.binary_curve(pred.reshape(-1), target.reshape(-1), self._thr_c, self._ws, self.state, segments=segments)

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        self.update(pred, target)

    def _synced_state(self) -> torch.Tensor:
        state = self.state.clone()
        if self.sync_on_compute:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.process_group) > 1:
                dist.all_reduce(state, op=dist.ReduceOp.SUM, group=self.process_group)
        return state

    def histogram(self) -> torch.Tensor:
        """The accumulated histogram of THIS process, int64 [2, T + 1] ([tiles, 2, T + 1] per tile), on the host;
        synchronises."""
        T = len(self.thresholds)
        h = self.state.cpu()[:, :2 * (T + 1)].reshape(-1, 2, T + 1)
        return h if self.per_tile else h[0]

    def compute(self) -> Dict[str, torch.Tensor]:
        T = len(self.thresholds)
        state = self._synced_state().cpu()
        if int(state[:, 2 * (T + 1)].sum()):
            raise ValueError(PRED_RANGE_ERROR)
        if int(state[:, 2 * (T + 1) + 1].sum()):
            raise ValueError(TARGET_RANGE_ERROR)
        hist = state[:, :2 * (T + 1)].reshape(-1, 2, T + 1)
        if int(hist.sum()) == 0:
            warnings.warn("BinarySegmentationCurve.compute() was called before any update(); returning zeros",
                          UserWarning)
        out = curve_from_hist(hist if self.per_tile else hist[0], self.thresholds, self.beta)
        dev = self.state.device
        return {k: v.to(dev) for k, v in out.items()}

    def average_precision(self) -> torch.Tensor:
        return self.compute()["AveragePrecision"]

    def best_threshold(self, metric: str = "F1Score"):
        """(tau, value) of the threshold where `metric` is largest, ties to the lowest threshold; per tile: two tensors
        [tiles] (fp64 thresholds, fp32 values).  Synchronises (compute())."""
        if metric not in METRIC_NAMES:
            raise KeyError(metric)
        vals = self.compute()[metric].cpu()
        if not self.per_tile:
            k = best_index(vals.tolist())
            return self.thresholds[k], float(vals[k])
        ks = [best_index(row) for row in vals.tolist()]
        return (torch.tensor([self.thresholds[k] for k in ks], dtype=torch.float64),
                torch.stack([vals[i, k] for i, k in enumerate(ks)]) if ks else vals.new_zeros(0))

    def at(self, tau: float) -> Dict[str, torch.Tensor]:
        """{name: value} of the counts and the five values at a threshold of the list (KeyError otherwise)."""
        if float(tau) not in self.thresholds:
            raise KeyError(tau)
        k = self.thresholds.index(float(tau))
        res = self.compute()
        return {n: res[n][..., k] for n in CURVE_COUNT_NAMES + METRIC_NAMES}

    @torch.no_grad()
    def reset(self) -> None:
        self.state.zero_()

    def extra_repr(self) -> str:
        return (f"thresholds={len(self.thresholds)} in [{self.thresholds[0]:.4g}, {self.thresholds[-1]:.4g}], "
                f"beta={self.beta}, per_tile={self.per_tile}")
