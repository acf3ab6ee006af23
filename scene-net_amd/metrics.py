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
"""
from __future__ import annotations

import warnings
from typing import Dict, Optional

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
