"""The threshold sweep, host side (no GPU): the C entry and its argument checks, the constructor's validation, and the
host arithmetic histogram -> per-threshold counts -> values -> average precision -> best threshold on hand-made
histograms."""
import copy
import ctypes

import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip
from scene_net_amd import metrics as snm

NAMES = ["JaccardIndex", "Precision", "Recall", "F1Score", "FBetaScore"]


def test_entry_is_bound_and_exported():
    assert "sn_binary_curve" in _hip.SYMBOLS and "sn_binary_curve_ws_bytes" in _hip.SYMBOLS
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(lib, "sn_binary_curve") and hasattr(lib, "sn_binary_curve_ws_bytes")
    assert _hip.SN_CURVE_MAX_THRESHOLDS == 255 and _hip.curve_record(20) == 44
    assert sna.BinarySegmentationCurve is snm.BinarySegmentationCurve and "BinarySegmentationCurve" in sna.__all__


def test_workspace_size_follows_the_grid():
    # one u32 record per workgroup; 4096 elements per workgroup at least, 1024 workgroups over all segments at most
    assert _hip.curve_ws_bytes(1, 1, 1) == 6 * 4
    assert _hip.curve_ws_bytes(4096, 1, 20) == 44 * 4 and _hip.curve_ws_bytes(4097, 1, 20) == 2 * 44 * 4
    assert _hip.curve_ws_bytes(32 * 64 ** 3, 1, 20) == 1024 * 44 * 4
    assert _hip.curve_ws_bytes(64 ** 3, 32, 255) == 1024 * 514 * 4
    assert _hip.curve_ws_bytes(1003, 5, 20) == 5 * 44 * 4
    assert _hip.curve_ws_bytes(100, 2000, 3) == 2000 * 10 * 4        # more segments than the cap: one workgroup each
    lib = _hip.load()
    for n, S, T in ((0, 1, 20), (16, 0, 20), (16, 1, 0), (16, 1, 256), (1 << 41, 1, 20), (1 << 30, 1 << 11, 20),
                    (16, (1 << 20) + 1, 20)):
        assert lib.sn_binary_curve_ws_bytes(n, S, T) == 0, (n, S, T)
        with pytest.raises(sna.HipLibraryError):
            _hip.curve_ws_bytes(n, S, T)


def test_argument_checks_need_no_gpu():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) // 64 * 64)   # aligned host address: never dereferenced here
    F32, F64, U8, OCC8, BF16, I32 = 0, 1, 2, 3, 4, 5
    lin = [0.5 + 0.45 * k / 19 for k in range(20)]

    def call(pred=p, pdt=F32, tgt=p, tdt=OCC8, n=16, S=1, thr=lin, T=None, ws=p, ws_bytes=1 << 20, state=p, batch=None):
        arr = None if thr is None else (ctypes.c_double * len(thr))(*thr)
        return lib.sn_binary_curve(pred, pdt, tgt, tdt, n, S, arr, len(thr) if T is None else T, ws, ws_bytes, state,
                                   batch, None)

    assert call(pred=None) == -1 and b"null" in lib.sn_last_error()
    assert call(tgt=None) == -1 and call(ws=None) == -1 and call(state=None) == -1
    assert call(thr=None, T=20) == -1
    assert call(n=0) == -1 and call(n=-5) == -1
    assert call(S=0) == -1 and call(S=-2) == -1
    assert call(n=1 << 41) == -2 and call(n=1 << 30, S=1 << 11) == -2 and call(S=(1 << 20) + 1) == -2
    assert call(T=0) == -1 and b"T must lie in [1, 255]" in lib.sn_last_error()
    assert call(thr=[0.001 * (k + 1) for k in range(256)]) == -1
    assert call(T=-3) == -1
    for bad in ([0.0, 0.5], [0.5, 1.0], [-0.1], [1.5], [float("nan")], [0.2, float("nan")]):
        assert call(thr=bad) == -1, bad
        assert b"(0, 1)" in lib.sn_last_error()
    for bad in ([0.5, 0.5], [0.6, 0.5], [0.2, 0.4, 0.3]):
        assert call(thr=bad) == -1, bad
        assert b"strictly increasing" in lib.sn_last_error()
    assert call(pdt=U8) == -2 and call(pdt=OCC8) == -2 and call(pdt=I32) == -2   # known dtypes, not a pred dtype
    assert call(pdt=9) == -1 and call(tdt=-1) == -1 and call(tdt=6) == -1        # not dtypes at all
    assert b"sn_binary_curve" in lib.sn_last_error()
    assert call(pred=ctypes.c_void_p(p.value + 2), pdt=F32) == -1
    assert call(tgt=ctypes.c_void_p(p.value + 4), tdt=F64) == -1
    assert call(pred=ctypes.c_void_p(p.value + 1), pdt=BF16) == -1
    assert call(state=ctypes.c_void_p(p.value + 4)) == -1
    assert call(ws=ctypes.c_void_p(p.value + 4)) == -1
    assert call(batch=ctypes.c_void_p(p.value + 4)) == -1
    need = _hip.curve_ws_bytes(10_000, 1, 20)
    assert call(n=10_000, ws_bytes=need - 1) == -1 and b"needed" in lib.sn_last_error()
    assert call(n=10_000, ws_bytes=0) == -1


def test_constructor_validation_mirrors_the_c_checks():
    c = sna.BinarySegmentationCurve()
    assert len(c.thresholds) == 20 and c.thresholds[0] == 0.5 and abs(c.thresholds[-1] - 0.95) < 1e-6
    assert c.beta == 0.5 and not c.per_tile and tuple(c.state.shape) == (1, 44)
    assert tuple(sna.BinarySegmentationCurve(per_tile=True).state.shape) == (0, 44)
    assert sna.BinarySegmentationCurve(thresholds=[0.65]).thresholds == (0.65,)
    assert len(sna.BinarySegmentationCurve(thresholds=torch.linspace(0.002, 0.998, 255)).thresholds) == 255
    for bad in ([], [0.0, 0.5], [0.5, 1.0], [0.5, 0.5], [0.6, 0.5], [float("nan")], torch.linspace(0.001, 0.999, 256)):
        with pytest.raises(ValueError):
            sna.BinarySegmentationCurve(thresholds=bad)
    for beta in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            sna.BinarySegmentationCurve(beta=beta)
    assert list(c.state_dict()) == []                      # no state-dict keys, like the metrics
    c2 = copy.deepcopy(c)
    assert c2.thresholds == c.thresholds and c2.state is not c.state


def test_cpu_tensors_raise():
    c = sna.BinarySegmentationCurve()
    with pytest.raises(sna.HipLibraryError, match="HIP device"):
        c.update(torch.rand(10), torch.ones(10))
    with pytest.raises(ValueError, match="same"):
        c.update(torch.rand(10), torch.ones(11))
    with pytest.raises(sna.HipLibraryError, match="HIP device"):
        sna.BinarySegmentationCurve(per_tile=True).update(torch.rand(2, 5), torch.ones(2, 5))
    with pytest.raises(ValueError, match="tiles"):
        sna.BinarySegmentationCurve(per_tile=True).update(torch.rand(10), torch.ones(10))
    with pytest.raises(sna.HipLibraryError, match="int32"):
        _hip.binary_curve(torch.rand(4), torch.ones(4, dtype=torch.int64), [0.5], c._ws, c.state)


def _direct(hist, k):
    """(tp, fp, fn, tn) at threshold k by the definition: predicted positive = bin > k."""
    neg, pos = hist
    return (sum(pos[k + 1:]), sum(neg[k + 1:]), sum(pos[:k + 1]), sum(neg[:k + 1]))


HISTS = {
    "plain": ([[50, 7, 5, 3, 2], [4, 3, 6, 9, 11]], [0.2, 0.4, 0.6, 0.8]),
    "all negative target": ([[90, 5, 3, 2], [0, 0, 0, 0]], [0.3, 0.5, 0.7]),
    "single threshold": ([[40, 6], [3, 9]], [0.65]),
    "nothing predicted": ([[70, 0, 0], [12, 0, 0]], [0.5, 0.9]),
    "everything predicted": ([[0, 0, 20], [0, 0, 30]], [0.5, 0.9]),
    "large": ([[2 ** 33 + 5, 98765, 4321], [17, 123456789, 2 ** 32 + 1]], [0.25, 0.75]),
    "empty": ([[0, 0, 0], [0, 0, 0]], [0.5, 0.6]),
}


@pytest.mark.parametrize("name", list(HISTS))
@pytest.mark.parametrize("beta", [0.5, 2.0])
def test_counts_and_values_per_threshold(name, beta):
    hist, thr = HISTS[name]
    res = snm.curve_from_hist(torch.tensor(hist, dtype=torch.int64), thr, beta)
    T = len(thr)
    assert res["thresholds"].tolist() == thr and res["thresholds"].dtype == torch.float64
    for k in range(T):
        want = _direct(hist, k)
        got = tuple(int(res[n][k]) for n in ("tp", "fp", "fn", "tn"))
        assert got == want, (k, got, want)
        assert sum(got) == sum(hist[0]) + sum(hist[1])
        col = snm.binary_metric_values(*want, beta=beta)       # each column IS the single-threshold arithmetic
        for n in NAMES:
            assert res[n].dtype == torch.float32 and tuple(res[n].shape) == (T,)
            assert float(res[n][k]) == col[n], (n, k)
    assert all(res[n].dtype == torch.int64 for n in ("tp", "fp", "fn", "tn"))
    assert res["AveragePrecision"].dim() == 0 and res["AveragePrecision"].dtype == torch.float32


def test_average_precision_by_hand():
    # T = 2: P = (6/11, 4/6), R = (6/7, 4/7), then (1, 0):  AP = (6/7 - 4/7) * 6/11 + (4/7 - 0) * 4/6
    hist = [[5, 3, 2], [1, 2, 4]]
    res = snm.curve_from_hist(torch.tensor(hist), [0.3, 0.6])
    want = (6 / 7 - 4 / 7) * (6 / 11) + (4 / 7) * (4 / 6)
    assert float(res["AveragePrecision"]) == float(torch.tensor(want, dtype=torch.float32))
    assert snm.binned_average_precision([6, 4], [5, 2], [1, 3]) == float(res["AveragePrecision"])
    # a perfect detector: every positive above every threshold, every negative below
    assert snm.binned_average_precision([10, 10], [0, 0], [0, 0]) == 1.0
    # single threshold: AP = R_0 * P_0
    assert snm.binned_average_precision([9], [6], [3]) == float(torch.tensor((9 / 12) * (9 / 15), dtype=torch.float32))


def test_all_negative_target_gives_zero_everywhere():
    hist, thr = HISTS["all negative target"]
    res = snm.curve_from_hist(torch.tensor(hist), thr)
    for n in ("Precision", "Recall", "F1Score", "FBetaScore"):
        assert res[n].tolist() == [0.0] * 3
    assert float(res["AveragePrecision"]) == 0.0
    assert res["tp"].tolist() == [0, 0, 0] and res["fn"].tolist() == [0, 0, 0]
    assert float(snm.curve_from_hist(torch.zeros(2, 4, dtype=torch.int64), thr)["AveragePrecision"]) == 0.0


def test_best_index_prefers_the_lowest_threshold_on_ties():
    assert snm.best_index([0.1, 0.7, 0.7, 0.3]) == 1
    assert snm.best_index([0.0, 0.0, 0.0]) == 0
    assert snm.best_index([0.2]) == 0
    assert snm.best_index([0.1, 0.2, 0.9]) == 2


def test_per_tile_histograms_keep_a_leading_dimension():
    a, b = HISTS["plain"][0], [[1, 2, 3, 4, 5], [5, 4, 3, 2, 1]]
    thr = HISTS["plain"][1]
    both = snm.curve_from_hist(torch.tensor([a, b]), thr)
    for i, h in enumerate((a, b)):
        one = snm.curve_from_hist(torch.tensor(h), thr)
        for n in ("tp", "fp", "fn", "tn", *NAMES, "AveragePrecision"):
            assert torch.equal(both[n][i], one[n]), (n, i)
    assert tuple(both["AveragePrecision"].shape) == (2,) and tuple(both["tp"].shape) == (2, 4)


def test_module_arithmetic_from_a_hand_made_state():
    """compute(), best_threshold() and at() on a state written by hand (the state is an ordinary buffer)."""
    hist, thr = HISTS["plain"]
    c = sna.BinarySegmentationCurve(thresholds=thr, beta=0.5, sync_on_compute=False)
    c.state[0, :10] = torch.tensor(hist[0] + hist[1])
    res = c.compute()
    want = snm.curve_from_hist(torch.tensor(hist), thr)
    assert list(res) == ["thresholds", "tp", "fp", "fn", "tn", *NAMES, "AveragePrecision"]
    for n in res:
        assert torch.equal(res[n], want[n]), n
    assert torch.equal(c.histogram(), torch.tensor(hist))
    f1 = want["F1Score"].tolist()
    tau, val = c.best_threshold()
    assert (tau, val) == (thr[snm.best_index(f1)], max(f1))
    tau_p, val_p = c.best_threshold("Precision")
    assert val_p == max(want["Precision"].tolist()) and tau_p in thr
    with pytest.raises(KeyError):
        c.best_threshold("Accuracy")
    at = c.at(0.6)
    assert (int(at["tp"]), int(at["fp"]), int(at["fn"]), int(at["tn"])) == _direct(hist, 2)
    assert float(at["F1Score"]) == snm.binary_metric_values(*_direct(hist, 2))["F1Score"]
    with pytest.raises(KeyError):
        c.at(0.65)
    assert float(c.average_precision()) == float(want["AveragePrecision"])
    c.state[0, 10] = 3                                          # bad preds, then bad targets: the metrics' own errors
    with pytest.raises(ValueError, match="probabilities"):
        c.compute()
    c.state[0, 10] = 0
    c.state[0, 11] = 1
    with pytest.raises(ValueError, match="target"):
        c.compute()
    c.reset()
    assert int(c.state.abs().sum()) == 0
    with pytest.warns(UserWarning, match="before any update"):
        z = c.compute()
    assert float(z["AveragePrecision"]) == 0.0 and z["F1Score"].tolist() == [0.0] * 4
