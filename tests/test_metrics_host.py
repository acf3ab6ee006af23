"""K6 training metrics, host side (no GPU): the C entry and its argument checks, the collection's names and module
contract, the fp64 value arithmetic, and the reference run's recorded numbers against it."""
import ctypes
import json
import os

import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip
from scene_net_amd import metrics as snm

NAMES = ["JaccardIndex", "Precision", "Recall", "F1Score", "FBetaScore"]


def test_entry_is_bound_and_exported():
    assert "sn_binary_stats" in _hip.SYMBOLS
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), "sn_binary_stats")
    assert _hip.SN_I32 == 5 and _hip.SN_METRIC_WS_BYTES == 1024 * 6 * 8
    assert torch.int32 not in _hip._DT   # int32 is a target dtype of sn_binary_stats only


def test_argument_checks_need_no_gpu():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(256)
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 63) // 64 * 64)   # 64-byte aligned host address: never dereferenced on these paths
    F32, F64, U8, OCC8, BF16, I32 = 0, 1, 2, 3, 4, 5

    def call(pred=p, pdt=F32, tgt=p, tdt=OCC8, n=16, tau=0.65, beta=0.5, ws=p, state=p, batch=None, values=None):
        return lib.sn_binary_stats(pred, pdt, tgt, tdt, n, tau, beta, ws, state, batch, values, None)

    assert call(pred=None) == -1 and b"null" in lib.sn_last_error()
    assert call(tgt=None) == -1
    assert call(ws=None) == -1
    assert call(state=None) == -1
    assert call(n=0) == -1 and call(n=-5) == -1
    assert call(n=1 << 41) == -2
    for tau in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert call(tau=tau) == -1, tau
        assert b"tau" in lib.sn_last_error()
    assert call(beta=0.0) == -1 and call(beta=float("nan")) == -1
    assert call(pdt=U8) == -2 and call(pdt=OCC8) == -2 and call(pdt=I32) == -2   # known dtypes, not a pred dtype
    assert call(pdt=9) == -1 and call(tdt=-1) == -1 and call(tdt=6) == -1        # not dtypes at all
    # element alignment only, but at least that
    assert call(pred=ctypes.c_void_p(p.value + 2), pdt=F32) == -1
    assert call(tgt=ctypes.c_void_p(p.value + 4), tdt=F64) == -1
    assert call(state=ctypes.c_void_p(p.value + 4)) == -1
    # SN_I32 stays refused by the other entries: the criterion's forward takes no int32 ground truth
    assert lib.sn_loss_forward(p, F32, p, I32, 1, 16, p, p, 1, 1, 1.0, 0.5, 1.0, 1.0, 1.0, 1.0, p, p, p, p, None) == -1


def test_cpu_tensors_raise():
    m = snm.BinarySegmentationMetrics()
    with pytest.raises(sna.HipLibraryError, match="HIP device"):
        m.update(torch.rand(10), torch.ones(10))
    with pytest.raises(ValueError, match="same"):
        m.update(torch.rand(10), torch.ones(11))
    with pytest.raises(sna.HipLibraryError, match="int32"):
        _hip.binary_stats(torch.rand(4), torch.ones(4, dtype=torch.int64), 0.65, 0.5, m._ws, m.state)


def test_names_iteration_and_keys_follow_the_reference():
    m = sna.init_metrics()
    assert isinstance(m, sna.BinarySegmentationMetrics) and m.tau == 0.65 and m.beta == 0.5
    assert list(m) == NAMES                                   # scripts/main.py: [str(met) for met in init_metrics()]
    assert list(m.keys()) == NAMES
    assert [k for k, _ in m.items()] == NAMES
    assert [str(v.name) for v in m.values()] == NAMES and len(m) == 5
    with pytest.raises(KeyError):
        m["Accuracy"]
    with pytest.raises(ValueError):
        snm.BinarySegmentationMetrics(tau=1.0)
    with pytest.raises(ValueError):
        snm.BinarySegmentationMetrics(beta=0.0)


def test_metrics_add_no_state_dict_keys(golden_dir):
    with open(os.path.join(golden_dir, "module_contract.json")) as f:
        contract = json.load(f)
    torch.manual_seed(contract["seed"])
    model = sna.SceneNet({"cy": 2, "cone": 1, "neg": 1}, (9, 9, 9))
    model.train_metrics = sna.init_metrics()
    model.val_metrics = sna.init_metrics()
    assert list(model.state_dict().keys()) == contract["state_dict_keys"]
    assert [n for n, _ in model.named_parameters()] == contract["named_parameters"]
    model.load_state_dict(model.state_dict())   # strict: loads back without missing or unexpected keys
    assert list(sna.init_metrics().state_dict()) == []


def _fp64(tp, fp, fn, tn, beta):
    r = lambda a, b: 0.0 if b == 0 else a / b   # noqa: E731
    P, R = r(tp, tp + fp), r(tp, tp + fn)
    return {"JaccardIndex": 0.5 * (r(tp, tp + fp + fn) + r(tn, tn + fp + fn)), "Precision": P, "Recall": R,
            "F1Score": r(2 * P * R, P + R), "FBetaScore": r((1 + beta ** 2) * P * R, beta ** 2 * P + R)}


@pytest.mark.parametrize("counts", [(0, 0, 0, 1000), (1000, 0, 0, 0), (0, 0, 0, 0), (0, 5, 0, 10), (0, 0, 5, 10),
                                    (0, 5, 5, 0), (3, 0, 0, 7), (7, 2, 1, 90), (123456789, 98765, 4321, 2 ** 33 + 5),
                                    (1, 10 ** 9, 10 ** 9, 0)])
@pytest.mark.parametrize("beta", [0.5, 1.0, 2.0])
def test_value_function_matches_the_fp64_formulas(counts, beta):
    got = snm.binary_metric_values(*counts, beta=beta)
    ref = _fp64(*[float(c) for c in counts], beta)
    assert list(got) == NAMES
    for k in NAMES:
        assert got[k] == float(torch.tensor(ref[k], dtype=torch.float32)), (k, got[k], ref[k])


def test_zero_division_cases():
    v = snm.binary_metric_values(0, 0, 0, 500)      # all negative, all correct
    assert v == {"JaccardIndex": 0.5, "Precision": 0.0, "Recall": 0.0, "F1Score": 0.0, "FBetaScore": 0.0}
    v = snm.binary_metric_values(500, 0, 0, 0)      # all positive, all correct: the background class is absent
    assert v == {"JaccardIndex": 0.5, "Precision": 1.0, "Recall": 1.0, "F1Score": 1.0, "FBetaScore": 1.0}
    v = snm.binary_metric_values(0, 0, 0, 0)
    assert set(v.values()) == {0.0}
    v = snm.binary_metric_values(0, 10, 10, 0)      # everything wrong
    assert set(v.values()) == {0.0}
    assert snm.f_beta(0.0, 0.0, 0.5) == 0.0


def test_reference_run_is_reproduced_by_the_value_arithmetic(golden_dir):
    with open(os.path.join(golden_dir, "reference_run_metrics.json")) as f:
        run = json.load(f)
    beta = run["beta"]
    for split in ("train", "val"):
        rec = run[split]
        P, R = rec["Precision"], rec["Recall"]
        # F1Score and FBetaScore follow from the recorded Precision and Recall
        assert abs(snm.f_beta(P, R, 1.0) - rec["F1Score"]) <= 2e-7 * rec["F1Score"], split
        assert abs(snm.f_beta(P, R, beta) - rec["FBetaScore"]) <= 2e-7 * rec["FBetaScore"], split
        # JaccardIndex is the macro mean over both classes: the tower IoU is F1 / (2 - F1), the background IoU
        # 2J - tower IoU must be a valid IoU; the tower IoU alone is nowhere near the recorded value
        J, F1 = rec["JaccardIndex"], rec["F1Score"]
        iou_tower = F1 / (2.0 - F1)
        assert 0.0 <= 2 * J - iou_tower <= 1.0, split
        assert abs(iou_tower - J) > 0.1, split
