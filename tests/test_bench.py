"""bench.py's own options: --dump-outputs writes what the last timed step computed (the head per voxel, fp32, capped in
size by a fixed sample), and a plain run reports the headline alone (everything else is --full's)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("_sn_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod._late_imports()
    return mod


def test_dump_outputs_writes_small_arrays_whole_and_a_fixed_sample_of_large_ones(tmp_path):
    bench = _bench()
    small = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    big = torch.arange(bench.DUMP_WHOLE_MAX + 5, dtype=torch.int32)
    bench.dump_outputs(str(tmp_path / "a"), {"small": small, "big": big, "half": small.half()})
    bench.dump_outputs(str(tmp_path / "b"), {"big": big})
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float64 and s.shape == (2, 3, 4) and np.array_equal(s, small.numpy())
    assert np.load(tmp_path / "a" / "half.npy").dtype == np.float32
    assert not (tmp_path / "a" / "big.npy").exists()
    b = np.load(tmp_path / "a" / "big_sample.npy")
    assert b.dtype == np.float32 and b.shape == (bench.DUMP_SAMPLE,)
    assert np.all(np.diff(b) > 0) and b[-1] < big.numel()                 # distinct positions, ascending
    assert np.array_equal(b, np.load(tmp_path / "b" / "big_sample.npy"))  # the same positions every time
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) < 64 << 20


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    from oracle import geneo_oracle as go
    from oracle import voxel_oracle as vo
    from scene_net_amd.synthetic import synthetic_bank_spec, synthetic_tile
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "2",
                        "--points", "20000", "--grid", "32", "--spinup-ms", "0", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "tiles/s" and line["higher_is_better"] is True and line["dtype"] == "i8"
    assert abs(line["value"] - 2 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    for k in ("roofline", "cpu_baseline", "value_cold", "value_fp32", "sustained", "graph_replay"):
        assert k not in line, k
    out = np.load(tmp_path / "head_out.npy")
    assert out.dtype == np.float32 and out.shape == (2, 1, 32, 32, 32)
    # the bench's inputs are a function of the arguments: tile b of rank 0 is synthetic_tile(b), the bank is the seeded spec
    specs, names, lambdas, last = synthetic_bank_spec({"cy": 6, "cone": 5, "neg": 5})
    for b in range(2):
        counts, _, _ = vo.voxel_counts(synthetic_tile(b, 20_000)[0], (32, 32, 32))
        occ = vo.to_full_dense(vo.normalize_xyz(counts.astype(np.float64)))
        ref = go.scenenet_forward(torch.from_numpy(occ)[None, None], specs, (9, 9, 9), lambdas, last, names=names)
        assert np.abs(out[b, 0].astype(np.float64) - ref[0, 0].numpy()).max() < 1e-4
