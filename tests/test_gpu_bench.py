"""-m gpu: the plain `bench.py` run (headline only, exactly --steps timed steps) and its --dump-outputs files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_times_the_steps_and_dumps_outputs(tmp_path):
    from agile3d_amd.synthetic import make_scene
    out_dir = tmp_path / "outputs"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "A3D_BENCH_ONE_GPU")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2",
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["timed_region"]["repetitions"] == 1 and len(d["timed_region"]["ms_per_step_all"]) == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "scenes/s" and d["dtype"] == "f32"
    for k in ("roofline", "latency_ms_per_scene", "value_batch4", "train_iter", "cpu_baseline", "iou_at_k",
              "emulated_fp32_products"):
        assert k not in d, f"{k} belongs to --full"

    names = sorted(os.listdir(out_dir))
    assert names == ["aux_pred_masks_0.npy", "aux_pred_masks_1.npy", "backbone_features.npy", "pred_masks.npy"], names
    assert sum(os.path.getsize(out_dir / n) for n in names) <= 64 << 20
    arrays = {n[:-4]: np.load(out_dir / n) for n in names}
    for n, a in arrays.items():
        assert a.dtype == np.float32 and a.ndim == 2 and np.isfinite(a).all(), n
    rows = sum(len(make_scene(80_000, seed=b, batch_index=b)["coords"]) for b in range(2))
    assert arrays["pred_masks"].shape == (rows, 6)                      # both samples' logits, 5 objects + background
    assert arrays["aux_pred_masks_0"].shape[1] == arrays["aux_pred_masks_1"].shape[1] == 6
    assert arrays["backbone_features"].shape[1] == 128
