"""`python bench.py` without --full: the lean headline run -- set-up, warm-up, the K timed steps, the line -- and what
`--dump-outputs DIR` writes of the last timed step (the losses it returned, the parameters and gradients it left)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    dump = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "8192", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(dump)]
    pr = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
    assert pr.returncode == 0, pr.stderr[-3000:]
    lines = [l for l in pr.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, pr.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["metric"] == "item-embeddings quantized/sec (RQ-VAE fwd+bwd)" and j["unit"] == "items/s" and j["higher_is_better"] is True
    assert j["dtype"].startswith("f32") and j["n_gpus"] == 1 and j["steps"] == 3 and j["warmup"] == 1
    assert j["config"]["rows_per_gpu_per_step"] == 8192
    assert j["ms_per_step"] > 0 and abs(j["value"] - 8192 / (j["ms_per_step"] * 1e-3)) <= 1e-3 * j["value"]
    # the measurements behind --full are not taken
    assert not {"roofline", "roofline_rq", "roofline_kernels", "breakdown_ms", "secondary", "long_run", "box", "parity",
                "cpu_baseline"} & set(j)

    files = sorted(os.listdir(dump))
    arrays = {f[:-4]: np.load(dump / f) for f in files}
    assert all(f.endswith(".npy") for f in files)
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum((dump / f).stat().st_size for f in files) <= 64 << 20
    assert {"out.loss", "out.reconstruction_loss", "out.rqvae_loss", "out.embs_norm", "out.p_unique_ids"} <= set(arrays)
    assert arrays["out.embs_norm"].shape == (8192, 3)
    assert round(float(arrays["out.loss"]), 6) == j["final_loss"]
    params = [k for k in arrays if k.startswith("param.")]
    assert "param.layers.0.embedding.weight" in params and arrays["param.layers.0.embedding.weight"].shape == (256, 32)
    grads = {k for k in arrays if k.startswith("grad.")}
    assert {"grad.encoder.mlp.0.weight", "grad.layers.0.embedding.weight"} <= grads <= {"grad." + k[len("param."):] for k in params}
    assert all(np.isfinite(a).all() for a in arrays.values())
