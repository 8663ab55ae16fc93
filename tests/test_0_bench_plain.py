"""A plain `bench.py --gpus 1 --steps K --warmup W` run on the GPU: it stops
at the headline figures (none of the --full lines), --steps sets the timed
steps, and --dump-outputs writes the last step's score / mask sample and the
per-row sums, consistent with each other."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_line_and_dump(tmp_path):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [x for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["unit"] == "queries/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["config"]["rows_per_rank"] == [40932]
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 40932) <= 40932 * 1e-3
    for key in ("roofline", "kernels_ms", "cpu_baseline", "reference_pytorch", "wn18rr_forward", "em_iteration"):
        assert key not in d
    got = {f: np.load(os.path.join(str(tmp_path), f)) for f in sorted(os.listdir(str(tmp_path)))}
    assert sorted(got) == ["mask.npy", "sample_rows.npy", "score.npy", "score_row_sum.npy"]
    assert sum(a.nbytes for a in got.values()) <= 64e6
    idx = got["sample_rows.npy"].astype(np.int64)
    E = got["score.npy"].shape[1]
    assert got["score.npy"].shape == got["mask.npy"].shape == (len(idx), E)
    assert got["score.npy"].dtype == np.float32 and got["score_row_sum.npy"].shape == (40932,)
    assert np.isfinite(got["score.npy"]).all() and set(np.unique(got["mask.npy"])) <= {0.0, 1.0}
    # the sampled rows are the rows the sums describe: float64 sums of the same fp32 scores, apart
    # only in the order of |E| float64 additions (~|E| * 2^-53 relative to the largest partial sum)
    np.testing.assert_allclose(got["score.npy"].astype(np.float64).sum(1), got["score_row_sum.npy"][idx],
                               rtol=1e-9, atol=1e-6)
