"""bench.py's command line: a plain run times exactly --steps steps and measures nothing else (the extra measurements
are behind --full), and --dump-outputs writes what the timed path computed in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY_KEYS = ("roofline", "roofline_pairwise", "pyramid", "wall_clock_to_output", "cpu_baseline", "kernel_families_ms_per_step")


def _bench(args, env_extra=None, timeout=600, drop=()):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT") + tuple(drop)}
    env.update(env_extra or {})
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                         timeout=timeout, cwd=ROOT)
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    return out, lines


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"]], ids=["no_steps", "negative_warmup"])
def test_bench_refuses_a_run_without_timed_steps(args):
    out, lines = _bench(["--rehearse"] + args)
    assert out.returncode != 0 and not lines and "--steps must be at least 1" in out.stderr


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_reproducible_outputs(tmp_path):
    """Two plain runs with the same arguments: each line reports the steps it timed and none of the --full measurements,
    and the two dumps are identical -- the same seeded inputs, and a timed step that sums its tap adjoint in a fixed order
    (no STROTSS_DETERMINISTIC in the environment: the benchmark's own default)."""
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        out, lines = _bench(["--steps", "3", "--warmup", "1", "--scale", "64", "--dump-outputs", str(d)],
                            drop=("STROTSS_DETERMINISTIC",))
        assert out.returncode == 0, out.stderr[-3000:]
        assert len(lines) == 1
        line = lines[0]
        assert line["config"]["tap_adjoint"].startswith("deterministic")
        assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "steps/s" and line["dtype"] == "f32"
        assert line["ms_per_step"] > 0 and abs(line["value"] - 1e3 / line["ms_per_step"]) < 0.01 * line["value"]
        assert not any(k in line for k in FULL_ONLY_KEYS) and line["long_window"] is None and line["box_calibration"] is None
        files = sorted(os.listdir(d))
        assert files == sorted(["stylized.npy", "losses.npy", "region_loss_terms.npy"] + [f"pyramid_{k}.npy" for k in range(6)])
        assert sum(os.path.getsize(d / f) for f in files) <= 64 * 10**6
        arrays = {f[:-4]: np.load(d / f) for f in files}
        for name, a in arrays.items():
            assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), name
        assert arrays["stylized"].shape == (1, 64, 64, 3) and arrays["pyramid_0"].shape == (1, 64, 64, 3)
        assert arrays["losses"].dtype == np.float64 and arrays["losses"].shape == (6,)
        assert abs(arrays["losses"][0] - line["loss_after"]) <= 1e-4 * abs(line["loss_after"]) + 1e-5
        dumps.append(arrays)
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name], dumps[1][name]), name
