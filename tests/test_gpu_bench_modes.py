"""GPU box: bench.py's plain run and --dump-outputs.

* A plain run (no --full) prints the headline line -- value, ms_per_step over exactly --steps
  timed steps, verified -- and leaves every other leg out (their fields are null).
* --dump-outputs writes what the last timed step computed as float32 arrays: the parity rows
  equal the oracle's encode of the same synthetic data, the restored rows equal the data.  At a
  batch this small the seeded sample is every group, so the check needs no sample rule.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from quicknet_amd.sharding import rank_seed  # noqa: E402
from quicknet_amd.synth import SEED_ENCODE, synth_bytes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
OTHER_LEGS = ("config4", "host_to_host_mixed", "host_to_host_encode", "rs_abi_host", "per_call", "cpu_baseline",
              "cpu_baseline_threads", "side_configs", "wire", "zfec", "probe_stream_gbs", "copy_d2d_gbs")


def test_plain_run_is_lean_and_dumps_its_outputs(oracle, tmp_path):
    k, m, B, G = 10, 3, 1024, 512
    env = {kk: v for kk, v in os.environ.items() if kk not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--groups", str(G),
                        "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True, timeout=120,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["verified"] is True and out["steps"] == 3 and out["warmup"] == 1
    assert out["unit"] == "GiB/s" and out["higher_is_better"] is True and out["dtype"] == "u8"
    assert out["ms_per_step"] > 0 and out["value"] > 0
    assert [leg for leg in OTHER_LEGS if out[leg] is not None] == []
    assert sorted(os.listdir(tmp_path / "dump")) == ["parity.npy", "restored.npy"]
    parity, restored = np.load(tmp_path / "dump" / "parity.npy"), np.load(tmp_path / "dump" / "restored.npy")
    assert parity.dtype == np.float32 and restored.dtype == np.float32
    data = synth_bytes(rank_seed(SEED_ENCODE, 0), G * k * B).reshape(G, k, B)
    ref = np.zeros((G, m, B), np.uint8)
    oracle.rs_encode(oracle.cauchy(k, m), data, ref, B)
    assert np.array_equal(parity, ref.astype(np.float32))
    assert np.array_equal(restored, data.astype(np.float32))
