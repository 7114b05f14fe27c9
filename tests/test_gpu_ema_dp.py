"""The parameter EMA under data parallel (needs an MI355X), in a fresh child process because it needs a
process group: ONE torchrun rank trains phased TrainSteps with ema_decay set and GradSync forced to issue
both all-reduce buckets at world 1 (force_sync=True). The EMA issues no collective, so `ema`, the parameters
and n_averaged must equal bit for bit those of the same steps without a collective (tools/ema_dp_check.py)."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_world1_forced_sync_step_keeps_the_same_average():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "ema_dp_check.py"),
           "--steps", "3", "--precision", "bf16x3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads(lines[-1])
    print(res)
    assert res["world"] == 1 and res["grad_sync_active"]
    assert res["ema_bit_identical"] and res["params_bit_identical"] and res["ema_lags_params"]
    assert res["n_averaged"] == [3, 3]
