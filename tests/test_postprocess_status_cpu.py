"""CPU-only: the pre-launch status contract of the detection post-processing entries (csrc/decode.hip, decode2d.hip,
nms.hip).  tests/golden/postprocess_status.json holds what the build BEFORE the shared layer (csrc/detect.h, the one NMS
pipeline) answered for ~5 000 argument tuples: the ones the six decode / NMS entries reject
-- NULL and misaligned pointers, sizes at and past each limit, bad dtypes, thresholds, factors and strides, and pairs of
violations (which check answers first) -- and every value of the four workspace size queries over a grid of their
arguments (a list in the grid's order); the built library must answer the same.  None of the recorded tuples reaches a launch, and
tools/postprocess_status_sweep.py, which makes the calls with host addresses, runs in a child process that sees no
device."""
import json
import os
import subprocess
import sys

from conftest import GOLDEN, ROOT


def test_postprocess_entries_answer_the_recorded_statuses():
    lib = os.path.join(ROOT, "bevformer_tensorrt_amd", "libbevops_hip.so")
    recorded = os.path.join(GOLDEN, "postprocess_status.json")
    table = json.load(open(recorded))
    queries = [n for n in table if n.endswith("_workspace_size")]
    assert len(table) == 10 and len(queries) == 4 and sum(len(t) for t in table.values()) > 5000
    assert all(s in (2, 3) for n, t in table.items() if n not in queries for s in t.values())
    assert all(any(v > 0 for v in table[n]) and any(v == 0 for v in table[n]) for n in queries)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) +
                       [os.path.join(ROOT, "tools", "postprocess_status_sweep.py"), lib, "--check", recorded],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, f"{r.stdout[-4000:]}\n{r.stderr[-2000:]}"
    assert "recorded tuples, 0 differ" in r.stdout
