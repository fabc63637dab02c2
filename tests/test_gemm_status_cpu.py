"""CPU-only: the pre-launch status contract of the dense GEMM entries (csrc/tsgemm.hip, tile_gemm.hip, small_gemm.hip).
tests/golden/gemm_status.json holds what the build BEFORE the shared host layer (csrc/gemm_host.h) answered for ~2 000
argument tuples it rejects -- NULL and misaligned pointers, sizes outside each family's domain, bad scales and dtype
codes, group strides, destination tables, and pairs of violations (which check answers first) -- and for m == 0; the
built library must answer the same.  None of these tuples reaches a launch, and tools/gemm_status_sweep.py, which makes
the calls with host addresses, runs in a child process that sees no device."""
import json
import os
import subprocess
import sys

from conftest import GOLDEN, ROOT


def test_dense_entries_answer_the_recorded_statuses():
    lib = os.path.join(ROOT, "bevformer_tensorrt_amd", "libbevops_hip.so")
    recorded = os.path.join(GOLDEN, "gemm_status.json")
    table = json.load(open(recorded))
    assert len(table) == 16 and sum(len(t) for t in table.values()) > 2000
    assert all(s in (2, 3) or (s == 0 and "m=0" in label.split()) for t in table.values() for label, s in t.items())
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) +
                       [os.path.join(ROOT, "tools", "gemm_status_sweep.py"), lib, "--check", recorded],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, f"{r.stdout[-4000:]}\n{r.stderr[-2000:]}"
    assert "recorded tuples, 0 differ" in r.stdout
