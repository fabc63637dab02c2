"""CPU-only: the pre-launch status contract of the DCNv2 entries (csrc/mdconv.hip, mdconv_s8.hip).
tests/golden/mdconv_status.json holds what the build BEFORE the shared call descriptor (DcnCall / DcnPlan, csrc/mdconv.h)
answered for ~1 100 argument tuples it rejects -- NULL and misaligned pointers, geometry ints <= 0, channel counts
outside each kernel's domain, offset-mask channel counts, dtype codes, bad scales, a short or misaligned workspace, and
pairs of violations (which check answers first) -- and for the size query; the built library must answer the same under
every accepted bevops_mdconv_set_variant value.  None of these tuples reaches a launch, and
tools/dcn_status_sweep.py, which makes the calls with host addresses, runs as a child process that hides every device
from itself."""
import json
import os
import subprocess
import sys

from conftest import GOLDEN, ROOT


def test_dcn_entries_answer_the_recorded_statuses():
    lib = os.path.join(ROOT, "bevformer_tensorrt_amd", "libbevops_hip.so")
    recorded = os.path.join(GOLDEN, "mdconv_status.json")
    table = json.load(open(recorded))
    assert len(table) == 7 and sum(len(t) for t in table.values()) >= 500
    flat = [s for t in table.values() for st in t.values() for s in (st if isinstance(st, list) else [st])]
    assert all(s in (2, 3) for name, t in table.items() if name != "workspace_size"
               for st in t.values() for s in (st if isinstance(st, list) else [st]))
    assert all(s in (0, 2, 3) for s in flat)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) +
                       [os.path.join(ROOT, "tools", "dcn_status_sweep.py"), lib, "--check", recorded],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, f"{r.stdout[-4000:]}\n{r.stderr[-2000:]}"
    assert "recorded calls, 0 differ" in r.stdout
