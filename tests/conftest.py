import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu)")


def golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


@pytest.fixture(scope="session")
def oracle_mod():
    import oracle
    oracle.lib()
    return oracle


# The bit-exact CPU checks against what the reference's own torch code computed depend on which MKL and ATen kernels
# the host CPU selects (an EPYC and a Xeon differ in the last bits of a GEMM or a 3x3 inverse).  They run in a fresh
# interpreter with those choices pinned to paths every x86-64 host has: MKL's CPU-independent mode, one thread, the
# AVX2 ATen kernels.  tests/golden/make_wrapper_golden.py records their fixtures under the same settings.
PINNED_CPU_ENV = {"MKL_CBWR": "COMPATIBLE", "OMP_NUM_THREADS": "1", "MKL_NUM_THREADS": "1",
                  "ATEN_CPU_CAPABILITY": "avx2"}


def run_pinned(module, func, timeout=600):
    """Run tests/<module>.py:<func>() in a new interpreter under PINNED_CPU_ENV; its assertions are the caller's."""
    code = f"import sys; sys.path[:0] = {[os.path.join(ROOT, 'tests'), ROOT]!r}; import {module}; {module}.{func}()"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    r = subprocess.run(cmd, env=dict(os.environ, **PINNED_CPU_ENV), capture_output=True, text=True, timeout=timeout,
                       cwd=ROOT)
    assert r.returncode == 0, f"{module}.{func} under {PINNED_CPU_ENV}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
