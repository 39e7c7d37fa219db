"""The GPU-memory owner (wanproxy_amd/csrc/xcg_devmem.h) on the CPU: the code
the library instantiates over HIP, run by oracle/devmem_harness.cc over a
counting malloc backend that aborts on a double or foreign free and can fail
the k-th allocation.  The failure paths are tested here, never on a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, 'oracle/build/devmem_harness')


@pytest.fixture(scope='module')
def harness_run():
    if not os.path.exists(HARNESS):
        from oracle import lib
        lib.build()
    return subprocess.run([HARNESS], capture_output=True, text=True, timeout=60)


def test_harness_exits_clean(harness_run):
    """No check failed (exit 1) and the backend saw no double or foreign free
    (abort)."""
    assert harness_run.returncode == 0, harness_run.stderr
    assert harness_run.stderr == ''


@pytest.mark.parametrize('case', [
    'table',          # six buffers, failure injected at every k = 1..6 and at none: reported, nothing live after
    'release_twice',  # release_all() twice, the destructor after it, the destructor alone
    'release_one',    # single-buffer release; a pointer not held is left alone
    'grow',           # no-op at capacity, free before allocate, null / 0 after a failed grow, each growth policy
    'guard',          # the stream-ordered scope guard: exactly one free on early return, failure and normal exit
    'live_zero',      # the backend's live counters are back at zero at the end
])
def test_case(harness_run, case):
    assert f'ok {case}' in harness_run.stdout.split('\n'), harness_run.stderr
