"""The ABI layer's host-only helpers (wanproxy_amd/csrc/xcg_api_host.h) on the
CPU: the driver-code map, the registry's UUID key, the fresh-cache and disk-flag
predicates and the two row unpackers that xcg_encode_call and
xcg_last_declarations / xcg_last_references share -- the code the library's
units include, run by oracle/api_host_harness.cc under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, 'oracle/build/api_host_harness')


@pytest.fixture(scope='module')
def harness_run():
    if not os.path.exists(HARNESS):
        from oracle import lib
        lib.build()
    return subprocess.run([HARNESS], capture_output=True, text=True, timeout=60)


def test_harness_exits_clean(harness_run):
    """No check failed (exit 1) and no sanitizer reported."""
    assert harness_run.returncode == 0, harness_run.stderr
    assert harness_run.stderr == ''


@pytest.mark.parametrize('case', [
    'status',     # each named driver code, 0 and unknown negatives -> the ABI status (unknown: XCG_EHIP)
    'uuid',       # mixed case lowercased; 35 characters, a dash out of place, a non-hex digit, null refused
    'decl_rows',  # counts 0, 1, 3; cap below, at, above; each output null in turn; nothing written past the cap
    'ref_rows',   # sorted by time, ties in row order; kind / index split at bit 30; the cap applies after the sort
    'fits',       # the fresh-cache predicate at and above the limit and on an unlimited context; the three bounds
    'results',    # the per-call decoder's result words: fallback 1 / 2, the sticky word, unknown and EXTRACT caps
])
def test_case(harness_run, case):
    assert f'ok {case}' in harness_run.stdout.split('\n'), harness_run.stderr
