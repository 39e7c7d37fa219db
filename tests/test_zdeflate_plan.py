"""The deflate stage's host plan (wanproxy_amd/csrc/xcg_zdeflate_plan.h) on the
CPU: the call-list check both batch drivers share, where each call's arrays and
each scratch section lie, the meta blocks and the host-buffer staging -- the
code xcg_zdeflate.hip's drivers run, run by oracle/zdeflate_plan_harness.cc
under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, 'oracle/build/zdeflate_plan_harness')


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
    'check',     # each refusal on its own: stream out of range, listed twice, out_off 1 / 2 / 3, len 2^24 + 1
    'sections',  # slow and fast level, lengths 0 .. 2^24 alone, mixed and 4096 x 1: sections inside, aligned, disjoint
    'calls',     # consecutive calls' X / table / mask / block ranges apart; blk_cap; the prefix maps; mo == 0 when slow
    'meta',      # the meta block's sections and content; level 0's with 0, 1 and many pieces
    'staging',   # doff 4-aligned with room for the bound; input, output, length and deliver regions apart
])
def test_case(harness_run, case):
    assert f'ok {case}' in harness_run.stdout.split('\n'), harness_run.stderr
