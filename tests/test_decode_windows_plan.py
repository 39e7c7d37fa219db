"""The host plan of a decode batch over several BACKREF windows
(wanproxy_amd/csrc/xcg_decode_windows_plan.h) on the CPU: the code
xcg_decode_batch_windows runs before it launches anything, run by
tests/native/decode_windows_plan_harness.cc as a process of its own, built
with AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests/native/decode_windows_plan_harness.cc')


@pytest.fixture(scope='module')
def harness_run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('plan') / 'decode_windows_plan_harness')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=undefined', '-o', exe, SRC], check=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=60)


def test_harness_exits_clean(harness_run):
    """No check failed (exit 1) and no sanitizer reported."""
    assert harness_run.returncode == 0, harness_run.stderr
    assert harness_run.stderr == ''


@pytest.mark.parametrize('case', [
    'order',     # no chunk, one window, unnamed windows, n windows of one chunk, the cap, random assignments: the naive model
    'refusals',  # no window, above the cap, a window index out of range, null arrays, a null or repeated window: nothing written
])
def test_case(harness_run, case):
    assert f'ok {case}' in harness_run.stdout.split('\n'), harness_run.stderr
