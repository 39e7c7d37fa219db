"""The host plan of the codec send path (wanproxy_amd/csrc/xcg_wire_plan.h) on
the CPU: the code xcg_codec_send_many runs between the encoder step and the
gather launch, run by tests/native/wire_plan_harness.cc as a process of its own,
built with AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests/native/wire_plan_harness.cc')


@pytest.fixture(scope='module')
def harness_run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('plan') / 'wire_plan_harness')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=undefined', '-o', exe, SRC], check=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_harness_exits_clean(harness_run):
    """No check failed (exit 1) and no sanitizer reported."""
    assert harness_run.returncode == 0, harness_run.stderr
    assert harness_run.stderr == ''


@pytest.mark.parametrize('case', [
    'zero_pipes',         # no pipe at all: an empty plan
    'eos_only',           # a pipe with only <EOS>, alone and between others: one literal piece of one byte
    'three_frames',       # 2 x 512 KiB + 1 bytes beside a new and a closing pipe: literal and device pieces together
    'largest_admitted',   # the longest consume the deflate stage's limit admits, every frame at its bound
])
def test_case(harness_run, case):
    """The pieces tile each wire exactly -- no gap, no overlap, nothing outside."""
    assert f'ok {case}' in harness_run.stdout.split('\n'), harness_run.stderr
