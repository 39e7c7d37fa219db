"""The XCodecDisk volume format (wanproxy_amd/csrc/xcg_volume.cpp: geometry,
registry, index blocks and their counters, the reload, the clock of a reloaded
ring) on the CPU: the code the library links, run by oracle/volume_harness.cc
as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
over volume images it builds from fixed seeds.  A sanitizer report is a
non-zero exit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, 'oracle/build/volume_harness')


def build_harness():
    if not os.path.exists(HARNESS):
        from oracle import lib
        lib.build()
    return HARNESS


@pytest.fixture(scope='module')
def harness_run(tmp_path_factory):
    return subprocess.run([build_harness(), 'cases', str(tmp_path_factory.mktemp('volumes'))], capture_output=True,
                          text=True, timeout=120)


def test_harness_exits_clean(harness_run):
    """No check failed (exit 1) and no sanitizer reported anything."""
    assert harness_run.returncode == 0, harness_run.stderr
    assert harness_run.stderr == ''


@pytest.mark.parametrize('case', [
    'geometry',    # -22 at 18 blocks or fewer and with no room for an index block; nb and D of 3 and 12 index blocks
    'fresh',       # a volume never written saves as zeros of exactly its size
    'roundtrip',   # two fronts, counters out of block order: the clock model's ring; write -> load -> write identical
    'dup_hash',    # the later of two entries of one hash by counter order survives
    'bad_entry',   # a checked entry with the wrong data is dropped; the head moves back; past 80 blocks no check
    'registry',    # non-UUID, zero and duplicate slots skipped; fronts without entries collected; a generated UUID
    'front_xuid',  # the table of which xuid and name a new front takes, and its refusals
    'advance',     # k appends at once = k times one, across index blocks and laps; the counter skips 0
    'damaged',     # cut, noise, xuid >= 1024, counters of ~0, a longer file: loads, then writes exactly `bytes`
])
def test_case(harness_run, case):
    assert f'ok {case}' in harness_run.stdout.split('\n'), harness_run.stderr
