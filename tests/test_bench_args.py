"""bench.py's launch contract (no GPU): `--gpus N` without an outer launcher
starts N ranks itself; under torchrun the launcher's WORLD_SIZE must equal
--gpus."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import launch_plan  # noqa: E402


def test_launch_plan():
    assert launch_plan(None, {}) == ('rank', 1)
    assert launch_plan(1, {}) == ('rank', 1)
    assert launch_plan(8, {}) == ('spawn', 8)
    assert launch_plan(4, {'WORLD_SIZE': '4'}) == ('rank', 4)
    assert launch_plan(None, {'WORLD_SIZE': '2'}) == ('rank', 2)
    with pytest.raises(ValueError):
        launch_plan(8, {'WORLD_SIZE': '2'})
    with pytest.raises(ValueError):
        launch_plan(1, {'WORLD_SIZE': '8'})
    with pytest.raises(ValueError):
        launch_plan(0, {})


def test_full_is_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'd'])
    a = bench.parse()
    assert a.full and a.dump_outputs == 'd'
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '0'])
    with pytest.raises(SystemExit):
        bench.parse()


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: float arrays of the caller's buffers, the sampled rows
    byte for byte and zero past each chunk's length, under 64 MB in all."""
    import numpy as np
    import torch
    import bench
    n = 70                                             # (more chunks than the sample)
    rng = np.random.default_rng(1)
    bound = 2 * bench.CHUNK + 16
    oo = np.arange(n, dtype=np.uint64) * bound
    ol = rng.integers(1, bound + 1, n).astype(np.int64)
    ol[0] = bound                                      # (a full slot)
    out = rng.integers(0, 256, n * bound).astype(np.uint8)
    st = rng.integers(0, 2**32, 4 * n, dtype=np.uint64).astype(np.uint32)
    args = (n, oo, torch.from_numpy(out), torch.from_numpy(ol), torch.from_numpy(st.view(np.int32)))
    bench.dump_outputs(str(tmp_path / 'a'), 0, *args)
    bench.dump_outputs(str(tmp_path / 'b'), 1, *args)
    names = ['out_len', 'stats', 'out_digest', 'out_sample', 'out_sample_chunks']
    got = {k: np.load(tmp_path / 'a' / f'{k}.npy') for k in names}
    assert sorted(os.listdir(tmp_path / 'a')) == sorted(k + '.npy' for k in names)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 10**6
    assert (got['out_len'] == ol).all() and (got['stats'] == st.reshape(n, 4)).all()
    pick = got['out_sample_chunks'].astype(int)
    assert pick.size == bench.DUMP_SAMPLE == len(set(pick)) and got['out_sample'].shape == (pick.size, bound)
    for r, i in enumerate(pick):
        row = got['out_sample'][r]
        assert (row[:ol[i]] == out[i * bound:i * bound + ol[i]]).all() and not row[ol[i]:].any()
    b = out[3 * bound:3 * bound + ol[3]].astype(np.int64)
    assert got['out_digest'][3].tolist() == [b.sum(), (b * (np.arange(b.size) % 251 + 1)).sum()]
    for k in names:                                    # same buffers, same files (rank 1 only renames them)
        assert (np.load(tmp_path / 'b' / f'{k}_rank1.npy') == got[k]).all()


def test_mismatched_world_exits_nonzero():
    env = dict(os.environ, WORLD_SIZE='2', RANK='0', LOCAL_RANK='0')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '4'], env=env,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and 'WORLD_SIZE 2' in r.stderr
