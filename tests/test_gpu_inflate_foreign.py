"""The inflate kernels on streams zlib's encoder never writes
(tests/inflate_cases.py, built by tests/deflate_writer.py): every case through
the wave, workgroup and quarter-workgroup kernels, call k of every case in
batch k, each call's (output, status) equal to zlib's on the same cuts; on a
refused call the status alone (the pipe discards that call's output)."""
import pytest

from tests.inflate_cases import cases, expected
from tests.test_gpu_zlib import inflate_streams

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

GROUPS = ('tree/', 'refused/', 'runs/', 'header/', 'symbol/', 'block/', 'trailer/', 'region/')
MODES = {1: 'wave', 2: 'workgroup', 3: 'quarter-workgroup'}


def _run(cs, mode, out_cap=None):
    from wanproxy_amd.zpipe import set_inflate_mode
    set_inflate_mode(mode)
    try:
        return inflate_streams([c.calls for c in cs], out_cap=out_cap)
    finally:
        set_inflate_mode(0)


def _compare(cs, got, what):
    """Every call of every case against zlib; all differences in one message."""
    diffs = []
    for c, g in zip(cs, got):
        exp = expected()[c.name]
        for k, ((eo, es), (go, gs)) in enumerate(zip(exp, g)):
            if gs != es:
                diffs.append(f'{c.name} call {k}: status {gs}, zlib {es}')
            elif es != -1 and go != eo:
                i = next((i for i in range(min(len(go), len(eo))) if go[i] != eo[i]), min(len(go), len(eo)))
                diffs.append(f'{c.name} call {k}: {len(go)} bytes, zlib {len(eo)}, first difference at byte {i}')
    assert not diffs, f'{what}: {len(diffs)} calls differ from zlib\n' + '\n'.join(diffs)


def test_groups_cover_the_list():
    assert all(c.name.startswith(GROUPS) for c in cases())
    assert all(any(c.name.startswith(g) for c in cases()) for g in GROUPS)


@pytest.mark.parametrize('group', GROUPS, ids=[g[:-1] for g in GROUPS])
def test_foreign_streams_vs_zlib(group):
    """One group of the case list through the three kernels; the workgroup
    kernels' results equal the wave kernel's exactly (refused calls' leftover
    output included)."""
    cs = [c for c in cases() if c.name.startswith(group)]
    got = {m: _run(cs, m) for m in MODES}
    for m, name in MODES.items():
        _compare(cs, got[m], name)
    assert got[2] == got[1] and got[3] == got[1]


@pytest.mark.parametrize('mode', [2, 3], ids=['workgroup', 'quarter-workgroup'])
def test_region_cases_reach_regions(mode):
    """A region case that never ran a region tested nothing: each one alone,
    the region counters read around it."""
    from wanproxy_amd.zpipe import inflate_region_stats
    rc = [c for c in cases() if c.region]
    assert len(rc) >= 4
    for c in rc:
        inflate_region_stats()
        got = _run([c], mode)
        regions, _, committed, _ = inflate_region_stats()
        _compare([c], got, c.name)
        assert regions >= 1 and committed > 0, (c.name, regions, committed)
    inflate_region_stats()
    _run(rc, 1)
    assert inflate_region_stats()[0] == 0      # the wave kernel has none


def test_foreign_streams_small_room():
    """The region cases and the long outputs again from 256 bytes of output
    room: every call is refused with -2 (nothing committed) and repeated with
    four times the room until it fits, in all three kernels."""
    cs = [c for c in cases() if c.region or c.name in (
        'tree/ladder/48-bit-symbol', 'block/stored-len-65535', 'symbol/distance-32768/straddling',
        'symbol/distance-32768/moved-history', 'symbol/every-distance/long-codes', 'block/types-interleaved/cut5')]
    assert len(cs) >= 10
    got = {m: _run(cs, m, out_cap=256) for m in MODES}
    for m, name in MODES.items():
        _compare(cs, got[m], name + ', 256 bytes of room')
    assert got[2] == got[1] and got[3] == got[1]


def test_foreign_streams_dropin_vs_reference_pipe():
    """The status a proxy sees: every case through the engine-backed
    InflatePipe (integration/zlib_pipes_xcgpu.cc) and through the reference's
    own class over zlib, (bytes, status) per consume up to the first error."""
    from oracle.zlib_pipe import ReferencePipes
    ref, gpu = ReferencePipes('ref'), ReferencePipes('dropin')
    diffs = []
    for c in cases():
        a, b = gpu.pipe('inflate'), ref.pipe('inflate')
        for k, x in enumerate(c.calls):
            g, e = a.consume(x), b.consume(x)
            if g[1] != e[1] or (e[1] != -1 and g[0] != e[0]):
                diffs.append(f'{c.name} call {k}: ({len(g[0])} bytes, {g[1]}), reference ({len(e[0])} bytes, {e[1]})')
            if e[1] == -1 or g[1] == -1:
                break
        a.close()
        b.close()
    assert not diffs, f'{len(diffs)} consumes differ from the reference pipe\n' + '\n'.join(diffs)
