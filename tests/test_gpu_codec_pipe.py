"""The configured codec (xcg_codec_*, wanproxy_amd/csrc/xcg_codec.cpp): the
XCodec pipe pair through the zlib stage, many pipes per call.

The scripted conversations of tests/codec_pipe_cases.py, run on the engine with
the fused send path on and off, must reproduce the transcripts the reference's
own classes produced (tests/golden/codec_pipe.json), byte for byte -- and the
layer's counters must show that each send turn was ONE batch of the selected
path and each receive turn ONE inflate batch (a fallback to serial calls would
pass every transcript).  xcg_gather_pieces alone against numpy; the calls the
ABI refuses leave nothing behind; the layer's GPU memory goes when it goes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import codec_pipe_cases as cc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XCG_EINVAL = -22


@pytest.fixture(scope='module')
def golden_codec():
    with open(os.path.join(ROOT, 'tests/golden/codec_pipe.json')) as f:
        return json.load(f)['conversations']


@pytest.fixture(scope='module')
def E():
    from wanproxy_amd.xcgpu import connect_registry_clear
    connect_registry_clear()
    return cc.EngineChain()


@pytest.fixture(params=[True, False], ids=['fused', 'host'])
def fused(request):
    from wanproxy_amd.xcgpu import set_codec_fused
    old = set_codec_fused(request.param)
    yield request.param
    set_codec_fused(old)


def same(T, exp, name):
    got = cc.record(T)
    assert len(got) == len(exp)
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g == e, f'{name}: step {k} ({cc.conversation(name).steps[k][:2]}) differs from the reference'


@pytest.mark.parametrize('name', cc.NAMES)
def test_engine_reproduces_reference(E, golden_codec, fused, name):
    from wanproxy_amd.xcgpu import codec_debug_counts
    conv = cc.conversation(name)
    turns = {'send': 0, 'recv': 0}

    def count(op, pipes, datas):
        turns[op] += 1

    before = codec_debug_counts()
    T = cc.run(conv, E, before_turn=count)
    d = [a - b for a, b in zip(codec_debug_counts(), before)]
    same(T, golden_codec[name], name)
    if conv.level is None:
        assert d[:3] == [0, 0, 0]                        # no zlib stage at all
    else:
        assert d[0] == (turns['send'] if fused else 0)   # one batch per send_many turn, on the selected path
        assert d[1] == (0 if fused else turns['send'])
        assert d[2] == turns['recv']                     # one inflate batch per receive_many turn
    assert d[3] <= turns['recv']                         # at most one decode batch per turn


# ---------------------------------------------------------------- xcg_gather_pieces

TILE = 8192                                              # GATHER_TILE, xcg_wire.hip
GATHER_LENGTHS = [0, 1, 15, 16, 17, 1023, 1024, 1025, TILE, TILE + 1, (1 << 20) + 21,
                  3, 40, 100, 4097, TILE - 1, 2 * TILE + 5]


def _gather_case():
    """Pieces of every length above, three times; piece i reads at residue i mod
    16.  Every fourth piece lies back to back with the one before; the others
    land behind a gap of canary bytes, the pieces of 16 bytes and more at
    residues 0, 1, 2, ... mod 16 in turn."""
    rng = np.random.default_rng(5)
    lens = GATHER_LENGTHS + GATHER_LENGTHS[::-1] + GATHER_LENGTHS
    src_off, dst_off, which = [], [], []
    s_cur, d_cur, turn = [0, 0], 64, 0
    for i, n in enumerate(lens):
        w = i % 3 == 2                                   # every third piece comes from the second allocation
        s = (s_cur[w] + 15) // 16 * 16 + i % 16
        src_off.append(s)
        which.append(w)
        s_cur[w] = s + n
        if i % 4 != 1:
            want = turn % 16
            turn += n >= 16
            d_cur += 1 + (want - (d_cur + 1)) % 16       # at least one canary byte between
        dst_off.append(d_cur)
        d_cur += n
    srcs = [rng.integers(0, 256, s_cur[w] + 64, dtype=np.uint8) for w in (0, 1)]
    return lens, src_off, dst_off, which, srcs, d_cur + 64


def test_gather_case_covers_every_residue():
    lens, src_off, dst_off, which, srcs, total = _gather_case()
    assert {s % 16 for s, n in zip(src_off, lens) if n >= 16} == set(range(16))
    assert {d % 16 for d, n in zip(dst_off, lens) if n >= 16} == set(range(16))
    assert len({(s - d) % 16 for s, d in zip(src_off, dst_off)}) >= 8
    ends = {d + n for d, n in zip(dst_off, lens) if n}
    assert sum(1 for d, n in zip(dst_off, lens) if n and d in ends) >= 8     # back to back


@pytest.mark.parametrize('max_len', [max(GATHER_LENGTHS), 1], ids=['grid_for_longest', 'grid_for_1'])
def test_gather_pieces_against_numpy(max_len):
    import torch
    from wanproxy_amd.xcgpu import Context, _check, _stream_ptr, lib
    lens, src_off, dst_off, which, srcs, total = _gather_case()
    dev = torch.device('cuda', 0)
    canary = (np.arange(total, dtype=np.uint32) * 37 + 11).astype(np.uint8)
    exp = canary.copy()
    for n, s, d, w in zip(lens, src_off, dst_off, which):
        exp[d:d + n] = srcs[w][s:s + n]
    d_srcs = [torch.from_numpy(x).to(dev) for x in srcs]
    d_dst = torch.from_numpy(canary.copy()).to(dev)
    # offsets relative to the first allocation; the second one's wrap (uint64 arithmetic)
    base = [0, (d_srcs[1].data_ptr() - d_srcs[0].data_ptr()) % (1 << 64)]
    so = np.array([(base[w] + s) % (1 << 64) for s, w in zip(src_off, which)], dtype=np.uint64)
    d_so = torch.from_numpy(so.view(np.int64)).to(dev)
    d_do = torch.from_numpy(np.array(dst_off, dtype=np.int64)).to(dev)
    d_ln = torch.from_numpy(np.array(lens, dtype=np.uint32).view(np.int32)).to(dev)
    ctx = Context(0, cache_segments=1 << 10)
    try:
        _check(lib().xcg_gather_pieces(ctx.h, C.c_void_p(d_srcs[0].data_ptr()), C.c_void_p(d_so.data_ptr()),
                                       C.c_void_p(d_do.data_ptr()), C.c_void_p(d_ln.data_ptr()), len(lens), max_len,
                                       C.c_void_p(d_dst.data_ptr()), _stream_ptr(None)))
        torch.cuda.synchronize(dev)
    finally:
        ctx.close()
    got = d_dst.cpu().numpy()
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f'{bad.size} bytes differ, the first at {bad[:8]}'


# ---------------------------------------------------------------- refused calls, memory

def _raw(fn, pipes, datas, lens, out=True):
    n = len(pipes)
    hs = (C.c_void_p * n)(*[p.h.value for p in pipes])
    ds = (C.c_char_p * n)(*datas)
    ls = (C.c_uint64 * n)(*lens)
    from wanproxy_amd.xcgpu import _PipeOut
    outs = (_PipeOut * n)()
    return fn(hs, ds, ls, n, outs if out else None, None)


def test_refused_calls_change_nothing(E, golden_codec):
    """In front of every turn of a conversation: null arguments, a pipe listed
    twice, pipes of two codecs, a send above the deflate stage's limit, a
    receive above the inflate stage's and -- once a pipe has closed its side --
    a send on it.  Every one is XCG_EINVAL, and the conversation still runs to
    the reference's transcript."""
    from wanproxy_amd.xcgpu import Codec, Context, lib
    L = lib()
    name = 'eos_a_first_l6'
    conv = cc.conversation(name)
    octx = Context(0, cache_segments=1 << 10)
    other = Codec(octx, octx, 6, 2, connect=True)
    stranger = other.pipe(cc.UUID_V)
    closed, seen = [], {'after_eos': 0, 'turns': 0}

    def refuse(op, pipes, datas):
        ps = [p.p for p in pipes]
        seen['turns'] += 1
        for fn in (L.xcg_codec_send_many, L.xcg_codec_receive_many):
            assert fn(None, None, None, 1, None, None) == XCG_EINVAL
            assert _raw(fn, ps, [b'x'] * len(ps), [1] * len(ps), out=False) == XCG_EINVAL
            assert _raw(fn, ps + ps[:1], [b'x'] * (len(ps) + 1), [1] * (len(ps) + 1)) == XCG_EINVAL
            assert _raw(fn, ps + [stranger], [b'x'] * (len(ps) + 1), [1] * (len(ps) + 1)) == XCG_EINVAL
        # 16 frames of 5 + xcg_encode_bound(512 KiB) bytes pass 2^24 (the length alone is refused: no byte is read)
        assert _raw(L.xcg_codec_send_many, ps, [b'x'] * len(ps), [8 << 20] * len(ps)) == XCG_EINVAL
        assert _raw(L.xcg_codec_receive_many, ps, [b'x'] * len(ps), [(1 << 26) + 1] * len(ps)) == XCG_EINVAL
        for p in closed:
            assert _raw(L.xcg_codec_send_many, [p], [b'x'], [1]) == XCG_EINVAL
            seen['after_eos'] += 1
        if op == 'send':
            closed.extend(p for p, d in zip(ps, datas) if not d)

    try:
        T = cc.run(conv, E, before_turn=refuse)
    finally:
        stranger.close()
        other.close()
        octx.close()
    assert seen['turns'] > 10 and seen['after_eos'] > 5
    same(T, golden_codec[name], name)


def test_memory_returns(E, fused):
    from test_gpu_mem import mem_live
    cc.run(cc.conversation('ask_learn_l6'), E)           # (whatever the process keeps for good is there now)
    before = mem_live()
    cc.run(cc.conversation('mixed_send_l1'), E)
    assert mem_live() == before
