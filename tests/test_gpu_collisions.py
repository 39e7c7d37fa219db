"""Constructed hash collisions through every encoder variant (the cases of
tests/collision_cases.py; tests/test_collision_cases.py proves on the CPU that
each reaches its branch and that a wrong treatment of it changes the output).

A window whose 64-bit XCodecHash is declared for other bytes is skipped and
may not become the candidate (xcodec_encoder.cc:215-216, :390-406); two blocks
that share only the low 32 bits, or only the direct-mapped probe key, are
ordinary misses.  Every case compares the device encoder's output bytes and
out_len with the oracle's and with the reference-made tests/golden/collisions.json;
the independent cases also compare the stats words with the model's
(n_extract, n_ref, n_collision) -- non-zero collision counts -- and every
in-band encoding is decoded back, by the oracle and on the GPU."""
import hashlib
import json
import os

import numpy as np
import pytest

import collision_cases as cc
from test_gpu_configs import MODES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEG = cc.SEG


def _of(mode):
    cs = [c for c in cc.all_cases() if c[4] == mode]
    return pytest.mark.parametrize('case', cs, ids=[c[0] for c in cs])


@pytest.fixture(scope='module')
def golden_collisions():
    with open(os.path.join(HERE, 'golden/collisions.json')) as f:
        return json.load(f)['cases']


@pytest.fixture(scope='module')
def ctxs():
    from wanproxy_amd.xcgpu import Context
    c = {False: Context(0), True: Context(0, out_of_band=True)}
    yield c
    for v in c.values():
        v.close()


@pytest.fixture(scope='module')
def expected(oracle):
    """Oracle and model runs of a case, computed once per case."""
    memo = {}

    def get(case):
        if case[0] not in memo:
            memo[case[0]] = (cc.oracle_case(oracle, case), cc.model_case(case))
        return memo[case[0]]
    return get


@pytest.fixture(params=[0, 2], ids=['screen_off', 'screen_on'])
def screen(request):
    from wanproxy_amd.xcgpu import lib
    old = lib().xcg_debug_set_screen(request.param)
    yield request.param
    lib().xcg_debug_set_screen(old)


@pytest.fixture(params=sorted(MODES))
def filter_mode(request):
    from wanproxy_amd.xcgpu import lib
    old = lib().xcg_debug_set_lds_filter_keys(MODES[request.param][0])
    oldp = lib().xcg_debug_set_lds_prefilter_keys(MODES[request.param][1])
    yield request.param
    lib().xcg_debug_set_lds_filter_keys(old)
    lib().xcg_debug_set_lds_prefilter_keys(oldp)


def _against_golden(golden, name, got):
    g = golden.get(name)
    if g is None:
        return None
    assert [len(o) for o in got] == g['lens'], name
    assert [hashlib.sha256(o).hexdigest()[:32] for o in got] == g['chunk_sha256'], name
    return g


def _oracle_decodes(oracle, encs, plain, shared):
    """Each encoding decodes to its chunk: on one cache (a stream) or on a
    fresh one per chunk."""
    c = oracle.cache_new() if shared else None
    for e, p in zip(encs, plain):
        ci = c if shared else oracle.cache_new()
        ok, back, cons, unk = oracle.decode(e, ci)
        if not shared:
            oracle.cache_free(ci)
        assert ok and not unk and cons == len(e) and back == p
    if shared:
        oracle.cache_free(c)


@_of('independent')
@pytest.mark.parametrize('mis', [0, 7])
def test_independent(ctxs, oracle, expected, golden_collisions, case, mis):
    """One launch per case, from a tensor `mis` bytes off 16-byte alignment
    whose last chunk ends at the allocation's last byte.  The chunks sit at
    in-tensor offsets 0 and 9 mod 16 in turn: with mis 0 the even ones start
    16-byte aligned in memory, with mis 7 the odd ones do (absolute
    misalignments 0, 9 and 7, 0), so every geometry runs both on the piece
    grid its name describes and off it."""
    import torch
    name, data, offs, lens, _, kw = case
    ctx = ctxs[kw['oob']]
    dev = torch.device('cuda', 0)
    n = offs.size
    assert int(offs[-1]) + int(lens[-1]) == data.size
    big = torch.zeros(mis + data.size, dtype=torch.uint8, device=dev)
    big[mis:] = torch.from_numpy(data.copy()).to(dev)
    d_in = big[mis:]
    assert d_in.data_ptr() % 16 == mis
    bounds = 2 * lens.astype(np.uint64) + 16
    oo = np.zeros(n, np.uint64)
    oo[1:] = np.cumsum(bounds)[:-1]
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_oo = torch.from_numpy(oo.view(np.int64)).to(dev)
    d_out = torch.zeros(int(bounds.sum()), dtype=torch.uint8, device=dev)
    d_ol = torch.zeros(n, dtype=torch.int64, device=dev)
    d_st = torch.zeros(4 * n, dtype=torch.int32, device=dev)
    assert (int(lens.max()) > 131072) == kw['large']          # (the launch's kernel class)
    ctx.encode_batch_device(d_in, d_off, d_len, n, int(lens.max()), d_out, d_oo, d_ol, d_st)
    torch.cuda.synchronize(dev)
    ctx.status()
    out = d_out.cpu().numpy()
    ol = d_ol.cpu().numpy()
    st = d_st.cpu().numpy().view(np.uint32).reshape(n, 4)
    (exp, _, _), model = expected(case)
    got = [out[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes() for i in range(n)]
    assert [int(v) for v in ol] == [len(e) for e in exp], name
    bad = [kw['geoms'][i] for i in range(n) if got[i] != exp[i]]
    assert not bad, (name, mis, bad)
    _against_golden(golden_collisions, name, got)
    counts = [tuple(int(v) for v in st[i, :3]) for i in range(n)]
    assert counts == [m[1] for m in model], (name, mis)
    if kw['tier'] == 'full':
        assert all(c[2] >= 1 for c in counts)
    if kw['oob']:
        return                              # (the declared segments travel out of band: nothing to decode from)
    plain = cc.chunks_of_case(case)
    _oracle_decodes(oracle, got, plain, shared=False)
    outs, dst, cons, _ = ctx.decode_chunks_independent(got)
    ctx.status()
    assert (dst == 0).all() and [int(c) for c in cons] == [len(g) for g in got], (name, dst)
    assert outs == plain, name


def _run_calls(ctx, oracle, case, golden, exp=None):
    """The case's calls on `ctx`; output bytes against the oracle and the
    golden file, cache_size() (a pair: its disk counters) after each call
    against the oracle's."""
    from wanproxy_amd.xcgpu import XCG_SEM_STREAM
    name, data, offs, lens, mode, kw = case
    exp, sizes, est = exp or cc.oracle_case(oracle, case)
    got, a = [], 0
    for k, m in enumerate(kw['calls']):
        got += ctx.encode_chunks(data, offs[a:a + m], lens[a:a + m], semantics=XCG_SEM_STREAM)
        a += m
        assert (ctx.pair_stats()[1:3] if mode == 'pair' else ctx.cache_size()) == sizes[k], (name, k)
    bad = [i for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, (name, bad, ctx.last_rounds())
    g = _against_golden(golden, name, got)
    return got, est, g


def _stream_round_trip(oracle, case, got):
    from wanproxy_amd.xcgpu import Context
    plain = cc.chunks_of_case(case)
    _oracle_decodes(oracle, got, plain, shared=True)
    dctx = Context(0, cache_segments=1 << 10)
    try:
        outs, st, cons, unk = dctx.decode_chunks(got)
    finally:
        dctx.close()
    assert (st == 0).all() and not unk and [int(c) for c in cons] == [len(g) for g in got], case[0]
    assert outs == plain, case[0]


@_of('stream')
def test_stream(oracle, expected, golden_collisions, stream_seed, case):
    from wanproxy_amd.xcgpu import Context
    ctx = Context(0, cache_segments=1 << 10)
    try:
        got, _, _ = _run_calls(ctx, oracle, case, golden_collisions, expected(case)[0])
    finally:
        ctx.close()
    _stream_round_trip(oracle, case, got)


_ROUND = [c for c in cc.all_cases() if c[5].get('round_view')]


@pytest.mark.parametrize('case', _ROUND, ids=[c[0] for c in _ROUND])
def test_stream_round_dependent_modes(oracle, expected, golden_collisions, stream_seed, screen, filter_mode, case):
    """A collision that only exists at the rounds' fixed point, and one that
    only exists before it, with the quiet-chunk screen off and on and every
    lane-filter mode forced."""
    from wanproxy_amd.xcgpu import Context
    ctx = Context(0, cache_segments=1 << 10)
    try:
        _run_calls(ctx, oracle, case, golden_collisions, expected(case)[0])
    finally:
        ctx.close()


@_of('lru')
def test_lru(oracle, expected, golden_collisions, stream_seed, case):
    from wanproxy_amd.xcgpu import Context
    ctx = Context(0, memory_cache_limit=case[5]['limit'])
    try:
        _run_calls(ctx, oracle, case, golden_collisions, expected(case)[0])
        assert ctx.cache_size() == cc.LRU_LIMIT
    finally:
        ctx.close()


@_of('pair')
def test_pair(oracle, expected, golden_collisions, stream_seed, case):
    from wanproxy_amd.xcgpu import Context
    kw = case[5]
    ctx = Context(0, memory_cache_limit=kw['limit'], disk_bytes=kw['disk'])
    try:
        _, est, g = _run_calls(ctx, oracle, case, golden_collisions, expected(case)[0])
        st = ctx.pair_stats()
    finally:
        ctx.close()
    assert (st[1], st[2]) == est, case[0]
    assert (st[1], st[2]) == (g['disk_entries'], g['disk_written']), case[0]
