"""GPU decode of <BACKREF> ops on bounded and pair contexts (and an unbounded
one as a control) against the yardstick of tests/backref_bounded_cases.py, which
tests/test_backref_bounded_cases.py pins to the compiled reference: outputs,
statuses, consumed bytes and unknown hashes of every call, the window slot by
slot, and the cache -- the bounded cache's export (size and LRU order), the
pair's disk counters, and the follow-up decodes the cases end with.  No case
may be declined: a call that returns XCG_ENOTSUP raises and fails its test."""
import ctypes as C
import os

import numpy as np
import pytest

import backref_bounded_cases as BB
from decode_windows_cases import B, X, probe_window

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def cases(oracle):
    return {c['name']: c for c in BB.all_cases(oracle)}


def make_ctx(kind):
    from wanproxy_amd.xcgpu import Context
    if kind == 'bounded':
        return Context(0, memory_cache_limit=BB.LIMIT)
    if kind == 'pair':
        return Context(0, memory_cache_limit=BB.LIMIT, disk_bytes=BB.DISK)
    return Context(0, cache_segments=1 << 12)


def account(ctx, kind):
    """What run_model's last entry holds, from the context."""
    if kind == 'pair':
        st = ctx.pair_stats()
        return {'pair_stats': (st[1], st[2]), 'order': None}
    return {'pair_stats': None, 'order': [int(h) for h in ctx.cache_export()[0]] if kind == 'bounded' else None}


def batch_result(n, outs, st, cons, unk):
    st = [int(s) for s in st]
    return {'outs': list(outs) + [b''] * (n - len(st)), 'status': st + [2] * (n - len(st)),
            'consumed': [int(c) for c in cons] + [0] * (n - len(st)), 'unknown': sorted(unk) if 1 in st else []}


def run_gpu(case, kind, split, decode=None):
    """run_model's steps on a context of `kind`.  decode(ctx, chunks, window)
    -> (outs, status, consumed, unknown): Context.decode_chunks by default."""
    from wanproxy_amd.xcgpu import Window
    decode = decode or (lambda ctx, chunks, window: ctx.decode_chunks(chunks, window=window))
    ctx = make_ctx(kind)
    win, learner = Window(ctx), Window(ctx)
    results, dead = [], False
    try:
        for step in case['steps']:
            if step[0] == 'decoder':
                win.close()
                win = Window(ctx)
                dead = False
                results.append(None)
            elif step[0] == 'batch' and dead:
                results.append(None)
            elif step[0] == 'learn':                 # (decoders of their own: the case's window does not move)
                for a in range(0, len(step[1]), 32):
                    _, st, _, _ = ctx.decode_chunks([X(s) for s in step[1][a:a + 32]], window=learner)
                    assert not st.any()
                results.append(None)
            elif step[0] == 'probe':
                def decode1(chunk):
                    outs, st, cons, _ = decode(ctx, [chunk], win)
                    return int(st[0]), outs[0], int(cons[0])
                results.append(probe_window(decode1))
            else:
                chunks = step[1]
                if not split:
                    r = batch_result(len(chunks), *decode(ctx, chunks, win))
                else:
                    outs, st, cons, unk = [], [], [], []
                    for e in chunks:
                        o, s, c, unk = decode(ctx, [e], win)
                        outs += o
                        st.append(int(s[0]))
                        cons.append(int(c[0]))
                        if st[-1] in (1, -1):
                            break
                    r = batch_result(len(chunks), outs, st, cons, unk)
                dead = -1 in r['status']
                results.append(r)
        results.append(account(ctx, kind))
    finally:
        win.close()
        learner.close()
        ctx.close()
    return results


def check(got, want, name):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, dict) and 'outs' in w:
            for key in ('status', 'consumed', 'unknown'):
                assert g[key] == w[key], (name, k, key, g[key], w[key])
            for i, (a, b) in enumerate(zip(g['outs'], w['outs'])):
                assert a == b, (name, k, 'output of chunk', i, len(a), len(b))
        else:
            assert g == w, (name, k)


CASE_NAMES = [f.__name__[5:] for f in BB.BUILDERS]


@pytest.mark.parametrize('split', [False, True], ids=['batch', 'chunk'])
@pytest.mark.parametrize('kind', BB.KINDS)
@pytest.mark.parametrize('name', CASE_NAMES)
def test_case(oracle, cases, name, kind, split):
    case = cases[name]
    check(run_gpu(case, kind, split), BB.run_model(oracle, case, kind, split=split), (name, kind, split))


@pytest.mark.parametrize('batch', BB.FUZZ_BATCHES)
@pytest.mark.parametrize('bad', BB.FUZZ_BAD)
@pytest.mark.parametrize('rate', BB.FUZZ_RATES)
@pytest.mark.parametrize('kind', BB.KINDS)
def test_fuzz(oracle, kind, rate, bad, batch):
    """(Chunk by chunk is the batch = 1 case: the streams do not depend on the batching.)"""
    case = BB.fuzz_case(oracle, rate, bad, batch)
    check(run_gpu(case, kind, False), BB.run_model(oracle, case, kind), (case['name'], kind))


# ------------------------------------------------------- other entry points

def decode_host(ctx, chunks, window):
    """xcg_decode_host: the batch from and to host memory."""
    from wanproxy_amd.xcgpu import XCG_EOVERFLOW, _check, lib
    L = lib()
    vp = C.c_void_p
    L.xcg_decode_host.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, C.c_uint64, vp, vp, vp, vp, vp,
                                  C.c_uint32, vp]
    L.xcg_decode_host.restype = C.c_int
    n = len(chunks)
    lens = np.array([len(e) for e in chunks], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
    blob = np.frombuffer(b''.join(chunks), dtype=np.uint8).copy()
    cap = (int(lens.sum()) // 3 + 1) * BB.SEG + int(lens.sum())
    out = np.zeros(cap, np.uint8)
    oo, ol, cons = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    st = np.zeros(n, np.int32)
    unk, nunk = np.zeros(4096, np.uint64), np.zeros(1, np.uint32)
    _check(L.xcg_decode_set_window(ctx.h, window.h))
    try:
        rc = L.xcg_decode_host(ctx.h, blob.ctypes.data, blob.size, offs.ctypes.data, lens.ctypes.data, n,
                               out.ctypes.data, cap, oo.ctypes.data, ol.ctypes.data, st.ctypes.data, cons.ctypes.data,
                               unk.ctypes.data, unk.size, nunk.ctypes.data)
        assert rc != XCG_EOVERFLOW
        _check(rc)
    finally:
        L.xcg_decode_set_window(ctx.h, None)
    outs = [out[int(oo[i]):int(oo[i] + ol[i])].tobytes() if st[i] != 2 else b'' for i in range(n)]
    return outs, st, cons, [int(u) for u in unk[:int(nunk[0])]]


def decode_call(ctx, chunks, window):
    """xcg_decode_call: one decode() from host memory."""
    from wanproxy_amd.xcgpu import _check, lib
    assert len(chunks) == 1
    e = chunks[0]
    _check(lib().xcg_decode_set_window(ctx.h, window.h))
    try:
        st, out, cons, unk, _ = ctx.decode_call(e, out_cap=(len(e) // 3 + 1) * BB.SEG + len(e))
    finally:
        lib().xcg_decode_set_window(ctx.h, None)
    return [out], np.array([st]), np.array([cons]), unk


@pytest.mark.parametrize('kind', ['bounded', 'pair'])
@pytest.mark.parametrize('name', ['evicted_in_batch', 'both_stops_bref_then_ref'])
def test_decode_host(oracle, cases, name, kind):
    check(run_gpu(cases[name], kind, False, decode_host), BB.run_model(oracle, cases[name], kind), (name, kind))


@pytest.mark.parametrize('kind', ['bounded', 'pair'])
@pytest.mark.parametrize('name', ['ghit_then_evicted', 'error_stop_no_skim'])
def test_decode_call(oracle, cases, name, kind):
    check(run_gpu(cases[name], kind, True, decode_call), BB.run_model(oracle, cases[name], kind, split=True), (name, kind))


def test_decoder_mirror_on_a_bounded_context(oracle):
    """XCodecDecoder (one decode() a call, its own window) over a fuzz stream."""
    from wanproxy_amd.xcgpu import XCodecDecoder
    case = BB.fuzz_case(oracle, 0.3, 0.0, 1)
    chunks = [step[1][0] for step in case['steps'][:8] if step[0] == 'batch']
    ctx = make_ctx('bounded')
    cache = BB.new_cache(oracle, 'bounded')
    dec, odec = XCodecDecoder(ctx), oracle.decoder_new(cache)
    try:
        for k, e in enumerate(chunks):
            assert dec.decode(e) == oracle.decode(e, cache, decoder=odec), k
    finally:
        oracle.decoder_free(odec)
        oracle.cache_free(cache)
        ctx.close()


@pytest.mark.parametrize('kind', ['bounded', 'pair'])
def test_refused_name_reuse_with_a_backref_changes_nothing(oracle, kind):
    """Two EXTRACTs of one hash with different bytes in one batch are still
    declined on these contexts (status bit 9), BACKREFs or not: XCG_ENOTSUP,
    and the cache, the window and later results are what they were."""
    from wanproxy_amd.xcgpu import Window, XCGError
    fa, fb = BB.family(0x77)[:2]
    s = BB.rnd_segs(0x77, 3)
    ctx = make_ctx(kind)
    win = Window(ctx)
    try:
        outs, st, _, _ = ctx.decode_chunks([X(s[0]) + X(s[1]) + B(1)], window=win)
        assert not st.any() and outs[0] == s[0] + s[1] + s[1]
        before = account(ctx, kind), ctx.cache_size()
        with pytest.raises(XCGError, match=r'\(-95\)'):
            ctx.decode_chunks([X(fa) + B(2) + B(0), X(s[2]) + X(fb) + B(1)], window=win)
        assert (account(ctx, kind), ctx.cache_size()) == before
        outs, st, cons, unk = ctx.decode_chunks([B(0) + B(1) + B(2)], window=win)     # (slot 2 was never written)
        assert [int(v) for v in st] == [-1] and outs[0] == s[0] + s[1] and int(cons[0]) == 9
    finally:
        win.close()
        ctx.close()


# ------------------------------------------------------------------ drop-in

@pytest.fixture(scope='module')
def dropin():
    if not os.path.exists(os.path.join(ROOT, 'oracle/_ref/libxcdropin.so')):
        pytest.skip('drop-in harness not built (needs the reference sources at build time)')
    from oracle.lib import Oracle
    return Oracle(dropin=True)


@pytest.mark.parametrize('kind', ['bounded', 'pair'])
def test_dropin_connected_caches_like_reference(dropin, ref_oracle, kind):
    """libxcdropin (the reference's classes over the engine) against libxcref,
    call by call, on the cache XCodecCache::connect makes for a peer -- bounded
    with the parent's limit, or a pair of connected levels: one stream with
    BACKREFs (some to empty slots: decode() false, and the next call goes on),
    longer than the cache, so REFs to evicted segments ask."""
    from backref_streams import stream_with_backrefs
    from wanproxy_amd import synth
    from test_gpu_pair_decode import uuid
    data = synth.stream(0xD0B, 12 * 16384, 60, 1)
    frames = stream_with_backrefs(ref_oracle, data, 16384, 0xD0B, 0.3, 0.02)
    u = uuid()
    res = []
    for o in (ref_oracle, dropin):
        parent = BB.new_cache(o, kind)
        conn = o.cache_connect(parent, u)
        dec = o.decoder_new(conn)
        calls = [o.decode(f, conn, decoder=dec) for f in frames]
        if kind == 'pair':
            calls.append(o.pair_stats(conn))
        o.decoder_free(dec)
        res.append(calls)
    for k, (a, b) in enumerate(zip(*res)):
        assert a == b, (kind, k)
    assert any(len(c[1]) > 16384 for c in res[0][:len(frames)]), 'no BACKREF decoded: the case tests nothing'


# --------------------------------------------------------------------- pipe

def test_pipe_on_a_bounded_decoder_context_like_reference():
    """FRAMEs whose payloads hold BACKREFs, to a pipe pair whose codec (and so
    the decoder cache connected at <HELLO>) is bounded: the first declares A,
    the second evicts it, decodes a BACKREF to A's slot and asks for the REF to
    A behind it; a FRAME with a BACKREF to an empty slot is decoder_error on
    the reference's XCodecPipePair and XCG_EPROTO on the engine's."""
    import pipe_cases as pc
    from oracle import refpipe
    from oracle.lib import Oracle
    if not refpipe.available('ref'):
        pytest.skip('oracle/_ref/libppref.so not built (needs the reference tree)')
    o = Oracle()
    b = BB.Builder(o, 1)
    s = BB.rnd_segs(0xF1FE, 80)
    talks = [[pc.hello(pc.UUID_B) + pc.frame(BB.LIT + b.x(0, s[0]) + BB.slot(b, s[0]) + BB.xs(b, s[1:31])),
              pc.frame(BB.xs(b, s[31:67]) + BB.slot(b, s[0]) + BB.slot(b, s[40]) + BB.LIT + b.r(0, s[0]) + BB.slot(b, s[0]))],
             [pc.hello(pc.UUID_B) + pc.frame(b'abc' + X(s[70]) + B(0)), pc.frame(B(0) + B(200) + X(s[71]))]]
    got = []
    for impl in (pc.RefImpl('ref'), pc.EngineImpl()):
        res = []
        for wires in talks:
            impl.reset()
            codec = impl.codec(pc.UUID_A, BB.LIMIT)
            pair = codec.pair()
            res += [pair.consume('dec', w) for w in wires]
            pair.close()
            codec.close()
        impl.reset()
        got.append(res)
    ref, eng = got
    for k, (r, e) in enumerate(zip(ref, eng)):
        assert e == r, k
    lit = BB.LIT.replace(b'\xf1\x00', b'\xf1')
    assert ref[0].to_local.count(s[0]) == 2 and ref[1].to_local.endswith(s[0] + s[40] + lit)
    assert pc.ask([o.hash(s[0])]) in ref[1].to_peer
    assert ref[2].to_local == b'abc' + s[70] + s[70] and ref[3] == pc.FAILED
