"""GPU decode of streams with <BACKREF> ops (XCodecWindow semantics,
xcodec/xcodec_decoder.cc:137,160,165-181, xcodec/xcodec_window.h) against the
reference decoder's results (tests/golden/backref.json) and the C oracle."""
import hashlib
import json
import os

import pytest

from wanproxy_amd import synth
from backref_streams import stream_with_backrefs

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'backref.json')))


def sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def streams(oracle, c):
    data = synth.stream(c['seed'], c['nbytes'], c['dup'], 0)
    encs = stream_with_backrefs(oracle, data, c['chunk'], c['seed'], c['rate'], c['bad'])
    assert sha(b''.join(encs)) == c['stream_sha256']
    return encs


def check_against_golden(c, outs, st, cons):
    calls = c['calls']
    for k, want in enumerate(calls):
        if want['ok']:
            assert int(st[k]) == 0, (c['name'], k, int(st[k]))
        else:
            assert int(st[k]) == -1, (c['name'], k, int(st[k]))
        assert int(cons[k]) == want['consumed'], (c['name'], k)
        assert len(outs[k]) == want['out_len'] and sha(outs[k]) == want['out_sha256'], (c['name'], k)
    for k in range(len(calls), len(st)):          # after decode() returned false
        assert int(st[k]) == 2, (c['name'], k)


@pytest.mark.parametrize('case', GOLDEN['cases'], ids=[c['name'] for c in GOLDEN['cases']])
def test_backref_one_batch(oracle, case):
    from wanproxy_amd.xcgpu import Context
    encs = streams(oracle, case)
    ctx = Context(0)
    outs, st, cons, unk = ctx.decode_chunks(encs)
    assert unk == []
    check_against_golden(case, outs, st, cons)


@pytest.mark.parametrize('case', GOLDEN['cases'], ids=[c['name'] for c in GOLDEN['cases']])
def test_backref_window_across_batches(oracle, case):
    """The window lives in the decoder, across xcg_decode_batch calls."""
    from wanproxy_amd.xcgpu import Context, Window
    encs = streams(oracle, case)
    ctx = Context(0)
    win = Window(ctx)
    outs, st, cons = [], [], []
    cuts = sorted({0, len(encs) // 3, len(encs) // 3 + 1, (2 * len(encs)) // 3, len(encs)})
    for a, b in zip(cuts, cuts[1:]):
        o, s, cn, _ = ctx.decode_chunks(encs[a:b], window=win)
        outs += o
        st += [int(v) for v in s]
        cons += [int(v) for v in cn]
        if min(st) < 0:
            break
    calls = case['calls']
    for k, want in enumerate(calls):
        if k >= len(st):
            break
        assert (st[k] == 0) == want['ok'] and cons[k] == want['consumed'], (case['name'], k)
        assert sha(outs[k]) == want['out_sha256'], (case['name'], k)


def test_backref_decoder_mirror_matches_oracle(oracle):
    """XCodecDecoder mirror (one decode() per call, own window) vs the C
    oracle's persistent decoder on more seeds."""
    from wanproxy_amd.xcgpu import Context, XCodecDecoder
    for seed in (21, 22, 23):
        data = synth.stream(seed, 1 << 19, 70, 1)
        encs = stream_with_backrefs(oracle, data, 16384, seed, 0.4, 0.03 if seed == 23 else 0.0)
        ctx = Context(0)
        dec = XCodecDecoder(ctx)
        cache = oracle.cache_new()
        odec = oracle.decoder_new(cache)
        try:
            for k, e in enumerate(encs):
                ok, out, cons, unk = dec.decode(e)
                wok, wout, wcons, wunk = oracle.decode(e, cache, decoder=odec)
                assert (ok, cons, unk) == (wok, wcons, wunk), (seed, k)
                assert out == wout, (seed, k)
                if not ok:
                    break
        finally:
            oracle.decoder_free(odec)
            oracle.cache_free(cache)


def test_backref_empty_window_is_an_error():
    """A BACKREF before any declare names an empty slot: decode() is false."""
    from wanproxy_amd.xcgpu import Context
    ctx = Context(0)
    outs, st, cons, _ = ctx.decode_chunks([b'abc\xf1\x03\x07tail', b'next'])
    assert int(st[0]) == -1 and int(cons[0]) == 6 and outs[0] == b'abc'
    assert int(st[1]) == 2


def test_backref_after_a_ref_run_longer_than_a_wave(oracle):
    """The declares a BACKREF sees are counted over runs of REFs: 70
    consecutive REFs (more than one wave's run of 64) against a warm cache,
    then BACKREFs into the run on both sides of lane 63; in the next chunk a
    BACKREF to a slot no declare has reached stops the stream in front of a
    truncated REF; a following batch reads the window that is left."""
    import struct

    import numpy as np
    from wanproxy_amd.xcgpu import Context
    segs = np.random.default_rng(0xB4C).integers(0, 256, 70 * 2048, dtype=np.uint8).tobytes()
    ctx = Context(0)
    hs = [int(h) for h in ctx.cache_learn(segs)]
    assert len(set(hs)) == 70
    ref = [b'\xf1\x02' + struct.pack('>Q', h) for h in hs]
    bref = lambda slot: b'\xf1\x03' + bytes([slot])
    encs = [b''.join(ref) + bref(2) + bref(68) + b'literal tail',
            ref[5] + ref[6] + bref(200) + ref[7][:6]]
    after = [bref(2) + bref(68)]
    cache = oracle.cache_new()
    odec = oracle.decoder_new(cache)
    try:
        # (warmed through a decoder of its own, so the one under test starts with an empty window)
        assert oracle.decode(b''.join(b'\xf1\x01' + segs[2048 * k:2048 * (k + 1)] for k in range(70)), cache)[0]
        want = [oracle.decode(e, cache, decoder=odec) for e in encs + after]
    finally:
        oracle.decoder_free(odec)
        oracle.cache_free(cache)
    assert [w[0] for w in want] == [True, False, True]       # (the reference's own verdicts)
    assert want[0][1] == segs + segs[2 * 2048:3 * 2048] + segs[68 * 2048:69 * 2048] + b'literal tail'
    outs, st, cons, unk = ctx.decode_chunks(encs)
    assert unk == []
    assert [int(s) for s in st] == [0, -1]
    for k in range(2):
        assert outs[k] == want[k][1] and int(cons[k]) == want[k][2], k
    outs, st, cons, unk = ctx.decode_chunks(after)
    assert unk == [] and int(st[0]) == 0
    assert outs[0] == want[2][1] and int(cons[0]) == want[2][2]
    assert outs[0] == segs[2 * 2048:3 * 2048] + segs[68 * 2048:69 * 2048]
    ctx.close()
