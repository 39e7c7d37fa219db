"""xcg_decode_batch_independent on the GPU: chunk i is one XCodecDecoder::decode
call on a decoder made for that chunk alone (an empty cache, an empty window),
n chunks in one asynchronous launch into caller-supplied slots.  Expected
values: tests/indep_decode_cases.py (the oracle on a fresh cache per chunk;
test_indep_decode_cases.py holds them against the compiled reference)."""
import ctypes as C
import gc

import numpy as np
import pytest

import indep_decode_cases as idc
from backref_streams import split_ops
from indep_decode_cases import BR, E, R, expect

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture
def ctx():
    from wanproxy_amd.xcgpu import Context
    c = Context(0, cache_segments=1 << 12)
    yield c
    c.status()
    c.close()


class Batch:
    """Device buffers of one raw launch: the chunks packed at odd offsets, the
    output slots (caps[i] bytes each) at odd offsets -- or adjacent, from an odd
    base -- in a buffer filled with 0xA5."""

    def __init__(self, encs, caps, adjacent=False):
        import torch
        self.dev = torch.device('cuda', 0)
        self.encs, self.n = encs, len(encs)
        self.lens = np.array([len(e) for e in encs], np.uint32)
        self.caps = np.array(caps, np.uint64)
        self.offs, self.oo = np.zeros(self.n, np.uint64), np.zeros(self.n, np.uint64)
        pos, opos = 1, 1
        blob = bytearray(b'\xf1')                     # (bytes between the chunks that no chunk may read as its own)
        for i, e in enumerate(encs):
            pad = (pos | 1) - pos
            blob += b'\xf1' * pad + e
            self.offs[i] = pos + pad
            pos += pad + len(e)
            if not adjacent:
                opos |= 1
            self.oo[i] = opos
            opos += int(self.caps[i])
        blob += b'\xf1\x01'
        self.total = opos + 64
        t = lambda a, v: torch.from_numpy(a.view(v)).to(self.dev)   # noqa: E731
        self.d_in = torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).to(self.dev)
        self.d_off, self.d_len = t(self.offs, np.int64), t(self.lens, np.int32)
        self.d_oo, self.d_cap = t(self.oo, np.int64), t(self.caps, np.int64)
        self.d_out = torch.full((self.total,), FILL, dtype=torch.uint8, device=self.dev)
        self.d_ol = torch.full((self.n,), -7, dtype=torch.int64, device=self.dev)
        self.d_st = torch.full((self.n,), -7, dtype=torch.int32, device=self.dev)
        self.d_cons = torch.full((self.n,), -7, dtype=torch.int64, device=self.dev)
        self.d_unk = torch.full((self.n,), -7, dtype=torch.int64, device=self.dev)

    def launch(self, ctx, max_len=None, stream=None, unknown=True):
        ctx.decode_batch_independent_device(
            self.d_in, self.d_off, self.d_len, self.n, int(self.lens.max()) if max_len is None else max_len,
            self.d_out, self.d_oo, self.d_cap, self.d_ol, self.d_st, self.d_cons,
            self.d_unk if unknown else None, stream=stream)

    def results(self):
        """Per chunk (status, stored bytes, consumed, first_unknown, out_len), after
        checking that no byte outside a chunk's min(cap, out_len) range changed."""
        out = self.d_out.cpu().numpy()
        ol = self.d_ol.cpu().numpy().view(np.uint64)
        st, cons = self.d_st.cpu().numpy(), self.d_cons.cpu().numpy().view(np.uint64)
        unk = self.d_unk.cpu().numpy().view(np.uint64)
        untouched = np.ones(self.total, bool)
        res = []
        for i in range(self.n):
            k = int(min(self.caps[i], ol[i]))
            untouched[int(self.oo[i]):int(self.oo[i]) + k] = False
            res.append((int(st[i]), out[int(self.oo[i]):int(self.oo[i]) + k].tobytes(), int(cons[i]), int(unk[i]),
                        int(ol[i])))
        assert (out[untouched] == FILL).all(), np.flatnonzero(untouched & (out != FILL))[:8]
        return res


def run(ctx, encs, caps=None, adjacent=False, max_len=None):
    import torch
    b = Batch(encs, [len(e) * 205 + 4096 for e in encs] if caps is None else caps, adjacent)
    b.launch(ctx, max_len)
    torch.cuda.synchronize()
    return b.results()


def check(ctx, oracle, encs, **kw):
    """Every chunk as the oracle decodes it on a fresh cache and decoder."""
    got = run(ctx, encs, **kw)
    exp = [expect(oracle, e) for e in encs]
    for i, (g, x) in enumerate(zip(got, exp)):
        assert (g[0], g[2], g[3], g[4]) == (x[0], x[2], x[3], len(x[1])), (i, g[0], g[2], g[3], g[4], x[0], x[2], x[3])
        assert g[1] == x[1], i
    return got


def mem_live():
    from wanproxy_amd.xcgpu import lib
    gc.collect()
    out = (C.c_uint64 * 4)()
    lib().xcg_debug_mem_live.restype = None
    lib().xcg_debug_mem_live.argtypes = [C.c_void_p]
    lib().xcg_debug_mem_live(out)
    return tuple(int(v) for v in out)


# ------------------------------------------------------------------ 1 round trip

@pytest.mark.parametrize('name', ['kat_a', 'magic_heavy'])
def test_round_trip_of_the_gpu_encoder(ctx, name):
    from wanproxy_amd.synth import chunks_of
    from wanproxy_amd.xcgpu import Context
    d = idc.data(name)
    offs, lens = chunks_of(d, 65536)
    offs, lens = offs[:4], lens[:4]
    plain = [d[int(o):int(o) + int(k)] for o, k in zip(offs, lens)]
    encs = ctx.encode_chunks(d, offs, lens)                       # independent semantics
    for n in (1, 3, 4, 5):                                        # (5: a second workgroup with one chunk)
        pick = [k % len(encs) for k in range(n)]
        got = run(ctx, [encs[k] for k in pick], caps=[len(plain[k]) + 9 for k in pick])
        for g, k in zip(got, pick):
            assert (g[0], g[2], g[3]) == (0, len(encs[k]), 0) and g[1] == plain[k], (n, k, g[0], g[2])
    for k, e in enumerate(encs):                                  # the stream decoder on a fresh context agrees
        c = Context(0, cache_segments=1 << 10)
        outs, st, cons, unk = c.decode_chunks([e])
        c.close()
        assert (outs[0], int(st[0]), int(cons[0]), unk) == (plain[k], 0, len(e), [])


# ------------------------------------------------------------------ 2 isolation

def test_chunks_and_context_are_isolated(ctx, oracle):
    import torch
    from wanproxy_amd import synth
    from wanproxy_amd.xcgpu import XCG_SEM_STREAM, Context
    # a stream on the context: half decoded before the call, half after it
    d = synth.stream(0x5eed, 4 * 65536, 50, 2)
    offs, lens = synth.chunks_of(d, 65536)
    ectx = Context(0, cache_segments=1 << 12)
    senc = ectx.encode_chunks(d, offs, lens, semantics=XCG_SEM_STREAM)
    ectx.close()
    assert sum(e.count(b'\xf1\x02') for e in senc[2:]) > 0
    W = idc.seg_of(40)
    first, st, _, unk = ctx.decode_chunks(senc[:2] + [E(W)])
    assert not st.any() and not unk
    ndecl = sum(kind != 'lit' for e in senc[:2] for kind, _ in split_ops(e)) + 1
    slot_w = (ndecl - 1) % 256                                    # the window slot E(W), the last declare, took
    size0, live0 = ctx.cache_size(), mem_live()
    assert size0 > 0

    chunks, h = idc.isolation(oracle)
    S = idc.seg_of(1)
    b = Batch(chunks, [4096 + 9] * 3)
    b.launch(ctx)
    torch.cuda.synchronize()
    assert mem_live() == live0                                    # no allocation
    got = b.results()
    assert [g[:4] for g in got] == [(0, S, 2050, 0), (1, b'ab', 2, h), (0, S + S, 2060, 0)]
    assert [g[:4] for g in got] == [expect(oracle, c) for c in chunks]
    assert ctx.cache_size() == size0                              # E(S) entered nothing
    # the cache and the window are as the stream left them
    outs, st, cons, unk = ctx.decode_chunks([BR(slot_w)] + senc[2:])
    assert outs[0] == W and b''.join(first[:2] + outs[1:]) == d and not st.any() and not unk
    # ... and hash(S) never reached the context's cache
    outs, st, cons, unk = ctx.decode_chunks([R(h)])
    assert int(st[0]) == 1 and unk == [h]


# ------------------------------------------------------------------ 3 errors

def test_errors_do_not_spread(ctx, oracle):
    c = idc.error_chunks(oracle)
    got = check(ctx, oracle, [c['good'], c['bad_opcode'], c['good'], c['lone_f1'], c['good']])
    assert [g[0] for g in got] == [0, -1, 0, 3, 0]
    assert got[1][1:3] == (b'xy', 2) and got[3][1:3] == (b'xy', 2)
    names = ['extract_cut', 'ref_cut', 'backref_cut', 'op_byte_only_after_extract', 'backref_empty',
             'backref_empty_after_declares']
    got = check(ctx, oracle, [c[k] for k in names])
    assert [g[0] for g in got] == [3, 3, 3, 3, -1, -1]
    assert got[4][1:3] == (b'xy', 5)                              # consumed past the BACKREF op


# ------------------------------------------------------------------ 4 literals

def test_literal_edges(ctx, oracle):
    c = idc.literal_edges(oracle)
    got = check(ctx, oracle, list(c.values()))
    assert [g[0] for g in got] == [1 if k == 'esc_then_op_at_1024' else 0 for k in c]


# ------------------------------------------------------------------ 5 REF order, name reuse

def test_ref_order_and_name_reuse(ctx, oracle):
    table = idc.reuse_table(oracle)
    encs = [idc.ref_order(oracle)] + [v[0] for v in table.values()]
    got = check(ctx, oracle, encs)
    assert got[0][0] == 1 and got[0][1] == b'head' and got[0][2] == 4
    for g, (k, (_, (st, out, cons))) in zip(got[1:], table.items()):
        assert (g[0], g[1], g[2]) == (st, out, cons), k


# ------------------------------------------------------------------ 6 window

def test_window(ctx, oracle):
    c = idc.window_chunks(oracle)
    got = check(ctx, oracle, list(c.values()))
    st = dict(zip(c, (g[0] for g in got)))
    assert st['valid0'] == st['valid1'] == st['valid2'] == 0 and st['wrap_live'] == 0 and st['wrap_emptied'] == -1


# ------------------------------------------------------------------ 7 largest class

def test_largest_class(ctx, oracle):
    from wanproxy_amd.xcgpu import XCGError
    big, need = idc.largest_chunk(oracle)
    _, small = idc.independent_encodings(oracle, 'kat_a', limit=1)
    xb = expect(oracle, big, out_cap=need + 4096)
    xs = expect(oracle, small[0])
    assert xb[0] == 0 and len(xb[1]) == need
    for encs, exp in (([big, small[0]], [xb, xs]), ([small[0], big, small[0]], [xs, xb, xs])):
        got = run(ctx, encs, caps=[len(x[1]) + 1 for x in exp], max_len=idc.CAP)
        for g, x in zip(got, exp):
            assert (g[0], g[2], g[3], g[4]) == (x[0], x[2], x[3], len(x[1])) and g[1] == x[1]
    with pytest.raises(XCGError, match=r'\(-22\)'):
        Batch([small[0]], [70000]).launch(ctx, max_len=idc.CAP + 1)


# ------------------------------------------------------------------ 8 slot too small

def test_slot_too_small(ctx, oracle):
    from wanproxy_amd.xcgpu import XCG_CHUNK_NOROOM
    S, T = idc.seg_of(50), idc.seg_of(51)
    h = oracle.hash(S)
    enc = b'abc' + E(S) + idc.LIT(b'mid\xf1dle') + R(h) + BR(1) + b'end'
    blocked = b'ab' + R(oracle.hash(T)) + b'cd'
    st, out, cons, _ = expect(oracle, enc)
    need = len(out)
    assert (st, cons) == (0, len(enc)) and need == 3 + 2048 + 7 + 2048 + 2048 + 3
    caps = [need - 1, 0, need, 1]
    got = run(ctx, [enc, enc, enc, blocked], caps=caps, adjacent=True)   # (results(): nothing outside the slots)
    assert [g[0] for g in got] == [XCG_CHUNK_NOROOM, XCG_CHUNK_NOROOM, 0, XCG_CHUNK_NOROOM]
    assert [g[4] for g in got] == [need, need, need, 2]
    assert [g[2] for g in got] == [len(enc)] * 3 + [2]            # consumed / first_unknown as if decoded
    assert [g[3] for g in got] == [0, 0, 0, oracle.hash(T)]
    assert got[2][1] == out
    outs, st, cons, unk = ctx.decode_chunks_independent([enc, enc, enc, blocked], out_caps=caps)
    assert outs == [out, out, out, b'ab'] and list(st) == [0, 0, 0, 1]
    assert list(cons) == [len(enc)] * 3 + [2] and list(unk) == [0, 0, 0, oracle.hash(T)]
    # the default slots need no retry
    outs, st, cons, unk = ctx.decode_chunks_independent([blocked, enc])
    assert outs == [b'ab', out] and list(st) == [1, 0]


# ------------------------------------------------------------------ 9 context types

def test_context_types(oracle):
    from wanproxy_amd.xcgpu import Context, XCGError
    plain, encs = idc.independent_encodings(oracle, 'kat_a', limit=2)
    assert max(map(len, encs)) // 2050 > 2
    bounded = Context(0, memory_cache_limit=64 * 2048)            # 64 segments >= the 63 EXTRACTs a chunk can hold
    outs, st, cons, unk = bounded.decode_chunks_independent(encs)
    assert outs == plain and not st.any()
    bounded.close()
    tiny = Context(0, memory_cache_limit=2 * 2048)
    with pytest.raises(XCGError, match=r'\(-95\)'):
        tiny.decode_chunks_independent(encs)
    assert tiny.decode_chunks_independent([b'lit' + E(plain[0][:2048])])[0] == [b'lit' + plain[0][:2048]]
    tiny.close()
    for kw in (dict(out_of_band=True), dict(null_cache=True)):
        c = Context(0, cache_segments=1 << 10, **kw)
        outs, st, cons, unk = c.decode_chunks_independent(encs)
        assert outs == plain and not st.any() and list(cons) == [len(e) for e in encs]
        c.status()
        c.close()


# ------------------------------------------------------------------ 10 asynchrony

def test_two_calls_queued_on_one_stream(ctx, oracle):
    import torch
    c = idc.error_chunks(oracle)
    plain, encs = idc.independent_encodings(oracle, 'magic_heavy', limit=3)
    a = Batch(encs + [c['bad_opcode']], [len(p) + 5 for p in plain] + [64])
    b = Batch([c['good'], c['lone_f1']] + encs[::-1], [8192, 64] + [len(p) for p in plain[::-1]])
    live0 = mem_live()
    s = torch.cuda.Stream(a.dev)
    s.wait_stream(torch.cuda.current_stream())
    a.launch(ctx, stream=s)
    b.launch(ctx, stream=s, unknown=False)
    assert ctx.decode_batch_independent_device(a.d_in, a.d_off, a.d_len, 0, 0, a.d_out, a.d_oo, a.d_cap, a.d_ol,
                                               a.d_st, a.d_cons, stream=s) is None    # n == 0: XCG_OK
    s.synchronize()
    assert mem_live() == live0
    ra, rb = a.results(), b.results()
    assert [g[1] for g in ra[:3]] == plain and [g[0] for g in ra] == [0, 0, 0, -1]
    assert [g[1] for g in rb[2:]] == plain[::-1] and [g[0] for g in rb] == [0, 3, 0, 0, 0]
    assert [g[3] for g in rb] == [2 ** 64 - 7] * 5                # a null d_first_unknown is left alone
    ctx.status()
