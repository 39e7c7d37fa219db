"""GPU tests of the encoder refmap (xcg_encode_refmap_batch and
xcg_encode_host_refmap): the (hash, input position) rows of every hash an
encode() call REF'd, first occurrence per hash, ascending by hash.  Expected
rows come from the plain walker of tests/refmap_cases.py over the oracle's
output (tests/test_refmap_cases.py pins it to the reference's own refmap) and,
where it is built, from the reference's encode(output, input, refmap) itself."""
import ctypes as C
import gc

import numpy as np
import pytest

import refmap_cases as rc
from collision_cases import PAIR_DISK, PAIR_LIMIT
from oracle.lib import MODE_INDEPENDENT, MODE_NULL
from test_refmap_cases import encode_batches, expected

pytestmark = pytest.mark.gpu
SEG = rc.SEG
CAP = rc.REFMAP_MAX
XCG_EINVAL, XCG_ENOTSUP = -22, -95
H_SENT, P_SENT, C_SENT, W_SENT = 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5, 0xC5C5C5C5, 0xD5D5D5D5D5D5D5D5
BOUNDED = 120 * SEG
KINDS = {'unbounded': dict(cache_segments=1 << 12), 'bounded': dict(memory_cache_limit=BOUNDED),
         'pair': dict(memory_cache_limit=PAIR_LIMIT * SEG, disk_bytes=PAIR_DISK)}


def pack(encs):
    """The encodings in one buffer at odd offsets, F1 02 bytes between and behind
    them: a walk that leaves its chunk finds a REF there."""
    blob, offs = bytearray(), []
    for e in encs:
        blob += b'\xf1\x02\xf1'
        if len(blob) % 2 == 0:
            blob += b'\x02'
        offs.append(len(blob))
        blob += e
    blob += b'\xf1\x02' * 8
    return bytes(blob), offs, [len(e) for e in encs]


def launch(ctx, blob, offs, lens, cap=CAP, max_len=None, first_chunk=0, walked=True, stream=None, rc_only=False):
    """xcg_encode_refmap_batch over sentinel-filled outputs.  Returns (count,
    hash [n, cap], pos [n, cap], walked) as numpy arrays, or the status."""
    import torch
    from wanproxy_amd.xcgpu import _stream_ptr, lib
    dev = torch.device('cuda', ctx.device)
    n = len(offs)

    def filled(k, v, dt):
        return torch.from_numpy(np.full(max(k, 1), v, dt).view({8: np.int64, 4: np.int32}[np.dtype(dt).itemsize])).to(dev)
    d_enc = torch.from_numpy(np.frombuffer(blob or b'\0', np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(np.array(offs or [0], np.uint64).view(np.int64)).to(dev)
    d_len = torch.from_numpy(np.array(lens or [0], np.uint64).view(np.int64)).to(dev)
    d_h, d_p = filled(n * cap, H_SENT, np.uint64), filled(n * cap, P_SENT, np.uint32)
    d_c, d_w = filled(n, C_SENT, np.uint32), filled(n, W_SENT, np.uint64)
    if max_len is None:
        max_len = max(lens) if lens else 0
    st = lib().xcg_encode_refmap_batch(
        ctx.h, C.c_void_p(d_enc.data_ptr()), C.c_void_p(d_off.data_ptr()), C.c_void_p(d_len.data_ptr()), n,
        int(max_len), int(first_chunk), C.c_void_p(d_h.data_ptr()), C.c_void_p(d_p.data_ptr()), int(cap),
        C.c_void_p(d_c.data_ptr()), C.c_void_p(d_w.data_ptr()) if walked else None, _stream_ptr(stream))
    torch.cuda.synchronize(dev)
    res = (d_c.cpu().numpy().view(np.uint32)[:n], d_h.cpu().numpy().view(np.uint64)[:n * cap].reshape(n, cap),
           d_p.cpu().numpy().view(np.uint32)[:n * cap].reshape(n, cap), d_w.cpu().numpy().view(np.uint64)[:n])
    if rc_only:
        return st, res
    assert st == 0, st
    return res


def check(res, exp, cap=CAP, walked=True):
    """res against [(entries, walked)] per chunk: the first min(count, cap)
    entries, nothing written past them."""
    cnt, hs, ps, wk = res
    assert [int(c) for c in cnt] == [len(e) for e, _ in exp]
    for i, (entries, w) in enumerate(exp):
        k = min(len(entries), cap)
        assert [(int(h), int(p)) for h, p in zip(hs[i, :k], ps[i, :k])] == entries[:k], i
        assert (hs[i, k:] == H_SENT).all() and (ps[i, k:] == P_SENT).all(), i
        assert int(wk[i]) == (w if walked else W_SENT), i


def host_call(ctx, parts, cap=CAP, semantics=1):
    """xcg_encode_host_refmap over sentinel-filled arrays: (encs, count, hash, pos)."""
    from wanproxy_amd.xcgpu import _check, lib
    d, offs, lens = rc.chunked(parts)
    n = len(parts)
    bounds = 2 * lens.astype(np.uint64) + 16
    oo = np.zeros(n, np.uint64)
    oo[1:] = np.cumsum(bounds)[:-1]
    out = np.zeros(int(bounds.sum()), np.uint8)
    ol = np.zeros(n, np.uint64)
    hs, ps = np.full(max(n * cap, 1), H_SENT, np.uint64), np.full(max(n * cap, 1), P_SENT, np.uint32)
    cn = np.full(n, C_SENT, np.uint32)
    src = np.ascontiguousarray(d) if d.size else np.zeros(1, np.uint8)
    _check(lib().xcg_encode_host_refmap(ctx.h, semantics, src.ctypes.data, d.size, offs.ctypes.data, lens.ctypes.data,
                                        n, out.ctypes.data, out.size, oo.ctypes.data, ol.ctypes.data,
                                        hs.ctypes.data, ps.ctypes.data, cap, cn.ctypes.data))
    encs = [out[int(oo[i]):int(oo[i] + ol[i])].tobytes() for i in range(n)]
    return encs, cn, hs[:n * cap].reshape(n, cap), ps[:n * cap].reshape(n, cap)


def oracle_cache(oracle, kind):
    if kind == 'pair':
        return oracle.cache_new_pair(PAIR_LIMIT * SEG, PAIR_DISK)
    return oracle.cache_new(BOUNDED if kind == 'bounded' else 0)


def mem_live():
    from wanproxy_amd.xcgpu import lib
    gc.collect()
    out = (C.c_uint64 * 4)()
    lib().xcg_debug_mem_live.restype = None
    lib().xcg_debug_mem_live.argtypes = [C.c_void_p]
    lib().xcg_debug_mem_live(out)
    return tuple(int(v) for v in out)


_EXPECTED = {}


def case_expectation(oracle, name, kind):
    """Per (case, context kind), once: per batch, per chunk (encoding, entries, walked)."""
    if (name, kind) not in _EXPECTED:
        c = oracle_cache(oracle, kind)
        _EXPECTED[name, kind] = expected(oracle, rc.stream_cases()[name][0], cache=c)
        oracle.cache_free(c)
    return _EXPECTED[name, kind]


# ------------------------------------------------------- the cases, end to end

@pytest.mark.parametrize('kind', sorted(KINDS))
@pytest.mark.parametrize('name', sorted(rc.stream_cases()))
def test_stream_cases(oracle, stream_seed, name, kind):
    """The host call gives the oracle's bytes and the walker's refmap, batch by
    batch on one context; the device call over the same bytes, packed at odd
    offsets, gives the same rows and walks every chunk to its end."""
    from wanproxy_amd.xcgpu import Context
    batches, _ = rc.stream_cases()[name]
    exp = case_expectation(oracle, name, kind)
    ctx = Context(0, **KINDS[kind])
    try:
        for parts, want in zip(batches, exp):
            d, offs, lens = rc.chunked(parts)
            encs, maps = ctx.encode_chunks_refmap(d, offs, lens)
            assert encs == [e for e, _, _ in want]
            for part, m, (_, entries, _) in zip(parts, maps, want):
                assert list(m.items()) == [(h, part[p:p + SEG]) for h, p in entries]
            blob, eo, el = pack(encs)
            check(launch(ctx, blob, eo, el), [(r, w) for _, r, w in want])
        ctx.status()
    finally:
        ctx.close()


def test_against_the_reference_encoder(ref_oracle):
    """XCodecEncoder.encode(data, refmap={}) call by call against the
    reference's encode(output, input, &refmap) on one persistent encoder: the
    cases, then a 1 MiB synthetic stream in 64 KiB calls."""
    from wanproxy_amd import synth
    from wanproxy_amd.xcgpu import Context, XCodecEncoder
    d = synth.stream(0x7EF, 1 << 20, 60, 2)
    d = d.tobytes() if isinstance(d, np.ndarray) else bytes(d)
    calls = [p for name in sorted(rc.stream_cases()) for b in rc.stream_cases()[name][0] for p in b if p]
    calls += [d[k:k + 65536] for k in range(0, len(d), 65536)]
    cache = ref_oracle.cache_new(0)
    renc = ref_oracle.encoder_new(cache)
    ctx = Context(0, cache_segments=1 << 12)
    try:
        enc = XCodecEncoder(ctx)
        nrefs = 0
        for part in calls:
            exp_out, exp_refs = ref_oracle.encode_refmap(renc, part)
            refmap = {}
            assert enc.encode(part, refmap=refmap) == exp_out
            assert list(refmap.items()) == list(exp_refs.items())
            nrefs += len(refmap)
        assert nrefs > 100
        assert enc.encode(calls[0]) == ref_oracle.encode_refmap(renc, calls[0])[0]    # the default call
        keep = {7: b'kept'}
        enc.encode(calls[1], refmap=keep)
        assert keep[7] == b'kept' and len(keep) > 1
    finally:
        ctx.close()
        ref_oracle.encoder_free(renc)
        ref_oracle.cache_free(cache)


# ------------------------------------------------- crafted bytes, device call

@pytest.fixture(scope='module')
def f1_encoding(oracle):
    (e, _, _), = expected(oracle, [[rc.f1_input()]])[0]
    return e


@pytest.fixture
def ctx():
    from wanproxy_amd.xcgpu import Context
    c = Context(0, cache_segments=1 << 10)
    yield c
    c.status()
    c.close()


def test_every_prefix_in_one_launch(ctx, f1_encoding):
    """Chunk n is the first n bytes of the f1 case's encoding (about 4140
    chunks): counts, entries and walked are the walker's on that prefix, so
    nothing past a chunk's end decides anything."""
    e = f1_encoding
    n = len(e) + 1
    exp = [rc.walk(e, k) for k in range(n)]
    assert {len(r) for r, _ in exp} == {0, 1, 2} and any(w < k for k, (_, w) in enumerate(exp))
    blob = b'\xf1' + e + b'\xf1\x02' * 8
    check(launch(ctx, blob, [1] * n, list(range(n)), cap=2), exp, cap=2)


def test_257_hashes_and_the_stops(ctx):
    enc, hs = rc.crafted_refs()
    stops = rc.stops()
    encs = [enc, enc[:2560], enc[:2560] + enc[:10] + enc[2560:]] + [s[0] for s in stops.values()]
    exp = [rc.walk(e) for e in encs]
    assert [(len(r), w) for r, w in exp[:3]] == [(256, 2560), (256, 2560), (256, 2570)]
    assert [(len(r), w) for r, w in exp[3:]] == [(s[1], s[2]) for s in stops.values()]
    blob, eo, el = pack(encs)
    res = launch(ctx, blob, eo, el)
    check(res, exp)
    assert [int(h) for h in res[1][0]] == sorted(hs[:256])


@pytest.mark.parametrize('cap', [1, 2, 3, CAP])
def test_ref_cap_below_at_and_above_the_count(ctx, oracle, f1_encoding, cap):
    """Counts 0, 1, 2 and 5: only the first ref_cap entries, in hash order, are
    written; the device call and the host call agree."""
    second = rc.stream_cases()['cross'][0]
    c = oracle.cache_new(0)
    exp = expected(oracle, [[rc.f1_input()]] + second, cache=c)
    oracle.cache_free(c)
    host = [host_call(ctx, parts, cap=cap) for parts in [[rc.f1_input()]] + second]
    flat = [x for b in exp for x in b]
    assert {len(r) for _, r, _ in flat} == {0, 1, 2, 5}
    encs = [e for h in host for e in h[0]]
    assert encs == [e for e, _, _ in flat]
    cnt = np.concatenate([h[1] for h in host])
    hs, ps = np.concatenate([h[2] for h in host]), np.concatenate([h[3] for h in host])
    want = [(r, W_SENT) for _, r, _ in flat]
    check((cnt, hs, ps, np.full(len(flat), W_SENT, np.uint64)), want, cap=cap, walked=False)
    blob, eo, el = pack(encs)
    res = launch(ctx, blob, eo, el, cap=cap, walked=False)        # a null d_ref_walked is left alone
    check(res, want, cap=cap, walked=False)
    assert (res[0] == cnt).all() and (res[1] == hs).all() and (res[2] == ps).all()


# ------------------------------------------------------- out of band, null cache

def test_out_of_band_declarations_are_no_entries(oracle, stream_seed):
    """A hash declared and later REF'd in one chunk: the declaration is out, the
    REF is in.  Expected rows: the walk of the in-band oracle's output for the
    same data (tests/test_refmap_cases.py::test_out_of_band_expectation)."""
    from wanproxy_amd.xcgpu import Context
    s = rc.segs()
    batches = [[rc.oob_input(), s[40] + s[41][:100]], [s[40] + rc.abc()[0] + s[42] + s[42], s[43]]]
    c = oracle.cache_new(0)
    inband = expected(oracle, batches, cache=c)
    oracle.cache_free(c)
    oob = encode_batches(oracle, batches, oob=True)
    assert [len(r) for _, r, _ in inband[0] + inband[1]] == [2, 0, 3, 0]
    ctx = Context(0, out_of_band=True, cache_segments=1 << 10)
    try:
        for parts, want, wire in zip(batches, inband, oob):
            d, offs, lens = rc.chunked(parts)
            encs, maps = ctx.encode_chunks_refmap(d, offs, lens)
            assert encs == wire
            for part, m, (_, entries, _) in zip(parts, maps, want):
                assert list(m.items()) == [(h, part[p:p + SEG]) for h, p in entries]
            # the device call on the same bytes: the whole batch, and its second chunk alone
            blob, eo, el = pack(encs)
            check(launch(ctx, blob, eo, el), [(r, len(e)) for (_, r, _), e in zip(want, encs)])
            check(launch(ctx, blob, eo[1:], el[1:], first_chunk=1), [(want[1][1], len(encs[1]))])
            st, res = launch(ctx, blob, eo, el, first_chunk=1, rc_only=True)
            assert st == XCG_EINVAL and (res[0] == C_SENT).all() and (res[1] == H_SENT).all()
        ctx.status()
    finally:
        ctx.close()


def test_out_of_band_rows_that_are_not_there(oracle):
    """XCG_ENOTSUP, nothing written: no stream batch yet, an independent batch
    last, and on a bounded context chunks before the last sub-batch -- the rule
    of xcg_last_declarations."""
    from wanproxy_amd.xcgpu import XCG_SEM_INDEPENDENT, XCG_SEM_STREAM, Context, lib
    s = rc.segs()
    parts = [b''.join(s[50 + 4 * k:54 + 4 * k]) for k in range(6)]
    d, offs, lens = rc.chunked(parts)

    def untouched(res):
        return (res[0] == C_SENT).all() and (res[1] == H_SENT).all() and (res[3] == W_SENT).all()
    ctx = Context(0, out_of_band=True, cache_segments=1 << 10)
    try:
        blob, eo, el = pack([b'\xf1\x02' + bytes(8)])
        st, res = launch(ctx, blob, eo, el, rc_only=True)
        assert st == XCG_ENOTSUP and untouched(res)
        encs = ctx.encode_chunks(d, offs, lens, semantics=XCG_SEM_STREAM)
        blob, eo, el = pack(encs)
        check(launch(ctx, blob, eo, el), [([], len(e)) for e in encs])      # declarations only
        ctx.encode_chunks(d, offs, lens, semantics=XCG_SEM_INDEPENDENT)
        st, res = launch(ctx, blob, eo, el, rc_only=True)
        assert st == XCG_ENOTSUP and untouched(res)
    finally:
        ctx.close()
    ctx = Context(0, out_of_band=True, memory_cache_limit=8 * SEG)       # 24 declarations: sub-batches
    try:
        encs = ctx.encode_chunks(d, offs, lens, semantics=XCG_SEM_STREAM)
        blob, eo, el = pack(encs)
        nd = C.c_uint32()
        assert lib().xcg_last_declarations(ctx.h, 0, None, None, 0, C.byref(nd)) == XCG_ENOTSUP
        st, res = launch(ctx, blob, eo, el, rc_only=True)
        assert st == XCG_ENOTSUP and untouched(res)
        check(launch(ctx, blob, eo[5:], el[5:], first_chunk=5), [([], len(encs[5]))])
        st, res = launch(ctx, blob, eo[5:] * 2, el[5:] * 2, first_chunk=5, rc_only=True)
        assert st == XCG_EINVAL and untouched(res)
    finally:
        ctx.close()


def test_null_cache_every_count_zero(oracle):
    from wanproxy_amd.xcgpu import Context
    parts = [rc.oob_input(), rc.f1_input(), b'']
    d, offs, lens = rc.chunked(parts)
    wire = oracle.encode_batch(d, offs, lens, mode=MODE_NULL, oob=True)
    assert sum(e.count(b'\xf1\x02') for e in wire) >= 8
    ctx = Context(0, out_of_band=True, null_cache=True)             # tack -N's TackNullCache is out of band
    try:
        encs, maps = ctx.encode_chunks_refmap(d, offs, lens)
        assert encs == wire and maps == [{}, {}, {}]
        blob, eo, el = pack(encs)
        check(launch(ctx, blob, eo, el), [([], len(e)) for e in encs])
        ctx.status()
    finally:
        ctx.close()


# -------------------------------------------------------- arguments, ordering

def test_arguments(f1_encoding):
    from wanproxy_amd.xcgpu import Context, XCGError, lib
    import torch
    ctx = Context(0, cache_segments=1 << 10)
    try:
        blob, eo, el = pack([f1_encoding, b'ab'])
        exp = [rc.walk(f1_encoding), ([], 2)]
        check(launch(ctx, blob, eo, el, max_len=2 * 524288 + 16), exp)
        st, res = launch(ctx, blob, eo, el, max_len=2 * 524288 + 17, rc_only=True)
        assert st == XCG_EINVAL and (res[0] == C_SENT).all()
        assert launch(ctx, b'', [], [], rc_only=True)[0] == 0                  # n == 0
        L = lib()
        t = torch.zeros(64, dtype=torch.int64, device='cuda:0')
        p = C.c_void_p(t.data_ptr())
        good = [ctx.h, p, p, p, 1, 16, 0, p, p, 1, p, None, None]
        assert L.xcg_encode_refmap_batch(*good) == 0
        for k in (0, 1, 2, 3, 7, 8, 10):
            bad = list(good)
            bad[k] = None
            assert L.xcg_encode_refmap_batch(*bad) == XCG_EINVAL, k
        torch.cuda.synchronize()
        a = np.zeros(64, np.uint64)
        q = a.ctypes.data
        hgood = [ctx.h, 1, q, 8, q, q, 1, q, 64, q, q, q, q, 1, q]
        for k in (11, 12, 14):
            bad = list(hgood)
            bad[k] = None
            assert L.xcg_encode_host_refmap(*bad) == XCG_EINVAL, k
        ctx.status()
        # a chunk longer than the bound: count 0, walked 0, bit 3 of the status word; the others are served
        cnt, _, _, wk = launch(ctx, blob, eo, el, max_len=100)
        assert [int(c) for c in cnt] == [0, 0] and [int(w) for w in wk] == [0, 2]
        with pytest.raises(XCGError):
            ctx.status()
    finally:
        ctx.close()


def test_ordered_behind_an_encode_on_another_stream(oracle):
    """An asynchronous independent batch on one stream, the refmap of its
    outputs on another, no synchronisation between: the context orders them."""
    import torch
    from wanproxy_amd.xcgpu import XCG_SEM_INDEPENDENT, Context
    s = rc.segs()
    r = np.random.default_rng(rc.SEED + 2)
    parts = []
    for k in range(128):
        x, y = s[k % 40], s[(k + 7) % 40]
        parts.append(x + y + x + r.integers(0, 256, 32768 - 4 * SEG - k, dtype=np.uint8).tobytes() + y)
    d, offs, lens = rc.chunked(parts)
    exp = [rc.walk(e) for e in oracle.encode_batch(d, offs, lens, mode=MODE_INDEPENDENT)]
    assert all(len(r_) == 2 for r_, _ in exp)
    dev = torch.device('cuda', 0)
    n = len(parts)
    bounds = 2 * lens.astype(np.uint64) + 16
    oo = np.zeros(n, np.uint64)
    oo[1:] = np.cumsum(bounds)[:-1]
    ctx = Context(0, cache_segments=1 << 10)
    try:
        d_in = torch.from_numpy(d.copy()).to(dev)
        d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
        d_oo = torch.from_numpy(oo.view(np.int64)).to(dev)
        d_out = torch.zeros(int(bounds.sum()), dtype=torch.uint8, device=dev)
        d_ol = torch.zeros(n, dtype=torch.int64, device=dev)
        d_h = torch.zeros(n * 4, dtype=torch.int64, device=dev)
        d_p = torch.zeros(n * 4, dtype=torch.int32, device=dev)
        d_c = torch.zeros(n, dtype=torch.int32, device=dev)
        d_w = torch.zeros(n, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        live = None
        for _ in range(2):                                    # (the second round: nothing is allocated)
            ctx.encode_batch_device(d_in, d_off, d_len, n, int(lens.max()), d_out, d_oo, d_ol, stream=s1,
                                    semantics=XCG_SEM_INDEPENDENT)
            ctx.encode_refmap_device(d_out, d_oo, d_ol, n, int(bounds.max()), d_h, d_p, 4, d_c, d_w, stream=s2)
            s2.synchronize()
            assert live is None or mem_live() == live
            live = mem_live()
        hs = d_h.cpu().numpy().view(np.uint64).reshape(n, 4)
        ps = d_p.cpu().numpy().view(np.uint32).reshape(n, 4)
        cnt, wk = d_c.cpu().numpy(), d_w.cpu().numpy()
        for i, (entries, w) in enumerate(exp):
            assert int(cnt[i]) == 2 and int(wk[i]) == w
            assert [(int(h), int(p)) for h, p in zip(hs[i, :2], ps[i, :2])] == entries
        ctx.status()
    finally:
        ctx.close()


def test_memory_is_unchanged_across_calls(f1_encoding):
    from wanproxy_amd.xcgpu import Context
    ctx = Context(0, cache_segments=1 << 10)
    try:
        parts = rc.stream_cases()['cross'][0][0]
        host_call(ctx, parts)
        blob, eo, el = pack([f1_encoding] * 5)
        launch(ctx, blob, eo, el)
        held = mem_live()
        for _ in range(3):
            host_call(ctx, parts)
            launch(ctx, blob, eo, el)
            assert mem_live() == held
    finally:
        ctx.close()


# ------------------------------------------------------------------------ pipe

def test_pipe_ask_for_a_refd_hash_gets_its_learn(oracle):
    """One conversation: the peer forgets its cache, the next frame is REFs, its
    <ASK> is answered with the segments the refmap rows name -- in-band and
    out of band -- and an <ASK> for a hash no frame REF'd is a protocol error."""
    from wanproxy_amd.xcgpu import Context, PipePair, XCGError
    ua, ub = b'0d1f4c8e-95a3-4b2d-8f6e-3c7a9b1d2e4f', b'a7c3e9f1-2b4d-4e6f-8a0c-1e3f5a7c9e0b'
    s = rc.segs()
    m = b''.join(s[60:90]) + b'tail\xf1'
    for oob in (False, True):
        enc, adec, benc, bdec = (Context(0, out_of_band=(oob and k == 0), cache_segments=1 << 10) for k in range(4))
        a, b = PipePair(enc, adec, ua), PipePair(benc, bdec, ub)
        try:
            to_a, local, _, _ = b.decoder_consume(a.encoder_consume(m))
            if oob:                                            # every segment is declared out of band: all asked
                assert local == b'' and to_a[:1] == b'\xf0' and int.from_bytes(to_a[1:3], 'big') == 30
                with pytest.raises(XCGError, match=r'\(-71\)'):
                    a.decoder_consume(to_a)                    # declarations are in no refmap
                continue
            assert local == m
            a.decoder_consume(to_a)                            # <ADVANCE>
            bdec.cache_clear()
            m2 = s[70] + b'\xf1\xf1' + s[61] + s[70] + s[89]
            to_a, local, _, _ = b.decoder_consume(a.encoder_consume(m2))
            assert local == b'' and to_a[:1] == b'\xf0' and int.from_bytes(to_a[1:3], 'big') == 3
            asked = [int.from_bytes(to_a[3 + 8 * k:11 + 8 * k], 'big') for k in range(3)]
            assert asked == sorted(oracle.hash(x) for x in (s[70], s[61], s[89]))
            learn, _, _, _ = a.decoder_consume(to_a)
            by_hash = {oracle.hash(x): x for x in (s[70], s[61], s[89])}
            assert learn == b'\xf1\x00\x03' + b''.join(by_hash[h] for h in asked)
            _, local, _, _ = b.decoder_consume(learn)
            assert local == m2
            with pytest.raises(XCGError, match=r'\(-71\)'):
                a.decoder_consume(b'\xf0\x00\x01' + oracle.hash(s[62]).to_bytes(8, 'big'))
        finally:
            a.close()
            b.close()
            for c in (enc, adec, benc, bdec):
                c.close()
