"""Name reuse inside a decode batch (xcodec/xcodec_decoder.cc:106-136): a second
<EXTRACT> of a hash with other bytes replaces the cache entry, and every later
<REF> of the hash reads the new bytes.  On an unbounded context a REF yields
the bytes of the latest preceding EXTRACT of its hash in the batch, else the
cache's; bounded and pair contexts decline such a batch.

Expected values come from the oracle restatement (one decode() call over the
batch's chunks joined, on a persistent decoder), and for the fixed cases from
literal byte strings as well.  The reference itself is not run in-process on
these streams: its XCodecMemoryCache::replace keeps the new segment without a
reference (xcodec_cache.h:333-336), see tests/test_gpu_pair_decode.py.

Colliding segments: XCodecHash is a pair of position-weighted sums, so adding
+2, -4, +2 to three consecutive odd bytes keeps it."""
import ctypes
import random

import pytest

from backref_streams import WindowModel
from collision_cases import family  # noqa: F401  (re-exported)
from golden_cases import data

pytestmark = pytest.mark.gpu

SEG = 2048


def E(seg):
    return b'\xf1\x01' + seg


def R(h):
    return b'\xf1\x02' + h.to_bytes(8, 'big')


def BR(i):
    return bytes([0xf1, 0x03, i])


def LIT(b):
    return b.replace(b'\xf1', b'\xf1\x00')


def filler(seed):
    r = random.Random(0xF111 + seed)
    return bytes(r.randrange(7, 202, 2) for _ in range(SEG))


@pytest.fixture(scope='module')
def fam(oracle):
    a, b, c = family(1)
    h = oracle.hash(a)
    assert h == oracle.hash(b) == oracle.hash(c) and len({a, b, c}) == 3
    f = [filler(k) for k in range(4)]
    fh = [oracle.hash(s) for s in f]
    assert len(set(fh + [h])) == 5
    return dict(A=a, B=b, C=c, h=h, F=f, fh=fh)


def gpu_batch(ctx, chunks):
    """decode_chunks as one decode() call: (ok, out, consumed, unknown)."""
    outs, st, cons, unk = ctx.decode_chunks(chunks)
    consumed = 0
    for k in range(len(chunks)):
        if st[k] == 2:
            break
        consumed += int(cons[k])
        if st[k] != 0:
            break
    assert all(outs[k] == b'' for k in range(len(chunks)) if st[k] == 2)
    return all(int(s) >= 0 for s in st), b''.join(outs), consumed, sorted(unk)


class Both:
    """An unbounded engine context and the oracle's persistent decoder, fed the
    same batches and compared call by call."""

    def __init__(self, oracle):
        from wanproxy_amd.xcgpu import Context
        self.o = oracle
        self.ctx = Context(0, cache_segments=1 << 12)
        self.oc = oracle.cache_new()
        self.od = oracle.decoder_new(self.oc)

    def batch(self, chunks, tag=None):
        ok, out, cons, unk = self.o.decode(b''.join(chunks), self.oc, decoder=self.od)
        got = gpu_batch(self.ctx, chunks)
        assert got[0] == ok and got[2] == cons and got[3] == sorted(unk), (tag, got[0], got[2], got[3], ok, cons, unk)
        assert got[1] == out, (tag, len(got[1]), len(out))
        assert self.ctx.cache_size() == self.o.lib.xco_cache_size(self.oc), tag
        return got

    def call(self, buf, tag=None):
        ok, out, cons, unk = self.o.decode(buf, self.oc, decoder=self.od)
        st, gout, gcons, gunk, _ = self.ctx.decode_call(buf)
        assert (st >= 0, gcons, gunk) == (ok, cons, sorted(unk)), (tag, st, gcons, gunk, ok, cons, unk)
        assert gout == out, (tag, len(gout), len(out))
        return st, gout, gcons, gunk

    def close(self):
        self.ctx.close()
        self.o.decoder_free(self.od)
        self.o.cache_free(self.oc)


@pytest.fixture
def both(oracle):
    b = Both(oracle)
    yield b
    b.close()


def case1_ops(fam):
    A, B, h = fam['A'], fam['B'], fam['h']
    return [E(A), E(B), R(h), E(A), R(h)]


def test_case1_extract_a_b_ref_a_ref(both, fam):
    """E(A) E(B) R(h) E(A) R(h) in one chunk: A B B A A, the cache then holds A.
    The first and the latest EXTRACT are equal, the middle one differs.
    (Before name reuse was modelled this decoded to A B A A A.)"""
    A, B, h = fam['A'], fam['B'], fam['h']
    ok, out, cons, unk = both.batch([b''.join(case1_ops(fam))])
    assert ok and not unk and cons == 3 * 2050 + 20
    assert out == A + B + B + A + A
    assert both.ctx.cache_lookup(h) == A
    dups, conflicts, ran = both.ctx.decode_reuse_stats()
    assert dups == 2 and conflicts >= 1 and ran


def test_case2_extract_a_b_ref(both, fam):
    """E(A) E(B) R(h): A B B, the cache holds B.  (Before: XCG_ENOTSUP.)"""
    A, B, h = fam['A'], fam['B'], fam['h']
    ok, out, cons, unk = both.batch([E(A) + E(B) + R(h)])
    assert ok and not unk and out == A + B + B
    assert both.ctx.cache_lookup(h) == B
    assert both.ctx.decode_reuse_stats() == (1, 1, True)


def test_case3_one_op_per_chunk(both, fam):
    """The ops of case 1, each chunk its own wave; then the EXTRACTs of the
    hash in chunks 0, 2 and 4."""
    A, B, h = fam['A'], fam['B'], fam['h']
    ok, out, cons, unk = both.batch(case1_ops(fam))
    assert ok and out == A + B + B + A + A
    assert both.ctx.cache_lookup(h) == A
    assert both.ctx.decode_reuse_stats()[1:] == (1, True)
    ok, out, cons, unk = both.batch([E(B), R(h), E(A), R(h), E(B) + R(h)])
    assert ok and out == B + B + A + A + B + B
    assert both.ctx.cache_lookup(h) == B
    assert both.ctx.decode_reuse_stats()[1:] == (1, True)


def case4_batches(fam):
    A, B, h, F = fam['A'], fam['B'], fam['h'], fam['F']
    return [E(A) + b'lit', R(h) + E(B) + R(h) + b'\xf1\x00', R(h) + E(F[0]) + BR(4) + BR(5)]


def test_case4_cached_then_batch(both, fam):
    """The hash is cached with A; the next batch reads A, replaces it with B and
    reads B; the third reads B from the cache and from the window."""
    A, B, h, F = fam['A'], fam['B'], fam['h'], fam['F']
    b1, b2, b3 = case4_batches(fam)
    assert both.batch([b1])[1] == A + b'lit'
    assert both.ctx.cache_lookup(h) == A
    assert both.batch([b2])[1] == A + B + B + b'\xf1'
    assert both.ctx.cache_lookup(h) == B
    assert both.ctx.decode_reuse_stats() == (0, 0, False)     # one EXTRACT of h per batch: a plain replace
    assert both.batch([b3])[1] == B + F[0] + B + F[0]


def test_case5_backref_after_redeclare(both, fam):
    """BACKREFs behind a re-declare with other bytes (the batch holds BACKREFs:
    every declare is recorded).  Window slots: 0 E(A), 1 E(F0), 2 E(B) (empties
    0), 3 R(h) (empties 2), 4 E(A) (empties 3); the last BACKREF names the
    emptied slot 0: decode() is false there."""
    A, B, h, F = fam['A'], fam['B'], fam['h'], fam['F']
    c0 = E(A) + E(F[0]) + E(B) + BR(2) + R(h) + BR(3)
    c1 = LIT(b'x\xf1y') + E(A) + BR(4) + BR(1) + BR(0) + b'tail'
    ok, out, cons, unk = both.batch([c0, c1])
    assert not ok and not unk
    assert out == A + F[0] + B + B + B + B + b'x\xf1y' + A + A + F[0]
    assert both.ctx.decode_reuse_stats()[1:] == (1, True)


@pytest.mark.parametrize('late', ['B', 'A'])
def test_case6_stop_point_straddle(both, fam, late):
    """EXTRACTs of the hash on both sides of the stop point (an unknown REF):
    the one behind it is not reached -- with other bytes, or with equal bytes --
    until the remainder is presented again."""
    A, h, F, fh = fam['A'], fam['h'], fam['F'], fam['fh']
    L = fam[late]
    U, u = F[3], fh[3]
    ops = [E(A), R(h), R(u), E(L), R(h)]
    ok, out, cons, unk = both.batch([b''.join(ops)])
    assert ok and unk == [u] and cons == 2050 + 10 and out == A + A
    assert both.ctx.cache_lookup(h) == A and both.ctx.cache_size() == 1
    both.ctx.cache_enter(u, U)
    # (the restatement's XCodecCache::enter)
    assert both.o.lib.xco_cache_enter(both.oc, u, (ctypes.c_uint8 * SEG).from_buffer_copy(U)) == 0
    ok, out, cons, unk = both.batch([b''.join(ops[2:])])
    assert ok and not unk and out == U + L + L
    assert both.ctx.cache_lookup(h) == L


def test_case7_ref_run_longer_than_a_wave(both, fam):
    """70 consecutive REFs, the conflicted hash mixed with ordinary ones."""
    A, B, C, h, F, fh = fam['A'], fam['B'], fam['C'], fam['h'], fam['F'], fam['fh']
    refs = [h if k % 3 != 1 else fh[k % 2] for k in range(70)]
    ops = [E(F[0]), E(F[1]), E(A), E(B)] + [R(x) for x in refs] + [E(C), R(h)]
    seg = {h: B, fh[0]: F[0], fh[1]: F[1]}
    ok, out, cons, unk = both.batch([b''.join(ops)])
    assert ok and out == F[0] + F[1] + A + B + b''.join(seg[x] for x in refs) + C + C
    assert both.ctx.cache_lookup(h) == C
    assert both.ctx.decode_reuse_stats() == (2, 1, True)


def test_case8_three_hundred_occurrences(both, fam):
    """One hash EXTRACTed 300 times with alternating bytes, a REF behind each,
    over 5 chunks."""
    A, B, h = fam['A'], fam['B'], fam['h']
    pairs = [E(A if k % 2 == 0 else B) + R(h) for k in range(300)]
    chunks = [b''.join(pairs[k:k + 60]) for k in range(0, 300, 60)]
    ok, out, cons, unk = both.batch(chunks)
    assert ok and out == b''.join((A if k % 2 == 0 else B) * 2 for k in range(300))
    assert both.ctx.cache_lookup(h) == B
    assert both.ctx.decode_reuse_stats() == (299, 1, True)


@pytest.mark.parametrize('seed', range(5))
def test_case9_random_sweep(oracle, seed):
    """8 families x 3 variants, ~300 ops a batch (EXTRACT, REF, literals with
    escapes, some BACKREFs to live window slots), chunks cut at random op
    boundaries, 3 batches on one context."""
    rng = random.Random(9000 + seed)
    fams = [family(100 + 10 * seed + f) for f in range(8)]
    hs = [oracle.hash(v[0]) for v in fams]
    for v, h in zip(fams, hs):
        assert all(oracle.hash(s) == h for s in v) and len(set(v)) == 3
    assert len(set(hs)) == 8
    both = Both(oracle)
    win = WindowModel()
    known = []                                                # hashes EXTRACTed so far in the stream
    last = {}                                                 # family -> the variant its latest EXTRACT carried
    ran = 0
    try:
        for b in range(3):
            ops = []
            for _ in range(300):
                x = rng.random()
                if x < 0.35 or not known:
                    f = rng.randrange(8)
                    last[f] = rng.randrange(3)
                    ops.append(E(fams[f][last[f]]))
                    if hs[f] not in known:
                        known.append(hs[f])
                    win.declare(hs[f])
                elif x < 0.70:
                    h = rng.choice(known)
                    ops.append(R(h))
                    win.declare(h)
                elif x < 0.92:
                    ops.append(LIT(bytes(rng.choice([0xf1, 0x00, 0x41, rng.randrange(256)])
                                         for _ in range(rng.randrange(1, 300)))))
                else:
                    ops.append(BR(rng.choice(win.live())))
            cuts = sorted(rng.sample(range(1, len(ops)), rng.randrange(0, 7)))
            chunks = [b''.join(ops[a:z]) for a, z in zip([0] + cuts, cuts + [len(ops)])]
            ok, out, cons, unk = both.batch(chunks, tag=(seed, b))
            assert ok and not unk and cons == sum(len(c) for c in chunks)
            ran += both.ctx.decode_reuse_stats()[2]
            for f, j in last.items():
                assert both.ctx.cache_lookup(hs[f]) == fams[f][j], (seed, b, f)
    finally:
        both.close()
    assert ran == 3


@pytest.mark.parametrize('name', ['kat_a', 'runs'])
def test_case10_goldens_take_the_fast_path(both, oracle, name):
    """An encoder's stream on a fresh decoder cache has no duplicate EXTRACTs."""
    from wanproxy_amd.synth import chunks_of
    d = data(name)
    offs, lens = chunks_of(d, 65536)
    enc = oracle.encode_batch(d, offs, lens, mode=1)
    ok, out, cons, unk = both.batch(enc)
    assert ok and not unk and out == d
    assert both.ctx.decode_reuse_stats() == (0, 0, False)


def test_case10_equal_bytes_duplicates(both, oracle):
    """The same chunk encoded independently twice: duplicate EXTRACTs with equal
    bytes are no conflict, and the resolver does not run."""
    from wanproxy_amd.synth import chunks_of
    d = data('kat_a')[:65536]
    offs, lens = chunks_of(d, 65536)
    enc = oracle.encode_batch(d, offs, lens, mode=1)[0]
    assert enc.count(b'\xf1\x01') > 0
    ok, out, cons, unk = both.batch([enc, enc])
    assert ok and not unk and out == d + d
    dups, conflicts, ran = both.ctx.decode_reuse_stats()
    assert dups > 0 and conflicts == 0 and not ran


def test_case11_decode_call_falls_back(both, oracle, fam):
    """xcg_decode_call on the inputs of cases 1 and 4: its one-launch kernel
    leaves name reuse to the batch path, which now decodes it."""
    A, B, h, F = fam['A'], fam['B'], fam['h'], fam['F']
    st, out, cons, unk = both.call(b''.join(case1_ops(fam)), 'case1')
    assert st == 0 and out == A + B + B + A + A
    assert both.ctx.cache_lookup(h) == A
    assert both.ctx.decode_reuse_stats() == (2, 1, True)
    four = Both(oracle)
    try:
        b1, b2, b3 = case4_batches(fam)
        assert four.call(b1, 'b1')[1] == A + b'lit'
        assert four.call(b2, 'b2')[1] == A + B + B + b'\xf1'
        assert four.ctx.cache_lookup(h) == B
        assert four.call(b3, 'b3')[1] == B + F[0] + B + F[0]
    finally:
        four.close()


@pytest.mark.parametrize('kind', ['bounded', 'pair'])
def test_case12_bounded_and_pair_decline(oracle, fam, kind):
    """Bounded and pair contexts decline name reuse inside a batch -- the
    middle EXTRACT alone differs here -- with nothing committed, and go on."""
    from wanproxy_amd.xcgpu import Context, XCGError
    A, B, h, F, fh = fam['A'], fam['B'], fam['h'], fam['F'], fam['fh']
    if kind == 'bounded':
        ctx = Context(0, memory_cache_limit=64 * SEG)
    else:
        ctx = Context(0, memory_cache_limit=64 * SEG, disk_bytes=(18 + 205) * SEG)
    try:
        assert gpu_batch(ctx, [E(F[0]) + b'lit']) == (True, F[0] + b'lit', 2050 + 3, [])
        size = ctx.cache_size()
        with pytest.raises(XCGError, match=r'\(-95\)'):
            ctx.decode_chunks([b''.join(case1_ops(fam))])
        assert ctx.cache_size() == size
        assert ctx.cache_lookup(h) is None
        assert gpu_batch(ctx, [R(fh[0]) + E(F[1]), R(fh[1]) + E(A) + R(h)]) == (True, F[0] + F[1] + F[1] + A + A,
                                                                               2060 + 2070, [])
        assert ctx.cache_lookup(h) == A
    finally:
        ctx.close()
