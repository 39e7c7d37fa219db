"""Cases for <BACKREF> ops decoded on a bounded XCodecMemoryCache(uuid, size)
and on an XCodecCachePair (test infrastructure, no GPU in here).

XCodecDecoder::decode dereferences its XCodecWindow whatever the cache is
(xcodec/xcodec_decoder.cc:165-181): a BACKREF makes no lookup, and a live slot
holds its own copy of the bytes, so it decodes after the hash was evicted,
pushed to disk, dropped from the disk FIFO or REPLACEd.  A BACKREF to an empty
slot ends the call (decode() is false) and nothing behind it is looked at,
whereas behind an unknown REF decode_skim (:196-272) goes on looking up REFs --
which refreshes a bounded cache's LRU order and promotes in a pair -- and steps
over BACKREFs unexamined.

A case is {'name', 'alt', 'steps'}; a step is
    ('learn', [segments])        enter segments through a decoder of their own
    ('batch', [chunks], ask)     successive decode() calls of THE decoder;
                                 ask: {kind: index of the chunk that stops at
                                 an unknown REF with chunks behind it}
    ('probe',)                   every slot of the decoder's window
    ('decoder',)                 a fresh decoder (an empty window) on the same
                                 cache from here on
and runs on each kind of cache (KINDS) with the geometry below.

run_model() is the yardstick: one persistent decoder_new(cache), the chunks of
a batch decoded one by one; after a stop (unknown REF or BACKREF to an empty
slot) the later chunks are not decoded (status 2).  A batch is one buffered
stream (a pipe pair appends every FRAME to the decoder's input,
xcodec/xcodec_pipe_pair.cc:425-483), so decode_skim runs to the end of the
batch: the chunk that `ask` names is handed to decode() with the rest of the
batch behind it.  An unknown REF in a chunk that `ask` does not name, with
chunks behind it, is an error of the case.  `split=True` runs every chunk as a
batch of its own (the skim then ends with the chunk).  `via_cache=True`
resolves every BACKREF by a lookup of the slot's hash in the cache instead of
the window's copy: each case whose BACKREFs decode ('alt': 'window') must come
out different, or it would not tell a decoder that does so from the reference.
`skim_after_error=True` lets decode_skim run behind a BACKREF to an empty slot
as it runs behind an unknown REF: the cases about that stop ('alt': 'skim')
must come out different on the bounded cache.

Every batch keeps its enters plus lookups of cached entries at or under the
memory limit of LIMIT_SEGS segments, the most one call on a bounded context may
make.  It follows that nothing a batch itself names can leave a bounded cache
inside that batch (that takes LIMIT_SEGS enters behind the reference), so the
eviction cases declare in one call and evict in the call that holds the
BACKREF, or in calls between the two.
"""
import random

from backref_streams import SEG, WindowModel, stream_with_backrefs
from collision_cases import family
from decode_windows_cases import LIT, B, Builder, R, X, probe_window, rnd_segs, status_of, walk

LIMIT_SEGS = 64
LIMIT = LIMIT_SEGS * SEG
DISK = (18 + 205) * SEG          # one index block: 204 entries, then the FIFO laps
KINDS = ('bounded', 'pair', 'unbounded')
UNKNOWN = 0x0123456789ABCDEF     # a hash no cache of a case holds


def new_cache(o, kind):
    if kind == 'bounded':
        return o.cache_new(LIMIT)
    if kind == 'pair':
        return o.cache_new_pair(LIMIT, DISK)
    return o.cache_new()


def xs(b, segs):
    return b''.join(b.x(0, s) for s in segs)


def slot(b, seg):
    return B(b.slot_of(0, seg))


class _Decoder:
    """The case's decoder on `cache`: decode(chunk) -> (ok, out, consumed,
    unknown).  via_cache: BACKREFs by a cache lookup of the slot's hash."""

    def __init__(self, o, cache, via_cache):
        self.o, self.cache, self.via = o, cache, via_cache
        self.dec = o.decoder_new(cache)
        self.wm = WindowModel()

    def close(self):
        self.o.decoder_free(self.dec)

    def _declares(self, e):
        for kind, a, z in walk(e):
            if kind == 'x':
                self.wm.declare(self.o.hash(e[a + 2:z]))
            elif kind == 'r':
                self.wm.declare(int.from_bytes(e[a + 2:z], 'big'))

    def decode(self, e):
        if not self.via:
            return self.o.decode(e, self.cache, decoder=self.dec)
        out, at = b'', 0
        cuts = [(a, z) for kind, a, z in walk(e) if kind == 'b'] + [(len(e), len(e))]
        for a, z in cuts:
            if a > at:
                ok, o1, c, unk = self.o.decode(e[at:a], self.cache, decoder=self.dec)
                self._declares(e[at:at + c])
                out += o1
                if not ok or unk or c < a - at:
                    return ok, out, at + c, unk
            if z > a:
                h = self.wm.slot[e[a + 2]]
                if h == 0:
                    return False, out, z, []
                ok, o1, c, unk = self.o.decode(R(h), self.cache)      # (a decoder of its own: no declare)
                if unk:
                    return True, out, a, unk
                out += o1
            at = z
        return True, out, len(e), []


def _lru_order(o, cache):
    """The hashes of a bounded cache, least recently used first (C oracle)."""
    import ctypes as C

    import numpy as np
    keys = np.zeros(LIMIT_SEGS, dtype=np.uint64)
    n = int(o.lib.xco_cache_export(cache, keys.ctypes.data_as(C.POINTER(C.c_uint64)), None, LIMIT_SEGS))
    return [int(k) for k in keys[:n]]


def run_model(o, case, kind, split=False, via_cache=False, skim_after_error=False):
    """The case on oracle `o` (the C oracle or the compiled reference) and a
    cache of `kind`.  Returns one result per step -- None for a learn,
    {'outs', 'status', 'consumed', 'unknown'} for a batch, 256 entries for a
    probe -- and, last, the cache's own account: {'pair_stats' (a pair),
    'order' (a bounded cache on the C oracle: its hashes in LRU order)}.  A batch behind a
    decode() that returned false is not decoded (None) until the next 'decoder'
    step: the error ended that decoder."""
    cache = new_cache(o, kind)
    d = _Decoder(o, cache, via_cache)
    results, dead = [], False
    try:
        for step in case['steps']:
            if step[0] == 'decoder':
                d.close()
                d = _Decoder(o, cache, via_cache)
                dead = False
                results.append(None)
            elif step[0] == 'batch' and dead:
                results.append(None)
            elif step[0] == 'learn':
                for seg in step[1]:
                    assert o.decode(X(seg), cache)[0]
                results.append(None)
            elif step[0] == 'probe':
                def decode1(chunk):
                    ok, out, c, unk = o.decode(chunk, cache, decoder=d.dec)
                    return status_of(ok, c, unk, len(chunk)), out, c
                results.append(probe_window(decode1))
            else:
                chunks = step[1]
                ask = (step[2] if len(step) > 2 else {}).get(kind)
                n = len(chunks)
                outs, st, cons, unknown, stopped = [], [], [], [], False
                for i, e in enumerate(chunks):
                    if stopped:
                        outs.append(b'')
                        st.append(2)
                        cons.append(0)
                        continue
                    joined = ask == i and not split and not via_cache
                    ok, out, c, unk = d.decode(e + b''.join(chunks[i + 1:]) if joined else e)
                    s = status_of(ok, c, unk, len(e))
                    if joined:
                        assert s == 1 and c < len(e), (case['name'], kind, i, s, c)
                    elif s == 1 and not split and not via_cache:
                        assert i == n - 1, (case['name'], kind, i, 'an unknown REF the case does not announce')
                    outs.append(out)
                    st.append(s)
                    cons.append(c)
                    if s == 1:
                        unknown = sorted(set(unk))
                    stopped = s in (1, -1)
                    if s == -1 and skim_after_error:       # (what the reference does NOT do: a skim behind the error)
                        o.decode(R(UNKNOWN) + e[c:] + b''.join(chunks[i + 1:]), cache)
                    if stopped and split:
                        break                      # (the chunks behind a stop are not presented)
                k = len(st)
                dead = -1 in st
                results.append({'outs': outs + [b''] * (n - k), 'status': st + [2] * (n - k),
                                'consumed': cons + [0] * (n - k), 'unknown': unknown})
        results.append({'pair_stats': o.pair_stats(cache) if kind == 'pair' else None,
                        'order': _lru_order(o, cache) if kind == 'bounded' and not o.ref else None})
    finally:
        d.close()
        o.cache_free(cache)
    return results


# ------------------------------------------------------------------- cases

def _case(name, b, alt='window'):
    return {'name': name, 'alt': alt, 'steps': b.steps}


def case_evicted_in_batch(o):
    """A is declared in the first call; the second call's own EXTRACTs push it
    out of the memory cache (a pair keeps it on disk), then a BACKREF to A's
    slot decodes A, and a REF to A right behind it is unknown on the bounded
    cache and stops the batch in front of two more chunks."""
    b = Builder(o, 1)
    s = rnd_segs(0xE1, 80)
    A = s[0]
    b.steps.append(('batch', [LIT + b.x(0, A), xs(b, s[1:31])]))
    c = [xs(b, s[31:61]),
         xs(b, s[61:67]) + slot(b, A) + LIT + b.r(0, A) + b.x(0, s[70]) + slot(b, s[70]),
         b.x(0, s[71]) + slot(b, A)]
    b.steps.append(('batch', c, {'bounded': 1}))
    b.steps.append(('probe',))
    b.steps.append(('batch', [R(o.hash(s[66])) + R(o.hash(s[2])) + R(o.hash(s[70]))]))
    return _case('evicted_in_batch', b)


def case_evicted_across_calls(o):
    """A is declared in the first call; four calls of 55 EXTRACTs each follow,
    so A leaves the memory cache and, on the pair, the disk FIFO (204 entries)
    too.  The window carried over still decodes the BACKREF; the REF behind it
    is unknown on both."""
    b = Builder(o, 1)
    s = rnd_segs(0xE2, 230)
    A = s[0]
    b.steps.append(('batch', [b.x(0, A) + LIT]))
    for k in range(4):
        part = s[1 + 55 * k:1 + 55 * (k + 1)]
        b.steps.append(('batch', [xs(b, part[:20]), xs(b, part[20:])]))
    b.steps.append(('batch', [LIT + slot(b, A) + slot(b, s[5]) + b.r(0, A) + slot(b, A), b.x(0, s[225])],
                    {'bounded': 0, 'pair': 0}))
    b.steps.append(('probe',))
    return _case('evicted_across_calls', b)


def case_ghit_then_evicted(o):
    """A REF hits the persistent entry P and declares it; the next call's
    enters evict P, then a BACKREF to the slot the REF declared gives P's
    bytes and a REF to P is unknown on the bounded cache."""
    b = Builder(o, 1)
    s = rnd_segs(0xE3, 80)
    P = s[0]
    b.steps.append(('learn', [P] + s[70:75]))
    b.steps.append(('batch', [b.r(0, P) + slot(b, P) + LIT, xs(b, s[1:41])]))
    c = [xs(b, s[41:65]) + slot(b, P), LIT + slot(b, P) + b.r(0, P) + b.x(0, s[66]), slot(b, P)]
    b.steps.append(('batch', c, {'bounded': 1}))
    b.steps.append(('probe',))
    return _case('ghit_then_evicted', b)


def case_ghit_run_then_evicted(o):
    """The same with the declaring REF inside a run of 70 REFs (more than one
    wave's 64): 30 to persistent entries, 40 to EXTRACTs of the batch, and
    BACKREFs into the run on both sides of lane 63, in that call and after the
    next call has evicted the persistent ones."""
    b = Builder(o, 1)
    s = rnd_segs(0xE4, 120)
    p, e = s[:30], s[30:40]
    b.steps.append(('learn', p))
    first = xs(b, e)
    run = b''.join(b.r(0, q) for q in p) + b''.join(b.r(0, e[k % 10]) for k in range(40))
    c = [first, run +slot(b, p[5]) + slot(b, e[5]) + slot(b, p[29]) + slot(b, e[9]) + LIT]
    assert b.slot_of(0, p[5]) == 10 + 5 and b.slot_of(0, e[5]) == 10 + 65
    b.steps.append(('batch', c))
    c = [xs(b, s[40:100]) + slot(b, p[5]) + slot(b, e[5]), slot(b, p[29]) + b.r(0, p[5]) + slot(b, p[5]), b.x(0, s[101])]
    b.steps.append(('batch', c, {'bounded': 1}))
    b.steps.append(('probe',))
    return _case('ghit_run_then_evicted', b)


def case_window_larger_than_cache(o):
    """250 declares over five calls on the 64-segment cache, ten more so the
    window wraps past 256; a BACKREF 200 declares back decodes, one to a slot
    that a re-declare of its hash cleared fails."""
    b = Builder(o, 1)
    s = rnd_segs(0xE5, 270)
    for k in range(5):
        b.steps.append(('batch', [xs(b, s[50 * k:50 * k + 25]), xs(b, s[50 * k + 25:50 * k + 50])]))
    old = b.slot_of(0, s[60])
    c = [xs(b, s[250:260]) + slot(b, s[59]) + slot(b, s[255]) + LIT,
         b.x(0, s[60]) + slot(b, s[60]) + slot(b, s[59]) + B(old) + slot(b, s[59]),
         b.x(0, s[261])]
    assert b.models[0].slot[old] == 0 and b.slot_of(0, s[60]) == (260 % 256) and b.slot_of(0, s[59]) == 59
    b.steps.append(('batch', c))
    b.steps.append(('probe',))
    return _case('window_larger_than_cache', b)


def _tail_setup(o, seed):
    """p1, p2 and 60 fillers learnt in that order: p1 and p2 are the next two
    a bounded cache of 64 evicts, two entries short of full."""
    b = Builder(o, 1)
    s = rnd_segs(seed, 80)
    p1, p2, fill = s[0], s[1], s[2:62]
    b.steps.append(('learn', [p1, p2] + fill))
    return b, s, p1, p2, fill


def _tail_followup(o, b, s, p1, p2, fill):
    """The window as the stop left it; then, on a fresh decoder (a decode()
    that returned false ended the first), three enters evict the tail (63 + 3
    = 66) and REFs show who went."""
    b.steps.append(('probe',))
    b.steps.append(('decoder',))
    b.steps.append(('batch', [xs(b, s[65:68])]))
    b.steps.append(('batch', [R(o.hash(fill[3])) + R(o.hash(p1)) + R(o.hash(p2)) + R(o.hash(fill[0])) + R(o.hash(fill[1]))]))
    b.steps.append(('probe',))


def case_error_stop_no_skim(o):
    """... B(empty) R(p1) R(p2), two more chunks: -1, 2, 2.  decode() is false
    at the BACKREF and nothing behind it is looked up, so p1 and p2 stay at the
    LRU tail and the follow-up's enters evict them."""
    b, s, p1, p2, fill = _tail_setup(o, 0xE6)
    c = [LIT + b.x(0, s[62]) + B(200) + R(o.hash(p1)) + R(o.hash(p2)), X(s[63]), R(o.hash(p1)) + X(s[64])]
    b.steps.append(('batch', c))
    _tail_followup(o, b, s, p1, p2, fill)
    return _case('error_stop_no_skim', b, 'skim')


def case_unknown_stop_skims(o):
    """The mirror: an unknown REF first, the BACKREF to an empty slot behind
    it: status 1, the skim refreshes p1 and p2 and never examines the BACKREF."""
    b, s, p1, p2, fill = _tail_setup(o, 0xE7)
    c = [LIT + b.x(0, s[62]) + R(UNKNOWN) + B(200) + R(o.hash(p1)) + R(o.hash(p2)), X(s[63]), R(o.hash(fill[0])) + X(s[64])]
    b.steps.append(('batch', c, {k: 0 for k in KINDS}))
    _tail_followup(o, b, s, p1, p2, fill)
    return _case('unknown_stop_skims', b, None)


def _both_stops(o, name, seed, chunks_of, alt):
    b, s, p1, p2, fill = _tail_setup(o, seed)
    bad, unk, touch = B(200), R(UNKNOWN), R(o.hash(p1)) + R(o.hash(p2))
    c, ask = chunks_of(b, s, bad, unk, touch)
    b.steps.append(('batch', c, {k: ask for k in KINDS} if ask is not None else {}))
    _tail_followup(o, b, s, p1, p2, fill)
    return _case(name, b, alt)


def case_both_stops_ref_then_bref_chunks(o):
    return _both_stops(o, 'both_stops_ref_then_bref_chunks', 0xE8,
                       lambda b, s, bad, unk, touch: ([b.x(0, s[62]) + slot(b, s[62]) + unk + LIT, bad + touch, X(s[63])], 0), None)


def case_both_stops_bref_then_ref_chunks(o):
    return _both_stops(o, 'both_stops_bref_then_ref_chunks', 0xE9,
                       lambda b, s, bad, unk, touch: ([b.x(0, s[62]) + slot(b, s[62]) + bad + LIT, unk + touch, X(s[63])], None), 'skim')


def case_both_stops_ref_then_bref(o):
    return _both_stops(o, 'both_stops_ref_then_bref', 0xEA,
                       lambda b, s, bad, unk, touch: ([b.x(0, s[62]) + slot(b, s[62]) + unk + bad + touch, touch + X(s[63])], 0), None)


def case_both_stops_bref_then_ref(o):
    return _both_stops(o, 'both_stops_bref_then_ref', 0xEB,
                       lambda b, s, bad, unk, touch: ([b.x(0, s[62]) + slot(b, s[62]) + bad + unk + touch, touch + X(s[63])], None), 'skim')


def case_many_backrefs_few_references(o):
    """8 cache references and 500 BACKREFs in one call on the 64-segment
    cache: BACKREFs are no references, so the call is within the limit."""
    b = Builder(o, 1)
    s = rnd_segs(0xEC, 20)
    b.steps.append(('learn', s[:12]))
    rng = random.Random(0xEC)
    head = b''.join(b.r(0, q) for q in s[:4]) + xs(b, s[12:16])
    c = [head + b''.join(B(rng.randrange(8)) for _ in range(300)) + LIT, b''.join(B(rng.randrange(8)) for _ in range(200))]
    b.steps.append(('batch', c))
    b.steps.append(('probe',))
    # (the four REFs refreshed s[0..3]; 500 lookups of the slots' hashes would have refreshed all eight alike)
    b.steps.append(('batch', [xs(b, s[16:20]) + b''.join(R(o.hash(q)) for q in s[4:12])]))
    fill = rnd_segs(0xEC0, 50)
    b.steps.append(('batch', [xs(b, fill[:25]), xs(b, fill[25:])]))
    b.steps.append(('batch', [b''.join(R(o.hash(q)) for q in s[:4])]))
    return _case('many_backrefs_few_references', b)


def case_pair_replace_then_backref(o):
    """The slot is declared by a REF to cached bytes; a later chunk EXTRACTs
    the same hash with other bytes (a REPLACE against the cache).  The
    re-declare cleared the old slot; the new slot gives the new bytes.
    ('alt' None: the window and the cache hold the same bytes throughout.  They
    differ only after a replace the decoder's window does not see, a <LEARN>,
    and there the reference's slot shares the segment the cache let go of:
    xcodec_cache.h:333-336.  REPLACE_CASE names the case: the reference runs
    it in a child process, as tests/test_pair_oracle.py runs its name reuse.)"""
    b = Builder(o, 1)
    fa, fb = family(0x5B)[:2]
    assert o.hash(fa) == o.hash(fb) and fa != fb
    s = rnd_segs(0xED, 6)
    b.steps.append(('learn', [s[0], fa, s[1]]))
    first = b.r(0, fa) + slot(b, fa) + b.x(0, s[2])
    old = b.slot_of(0, fa)
    c = [first, LIT + b.x(0, fb) + slot(b, fb) + b.r(0, fa) + slot(b, s[2]), slot(b, fb) + B(old) + b.x(0, s[3]), X(s[4])]
    assert old != b.slot_of(0, fb) and b.models[0].slot[old] == 0
    b.steps.append(('batch', c))
    b.steps.append(('probe',))
    b.steps.append(('decoder',))
    b.steps.append(('batch', [R(o.hash(fa)) + R(o.hash(s[2]))]))
    return _case(REPLACE_CASE, b, None)


REPLACE_CASE = 'pair_replace_then_backref'
BUILDERS = [case_evicted_in_batch, case_evicted_across_calls, case_ghit_then_evicted, case_ghit_run_then_evicted,
            case_window_larger_than_cache, case_error_stop_no_skim, case_unknown_stop_skims,
            case_both_stops_ref_then_bref_chunks, case_both_stops_bref_then_ref_chunks, case_both_stops_ref_then_bref,
            case_both_stops_bref_then_ref, case_many_backrefs_few_references, case_pair_replace_then_backref]


def all_cases(o):
    return [f(o) for f in BUILDERS]


# -------------------------------------------------------------------- fuzz

FUZZ_RATES, FUZZ_BAD, FUZZ_SEEDS, FUZZ_BATCHES = (0.05, 0.3), (0.0, 0.02), range(6), (1, 3, 6)
FUZZ_CHUNK, FUZZ_CHUNKS = 16384, 6         # a stream is at most 48 references: one call may hold all of it


def fuzz_case(o, rate, bad, batch):
    """stream_with_backrefs over synth data: six streams (seeds), each on a
    fresh decoder, one after the other on ONE cache -- about 290 segments
    through 64, so the cache evicts and the pair's disk laps while every REF of
    a stream still resolves (it names a segment of its own stream, at most 48
    enters back).  Decoded `batch` chunks a call, 6 being the whole stream; the
    streams do not depend on it.  A
    BACKREF to an empty slot (bad > 0) ends its decoder: the rest of that
    stream is not presented."""
    from wanproxy_amd import synth
    steps = []
    for seed in FUZZ_SEEDS:
        data = synth.stream(0xBF00 + seed, FUZZ_CHUNK * FUZZ_CHUNKS, 60, 1)
        encs = stream_with_backrefs(o, data, FUZZ_CHUNK, 0xC00 + seed, rate, bad)
        steps.append(('decoder',))
        steps += [('batch', encs[a:a + batch]) for a in range(0, len(encs), batch)]
        steps.append(('probe',))
    return {'name': 'fuzz-%g-%g-%d' % (rate, bad, batch), 'alt': 'window', 'steps': steps}


def fuzz_cases(o, rate, bad):
    return [fuzz_case(o, rate, bad, batch) for batch in FUZZ_BATCHES]
