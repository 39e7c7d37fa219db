"""Cases for decode batches over several BACKREF windows (test infrastructure,
no GPU in here): the chunks are successive XCodecDecoder::decode calls of
several decoders -- one XCodecWindow each -- on one cache.

A case is {'name', 'n_windows', 'steps'}; a step is
    ('learn', [segments])             new segments enter the shared cache (a <LEARN> each)
    ('batch', [chunks], [window of each chunk])
    ('probe',)                        what every slot of every window holds
run_model() runs a case on the yardstick: `n_windows` decoders made by
Oracle.decoder_new on one cache_new() cache, the chunks decoded one by one in
order; a batch ends at its first unknown REF or BACKREF to an empty slot, and
the chunks behind that are not decoded (status 2).  `single=True` runs every
chunk on ONE decoder instead: the BACKREF cases must come out different, or a
one-window implementation would pass them.

The streams are built op by op; each builder keeps a WindowModel per window
(backref_streams) to aim its BACKREFs.
"""
import struct

import numpy as np

from backref_streams import MAGIC, SEG, WindowModel
from collision_cases import family

LIT = b'windows-literal-\xf1\x00-run '          # (holds one escaped F1)


def rnd_segs(seed, n):
    a = np.random.default_rng([0xD3C0, int(seed)]).integers(0, 256, n * SEG, dtype=np.uint8).tobytes()
    return [a[k * SEG:(k + 1) * SEG] for k in range(n)]


def X(seg):
    return bytes([MAGIC, 0x01]) + seg


def R(h):
    return bytes([MAGIC, 0x02]) + struct.pack('>Q', h)


def B(idx):
    return bytes([MAGIC, 0x03, idx])


def walk(enc: bytes):
    """Whole ops of a stream with BACKREFs: (kind, offset, end) with kind 'x',
    'r', 'b'; stops at a cut op."""
    i, n = 0, len(enc)
    while i < n:
        if enc[i] != MAGIC:
            i += 1
            continue
        if i + 1 >= n:
            return
        op = enc[i + 1]
        size = {0x00: 2, 0x01: 2 + SEG, 0x02: 10, 0x03: 3}[op]
        if i + size > n:
            return
        if op:
            yield 'xrb'[op - 1], i, i + size
        i += size


def probe_window(decode1):
    """Every slot of a window through BACKREFs alone (they declare nothing, and
    one to an empty slot only fails its call): decode1(chunk) -> (status, out,
    consumed) on that window.  Returns 256 entries, bytes or None."""
    res, k = [None] * 256, 0
    while k < 256:
        st, out, cons = decode1(b''.join(B(c) for c in range(k, 256)))
        live = len(out) // SEG
        assert len(out) == live * SEG
        for j in range(live):
            res[k + j] = out[j * SEG:(j + 1) * SEG]
        if st == 0:
            assert k + live == 256
            break
        assert st == -1 and cons == 3 * (live + 1), (st, cons, live)
        k += live + 1
    return res


def status_of(ok, consumed, unknown, length):
    if not ok:
        return -1
    if unknown:
        return 1
    return 3 if consumed < length else 0


def run_model(oracle, case, single=False):
    """The case on `oracle` (the C oracle or the reference through the same
    interface).  Returns (results, cache): one result per step -- None for a
    learn, {'outs', 'status', 'consumed', 'stop'} for a batch, [[256 entries]
    per window] for a probe -- and the cache's {hash: bytes} at the end."""
    cache = oracle.cache_new()
    decs = [oracle.decoder_new(cache) for _ in range(1 if single else case['n_windows'])]
    dec = (lambda w: decs[0]) if single else (lambda w: decs[w])
    held, results = {}, []
    try:
        for step in case['steps']:
            if step[0] == 'learn':
                for seg in step[1]:          # (entered through a decoder of its own: no window of the case moves)
                    assert oracle.hash(seg) not in held and oracle.decode(X(seg), cache)[0]
                    held[oracle.hash(seg)] = seg
                results.append(None)
            elif step[0] == 'batch':
                chunks, cw = step[1], step[2]
                n = len(chunks)
                outs, st, cons, stop = [], [], [], n
                for i, (e, w) in enumerate(zip(chunks, cw)):
                    if stop < n:
                        outs.append(b'')
                        st.append(2)
                        cons.append(0)
                        continue
                    ok, out, c, unk = oracle.decode(e, cache, decoder=dec(w))
                    s = status_of(ok, c, unk, len(e))
                    outs.append(out)
                    st.append(s)
                    cons.append(c)
                    for kind, a, b in walk(e[:c]):
                        if kind == 'x':
                            held[oracle.hash(e[a + 2:b])] = e[a + 2:b]
                    if s in (1, -1):
                        stop = i
                results.append({'outs': outs, 'status': st, 'consumed': cons, 'stop': stop})
            else:
                def one(w):
                    def decode1(chunk):
                        ok, out, c, unk = oracle.decode(chunk, cache, decoder=dec(w))
                        return status_of(ok, c, unk, len(chunk)), out, c
                    return decode1
                results.append([probe_window(one(w)) for w in range(case['n_windows'])])
    finally:
        for d in decs:
            oracle.decoder_free(d)
        oracle.cache_free(cache)
    return results, held


class Builder:
    """Chunks op by op, with a WindowModel per window for the BACKREF indices."""

    def __init__(self, oracle, n_windows):
        self.o = oracle
        self.n_windows = n_windows
        self.models = [WindowModel() for _ in range(n_windows)]
        self.steps = []

    def declare(self, w, h):
        self.models[w].declare(h)

    def x(self, w, seg):
        self.declare(w, self.o.hash(seg))
        return X(seg)

    def r(self, w, seg_or_hash):
        h = seg_or_hash if isinstance(seg_or_hash, int) else self.o.hash(seg_or_hash)
        self.declare(w, h)
        return R(h)

    def slot_of(self, w, seg):
        """The slot of window w that holds seg's hash now."""
        return self.models[w].slot.index(self.o.hash(seg))

    def own_slot(self, w, seg):
        """B() of that slot, which every other window holds differently (another hash or nothing)."""
        k = self.slot_of(w, seg)
        for v in range(self.n_windows):
            assert v == w or self.models[v].slot[k] != self.models[w].slot[k], (w, v, k)
        return B(k)

    def bref(self, w, pick):
        """B() of a live slot of window w that every other window holds
        differently: the pick-th such slot (Python indexing)."""
        m = self.models
        ks = [k for k in m[w].live() if all(v == w or m[v].slot[k] != m[w].slot[k] for v in range(self.n_windows))]
        assert ks, (w, 'no slot tells this window from the others')
        return B(ks[pick % len(ks)])

    def case(self, name):
        return {'name': name, 'n_windows': self.n_windows, 'steps': self.steps}


def case_interleave(oracle):
    """3 windows, 7 chunks in window order 0,1,0,2,1,0,2: EXTRACTs, REFs to the
    EXTRACTs of other windows' chunks, BACKREFs to the chunk's own window."""
    b = Builder(oracle, 3)
    s = rnd_segs(1, 12)
    c = []
    c.append(LIT + b.x(0, s[0]) + b.x(0, s[1]) + b.bref(0, 0) + b'a')                                # w0: 2 declares
    c.append(b.x(1, s[2]) + LIT + b.r(1, s[1]) + b.r(1, s[0]) + b.x(1, s[3]) + b.bref(1, 0) + b.bref(1, -1))   # w1: 4
    c.append(b.r(0, s[2]) + b.bref(0, -1) + b.x(0, s[4]) + b.bref(0, 0) + LIT)                          # w0: 4
    c.append(b.x(2, s[5]) + b.bref(2, 0) + b.r(2, s[4]) + b.r(2, s[3]) + b.r(2, s[0]) + b.x(2, s[6]) +
             b.x(2, s[7]) + b.bref(2, 1) + b.bref(2, -1))                                                # w2: 6
    c.append(LIT + b.r(1, s[5]) + b.bref(1, -1) + b.bref(1, 1) + b.x(1, s[8]))                           # w1: 6
    c.append(b.r(0, s[8]) + b.r(0, s[6]) + b.x(0, s[9]) + b.bref(0, -1) + b.bref(0, 2) + b'z')          # w0: 7
    c.append(b.r(2, s[9]) + b.bref(2, -1) + b.bref(2, 3) + LIT + b.x(2, s[10]))                          # w2: 8
    b.steps.append(('batch', c, [0, 1, 0, 2, 1, 0, 2]))
    b.steps.append(('probe',))
    return b.case('interleave')


def case_wrap(oracle):
    """Tail records per window, slots emptied by a re-declare, cursors: counts
    that are no multiple of 256, then 300 declares of one hash in one window
    and 5 in another in one batch, then every slot read."""
    b = Builder(oracle, 2)
    s = rnd_segs(2, 16)
    b.steps.append(('learn', [s[15]]))
    first = [b''.join(b.x(0, s[k]) for k in range(7)) + b.own_slot(0, s[3]),
             b''.join(b.x(1, s[k]) for k in range(7, 10)) + b.r(1, s[2])]
    b.steps.append(('batch', first, [0, 1]))
    big = b''.join(b.r(0, s[15]) for _ in range(300))
    small = b''.join(b.x(1, s[k]) for k in range(10, 13)) + b.r(1, s[15]) + b.r(1, s[7])
    b.steps.append(('batch', [big[:1500], small, big[1500:]], [0, 1, 0]))
    b.steps.append(('probe',))
    return b.case('wrap')


def case_stop_ref(oracle):
    """6 chunks on 3 windows, an unknown REF in the middle of chunk 3: statuses
    0,0,0,1,2,2; then a <LEARN> and the rest of chunk 3 with chunks 4 and 5."""
    b = Builder(oracle, 3)
    s = rnd_segs(3, 12)
    missing = s[11]
    c = [b.x(0, s[0]) + LIT + b.x(0, s[1]),
         b.x(1, s[2]) + b.r(1, s[0]) + b.own_slot(1, s[0]),
         b.x(2, s[3]) + b.r(2, s[2]) + LIT,
         None, None, None]
    head = LIT + b.x(1, s[4]) + b.r(1, s[3]) + b.own_slot(1, s[4])
    rest = b.r(1, missing) + b.x(1, s[5]) + b.own_slot(1, missing) + LIT
    c[3] = head + rest
    c[4] = b.r(0, s[5]) + b.x(0, s[6]) + b.own_slot(0, s[5])
    c[5] = b.r(2, s[6]) + b.r(2, missing) + b.own_slot(2, s[6]) + b.x(2, s[7])
    cw = [0, 1, 2, 1, 0, 2]
    b.steps.append(('batch', c, cw))
    b.steps.append(('probe',))            # each window advanced only by the declares before the stop
    b.steps.append(('learn', [missing]))
    b.steps.append(('batch', [rest, c[4], c[5]], cw[3:]))
    b.steps.append(('probe',))
    case = b.case('stop_ref')
    case['expect'] = {0: {'status': [0, 0, 0, 1, 2, 2], 'stop': 3, 'consumed3': len(head)}}
    return case


def case_stop_empty_slot(oracle):
    """A BACKREF to a slot that is empty in its own window and live in
    another's: status -1 there, consumed past the op, the rest not reached."""
    b = Builder(oracle, 2)
    s = rnd_segs(4, 6)
    c = [b.x(0, s[0]) + b.x(0, s[1]) + b.x(0, s[2]),
         b.x(1, s[3]) + b.own_slot(1, s[3]) + LIT + B(2) + b.x(1, s[4]),
         b.x(0, s[5])]
    assert b.models[0].slot[2] != 0
    b.steps.append(('batch', c, [0, 1, 0]))
    b.steps.append(('probe',))
    case = b.case('stop_empty_slot')
    case['expect'] = {0: {'status': [0, -1, 2], 'stop': 1, 'consumed1': 2 + SEG + 3 + len(LIT) + 3}}
    return case


def case_name_reuse(oracle):
    """EXTRACT A in window 0, EXTRACT B of the same hash in window 1, REFs in
    both windows after each, BACKREFs to the slots that declared A and B."""
    b = Builder(oracle, 2)
    fa, fb = family(0x51)[:2]
    assert oracle.hash(fa) == oracle.hash(fb) and fa != fb
    s = rnd_segs(5, 5)
    c = [b.x(0, s[0]) + b.x(0, fa) + b.own_slot(0, fa) + b.r(0, fa) + b.own_slot(0, fa),      # A, A, A
         b.x(1, fb) + b.own_slot(1, fb) + b.x(1, s[1]) + b.x(1, s[2]) + b.r(1, fb) + b.own_slot(1, fb),   # B, B, B
         # A (window 0's own copy, though the cache now holds B), then B, B
         b.own_slot(0, fa) + b.x(0, s[3]) + b.r(0, fa) + b.own_slot(0, fa) + LIT,
         b.own_slot(1, fb) + b.r(1, s[0]) + b.r(1, fa)]
    b.steps.append(('batch', c, [0, 1, 0, 1]))
    b.steps.append(('probe',))
    b.steps.append(('batch', [b.x(0, s[4]) + b.r(0, fb) + b.own_slot(0, fb), b.own_slot(1, fa)], [0, 1]))
    case = b.case('name_reuse')
    case['expect'] = {0: {'out2': fa + s[3] + fb + fb + LIT.replace(b'\xf1\x00', b'\xf1')}}
    return case


def case_partial_op(oracle):
    """Status 3 in one chunk (an EXTRACT cut short), the following chunks of
    other windows decoded."""
    b = Builder(oracle, 3)
    s = rnd_segs(6, 6)
    c = [b.x(0, s[0]) + LIT,
         b.x(1, s[1]) + b.own_slot(1, s[1]) + X(s[2])[:700],
         b.r(2, s[0]) + b.r(2, s[1]) + b.own_slot(2, s[1]),
         b.x(0, s[3]) + b.r(0, s[1]) + b.own_slot(0, s[1])]
    b.steps.append(('batch', c, [0, 1, 2, 0]))
    b.steps.append(('probe',))
    case = b.case('partial_op')
    case['expect'] = {0: {'status': [0, 3, 0, 0], 'stop': 4}}
    return case


BUILDERS = [case_interleave, case_wrap, case_stop_ref, case_stop_empty_slot, case_name_reuse, case_partial_op]
# the cases whose BACKREFs tell one window from several
BACKREF_CASES = ('interleave', 'wrap', 'stop_ref', 'stop_empty_slot', 'name_reuse', 'partial_op')


def all_cases(oracle):
    return [f(oracle) for f in BUILDERS]
