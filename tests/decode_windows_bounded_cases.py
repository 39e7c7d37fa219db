"""Cases for decode batches over several BACKREF windows on a BOUNDED cache or
a PAIR (test infrastructure, no GPU in here): the contract of
xcg_decode_batch_windows_bounded.

The chunks of a batch are successive XCodecDecoder::decode calls of several
decoders -- one XCodecWindow each -- on one XCodecMemoryCache(uuid, limit) or
XCodecCachePair, so every EXTRACT and REF sees what the chunks before it did to
the cache (enters, LRU refreshes, evictions, promotions, disk writes),
whichever window they name.  A case is {'name', 'n_windows', 'steps'} and may
set 'limit_segs' and 'disk' (default: backref_bounded_cases' geometry); a step
is
    ('learn', [segments])        enter segments through a decoder of their own
    ('batch', [chunks], [window of each chunk])
    ('batch', [chunks], [windows], kinds)   the same, and the call REFUSES the
                                 batch as a whole on the kinds named
    ('rest',)                    the remainder of the chunk the last batch
                                 stopped in at an unknown REF, in one decode()
                                 on that chunk's decoder
    ('probe',)                   what every slot of every window holds

run_model() is the yardstick.  A batch is decoded chunk by chunk and ends at
its first unknown REF or BACKREF to an empty slot; the chunks behind are not
decoded (status 2).  The call makes no lookup behind its stop point, so the
model decodes a chunk ONE OP AT A TIME (a decode() call per op, each with the
literal bytes in front of it: the decoder keeps nothing between calls but its
window and the cache): the call on the stopping op looks at nothing behind it.
A 'rest' step then hands the stopped chunk from its stop on to decode() in one
piece: that call blocks on its first op and skims the rest (decode_skim,
xcodec_decoder.cc:196-272) -- on these caches every REF the skim finds
refreshes, promotes and may evict.  A refused batch changes nothing; the model
then decodes its chunks whole, one decode() each, as the caller of a refused
batch does ('serial').  `single=True` runs every chunk on ONE decoder.

Every batch holds at most the limit's worth of EXTRACT + REF ops, so no call
on a bounded context comes near what xcg_decode_batch declines; the refusal
cases say so themselves.
"""
from backref_bounded_cases import DISK, LIMIT_SEGS, UNKNOWN
from backref_streams import SEG
from collision_cases import family
from decode_windows_cases import LIT, B, Builder, R, X, probe_window, rnd_segs, status_of, walk

KINDS = ('bounded', 'pair', 'unbounded')
DISK_4 = (18 + 4 * 205) * SEG          # four index blocks: 816 entries


def geometry(case):
    return case.get('limit_segs', LIMIT_SEGS) * SEG, case.get('disk', DISK)


def new_cache(o, case, kind):
    limit, disk = geometry(case)
    if kind == 'bounded':
        return o.cache_new(limit)
    if kind == 'pair':
        return o.cache_new_pair(limit, disk)
    return o.cache_new()


def pieces(e: bytes):
    """A chunk cut behind every whole op: each piece is one op with the
    literal bytes in front of it; the last is what follows the last op."""
    cuts, at = [], 0
    for _, _, z in walk(e):
        cuts.append(e[at:z])
        at = z
    if at < len(e) or not cuts:
        cuts.append(e[at:])
    return cuts


def hashes_of(o, case):
    """Every hash the case names, sorted: EXTRACT and <LEARN> payloads, REFs."""
    hs = set()
    for step in case['steps']:
        if step[0] == 'learn':
            hs |= {o.hash(s) for s in step[1]}
        elif step[0] == 'batch':
            for e in step[1]:
                for kind, a, z in walk(e):
                    if kind == 'x':
                        hs.add(o.hash(e[a + 2:z]))
                    elif kind == 'r':
                        hs.add(int.from_bytes(e[a + 2:z], 'big'))
    return sorted(hs)


def lru_order(o, cache, case):
    """The hashes of a bounded cache, least recently used first (C oracle)."""
    import ctypes as C

    import numpy as np
    cap = case.get('limit_segs', LIMIT_SEGS)
    keys = np.zeros(cap, dtype=np.uint64)
    n = int(o.lib.xco_cache_export(cache, keys.ctypes.data_as(C.POINTER(C.c_uint64)), None, cap))
    return [int(k) for k in keys[:n]]


def refused_on(step, kind):
    return len(step) > 3 and kind in step[3]


def run_model(o, case, kind, single=False):
    """The case on oracle `o` (the C oracle or the compiled reference) and a
    cache of `kind`.  One result per step: None for a learn; {'outs', 'status',
    'consumed', 'stop', 'order'} for a batch ({'refused': True, 'serial': [(status,
    out, consumed, unknown) per chunk], 'order'} for a refused one); {'status',
    'out', 'consumed', 'unknown', 'order'} for a rest (None when the last batch
    did not stop at an unknown REF); [[256 entries] per window] for a probe.
    'order': a bounded cache's hashes in LRU order behind that step (C oracle;
    None otherwise).  Last, the cache's account: {'order', 'pair_stats',
    'found': is each of hashes_of() found -- a REF each, in that order, through
    a decoder of its own}."""
    cache = new_cache(o, case, kind)
    decs = [o.decoder_new(cache) for _ in range(1 if single else case['n_windows'])]
    dec = (lambda w: decs[0]) if single else (lambda w: decs[w])
    order = lambda: lru_order(o, cache, case) if kind == 'bounded' and not o.ref else None
    results, rest = [], None
    try:
        for step in case['steps']:
            if step[0] == 'learn':
                for seg in step[1]:
                    assert o.decode(X(seg), cache)[0]
                results.append(None)
            elif step[0] == 'probe':
                def one(w):
                    def decode1(chunk):
                        ok, out, c, unk = o.decode(chunk, cache, decoder=dec(w))
                        return status_of(ok, c, unk, len(chunk)), out, c
                    return decode1
                results.append([probe_window(one(w)) for w in range(case['n_windows'])])
            elif step[0] == 'rest':
                if rest is None:
                    results.append(None)
                    continue
                w, e = rest
                rest = None
                ok, out, c, unk = o.decode(e, cache, decoder=dec(w))
                results.append({'status': status_of(ok, c, unk, len(e)), 'out': out, 'consumed': c,
                                'unknown': sorted(set(unk)), 'order': order()})
            elif refused_on(step, kind):
                serial = []
                for e, w in zip(step[1], step[2]):
                    ok, out, c, unk = o.decode(e, cache, decoder=dec(w))
                    serial.append((status_of(ok, c, unk, len(e)), out, c, sorted(set(unk))))
                rest = None
                results.append({'refused': True, 'serial': serial, 'order': order()})
            else:
                chunks, cw = step[1], step[2]
                n = len(chunks)
                outs, st, cons, stop = [], [], [], n
                rest = None
                for i, (e, w) in enumerate(zip(chunks, cw)):
                    if stop < n:
                        outs.append(b'')
                        st.append(2)
                        cons.append(0)
                        continue
                    out, at, s = b'', 0, 0
                    for p in pieces(e):
                        ok, o1, c, unk = o.decode(p, cache, decoder=dec(w))
                        out += o1
                        at += c
                        s = status_of(ok, c, unk, len(p))
                        if s:
                            break
                    outs.append(out)
                    st.append(s)
                    cons.append(at)
                    if s in (1, -1):
                        stop = i
                        if s == 1:
                            rest = (w, e[at:])
                results.append({'outs': outs, 'status': st, 'consumed': cons, 'stop': stop, 'order': order()})
        found = []
        for h in hashes_of(o, case):
            ok, _, _, unk = o.decode(R(h), cache)
            found.append(bool(ok and not unk))
        results.append({'order': order(), 'pair_stats': o.pair_stats(cache) if kind == 'pair' else None,
                        'found': found})
    finally:
        for d in decs:
            o.decoder_free(d)
        o.cache_free(cache)
    return results


def without_order(results):
    """The results with the LRU orders taken out (the C oracle's alone)."""
    return [{k: v for k, v in r.items() if k != 'order'} if isinstance(r, dict) else r for r in results]


def batch_ops(step):
    """EXTRACT + REF ops of a batch step."""
    return sum(1 for e in step[1] for kind, _, _ in walk(e) if kind in 'xr')


# ------------------------------------------------------------------- cases

def xs(b, w, segs):
    return b''.join(b.x(w, s) for s in segs)


def case_cross_refs(o):
    """(a) Window 0's EXTRACT is REF'd by a chunk on window 1, and the
    reverse, with BACKREFs that tell the windows apart."""
    b = Builder(o, 2)
    s = rnd_segs(0xA1, 6)
    c = [LIT + b.x(0, s[0]) + b.x(0, s[1]),
         b.x(1, s[2]) + b.r(1, s[0]) + b.own_slot(1, s[0]) + LIT,
         b.r(0, s[2]) + b.own_slot(0, s[2]) + b.x(0, s[3]) + b.own_slot(0, s[1]),
         b.r(1, s[3]) + b.r(1, s[1]) + b.own_slot(1, s[3]) + b'z']
    b.steps.append(('batch', c, [0, 1, 0, 1]))
    b.steps.append(('probe',))
    return b.case('cross_refs')


def case_evict_then_ref(o):
    """(b) A full cache: window 0's one EXTRACT evicts the oldest entry, and
    window 1's chunk REFs that entry: the stop (a pair finds it on disk)."""
    b = Builder(o, 2)
    f = rnd_segs(0xB1, LIMIT_SEGS)
    s = rnd_segs(0xB2, 3)
    b.steps.append(('learn', f))
    c = [LIT + b.x(0, s[0]) + b.own_slot(0, s[0]), b.x(1, s[1]) + b.r(1, f[0]) + b.own_slot(1, s[1]), b.x(0, s[2])]
    b.steps.append(('batch', c, [0, 1, 0]))
    b.steps.append(('rest',))
    b.steps.append(('probe',))
    return b.case('evict_then_ref')


def case_ref_then_evict(o):
    """(b), mirrored: the REF comes first and refreshes the oldest entry, so
    the EXTRACT behind it evicts the next oldest; a REF to that one stops."""
    b = Builder(o, 2)
    f = rnd_segs(0xB3, LIMIT_SEGS)
    s = rnd_segs(0xB4, 3)
    b.steps.append(('learn', f))
    c = [b.r(1, f[0]) + b.own_slot(1, f[0]), LIT + b.x(0, s[0]), b.r(1, f[0]) + b.x(1, s[1]) + b.r(1, f[1]) + LIT,
         b.x(0, s[2])]
    b.steps.append(('batch', c, [1, 0, 1, 0]))
    b.steps.append(('rest',))
    b.steps.append(('probe',))
    return b.case('ref_then_evict')


def case_slots_outlive_cache(o):
    """(c) Windows 0 and 1 declare different segments at slot 0; a batch on
    window 3 evicts both hashes; then each window's BACKREF to slot 0 gives its
    own bytes, and window 2's, whose slot 0 is empty, is the stop (-1).  A last
    batch REFs the two hashes: unknown where the cache let go of them."""
    b = Builder(o, 4)
    s = rnd_segs(0xC1, 4)
    fill = rnd_segs(0xC2, LIMIT_SEGS)
    b.steps.append(('batch', [b.x(0, s[0]) + LIT, b.x(1, s[1])], [0, 1]))
    assert b.slot_of(0, s[0]) == 0 and b.slot_of(1, s[1]) == 0
    b.steps.append(('batch', [xs(b, 3, fill[:40]), xs(b, 3, fill[40:])], [3, 3]))
    c = [B(0) + LIT, b'q' + B(0), LIT + B(0) + X(s[2]), X(s[3])]
    b.steps.append(('batch', c, [0, 1, 2, 0]))
    b.steps.append(('probe',))
    b.steps.append(('batch', [R(o.hash(fill[63])) + R(o.hash(s[1])), R(o.hash(s[0]))], [1, 0]))
    b.steps.append(('rest',))
    return b.case('slots_outlive_cache')


def case_stop_leaves_lru(o):
    """(d) A stop in the middle chunk and, behind it in that chunk, a REF to
    the least recently used entry: after the batch that entry is still the
    oldest, after the rest step (the skim) it is the newest.  The chunks behind
    are status 2 and decode in the next batch; enters then evict the tail and
    REFs show who went."""
    b = Builder(o, 2)
    f = rnd_segs(0xD1, 60)
    s = rnd_segs(0xD2, 12)
    missing = s[11]
    b.steps.append(('learn', f))
    head = b.x(1, s[1]) + LIT
    tail = b.r(1, missing) + LIT + b.r(1, f[0]) + b.x(1, s[2]) + b.own_slot(1, s[1])
    c = [b.x(0, s[0]), head + tail, b.x(0, s[3]) + b.own_slot(0, s[0])]
    b.steps.append(('batch', c, [0, 1, 0]))
    b.steps.append(('rest',))
    b.steps.append(('learn', [missing]))
    b.steps.append(('batch', [tail, c[2]], [1, 0]))
    b.steps.append(('batch', [xs(b, 0, s[4:8])], [0]))
    b.steps.append(('batch', [R(o.hash(f[0])), R(o.hash(f[1]))], [0, 1]))
    b.steps.append(('rest',))
    b.steps.append(('probe',))
    case = b.case('stop_leaves_lru')
    case['expect'] = {'f0': o.hash(f[0])}
    return case


def case_pair_promote(o):
    """(e) 70 segments through the 64-segment memory level: a REF to one the
    memory level let go of is unknown on a bounded cache; a pair finds it on
    disk and promotes it, which evicts the memory level's oldest entry, and a
    later chunk on another window names that one (on disk again).  Three
    batches of EXTRACTs then lap the disk's one index block, and the REF is
    unknown on the pair too."""
    b = Builder(o, 3)
    f = rnd_segs(0xE1, 70)
    fill = rnd_segs(0xE2, 3 * LIMIT_SEGS)
    b.steps.append(('learn', f))
    c = [LIT + b.r(0, f[0]) + b.own_slot(0, f[0]), b.r(1, f[6]) + b.r(1, f[0]) + b.own_slot(1, f[6]), b.r(0, f[7]) + LIT]
    b.steps.append(('batch', c, [0, 1, 0]))
    b.steps.append(('rest',))
    for k in range(3):
        part = fill[LIMIT_SEGS * k:LIMIT_SEGS * (k + 1)]
        b.steps.append(('batch', [xs(b, 2, part[:30]), xs(b, 2, part[30:])], [2, 2]))
    b.steps.append(('batch', [b.own_slot(0, f[0]) + R(o.hash(fill[-1])), R(o.hash(f[1])) + LIT], [0, 1]))
    b.steps.append(('rest',))
    b.steps.append(('probe',))
    return b.case('pair_promote')


def case_interleave(o):
    """(f) Three chunks of window 0 interleaved with window 1's, a window no
    chunk names, an empty chunk and an EXTRACT cut short at a chunk's end."""
    b = Builder(o, 3)
    s = rnd_segs(0xF1, 8)
    c = [b.x(0, s[0]) + LIT + b.x(0, s[1]),
         b.x(1, s[2]) + b.own_slot(1, s[2]) + b.r(1, s[0]),
         b'',
         b.r(0, s[2]) + b.own_slot(0, s[1]) + X(s[3])[:700],
         b.r(1, s[1]) + b.own_slot(1, s[1]) + LIT,
         b.x(0, s[4]) + b.own_slot(0, s[2]) + b.own_slot(0, s[4])]
    b.steps.append(('batch', c, [0, 1, 0, 0, 1, 0]))
    b.steps.append(('probe',))
    case = b.case('interleave')
    case['expect'] = {'status': [0, 0, 0, 3, 0, 0]}
    return case


def case_slot_wrap(o):
    """(g) On a limit of 320 segments, window 0 takes 260 declares in one
    batch -- its slots wrap -- with a chunk of window 1 in between; BACKREFs
    then read a slot the wrap wrote over and one it did not."""
    b = Builder(o, 2)
    s = rnd_segs(0x61, 264)
    c = [xs(b, 0, s[:60]), xs(b, 0, s[60:120]), xs(b, 1, s[260:263]) + b.r(1, s[5]), xs(b, 0, s[120:180]),
         xs(b, 0, s[180:240]), xs(b, 0, s[240:260]) + b.own_slot(0, s[258]) + b.own_slot(0, s[10]) + LIT,
         b.own_slot(1, s[5]) + b.x(1, s[263])]
    assert b.slot_of(0, s[258]) == 2 and b.slot_of(0, s[10]) == 10
    b.steps.append(('batch', c, [0, 0, 1, 0, 0, 0, 1]))
    b.steps.append(('probe',))
    case = b.case('slot_wrap')
    case['limit_segs'] = 320
    case['disk'] = DISK_4
    return case


def case_refused_name_reuse(o):
    """(h) Two EXTRACTs of one hash with different bytes, in chunks of two
    windows: refused as a whole on bounded and pair contexts, nothing changed."""
    b = Builder(o, 2)
    fa, fb = family(0x5D)[:2]
    assert o.hash(fa) == o.hash(fb) and fa != fb
    s = rnd_segs(0x71, 3)
    b.steps.append(('batch', [b.x(0, s[0]) + b.own_slot(0, s[0]), b.x(1, s[1])], [0, 1]))
    c = [b.x(0, fa) + LIT, b.x(1, s[2]) + b.x(1, fb)]
    b.steps.append(('batch', c, [0, 1], ('bounded', 'pair')))
    b.steps.append(('probe',))
    return b.case('refused_name_reuse')


def case_refused_over_limit(o):
    """(h) 65 distinct EXTRACTs on a limit of 64: more enters than the limit,
    which a bounded context refuses (a pair's disk level takes what the memory
    level lets go of, and xcg_decode_batch declines nothing there either)."""
    b = Builder(o, 2)
    s = rnd_segs(0x72, 66)
    c = [xs(b, 0, s[:33]), xs(b, 1, s[33:65]) + b.own_slot(1, s[40])]
    b.steps.append(('batch', c, [0, 1], ('bounded',)))
    b.steps.append(('probe',))
    return b.case('refused_over_limit')


BUILDERS = [case_cross_refs, case_evict_then_ref, case_ref_then_evict, case_slots_outlive_cache, case_stop_leaves_lru,
            case_pair_promote, case_interleave, case_slot_wrap, case_refused_name_reuse, case_refused_over_limit]
CASE_NAMES = [f.__name__[5:] for f in BUILDERS]
# whose batches may hold more EXTRACT + REF ops than LIMIT_SEGS: (g) by its own limit, (h) to be refused
OWN_LIMIT = {'slot_wrap': 320, 'refused_over_limit': None}
# a one-window decoder comes out different
SINGLE_DIFFERS = ('slots_outlive_cache', 'slot_wrap')
# an unbounded cache comes out different from the bounded one
UNBOUNDED_DIFFERS = ('evict_then_ref', 'ref_then_evict', 'slots_outlive_cache', 'stop_leaves_lru')


def all_cases(o):
    return [f(o) for f in BUILDERS]
