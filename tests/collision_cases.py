"""Constructed XCodecHash collisions for the encoder tests: blocks related by
hash tier, a plain Python model of XCodecEncoder::encode that can be made
deliberately wrong, and the cases built from both.  No GPU in here.

XCodecHash (xcodec/xcodec_hash.h:117-174) is two pairs of position-weighted
sums over the 2048 bytes: s1 = sum (x_k + 1), s2 = sum (2048 - k)(x_k + 1) over
the bytes, and b1, b2 the same over ffs(x_k).  The 64-bit hash is
((b1 << 16) + b2) << 36 plus (s1 << 20) + s2 in 32 bits, so its low 32 bits
(`lo`) come from the bytes alone and the high 28 from the ffs() values alone.

- adding +2, -4, +2 to three neighbouring bytes keeps s1 and s2; on odd bytes
  ffs() stays 1, so the whole hash is kept ('full');
- the same change from 6, 12, 6 to 8, 8, 8 keeps s1 and s2 and moves the
  ffs() sums: equal `lo`, different `hi` ('lo');
- x[2046] += 1, x[2047] -= 2 keeps X2 = sum (2048 - k) x_k, the value the
  independent kernel's direct-mapped table is probed by, and changes s1, so
  `lo` differs ('key').

The encoder skips a window whose hash is declared for other bytes
(xcodec_encoder.cc:215-216, :390-406): it is no REF and no candidate.  Whether
"no candidate" can be observed depends on the parse state: while an earlier
candidate is pending, a miss would not have become the candidate either.  So
each case names the wrong policies (see encode_model) that must change its
output: `*_is_ref` always, `*_is_miss` / `*_is_collision` only where no
candidate is pending at the twin's window.
"""
from __future__ import annotations

import random
from collections import OrderedDict

import numpy as np

SEG = 2048
M32 = 0xFFFFFFFF
CLO = 0x80200400                      # (2048 << 20) + 2048 * 2049 / 2: lo = (sum x << 20) + X2 + CLO
LARGE = 131072 + SEG                  # the one chunk length of the large kernel class
AT = (0, 14, 30, 100, 1023, 2045)     # first / across byte 16 / across byte 32 / middle / last bytes
TIERS = ('full', 'lo', 'key', 'none')
POLICIES = ('exact', 'collision_is_miss', 'collision_is_ref', 'lo_is_collision', 'lo_is_ref', 'key_is_collision',
            'key_is_ref', 'no_touch')


def family(seed, nvar=3):
    """`nvar` distinct segments of one XCodecHash: a seeded base of odd bytes in
    7..201, variant j with +2, -4, +2 at offset 100 + 40 j."""
    r = random.Random(seed)
    base = bytearray(r.randrange(7, 202, 2) for _ in range(SEG))
    out = []
    for j in range(nvar):
        v = bytearray(base)
        o = 100 + 40 * j
        v[o] += 2
        v[o + 1] -= 4
        v[o + 2] += 2
        out.append(bytes(v))
    return out


def dm_key(block: bytes) -> int:
    """The direct-mapped probe key of a 2048-byte window: -(X2 + CLO) mod 2^32."""
    w = np.arange(SEG, 0, -1, dtype=np.uint64)
    x2 = int((w * np.frombuffer(block, np.uint8).astype(np.uint64)).sum()) & M32
    return (-(x2 + CLO)) & M32


def rnd(seed, n: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def twins(seed, tier: str, at: int = 100, nvar: int = 2):
    """`nvar` (2 or 3) different 2048-byte blocks related by `tier`; the bytes
    that differ are at [at, at + 3) ('key': at 2046 and 2047, whatever `at`)."""
    assert tier in TIERS and nvar in (2, 3)
    rng = np.random.default_rng([0xC011, int(seed)])
    if tier == 'none':
        return [rng.integers(0, 256, SEG, dtype=np.uint8).tobytes() for _ in range(nvar)]
    base = bytearray(rng.integers(0, 256, SEG, dtype=np.uint8).tobytes())
    if tier == 'key':
        pats = [(100 + j, 100 - 2 * j) for j in range(nvar)]
        at = SEG - 2
    else:
        assert 0 <= at <= SEG - 3
        pats = ([(101 + 2 * j, 101 - 4 * j, 101 + 2 * j) for j in range(nvar)] if tier == 'full'
                else [(6, 12, 6), (8, 8, 8), (7, 10, 7)][:nvar])
    out = []
    for p in pats:
        v = bytearray(base)
        v[at:at + len(p)] = bytes(p)
        out.append(bytes(v))
    return out


# ---------------------------------------------------------------------- model

_ORACLE = None


def _window_hashes(x: bytes) -> np.ndarray:
    global _ORACLE
    if _ORACLE is None:
        from oracle.lib import Oracle
        _ORACLE = Oracle()
    return _ORACLE.window_hashes(x)


class _Cache:
    """XCodecMemoryCache: hash -> segment, with `limit` segments the exact LRU
    of xcodec_cache.h:303-364 (enter evicts the least recently entered / used
    entry first; a lookup that finds the hash is a use).  Also indexed by `lo`
    and by the probe key, for the wrong policies."""

    def __init__(self, limit: int = 0):
        self.limit = limit
        self.d = OrderedDict()            # hash -> (segment, probe key), least recent first
        self.lo = {}                      # lo -> a hash holding it
        self.key = {}

    def use(self, h):
        self.d.move_to_end(h)

    def enter(self, h, seg, k):
        if h in self.d:                   # (wrong policies only: the reference asserts the hash is new)
            self.d[h] = (seg, k)
            self.d.move_to_end(h)
            return
        if self.limit and len(self.d) == self.limit:
            o, (_, ok) = self.d.popitem(last=False)
            if self.lo.get(o & M32) == o:
                del self.lo[o & M32]
            if self.key.get(ok) == o:
                del self.key[ok]
        self.d[h] = (seg, k)
        self.lo[h & M32] = h
        self.key[k] = h


def _esc(b: bytes) -> bytes:
    return b.replace(b'\xf1', b'\xf1\x00')


def _ref(h: int) -> bytes:
    return b'\xf1\x02' + h.to_bytes(8, 'big')


def _encode_one(x: bytes, cache: _Cache, oob: bool, policy: str):
    """One XCodecEncoder::encode call (xcodec_encoder.cc:74-274) over x."""
    n = len(x)
    if n < SEG:
        return _esc(x), (0, 0, 0)
    W = n - SEG + 1
    Hn = _window_hashes(x)
    lon = Hn & np.uint64(M32)
    cs = np.concatenate([np.zeros(1, np.uint64), np.cumsum(np.frombuffer(x, np.uint8), dtype=np.uint64)])
    Kn = (((cs[SEG:] - cs[:-SEG]) << np.uint64(20)) - lon) & np.uint64(M32)          # -(X2 + CLO)
    # A window can only be found if its lo (or probe key) is held by the cache
    # or by another window of this chunk; every other window is a plain miss,
    # and between two such windows only the candidate's declaration happens.
    hot = np.zeros(W, bool)
    for v, held in ((lon, cache.lo), (Kn, cache.key)):
        _, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
        hot |= cnt[inv] > 1
        if held:
            hot |= np.isin(v, np.fromiter(held.keys(), np.uint64, len(held)))
    nxt = np.minimum.accumulate(np.where(hot, np.arange(W), W)[::-1])[::-1].tolist()
    hot = hot.tolist()
    H, K = Hn.tolist(), Kn.tolist()

    out = bytearray()
    ne = nr = nc = 0
    base, s, cand = 0, 0, -1

    def declare():                                            # :276-313
        nonlocal base, cand, ne
        if cand > base:
            out.extend(_esc(x[base:cand]))
        cache.enter(H[cand], x[cand:cand + SEG], K[cand])
        out.extend(_ref(H[cand]) if oob else b'\xf1\x01' + x[cand:cand + SEG])
        ne += 1
        base = cand + SEG
        cand = -1

    while s < W:
        if cand >= 0 and cand + SEG <= s:                     # :183-190
            declare()
        if not hot[s]:
            if cand < 0:
                cand = s                                      # :246-248
            s = min(nxt[s], cand + SEG)
            continue
        h = H[s]
        ent = cache.d.get(h)                                  # find_reference, :374-416
        act, rh = 'miss', h
        if ent is not None:
            if ent[0] == x[s:s + SEG]:
                cache.use(h)
                act = 'ref'
            else:                                             # :215-216, :390-406
                nc += 1
                if policy != 'no_touch':
                    cache.use(h)                              # XCodecMemoryCache::lookup, :348-364
                act = {'collision_is_miss': 'miss', 'collision_is_ref': 'ref'}.get(policy, 'skip')
        elif policy in ('lo_is_collision', 'lo_is_ref') and (h & M32) in cache.lo:
            act, rh = ('skip' if policy == 'lo_is_collision' else 'ref'), cache.lo[h & M32]
        elif policy in ('key_is_collision', 'key_is_ref') and K[s] in cache.key:
            act, rh = ('skip' if policy == 'key_is_collision' else 'ref'), cache.key[K[s]]
        if act == 'ref':
            if s > base:
                out.extend(_esc(x[base:s]))
            out.extend(_ref(rh))
            nr += 1
            base = s + SEG
            s = base
            cand = -1                                         # :208
            continue
        if act == 'miss' and cand < 0:
            cand = s
        s += 1
    if cand >= 0:                                             # :257-261
        declare()
    if base < n:
        out.extend(_esc(x[base:]))                            # :267-269
    return bytes(out), (ne, nr, nc)


def encode_model(chunks, *, limit=0, oob=False, policy='exact', fresh=False):
    """XCodecEncoder::encode over each of `chunks` in order, on one cache
    (`limit` segments: the bounded LRU one), or with `fresh` on a new cache per
    chunk.  Returns [(output bytes, (n_extract, n_ref, n_collision))].

    `policy` other than 'exact' is a deliberately wrong encoder, to prove a case
    can tell the difference: a window whose hash is declared for other bytes
    may be a candidate ('collision_is_miss') or is referenced
    ('collision_is_ref'); a declared hash with the window's low 32 bits, or
    with its direct-mapped probe key, counts as that hash's collision
    ('lo_is_collision', 'key_is_collision') or is referenced ('lo_is_ref',
    'key_is_ref'); a colliding lookup leaves the LRU order alone ('no_touch')."""
    assert policy in POLICIES
    cache = _Cache(limit)
    res = []
    for x in chunks:
        if fresh:
            cache = _Cache(limit)
        res.append(_encode_one(bytes(x), cache, oob, policy))
    return res


# ---------------------------------------------------------------------- cases

def pack(chunks):
    """(data, offs, lens): the chunks at in-tensor offsets = 0 and 9 mod 16 in
    turn; the last one ends the array."""
    parts, offs, pos = [], [], 0
    for i, c in enumerate(chunks):
        pad = ((9 if i % 2 else 0) - pos) % 16
        parts.append(bytes(pad))
        offs.append(pos + pad)
        parts.append(c)
        pos += pad + len(c)
    data = np.frombuffer(b''.join(parts), np.uint8)
    return data, np.array(offs, np.uint64), np.array([len(c) for c in chunks], np.uint32)


def chunks_of_case(case):
    _, data, offs, lens, _, _ = case
    return [data[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)]


WRONG = {'full': ('collision_is_miss', 'collision_is_ref'), 'lo': ('lo_is_collision', 'lo_is_ref'),
         'key': ('key_is_collision', 'key_is_ref'), 'none': ()}

# Independent geometries: A is the chunk's first declaration, made at window
# 2048; the twin B sits at ...  (free: no candidate is pending at B's window)
# The kernel's pieces start at the chunk's first byte rounded down to 16 bytes
# in memory and follow each other every 2048 positions (a REF's jump starts one
# afresh), so "piece start" and "a lane's first window" are meant for a chunk
# that starts 16-byte aligned; the GPU test runs every chunk aligned and not.
INDEP_GEOMS = (
    ('end', True),           # A's end: a piece start, the compare against registers
    ('end1', False),         # one further on
    ('lane_first', False),   # a lane's first window in mid-piece: (s - p) % 32 == 0
    ('lane_mid', False),     # not a lane's first window
    ('after_ref', True),     # the window a REF jumped to
    ('last', True),          # the chunk's last window
    ('last2', True),         # its second-to-last window
    ('pending', False),      # under a pending candidate that overlaps it
    ('abc', True),           # A, B, C of one hash in a row
    ('chain', True),         # B at A's end moves the grid by one; C then meets no candidate in mid-piece
)


def _indep_chunk(geom, tw, seed):
    A, B, C = tw
    R = lambda k, n: rnd([seed, k], n)     # noqa: E731
    F = R(0, SEG)
    return {
        'end': lambda: A + B + R(1, 2500),
        'end1': lambda: A + R(1, 1) + B + R(2, 2500),
        'lane_first': lambda: A + R(1, 640) + B + R(2, 2000),
        'lane_mid': lambda: A + R(1, 653) + B + R(2, 2000),
        'after_ref': lambda: A + F + A + B + R(1, 2100),
        'last': lambda: A + F + B,
        'last2': lambda: A + F + B + R(1, 1),
        'pending': lambda: A + R(1, 1000) + B + R(2, 3000),
        'abc': lambda: A + B + C + R(1, 1000),
        'chain': lambda: A + B + R(1, 1) + C + R(2, 1500),
        'large_last': lambda: A + R(1, LARGE - 2 * SEG) + B,
    }[geom]()


def _policies(tier, free):
    return [p for p in WRONG[tier] if free or p.endswith('_is_ref')]


def indep_cases():
    """One case per (tier, at, in-band / out-of-band, kernel class): a launch
    of one chunk per geometry; the large class has a chunk of 131072 + 2048
    bytes more (twin at its last window), which puts the whole launch into the
    large kernel."""
    cases = []
    variants = [('full', at) for at in AT] + [('lo', 100), ('key', SEG - 2), ('none', 100)]
    for vi, (tier, at) in enumerate(variants):
        for oob in (False, True):
            for large in (False, True):
                geoms = list(INDEP_GEOMS) + ([('large_last', True)] if large else [])
                chunks = []
                for gi, (g, _) in enumerate(geoms):
                    seed = 1000 * vi + 10 * gi + 500 * oob + 250 * large
                    chunks.append(_indep_chunk(g, twins(seed, tier, at, 3), 0x1D00000 + seed))
                data, offs, lens = pack(chunks)
                name = f"indep_{tier}_at{at}_{'oob' if oob else 'inband'}_{'large' if large else 'small'}"
                cases.append((name, data, offs, lens, 'independent',
                              dict(tier=tier, oob=oob, large=large, geoms=[g for g, _ in geoms],
                                   policies=[_policies(tier, free) for _, free in geoms])))
    return cases


def _stream_case(geom, tier, seed):
    A, B = twins(seed, tier, 100)
    P = rnd([seed, 99], SEG)
    R = lambda k, n: rnd([seed, k], n)     # noqa: E731
    reach, calls = 1, None
    if geom == 'cache':                    # A in the persistent cache from an earlier call
        chunks, calls = [A + R(1, 2348), B + R(2, 2348)], [1, 1]
    elif geom == 'earlier_chunk':          # A declared by an earlier chunk of the call, elsewhere in its chunk
        chunks = [R(1, SEG) + A + R(2, 500), R(3, 4096), B + R(4, 3000)]
    elif geom == 'same_chunk':
        chunks = [R(1, 4096), A + B + R(2, 1000)]
    elif geom == 'same_offset':            # chunks k and k + 1 declare A and B at one offset: only A gets in
        chunks = [R(1, 4096), A + R(2, 2400), B + R(3, 2400)]
    elif geom == 'round_dep':              # A is a declaration only once P is referenced
        chunks = [P + R(1, 2100), R(2, 100) + P + A + R(3, 2300), B + R(4, 2500)]
    elif geom == 'mirror':                 # A is a declaration only while P is not referenced
        chunks = [P + R(1, 2100), R(2, 100) + P + R(3, SEG - 100) + A + R(4, 2300), B + R(5, 2500)]
        reach = 0
    data, offs, lens = pack(chunks)
    kw = dict(tier=tier, calls=calls or [len(chunks)], policies=_policies(tier, True) if reach else [],
              reach=reach if tier == 'full' else 0, round_view=geom in ('round_dep', 'mirror'))
    return (f'stream_{geom}_{tier}', data, offs, lens, 'stream', kw)


STREAM_GEOMS = ('cache', 'earlier_chunk', 'same_chunk', 'same_offset', 'round_dep', 'mirror')


def stream_cases():
    return [_stream_case(g, t, 7000 + 10 * gi + ti) for gi, g in enumerate(STREAM_GEOMS)
            for ti, t in enumerate(('full', 'lo'))]


LRU_LIMIT = 24                            # segments


def lru_cases():
    """A colliding lookup of A (by B) refreshes A.  30 segments enter after A
    in all, 17 of them after the refresh: a cache of 24 keeps A only because
    of the refresh, and the last chunk repeats A."""
    cases = []
    for ci, (name, calls) in enumerate((('one_call', [17]), ('same_call', [7, 10]), ('earlier_call', [7, 1, 9]))):
        seed = 8000 + ci
        A, B = twins(seed, 'full', AT[ci])
        R = lambda k, n: rnd([seed, k], n)     # noqa: E731
        chunks = [A + R(0, SEG)] + [R(1 + k, 4096) for k in range(6)] + [B + R(7, SEG)]
        chunks += [R(8 + k, 4096) for k in range(8)] + [A + R(16, SEG)]
        data, offs, lens = pack(chunks)
        cases.append((f'lru_refresh_{name}', data, offs, lens, 'lru',
                      dict(tier='full', calls=calls, limit=LRU_LIMIT * SEG, reach=1,
                           policies=['no_touch', 'collision_is_miss', 'collision_is_ref'])))
    return cases


PAIR_LIMIT = 8                            # segments in the memory level
PAIR_DISK = (18 + 205) * SEG              # one index block: 204 entries, never lapped here


def pair_cases():
    """A leaves the memory level (8 segments) and is found on the disk level
    when B is looked up; then A is repeated.  The disk is never lapped, so the
    pair finds exactly what an unbounded cache finds (the model's view)."""
    seed = 9000
    A, B = twins(seed, 'full', 1023)
    R = lambda k, n: rnd([seed, k], n)     # noqa: E731
    chunks = [A + R(0, SEG)] + [R(1 + k, 4096) for k in range(5)] + [B + R(6, SEG), A + R(7, SEG)]
    data, offs, lens = pack(chunks)
    return [('pair_disk_only', data, offs, lens, 'pair',
             dict(tier='full', calls=[6, 2], limit=PAIR_LIMIT * SEG, disk=PAIR_DISK, reach=1,
                  policies=['collision_is_miss', 'collision_is_ref']))]


def all_cases(_memo=[]):
    if not _memo:
        _memo.extend(indep_cases() + stream_cases() + lru_cases() + pair_cases())
    return _memo


def model_case(case, policy='exact'):
    """The model over a case's chunks: [(bytes, (n_extract, n_ref, n_collision))]."""
    _, _, _, _, mode, kw = case
    limit = kw.get('limit', 0) // SEG if mode == 'lru' else 0
    return encode_model(chunks_of_case(case), limit=limit, oob=kw.get('oob', False), policy=policy,
                        fresh=mode == 'independent')


def oracle_case(o, case):
    """The oracle (or the compiled reference) over a case, call by call:
    (per-chunk outputs, after each call cache_size -- for a pair its disk
    counters -- or None, the pair's final disk counters or None)."""
    from oracle.lib import MODE_INDEPENDENT, MODE_STREAM
    _, data, offs, lens, mode, kw = case
    if mode == 'independent':
        return o.encode_batch(data, offs, lens, mode=MODE_INDEPENDENT, oob=kw['oob']), None, None
    c = (o.cache_new_pair(kw['limit'], kw['disk']) if mode == 'pair' else o.cache_new(kw.get('limit', 0)))
    outs, sizes, a = [], [], 0
    for m in kw['calls']:
        outs += o.encode_batch(data, offs[a:a + m], lens[a:a + m], mode=MODE_STREAM, cache=c)
        a += m
        sizes.append(o.pair_stats(c) if mode == 'pair' else None if o.ref else int(o.lib.xco_cache_size(c)))
    st = o.pair_stats(c) if mode == 'pair' else None
    o.cache_free(c)
    return outs, sizes, st
