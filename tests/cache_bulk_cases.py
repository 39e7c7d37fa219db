"""Cases for the bulk cache learn / export (xcg_cache_learn_batch,
xcg_cache_export) and a plain Python model of what a learn comes to.  No GPU
in here.

A learn of n segments is by definition n <LEARN> sequences in order
(xcodec/xcodec_pipe_pair.cc:311-327): lookup the segment's XCodecHash; equal
bytes -> nothing more; other bytes -> replace; absent -> enter (a bounded cache
evicts its least recently used entry at the limit; a lookup that finds the hash
is a use).  `model_learn` is the closed form of that: the last occurrence of a
hash supplies its bytes and its place in the LRU order, everything the batch
does not name keeps its place below, and a bounded cache keeps the `limit`
most recent.  tests/test_cache_bulk_cases.py pins the model to the sequential
result of the C restatement (and of the reference, where it is built).
"""
from __future__ import annotations

import random
from collections import OrderedDict

import numpy as np

from collision_cases import LRU_LIMIT, family, rnd, twins

SEG = 2048
SIZES = (1, 63, 64, 65, 300)
OFFSETS = (0, 1, 3, 16)                   # byte offsets of d_segs in its buffer


def model_learn(cache: OrderedDict, limit: int, hashes, segs):
    """The closed form on `cache` (hash -> bytes, least recently used first;
    limit in segments, 0 = unbounded)."""
    last = {}
    for i, h in enumerate(hashes):
        last[h] = i                                   # the last occurrence wins
    for h, i in sorted(last.items(), key=lambda kv: kv[1]):
        cache.pop(h, None)                            # referenced: above everything not referenced,
        cache[h] = segs[i]                            # in the order of last reference
    while limit and len(cache) > limit:
        cache.popitem(last=False)                     # the `limit` most recent stay
    return cache


def sequential_learn(cache: OrderedDict, limit: int, hashes, segs, trace=None):
    """The definition itself, step by step (for the cases' own feature checks)."""
    for h, s in zip(hashes, segs):
        if h in cache:
            if trace is not None:
                trace.append(('hit' if cache[h] == s else 'replace', h))
            cache[h] = s
            cache.move_to_end(h)
            continue
        if limit and len(cache) == limit:
            o, _ = cache.popitem(last=False)
            if trace is not None:
                trace.append(('evict', o))
        if trace is not None:
            trace.append(('enter', h))
        cache[h] = s
    return cache


def segment_set(n: int, seed: int = 0):
    """n segments for the equivalence test: random ones, an exact duplicate, a
    family of three same-hash variants in order (the last must win), `lo` twins
    (both must be held), an all-zero, an all-0xFF and an all-0xF1 segment.
    n = 1 is one random segment."""
    if n == 1:
        return [rnd([0xB01C, seed, 0], SEG)]
    fam = family(0xB01C + seed)
    lo = twins(0xB01C + seed, 'lo')
    special = [fam[0], bytes(SEG), lo[0], fam[1], b'\xff' * SEG, lo[1], b'\xf1' * SEG, fam[2]]
    assert n >= len(special) + 3
    out = [rnd([0xB01C, seed, k], SEG) for k in range(n - len(special) - 1)]
    step = len(out) // len(special)
    for k, s in enumerate(special):                   # spread through the batch, in order
        out.insert(1 + k * (step + 1), s)
    out.append(out[0])                                # the exact duplicate, far from its first occurrence
    assert len(out) == n
    return out


def lru_batch(seed: int = 0):
    """100 segments over 40 distinct hashes for a cache of LRU_LIMIT = 24:
    hits that refresh, an eviction followed by the re-entry of the same hash
    with other bytes, and name reuse between two live occurrences.  Names 0 and
    20..23 are families of three same-hash variants; the others one random
    segment each."""
    fams = {k: family(0x1B00 + 10 * seed + j) for j, k in enumerate((0, 20, 21, 22, 23))}
    one = {k: rnd([0x1B01, seed, k], SEG) for k in range(40) if k not in fams}

    def seg(name, var=0):
        return fams[name][var] if name in fams else one[name]

    seq = [(k, 0) for k in range(30)]                 # 0..5 leave as 24..29 enter
    seq += [(0, 1)]                                   # evicted, re-entered with other bytes
    seq += [(10, 0), (11, 0), (12, 0)]                # hits that refresh
    seq += [(20, 1), (25, 0), (20, 2)]                # name reuse between two live occurrences
    seq += [(k, 0) for k in range(30, 40)]
    r = random.Random(0x1B02 + seed)
    while len(seq) < 100:
        k = r.randrange(40)
        seq.append((k, r.randrange(3) if k in fams else 0))
    return [seg(k, v) for k, v in seq]


def lru_earlier(seed: int = 0):
    """24 earlier entries for the same cache: 20 unrelated segments and four the
    batch names (one of them with other bytes than the batch's)."""
    b = lru_batch(seed)
    fam20 = family(0x1B00 + 10 * seed + 1)
    assert b[20] == fam20[0]
    pre = [rnd([0x1B03, seed, k], SEG) for k in range(20)]
    pre[3:3] = [b[5]]
    pre[9:9] = [fam20[2]]
    pre[15:15] = [b[11]]
    pre.append(b[35])
    assert len(pre) == LRU_LIMIT
    return pre


def splits(n: int):
    """One call, and two calls cut at every third position."""
    return [None] + list(range(3, n, 3))


def cases():
    """(name, limit in segments, earlier segments, batch)."""
    out = [(f'set{n}', 0, [], segment_set(n, n)) for n in SIZES]
    out.append(('set65_on_set64', 0, segment_set(64, 64), segment_set(65, 64)))   # same seed: shared hashes
    out.append(('lru_empty', LRU_LIMIT, [], lru_batch()))
    out.append(('lru_full', LRU_LIMIT, lru_earlier(), lru_batch()))
    out.append(('lru_set300', LRU_LIMIT, [], segment_set(300, 300)))              # n > 12 x limit
    out.append(('lru_limit1', 1, [], segment_set(63, 63)))
    return out


def without_reuse(hash_of, *lists):
    """The same lists with every segment replaced by the last segment of its
    hash: no <LEARN> then finds other bytes under a hash.  The reference's own
    classes can only run such a sequence -- XCodecMemoryCache::replace
    (xcodec/xcodec_cache.h:327-337) assigns its CacheEntry without taking a
    reference, so the entry it leaves points at a freed segment."""
    last = {}
    for lst in lists:
        for s in lst:
            last[hash_of(s)] = s
    return [[last[hash_of(s)] for s in lst] for lst in lists]


def later_stream(batch, seed: int = 0):
    """A stream to encode on a learned cache: learned segments (REFs, and on a
    bounded cache lookups of evicted ones), new data that enters and evicts, and
    learned segments again."""
    r = random.Random(0x1B04 + seed)
    pick = [batch[r.randrange(len(batch))] for _ in range(12)]
    parts = pick[:6] + [rnd([0x1B05, seed, k], 3 * SEG + 100) for k in range(6)] + pick[6:] + pick[:3]
    return np.frombuffer(b''.join(parts), np.uint8)
