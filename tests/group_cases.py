"""Cases for the grouped batch calls (xcg_encode_batch_grouped /
xcg_decode_batch_grouped): a group is a short stream, its chunks successive
encode() / decode() calls on one fresh cache (and window) made for that group.
Test infrastructure shared by the CPU check of the expectations
(test_group_cases.py) and the GPU tests (test_gpu_group.py).  No GPU in here.

Encode expectation of a group: oracle.encode_batch(d, offs[a:b], lens[a:b],
mode=1) with cache=None (a fresh cache).  Decode expectation: oracle.decode on
one decoder per group, chunk by chunk until it stops."""
import random

import numpy as np

from indep_decode_cases import error_chunks, largest_chunk, ref_order, seg_of, window_chunks
from test_gpu_decode_reuse import BR, LIT, SEG, E, R, family

MIXED_SEED = 1
SMALL_ENC = 1 << 17              # encode: the small kernel class ends here (group total)
LARGE_ENC = 1 << 19              # ... and the large one
SMALL_DEC = 2 * 65536 + 16       # decode: the 128-slot class ends here
LARGE_DEC = 2 * LARGE_ENC + 16


# ---------------------------------------------------------------------- encode

def lay_out(chunks, rng=None, gaps=None):
    """(data, offs, lens): the chunks laid into one buffer with the given gaps
    in front of each (default: random 0..39 bytes, so every base alignment occurs)."""
    parts, offs, pos = [], [], 0
    for i, c in enumerate(chunks):
        gap = int(gaps[i]) if gaps is not None else int(rng.integers(0, 40))
        parts.append(bytes(gap))
        pos += gap
        offs.append(pos)
        parts.append(bytes(c))
        pos += len(c)
    parts.append(bytes(16))
    return (np.frombuffer(b''.join(parts), np.uint8), np.array(offs, np.uint64),
            np.array([len(c) for c in chunks], np.uint32))


def group_first_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)


def mixed_batch(seed=MIXED_SEED, nchunks=180):
    """(data, offs, lens, group_first): ragged chunks over a pool of 24 blocks,
    groups of 1..9 chunks."""
    rng = np.random.default_rng([0x6409, seed])
    pool = [rng.integers(0, 256, SEG, dtype=np.uint8).tobytes() for _ in range(24)]
    rb = lambda n: rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()     # noqa: E731
    chunks = []
    for _ in range(nchunks):
        c = b'' if rng.integers(0, 4) else rb(rng.integers(1, SEG))
        for _ in range(int(rng.integers(0, 6))):
            c += pool[int(rng.integers(0, 24))] if rng.random() < 0.5 else rb(SEG)
        if rng.random() < 0.3:
            c += rb(rng.integers(0, SEG))
        chunks.append(c)
    data, offs, lens = lay_out(chunks, rng)
    sizes, left = [], nchunks
    while left:
        k = min(left, int(rng.integers(1, 10)))
        sizes.append(k)
        left -= k
    return data, offs, lens, group_first_of(sizes)


def expect_groups(oracle, data, offs, lens, gf, oob=False):
    """Per-chunk encodings: each group one stream on a fresh cache."""
    out = []
    for a, b in zip(gf[:-1], gf[1:]):
        if b > a:
            out += oracle.encode_batch(data, offs[a:b], lens[a:b], mode=1, oob=oob)
    return out


def op_counts(enc):
    """(EXTRACTs, REFs) of an encoding (the first two stats words)."""
    i, ne, nr = 0, 0, 0
    while i < len(enc):
        if enc[i] != 0xf1:
            i += 1
        elif enc[i + 1] == 0:
            i += 2
        elif enc[i + 1] == 1:
            ne += 1
            i += 2 + SEG
        else:
            assert enc[i + 1] == 2
            nr += 1
            i += 10
    return ne, nr


def pool_chunks(seed, sizes, npool=12, p_pool=0.5):
    """Chunks of the given sizes made of 2 KiB blocks (a ragged tail where the
    size is no multiple), each block from a small pool with p_pool, else fresh:
    later chunks REF earlier ones."""
    rng = np.random.default_rng([0x9001, seed])
    pool = [rng.integers(0, 256, SEG, dtype=np.uint8).tobytes() for _ in range(npool)]
    out = []
    for n in sizes:
        c = b''
        while len(c) + SEG <= n:
            c += pool[int(rng.integers(0, npool))] if rng.random() < p_pool else \
                rng.integers(0, 256, SEG, dtype=np.uint8).tobytes()
        c += rng.integers(0, 256, n - len(c), dtype=np.uint8).tobytes()
        out.append(c)
    return out


def class_edge_groups():
    """name -> chunks of one group, by group total."""
    return {
        '128k_8x16k': pool_chunks(1, [16384] * 8),
        '128k_plus_2048': pool_chunks(2, [16384] * 8 + [2048]),
        '512k_8x64k': pool_chunks(3, [65536] * 8, npool=40),
        '512k_256x2k': pool_chunks(4, [2048] * 256, npool=60, p_pool=0.3),
        '1024x512': pool_chunks(5, [512] * 1024),
    }


# ---------------------------------------------------------------------- decode

def _status(enc, ok, cons, unk):
    if not ok:
        return -1, 0
    if unk:
        h = int.from_bytes(enc[cons + 2:cons + 10], 'big')
        assert enc[cons:cons + 2] == b'\xf1\x02' and h in unk
        return 1, h
    return (3 if cons < len(enc) else 0), 0


def decode_expect(oracle, group):
    """[(status, out, consumed, first_unknown)] of a group's chunks on ONE fresh
    decoder; the chunks after the first non-zero status are not reached."""
    c = oracle.cache_new()
    d = oracle.decoder_new(c)
    res, stopped = [], False
    try:
        for enc in group:
            if stopped:
                res.append((2, b'', 0, 0))
                continue
            ok, out, cons, unk = oracle.decode(enc, c, decoder=d)
            st, h = _status(enc, ok, cons, unk)
            res.append((st, out, cons, h))
            stopped = st != 0
    finally:
        oracle.decoder_free(d)
        oracle.cache_free(c)
    return res


def decode_expect_fresh(oracle, group):
    """The same chunks, each on a fresh decoder of its own (independent semantics)."""
    return [decode_expect(oracle, [enc])[0] for enc in group]


def ops_of(enc):
    """Split an encoding at its op boundaries: literal runs and ops, in order."""
    i, parts, lit = 0, [], 0
    n = len(enc)
    while i < n:
        if enc[i] != 0xf1 or (i + 1 < n and enc[i + 1] == 0):
            i += 2 if enc[i] == 0xf1 else 1
            continue
        if i > lit:
            parts.append(enc[lit:i])
        ln = {1: 2 + SEG, 2: 10, 3: 3}[enc[i + 1]]
        parts.append(enc[i:i + ln])
        i += ln
        lit = i
    if n > lit:
        parts.append(enc[lit:])
    assert b''.join(parts) == enc
    return parts


def cut_at_ops(enc, nparts, seed=0):
    """enc cut into nparts non-empty chunks at op boundaries (seeded cut points)."""
    ops = ops_of(enc)
    assert len(ops) >= nparts
    cuts = sorted(random.Random(0xC07 + seed).sample(range(1, len(ops)), nparts - 1))
    return [b''.join(ops[a:b]) for a, b in zip([0] + cuts, cuts + [len(ops)])]


def cross_chunk_groups(oracle):
    """name -> group: state that must live across the chunks of a group."""
    S, T = seg_of(31), seg_of(32)
    h, t = oracle.hash(S), oracle.hash(T)
    A, B = family(1)[:2]
    ha = oracle.hash(A)
    assert ha == oracle.hash(B) and A != B
    out = {
        'extract_then_ref': [E(S), R(h)],
        'name_reuse': [E(A), E(B) + R(ha), R(ha) + E(A) + R(ha)],
        'backref_chunk2_to_chunk0': [E(S) + b'a', LIT(b'mid\xf1') + E(T), BR(0) + BR(1) + R(h) + BR(2)],
        'short_chunks_between': [E(S), b'x', b'', LIT(seg_of(33)[:2047]), R(h) + BR(1)],
    }
    w = window_chunks(oracle)
    for k, (name, parts) in enumerate((('wrap_live', 3), ('wrap_emptied', 4), ('wrap_two', 5))):
        out[name] = cut_at_ops(w[name], parts, seed=k)
    return out


def stop_groups(oracle):
    """name -> (group, neighbour group): each of error_chunks()'s ways to stop as
    chunk 1 of a 4-chunk group.  Chunk 0 is literal bytes, so the cache and the
    window are as empty at chunk 1 as error_chunks() assumes; chunks 2 and 3
    would decode (on any decoder) if they were reached."""
    S = seg_of(34)
    h = oracle.hash(S)
    out = {}
    for name, bad in error_chunks(oracle).items():
        if name == 'good':
            continue
        out[name] = [LIT(b'zero\xf1'), bad, E(S) + b'two', E(S) + R(h) + BR(1) + b'three']
    out['ref_order_first'] = [ref_order(oracle), E(S), R(h)]
    return out, [E(seg_of(35)) + b'n0', R(oracle.hash(seg_of(35))) + BR(1) + b'n1']


def room_groups(oracle):
    """(group that decodes, group whose chunk 1 blocks on an unknown REF): the
    slot-size cases; every later chunk uses a declare of an earlier one."""
    S, T, U = seg_of(60), seg_of(61), seg_of(62)
    h, t = oracle.hash(S), oracle.hash(T)
    grp = [b'one' + E(S) + LIT(b'x\xf1y'), E(T) + R(h) + BR(1) + b'mid', R(t) + BR(2) + R(h) + b'end']
    blocked = [E(S), b'ab' + R(oracle.hash(U)) + b'cd', R(h)]
    return grp, blocked


def capacity_group(oracle, nchunks=8):
    """511 EXTRACTs spread over `nchunks` chunks, total <= 1 MiB + 16."""
    enc, plain_len = largest_chunk(oracle)
    return cut_at_ops(enc, nchunks, seed=9), plain_len


def over_capacity_group():
    """8 chunks of 64 EXTRACTs: 512 in all.  That is 1,049,600 bytes, more than
    the 1 MiB + 16 a group may total, so the call refuses it by its LENGTH: while
    the length bound holds a group has at most 511 EXTRACTs, and the kernel's
    check of the EXTRACT count itself can never be the one that fires."""
    rng = random.Random(0x0FE8)
    return [b''.join(E(rng.randbytes(SEG)) for _ in range(64)) for _ in range(8)]
