"""Cases for the encoder refmap (xcg_encode_refmap_batch, xcg_encode_host_refmap)
and a plain Python walker with the kernel's rules.  No GPU in here.

The refmap of one XCodecEncoder::encode(output, input, refmap) call
(xcodec/xcodec_encoder.h:42) maps every hash the call REF'd to its segment, the
first REF of a hash winning (xcodec_encoder.cc:364-371), iterated in ascending
hash order (std::map).  It is a function of the call's output: `walk` goes over
the encoding op by op, tracks the input position, and ends at the first thing
no encoder writes.  tests/test_refmap_cases.py pins the walker to the
reference's own refmap.
"""
from __future__ import annotations

import numpy as np

SEG = 2048
REFMAP_MAX = 256
SEED = 0x7EF
IDX_A, IDX_B, IDX_C = 237, 12, 0     # hash ends in F1 / has F1 in a middle byte / has the top bit set


def walk(enc: bytes, n: int = None, decls=(), collect: bool = True):
    """The refmap of enc[:n] as ([(hash, input position)] ascending by hash,
    encoded bytes walked).  decls: (position, hash) of out-of-band declarations,
    which are no entries; collect=False: the null cache, where no REF is one."""
    n = len(enc) if n is None else n
    i = pos = 0
    refs = {}
    while i < n:
        m = enc.find(b'\xf1', i, n)
        m = n if m < 0 else m
        pos += m - i                                   # literal bytes
        i = m
        if n - i < 2:
            break                                      # the end, or a lone trailing F1
        op = enc[i + 1]
        if op == 0:                                    # ESCAPE: one input byte
            i, pos = i + 2, pos + 1
            continue
        if op == 1:                                    # EXTRACT
            if n - i < 2 + SEG:
                break
            i += 2 + SEG
        elif op == 2:                                  # REF
            if n - i < 10:
                break
            h = int.from_bytes(enc[i + 2:i + 10], 'big')
            if collect and (pos, h) not in decls and h not in refs:
                if len(refs) == REFMAP_MAX:
                    break                              # entry 257 ends the walk at its REF
                refs[h] = pos
            i += 10
        else:
            break                                      # BACKREF, or no opcode
        pos += SEG
    return sorted(refs.items()), i


_SEGS = None


def segs():
    """The first 300 segments of the seeded generator."""
    global _SEGS
    if _SEGS is None:
        r = np.random.default_rng(SEED)
        _SEGS = [r.integers(0, 256, SEG, dtype=np.uint8).tobytes() for _ in range(300)]
    return _SEGS


def abc():
    s = segs()
    return s[IDX_A], s[IDX_B], s[IDX_C]


def payload_segment():
    """2048 bytes of F1 02 <8 bytes> and F1 00 patterns: as an EXTRACT payload it
    looks like REFs and ESCAPEs to anything that scans for F1."""
    unit = b'\xf1\x02' + bytes(range(0x10, 0x18)) + b'\xf1\x00' + b'\xf1\x02\xf1\x00'
    return (unit * (SEG // len(unit) + 1))[:SEG]


def f1_input():
    """A 'ab' F1 F1 A 00 02 A B F1 B: A is declared; an escape run stands right
    before a REF; the REF whose hash ends in F1 is followed by literal 00 02;
    a further REF of A is deduplicated to the first; B's REF follows an escaped
    F1.  Two entries."""
    a, b, _ = abc()
    return a + b'ab' + b'\xf1\xf1' + a + b'\x00\x02' + a + b + b'\xf1' + b


F1_REFS = {IDX_A: SEG + 4, IDX_B: 4 * SEG + 7}        # segment index -> the input position of its entry


def chunked(parts):
    """(data, offs, lens) of chunks given as byte strings."""
    lens = np.array([len(p) for p in parts], dtype=np.uint32)
    offs = np.zeros(len(parts), dtype=np.uint64)
    offs[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
    return np.frombuffer(b''.join(parts) or b'\0', np.uint8)[:int(lens.sum())], offs, lens


def stream_cases():
    """name -> list of batches, each a list of chunks (bytes), encoded in order
    on one cache with stream semantics; `refs` -> per batch, per chunk, the
    number of entries the case is built to have."""
    s = segs()
    a, b, c = abc()
    p = payload_segment()
    out = {}
    # a chunk with no REF, one of 0 bytes, one under 2048 bytes.  (The declaring chunk goes first: a pair
    # context cuts this batch into one sub-batch per chunk, and its replay takes no first sub-batch
    # without a single cache reference on an empty primary.)
    out['edges'] = ([[s[2] + s[3] + s[4][:904], b'', s[1][:1000]]], [[0, 0, 0]])
    out['f1'] = ([[f1_input()]], [[2]])
    out['payload'] = ([[a + p + b'\xf1' + a + p]], [[2]])
    # 9 chunks in one launch (a partial last workgroup), odd lengths; chunk k REFs
    # the declaration of chunk k - 1 and, every third, C of chunk 0; then a second
    # batch REFs the first one's declarations and its own
    first = []
    for k in range(9):
        part = s[20 + k] + b'x' * k
        if k:
            part += s[20 + k - 1]
        else:
            part += c
        if k and k % 3 == 0:
            part += b'\xf1' + c
        first.append(part)
    second = [s[22] + s[100] + a + b'y' + s[100] + c + s[28], s[100][:777]]
    out['cross'] = ([first, second], [[0, 1, 1, 2, 1, 1, 2, 1, 1], [4, 0]])
    return out


def oob_input():
    """Out of band: A and B are declared (F1 02, no entries) and REF'd later in
    the same chunk (entries); S5 is declared only."""
    a, b, _ = abc()
    return a + b + b'\xf1q' + a + segs()[5] + b


def crafted_refs(count: int = REFMAP_MAX + 1):
    """`count` REF ops of distinct hashes, not in hash order, with and without
    the top bit; every hash byte pattern may hold F1."""
    r = np.random.default_rng(SEED + 1)
    hs = []
    seen = set()
    while len(hs) < count:
        h = int(r.integers(0, 1 << 63, dtype=np.uint64)) | ((len(hs) & 1) << 63)
        if len(hs) % 7 == 0:
            h = (h & ~0xFF00) | 0xF100
        if h not in seen:
            seen.add(h)
            hs.append(h)
    return b''.join(b'\xf1\x02' + h.to_bytes(8, 'big') for h in hs), hs


def stops():
    """Encodings that end in something no encoder writes -> (entries, walked)."""
    ref = b'\xf1\x02' + (0x0102030405060708).to_bytes(8, 'big')
    return {
        'lone_f1': (b'ab' + ref + b'cd\xf1', 1, 14),
        'cut_ref': (ref + b'\xf1\x02\x01\x02', 1, 10),
        'cut_extract': (ref + b'\xf1\x01' + bytes(2047), 1, 10),
        'backref': (b'q' + ref + b'\xf1\x03\x00' + ref, 1, 11),
        'bad_op': (b'\xf1\x00' + ref + b'\xf1\xf1\x00' + ref, 1, 12),
        'whole': (b'\xf1\x00' + ref + b'zz', 1, 14),
    }


def extract_to_oob(enc: bytes, hash_of) -> bytes:
    """An in-band encoding with every EXTRACT rewritten as the out-of-band
    declaration of the same segment (F1 02 hash): how the two modes differ."""
    out = bytearray()
    i, n = 0, len(enc)
    while i < n:
        m = enc.find(b'\xf1', i)
        m = n if m < 0 else m
        out += enc[i:m]
        i = m
        if i >= n:
            break
        op = enc[i + 1]
        if op == 1:
            out += b'\xf1\x02' + hash_of(enc[i + 2:i + 2 + SEG]).to_bytes(8, 'big')
            i += 2 + SEG
        else:
            k = 2 if op == 0 else 10
            out += enc[i:i + k]
            i += k
    return bytes(out)
