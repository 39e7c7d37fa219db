"""A deflate / zlib stream *writer* for tests, from RFC 1950 and RFC 1951.

zlib's own encoder writes a small corner of the format; this module writes
the rest: any code lengths (refused sets included), any coding of a dynamic
header's length sequence, any length / distance symbol with any extra bits,
stored blocks at any bit offset, codes that do not exist.  Pure Python, no
project imports.

A block body is a list of symbols:
  int                      a literal byte
  (length, distance)       a match
  Match(length, distance, length_symbol=284)   a match with a chosen length symbol
  Match(length, None)      a length symbol and its extra bits, no distance
  Raw('1011')              bits written as they stand, first character first
`expand(symbols)` gives the bytes such a list means without going through zlib.
"""
from __future__ import annotations

import zlib  # adler32 only

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
         4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8      # 288 codes: 286 and 287 exist but mean nothing
FIXED_DIST = [5] * 32                                        # 30 and 31 likewise


class Match:
    """A match whose length symbol is chosen by the caller (length 258 is
    symbol 285, or symbol 284 with extra 31)."""

    def __init__(self, length, distance, length_symbol=None):
        self.length, self.distance, self.length_symbol = length, distance, length_symbol


class Raw:
    """Bits for the stream as they stand ('0' / '1', first character first)."""

    def __init__(self, bits: str):
        assert set(bits) <= {'0', '1'}
        self.bits = bits


def length_symbol(length: int):
    """-> (symbol, extra bit count, extra value), the RFC's own choice (258 = 285)."""
    if not 3 <= length <= 258:
        raise ValueError(f'length {length}')
    i = 28 if length == 258 else max(k for k in range(28) if LBASE[k] <= length)
    return 257 + i, LEXT[i], length - LBASE[i]


def distance_symbol(distance: int):
    if not 1 <= distance <= 32768:
        raise ValueError(f'distance {distance}')
    i = max(k for k in range(30) if DBASE[k] <= distance)
    return i, DEXT[i], distance - DBASE[i]


def canonical_codes(lengths):
    """RFC 1951 3.2.2: codes of one length are consecutive in symbol order,
    shorter codes come first.  No check of the set: an over-subscribed one
    gets codes that overflow their length, as the format's arithmetic gives."""
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for n in lengths:
        if n:
            out.append(nxt[n] & ((1 << n) - 1))
            nxt[n] += 1
        else:
            out.append(None)
    return out


def code_bits(lengths, sym) -> str:
    """The code of `sym` as Raw() takes it."""
    return format(canonical_codes(lengths)[sym], f'0{lengths[sym]}b')


def balanced_lengths(k: int):
    """Lengths of a complete prefix code of k >= 2 symbols, as flat as it gets."""
    p = k.bit_length() - 1
    short = (1 << (p + 1)) - k
    return [p] * short + [p + 1] * (k - short)


def random_complete_lengths(rng, k: int, max_len: int = 15):
    """Lengths of a random complete prefix code of k >= 2 symbols: split random
    leaves of a binary tree until it has k."""
    leaves = [1, 1]
    while len(leaves) < k:
        cand = [i for i, d in enumerate(leaves) if d < max_len]
        i = rng.choice(cand)
        d = leaves.pop(i)
        leaves += [d + 1, d + 1]
    rng.shuffle(leaves)
    return leaves


def expand(symbols) -> bytes:
    """The bytes a symbol list means (Raw bits mean nothing)."""
    out = bytearray()
    for s in symbols:
        if isinstance(s, Raw):
            continue
        if isinstance(s, int):
            out.append(s)
            continue
        length, dist = (s.length, s.distance) if isinstance(s, Match) else s
        if dist > len(out):
            raise ValueError(f'distance {dist} at output position {len(out)}')
        for _ in range(length):
            out.append(out[-dist])
    return bytes(out)


def random_symbols(rng, count, literals, length_syms=range(257, 286), dist_syms=range(30), p_match=0.5, produced=0,
                   dist_min=1, dist_max=32768):
    """`count` seeded random symbols after `produced` bytes of output: literals
    from `literals`, matches (probability p_match where one is possible) with
    a length symbol from length_syms and a distance symbol from dist_syms, any
    extra bits, the distance valid (at most the bytes produced so far) and
    within dist_min..dist_max."""
    literals, length_syms, dist_syms = list(literals), list(length_syms), list(dist_syms)
    out = []
    for _ in range(count):
        hi = min(produced, dist_max)
        ds = [d for d in dist_syms if DBASE[d] <= hi and DBASE[d] + (1 << DEXT[d]) - 1 >= dist_min]
        if ds and length_syms and rng.random() < p_match:
            ls = rng.choice(length_syms) - 257
            length = LBASE[ls] + rng.randrange(1 << LEXT[ls])
            d = rng.choice(ds)
            lo = max(DBASE[d], dist_min)
            dist = rng.randint(lo, min(hi, DBASE[d] + (1 << DEXT[d]) - 1))
            # (length 258 through symbol 284 when the draw says so)
            out.append(Match(length, dist, 257 + ls) if length == 258 and ls == 27 else (length, dist))
            produced += length
        else:
            out.append(rng.choice(literals))
            produced += 1
    return out


def run_length_code(seq):
    """Greedy 16 / 17 / 18 coding of a length sequence (RFC 1951 3.2.7) ->
    [(symbol, extra value)].  The sequence is literal/length and distance
    lengths back to back, so a run may cross from one into the other."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        r = 1
        while i + r < n and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 11:
            k = min(r, 138)
            out.append((18, k - 11))
        elif v == 0 and r >= 3:
            k = r
            out.append((17, k - 3))
        elif i > 0 and seq[i - 1] == v and r >= 3:
            k = min(r, 6)
            out.append((16, k - 3))
        else:
            k = 1
            out.append((v, 0))
        i += k
    return out


class BitWriter:
    def __init__(self):
        self.b = bytearray()     # one bit per element, in stream order

    @property
    def nbits(self):
        return len(self.b)

    def bits(self, value: int, n: int):
        """A field: least significant bit first."""
        self.b.extend((value >> i) & 1 for i in range(n))

    def code(self, code: int, n: int):
        """A Huffman code: most significant bit first."""
        self.b.extend((code >> (n - 1 - i)) & 1 for i in range(n))

    def raw(self, bits: str):
        self.b.extend(int(c) for c in bits)

    def align(self):
        self.b.extend([0] * (-len(self.b) % 8))

    def getvalue(self) -> bytes:
        b = self.b + bytearray(-len(self.b) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


class DeflateWriter(BitWriter):
    """Blocks and the zlib wrapper on top of the bit writer."""

    # ---- zlib wrapper (RFC 1950)
    def zlib_header(self, cinfo=7, cm=8, flevel=2, fdict=0, fcheck=None, dictid=None):
        """CMF, FLG.  fcheck None: the value that makes the header valid; an
        int: that value, right or wrong.  dictid: four more bytes (FDICT)."""
        assert self.nbits % 8 == 0
        cmf = (cinfo << 4) | cm
        flg = (flevel << 6) | (fdict << 5)
        if fcheck is None:
            fcheck = (31 - ((cmf << 8) | flg) % 31) % 31
        self.bits(cmf, 8)
        self.bits(flg | fcheck, 8)
        if dictid is not None:
            for k in (24, 16, 8, 0):
                self.bits((dictid >> k) & 255, 8)

    def zlib_trailer(self, data: bytes = None, adler: int = None):
        """The adler32 of `data`, or the value given (right or wrong), big-endian
        after the last block's padding."""
        self.align()
        if adler is None:
            adler = zlib.adler32(data)
        for k in (24, 16, 8, 0):
            self.bits((adler >> k) & 255, 8)

    # ---- blocks (RFC 1951)
    def block_header(self, final: bool, btype: int):
        self.bits(1 if final else 0, 1)
        self.bits(btype, 2)

    def stored(self, data: bytes, final=False, nlen=None, length=None):
        """LEN 0..65535 from wherever the last block ended (the header's three
        bits, padding to the byte, LEN, NLEN, the bytes).  nlen: a value of the
        caller's (wrong ones included) instead of ~LEN."""
        n = len(data) if length is None else length
        assert 0 <= n <= 65535
        self.block_header(final, 0)
        self.align()
        self.bits(n, 16)
        self.bits((n ^ 0xffff) if nlen is None else nlen, 16)
        for c in data:
            self.bits(c, 8)

    def body(self, symbols, litlens, distlens, eob=True):
        """Symbols through the codes that litlens / distlens give."""
        lc, dc = canonical_codes(litlens), canonical_codes(distlens)

        def put(codes, lens, sym, what):
            if sym >= len(lens) or not lens[sym]:
                raise ValueError(f'{what} symbol {sym} has no code')
            self.code(codes[sym], lens[sym])
        for s in symbols:
            if isinstance(s, Raw):
                self.raw(s.bits)
            elif isinstance(s, int):
                put(lc, litlens, s, 'literal')
            else:
                m = s if isinstance(s, Match) else Match(*s)
                if m.length_symbol is None:
                    ls, xb, xv = length_symbol(m.length)
                else:
                    ls = m.length_symbol
                    xb, xv = LEXT[ls - 257], m.length - LBASE[ls - 257]
                    if not 0 <= xv < (1 << xb):
                        raise ValueError(f'length {m.length} is not symbol {ls}')
                put(lc, litlens, ls, 'length')
                self.bits(xv, xb)
                if m.distance is None:      # the length alone: the caller writes what follows it
                    continue
                ds, db, dv = distance_symbol(m.distance)
                put(dc, distlens, ds, 'distance')
                self.bits(dv, db)
        if eob:
            put(lc, litlens, 256, 'end-of-block')

    def fixed(self, symbols, final=False, eob=True):
        self.block_header(final, 1)
        self.body(symbols, FIXED_LIT, FIXED_DIST, eob)

    def dynamic_header(self, litlens, distlens, nlen=None, ndist=None, cl_lens=None, ncl=None, coding='single'):
        """HLIT, HDIST, HCLEN, the code-length code, the length sequence.

        litlens / distlens are cut or zero-filled to nlen / ndist entries
        (defaults: their own sizes, at least 257 and 1); counts the format
        cannot mean (nlen 287..288, ndist 31..32) are written as they are.
        cl_lens: the 19 code-length code lengths by symbol (default: a flat
        complete code over the symbols the sequence uses); ncl: how many of
        them are sent (default: up to the last nonzero one, at least 4).
        coding: 'single' (one symbol per length), 'runs' (greedy 16/17/18 over
        literal and distance lengths as one sequence), or the symbols
        themselves as [(symbol, extra value)]."""
        nlen = max(257, len(litlens)) if nlen is None else nlen
        ndist = max(1, len(distlens)) if ndist is None else ndist
        assert 257 <= nlen <= 288 and 1 <= ndist <= 32
        seq = (list(litlens) + [0] * nlen)[:nlen] + (list(distlens) + [0] * ndist)[:ndist]
        if coding == 'single':
            cls = [(v, 0) for v in seq]
        elif coding == 'runs':
            cls = run_length_code(seq)
        else:
            cls = list(coding)
        if cl_lens is None:
            used = sorted({s for s, _ in cls})
            if len(used) < 2:           # a one-code set is incomplete: zlib refuses it here
                used = sorted(set(used) | {0, 18})[:2]
            cl_lens = [0] * 19
            for s, n in zip(used, balanced_lengths(len(used))):
                cl_lens[s] = n
        assert len(cl_lens) == 19 and max(cl_lens) <= 7
        if ncl is None:
            ncl = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
        assert 4 <= ncl <= 19
        self.bits(nlen - 257, 5)
        self.bits(ndist - 1, 5)
        self.bits(ncl - 4, 4)
        for s in CL_ORDER[:ncl]:
            self.bits(cl_lens[s], 3)
        self.cl_end = self.nbits        # where the code-length code is complete
        cc = canonical_codes(cl_lens)
        for s, x in cls:
            if not cl_lens[s]:
                raise ValueError(f'code-length symbol {s} has no code')
            self.code(cc[s], cl_lens[s])
            self.bits(x, {16: 2, 17: 3, 18: 7}.get(s, 0))

    def dynamic(self, symbols, litlens, distlens, final=False, eob=True, **header):
        self.block_header(final, 2)
        self.dynamic_header(litlens, distlens, **header)
        self.body(symbols, litlens, distlens, eob)
