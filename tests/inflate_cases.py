"""Inflate inputs that zlib's own encoder never writes, built with
tests/deflate_writer.py: trees, symbols, blocks and headers at the corners of
RFC 1950 / 1951, each at the smallest shape that reaches the path it is for.

`cases()` -> [Case(name, calls, expect, symbols, region)]:
  calls    the input cuts, one per consume
  expect   the decoded bytes of the whole stream (it ends on the last call),
           or Error(k): a data error on call k (every later call fails too)
  symbols  what the stream means as a deflate_writer symbol list (stored
           bytes as literals), None for refused streams
  region   the case is there for the workgroup kernels' speculative regions

`oracle(calls)` -> [(bytes, status)] is zlib itself, a fresh
decompressobj(15) fed the same cuts: -1 where the call raises or leaves
unused_data (and on every call after that), 1 at eof, else 0.
"""
from __future__ import annotations

import collections
import functools
import random
import zlib

from tests.deflate_writer import (DBASE, DEXT, FIXED_DIST, FIXED_LIT, LBASE, LEXT, DeflateWriter, Match, Raw,
                                  code_bits, expand, random_symbols)

Case = collections.namedtuple('Case', 'name calls expect symbols region')
Error = collections.namedtuple('Error', 'call')


def oracle(calls):
    z, out, dead = zlib.decompressobj(15), [], False
    for c in calls:
        if dead:
            out.append((b'', -1))
            continue
        try:
            o = z.decompress(c)
        except zlib.error:
            dead = True
            out.append((b'', -1))
            continue
        if z.unused_data:
            dead = True
            out.append((o, -1))
        else:
            out.append((o, 1 if z.eof else 0))
    return out


def _rand(seed, n):
    return random.Random(seed).randbytes(n)


def lens_of(n, table):
    """A length list of n entries from {symbol: length}."""
    out = [0] * n
    for s, l in table.items():
        out[s] = l
    return out


# Ladder trees: one code of every length 1..14 and two of 15 bits, the long
# codes on the symbols the cases use most, end-of-block on the 1-bit code.
LADDER_LIT = lens_of(286, {0x41: 15, 284: 15, 0x42: 14, 281: 13, 0x43: 12, 273: 11, 0x44: 10, 265: 9, 0x45: 8,
                           257: 7, 0x46: 6, 285: 5, 0x47: 4, 0x48: 3, 0x49: 2, 256: 1})
LADDER_DIST = lens_of(30, {29: 15, 28: 15, 0: 14, 27: 13, 1: 12, 20: 11, 2: 10, 10: 9, 3: 8, 16: 7, 4: 6, 22: 5,
                           5: 4, 24: 3, 6: 2, 26: 1})
# Long trees: three short codes on literals 0..2 and six on distance symbols
# 0..5; every other code is past the primary tables (11 / 12 bits of a 10-bit
# table, 10 / 11 bits of a 9-bit one).
LONG_LIT = [1, 2, 3] + [11] * 229 + [12] * 54
LONG_DIST = [1, 2, 3, 4, 5, 6] + [10] * 8 + [11] * 16
# A small everyday tree for cases that are about something else.
SMALL_LIT = lens_of(286, dict(zip([0x61, 0x62, 0x63, 0x64, 256, 257, 258, 285], [3] * 8)))
SMALL_DIST = lens_of(30, dict(zip([0, 1, 2, 3], [2] * 4)))
ONE_LIT = lens_of(257, {0x78: 1, 256: 1})          # one literal and end-of-block
EOB_ONLY = lens_of(257, {256: 1})                  # a single 1-bit code: incomplete, and legal


class Stream:
    """A zlib stream under construction: the writer, the symbols written so far
    and the byte positions where the case cuts its calls."""

    def __init__(self, header=True, **hdr):
        self.w = DeflateWriter()
        self.syms, self.cuts = [], []
        if header:
            self.w.zlib_header(**hdr)

    def cut(self, bit=None):
        """A call ends with the byte that holds the last bit written (or `bit`)."""
        self.cuts.append(((self.w.nbits if bit is None else bit) + 7) // 8)

    def stored(self, data, **kw):
        self.w.stored(data, **kw)
        self.syms += list(data)

    def fixed(self, symbols, **kw):
        self.w.fixed(symbols, **kw)
        self.syms += symbols

    def dynamic(self, symbols, litlens, distlens, **kw):
        self.w.dynamic(symbols, litlens, distlens, **kw)
        self.syms += symbols

    def end(self, adler=None):
        self.w.zlib_trailer(expand(self.syms) if adler is None else b'', adler)

    def calls(self, every=None, start=0, tail=False):
        """The stream cut at the marked places, or (every) into equal pieces
        from byte `start` on."""
        z = self.w.getvalue()
        if every:
            cs = [z[:start]] * (start > 0) + [z[i:i + every] for i in range(start, len(z), every)]
        else:
            edges = [0] + [c for c in self.cuts if 0 < c < len(z)] + [len(z)]
            cs = [z[a:b] for a, b in zip(edges, edges[1:])]
        return cs + ([b''] if tail else [])


def ok(name, s, region=False, **kw):
    return Case(name, s.calls(**kw), expand(s.syms), s.syms, region)


def bad(name, s, call, **kw):
    return Case(name, s.calls(**kw), Error(call), None, False)


# ------------------------------------------------------------------- trees
def _tree_cases():
    out = []
    lits = [0x61, 0x62, 0x63, 0x64] * 50
    for name, dl, nd in (('ndist1', [0], 1), ('ndist30', [0] * 30, 30)):
        s = Stream()
        s.dynamic(lits, SMALL_LIT, dl, ndist=nd, final=True)
        s.end()
        out.append(ok(f'tree/no-distance-code/{name}', s))
    # one distance code of length 1
    s = Stream()
    s.dynamic([0x61, 0x62, (3, 1), 0x63, (258, 1), (4, 1)], SMALL_LIT, [1], final=True)
    s.end()
    out.append(ok('tree/one-distance-code/sym0', s))
    s = Stream()
    s.stored(_rand(1, 32768))
    s.dynamic([0x61, (3, 24577), 0x62, (258, 32768), (4, 30000), (258, 24578)], SMALL_LIT, [0] * 29 + [1], final=True)
    s.end()
    out.append(ok('tree/one-distance-code/sym29', s))
    # the code that does not exist: '1' where the tree has '0' alone (or nothing)
    trees = {'one-distance-code': (SMALL_LIT, [1]), 'no-distance-code': (SMALL_LIT, [0]),
             'sym29-only': (SMALL_LIT, [0] * 29 + [1])}
    for tname, (ll, dl) in trees.items():
        for where in ('mid', 'last-more', 'last-nothing'):
            s = Stream()
            s.dynamic([0x61, 0x62, 0x63, Match(3, None), Raw('1')], ll, dl, eob=False)
            if where != 'mid':
                s.cut()
            if where != 'last-nothing':
                s.w.body([0x61] * 40, ll, dl)
                s.w.stored(b'after', final=True)
            out.append(bad(f'tree/{tname}/bad-code/{where}', s, 0))
    for where in ('mid', 'last-more', 'last-nothing'):
        s = Stream()
        s.dynamic([], EOB_ONLY, [0])
        s.dynamic([Raw('1')], EOB_ONLY, [0], eob=False)
        if where != 'mid':
            s.cut()
        if where != 'last-nothing':
            s.w.raw('0')
            s.w.stored(b'after', final=True)
        out.append(bad(f'tree/eob-only/bad-code/{where}', s, 0))
    # a literal tree that holds end-of-block alone
    for n in (1, 50):
        s = Stream()
        for _ in range(n):
            s.dynamic([], EOB_ONLY, [0])
        s.fixed([0x68, 0x69, (4, 2)], final=True)
        s.end()
        out.append(ok(f'tree/eob-only/{n}-blocks', s))
    # ladder trees; the 48-bit symbol: a 15-bit length code with 5 extra bits,
    # a 15-bit distance code with 13
    s = Stream()
    s.stored(_rand(2, 32768))
    body_at = s.w.nbits // 8
    sy = [0x41, 0x42, Match(258, 32768, 284), Match(227, 24577, 284), 0x41, (257, 32767), (250, 16385 + 8191),
          (131, 16385), 0x43, (3, 1), (258, 2), (35, 1025), 0x49, (11, 33), (12, 6144)]
    sy += random_symbols(random.Random(3), 150, [0x41] * 5 + [0x42] * 3 + [0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49],
                         [284] * 4 + [281, 273, 265, 257, 285], [29] * 4 + [28] * 4 + [0, 27, 1, 20, 2, 10, 3, 16],
                         0.4, produced=40000)
    s.dynamic(sy, LADDER_LIT, LADDER_DIST, final=True)
    s.end()
    out.append(ok('tree/ladder/48-bit-symbol', s))
    out.append(ok('tree/ladder/48-bit-symbol/cut7', s, every=7, start=body_at))
    return out


def _refused_header(litlens, distlens, **kw):
    """-> (whole, cut after the header, cut after the code-length code)."""
    s = Stream()
    s.w.block_header(True, 2)
    s.w.dynamic_header(litlens, distlens, **kw)
    hdr = s.w.nbits
    s.w.raw('0' * 400)
    return s, hdr, s.w.cl_end


def _refused_cases():
    out = []
    zeros = lambda n: [(0, 0)] * n
    sets = {
        'lit-over': (lens_of(257, {0: 1, 1: 1, 256: 1}), [1], {}),
        'lit-incomplete': (lens_of(257, {0: 2, 256: 2}), [1], {}),
        'lit-no-eob': (lens_of(257, {0: 1}), [1], {}),
        'dist-over': (ONE_LIT, [1, 1, 1], {}),
        'dist-incomplete': (ONE_LIT, [2, 2], {}),
        'dist-one-2bit': (ONE_LIT, [0, 2], {}),
        'hlit30': (ONE_LIT + [0] * 30, [1], {'nlen': 287}),
        'hlit31': (ONE_LIT + [0] * 31, [1], {'nlen': 288}),
        'hdist30': (ONE_LIT, [1] * 2, {'ndist': 31}),
        'hdist31': (ONE_LIT, [1] * 2, {'ndist': 32}),
    }
    for name, (ll, dl, kw) in sets.items():
        s, hdr, _ = _refused_header(ll, dl, **kw)
        out.append(bad(f'refused/{name}/whole', s, 0))
        s, hdr, _ = _refused_header(ll, dl, **kw)
        s.cut(hdr)
        out.append(bad(f'refused/{name}/cut-after-header', s, 0))
    # code-length sets: zlib refuses them before it reads a single length
    cl = {
        'cl-over': lens_of(19, {0: 1, 1: 1, 2: 1}),
        'cl-incomplete': lens_of(19, {0: 2, 1: 2}),
        'cl-one-1bit': lens_of(19, {0: 1}),
    }
    for name, cll in cl.items():
        for cutat in ('whole', 'cut-after-header', 'cut-after-code-lengths'):
            s, hdr, cle = _refused_header([0] * 257, [0], cl_lens=cll, coding=zeros(258))
            if cutat != 'whole':
                s.cut(hdr if cutat == 'cut-after-header' else cle)
            out.append(bad(f'refused/{name}/{cutat}', s, 0))
    # an empty code-length code is not refused as a set: zlib reads one bit per
    # length from its table's filler entry (each a length 0) and then misses
    # the end-of-block code -- on the call that brings those 258 bits
    for cutat in ('whole', 'cut-after-code-lengths'):
        s, hdr, cle = _refused_header([0] * 257, [0], cl_lens=[0] * 19, coding=[])
        if cutat != 'whole':
            s.cut(cle)
        out.append(bad(f'refused/cl-empty/{cutat}', s, 0 if cutat == 'whole' else 1))
    return out


def _run_cases():
    out = []
    body = [0x61] * 6 + [(3, 5), 0x61, (4, 6), (3, 5)]

    def add(name, ll, dl, coding, body, want=None):
        s = Stream()
        s.dynamic(body, ll, dl, coding=coding, final=True)
        s.end()
        if want is not None:        # the run the case is named for is really there
            from tests.deflate_writer import run_length_code
            cls = run_length_code(ll + dl) if coding == 'runs' else coding
            n = 0
            for sym, x in cls:
                k = {16: 3, 17: 3, 18: 11}.get(sym, 1) + (x if sym >= 16 else 0)
                if sym == want and n < len(ll) < n + k:
                    break
                n += k
            else:
                raise AssertionError(f'{name}: no {want}-run across the boundary')
        out.append(ok(f'runs/{name}', s))
    # zeros from the last literal/length lengths into the first distance lengths
    tree = {0x61: 1, 256: 2, 257: 3, 258: 3}
    add('17-crossing', lens_of(260, tree), [0, 0, 0, 0, 1], 'runs', body, 17)
    add('18-crossing', lens_of(270, tree), [0] * 10 + [1], 'runs', [0x61] * 42 + [(3, 40), (4, 33)], 18)
    # length 3 from symbols 257, 258 into distance symbols 0..3
    ll = lens_of(259, tree)
    add('16-crossing', ll, [3, 3, 3, 3, 1], 'runs', [0x61, 0x61, 0x61, 0x61, 0x61, (3, 1), (4, 2), (3, 3), (4, 4), (3, 5)], 16)
    # a 16 as the first distance length: it repeats the last literal/length length
    add('16-first-distance', ll, [3, 3, 3, 3, 1], [(v, 0) for v in ll] + [(16, 1), (1, 0)],
        [0x61, 0x61, 0x61, 0x61, 0x61, (3, 4), (4, 3), (3, 2), (4, 1), (4, 6)])
    # a 16 after a 17: it repeats zero
    l2 = lens_of(258, {0x61: 1, 0x62: 2, 256: 3, 257: 3})
    add('16-after-17', l2, [1], [(18, 97 - 11), (1, 0), (2, 0), (17, 7), (16, 3), (18, 127), (17, 0), (3, 0), (3, 0), (1, 0)],
        [0x61, 0x62, (3, 1), 0x61])
    return out


def _largest_header():
    ll, dl = [8] * 226 + [9] * 60, [4] * 2 + [5] * 28
    cl = lens_of(19, {16: 1, 17: 2, 18: 3})
    for v in range(16):
        cl[v] = 7
    s = Stream()
    s.dynamic([0, 255, 144, (258, 1), (3, 3), 7], ll, dl, cl_lens=cl, ncl=19, coding='single', final=True)
    s.end()
    return [ok('header/largest/whole', s), ok('header/largest/bytes', s, every=1), ok('header/largest/cut3', s, every=3)]


# ----------------------------------------------------------------- symbols
def _symbol_cases():
    out = []
    for sym in (286, 287):
        for where in ('mid', 'last'):
            s = Stream()
            s.fixed([0x61, 0x62, Raw(code_bits(FIXED_LIT, sym))], eob=False)
            if where == 'last':
                s.cut()
            s.w.body([0x61] * 20, FIXED_LIT, FIXED_DIST)
            out.append(bad(f'symbol/fixed-literal-{sym}/{where}', s, 0))
    for sym in (30, 31):
        for where in ('mid', 'last', 'last-nothing'):
            s = Stream()
            s.fixed([0x61, 0x62, 0x63, Match(3, None), Raw(code_bits(FIXED_DIST, sym))], eob=False)
            if where != 'mid':
                s.cut()
            if where != 'last-nothing':
                s.w.body([0x61] * 20, FIXED_LIT, FIXED_DIST)
            out.append(bad(f'symbol/fixed-distance-{sym}/{where}', s, 0))
    # every length symbol, every distance symbol: base and largest extra
    sy = [0x7a]
    for i in range(29):
        sy += [(LBASE[i], 1), i & 255, (LBASE[i] + (1 << LEXT[i]) - 1, 2)]
    sy += [Match(258, 1, 284), 0x31, Match(258, 2, 285)]
    s = Stream()
    s.fixed(sy, final=True)
    s.end()
    out.append(ok('symbol/every-length', s))
    s = Stream()
    s.dynamic(sy, LONG_LIT, LONG_DIST, final=True)
    s.end()
    out.append(ok('symbol/every-length/long-codes', s))
    sy = []
    for i in range(30):
        sy += [(3, DBASE[i]), 0x41 + i, (4, DBASE[i] + (1 << DEXT[i]) - 1)]
    for blk in ('fixed', 'long-codes'):
        s = Stream()
        s.stored(_rand(4, 32768))
        s.fixed(sy, final=True) if blk == 'fixed' else s.dynamic(sy, LONG_LIT, LONG_DIST, final=True)
        s.end()
        out.append(ok(f'symbol/every-distance/{blk}', s))
    # the far end of the window, the source in this call, in earlier ones, in both
    for d in (32506, 32507, 32767, 32768):
        s = Stream()
        s.stored(_rand(d, d))
        s.fixed([(100, d), 0x2e], final=True)
        s.end()
        out.append(ok(f'symbol/distance-{d}/same-call', s))
        s = Stream()
        s.stored(_rand(d, d))
        s.cut()
        s.fixed([(100, d), 0x2e, (258, d)], final=True)
        s.end()
        out.append(ok(f'symbol/distance-{d}/history', s))
        s = Stream()
        s.stored(_rand(d, 60))
        s.cut()
        s.stored(_rand(d + 1, d - 50))
        s.fixed([(100, d), 0x2e], final=True)       # source [10, 110): 50 bytes of it from the call before
        s.end()
        out.append(ok(f'symbol/distance-{d}/straddling', s))
        s = Stream()
        s.stored(_rand(d, 40000))
        s.cut()
        s.stored(_rand(d + 2, 500))
        s.cut()
        s.fixed([(258, d), 0x2e, (3, 32768)], final=True)   # through a history that has moved
        s.end()
        out.append(ok(f'symbol/distance-{d}/moved-history', s))
    # back to byte 0, and one byte before it
    s = Stream()
    s.fixed([1, 2, 3, 4, 5, (10, 5), (3, 15), (258, 18)], final=True)
    s.end()
    out.append(ok('symbol/distance-to-byte-0', s))
    s = Stream()
    s.stored(_rand(5, 100))
    s.cut()
    s.fixed([(3, 100), (7, 103)], final=True)
    s.end()
    out.append(ok('symbol/distance-to-byte-0/later-call', s))
    s = Stream()
    s.fixed([1, 2, 3, 4, 5, (3, 6), 7], final=True)
    out.append(bad('symbol/too-far/first-call', s, 0))
    s = Stream()
    s.stored(_rand(5, 100))
    s.cut()
    s.fixed([(3, 100), (3, 104), 7], final=True)
    out.append(bad('symbol/too-far/later-call', s, 1))
    for d in (1, 2, 3):
        for ls in (285, 284):
            s = Stream()
            s.fixed(list(range(0x30, 0x30 + d)) + [Match(258, d, ls), 0x21, Match(258, d, ls)], final=True)
            s.end()
            out.append(ok(f'symbol/258-at-distance-{d}/symbol-{ls}', s))
    return out


# ------------------------------------------------------- blocks and header
def _block_cases():
    out = []
    s = Stream()
    s.stored(b'')
    s.fixed([0x61])
    for _ in range(40):
        s.stored(b'')
    s.stored(b'xyz')
    s.stored(b'', final=True)
    s.end()
    out.append(ok('block/stored-len-0', s))
    out.append(ok('block/stored-len-0/bytes', s, every=1, tail=True))
    s = Stream()
    s.stored(_rand(6, 65535), final=True)
    s.end()
    out.append(ok('block/stored-len-65535', s))
    for where in ('whole', 'cut-in-nlen'):
        s = Stream()
        s.stored(b'abc')
        s.w.stored(b'defgh', nlen=0xfffb, final=True)     # ~5 is 0xfffa
        if where != 'whole':
            s.cuts.append(len(s.w.getvalue()) - 5 - 1)      # the call ends inside NLEN
        out.append(bad(f'block/stored-bad-nlen/{where}', s, 0 if where == 'whole' else 1))
    # a stored block from every bit offset: 3 header bits, b nine-bit literals
    # and a 7-bit end-of-block leave the next block at bit (10 + b) % 8
    s = Stream()
    seen = set()
    for b in range(8):
        s.fixed([0x61, 0x62] + [200 + b] * b)
        seen.add(s.w.nbits % 8)
        s.stored(bytes([b]) * (b + 1), final=b == 7)
    assert seen == set(range(8))
    s.end()
    out.append(ok('block/stored-at-every-bit-offset', s))
    out.append(ok('block/stored-at-every-bit-offset/bytes', s, every=1))
    for where in ('mid', 'last'):
        s = Stream()
        s.fixed([0x61])
        s.w.block_header(False, 3)
        if where == 'last':
            s.cut()
        s.w.raw('0' * 64)
        out.append(bad(f'block/type-3/{where}', s, 0))
    s = Stream()
    for i in range(300):
        s.dynamic([0x78], ONE_LIT, [0], final=i == 299)
    s.end()
    out.append(ok('block/300-dynamic-blocks', s))
    s = Stream()
    for i in range(4):
        s.stored(_rand(7 + i, 37))
        s.fixed([0x61, (5, 20), 0x62])
        s.dynamic([0x63, (3, 1), 0x64, (258, 4)], SMALL_LIT, SMALL_DIST, final=i == 3)
    s.end()
    out.append(ok('block/types-interleaved', s))
    out.append(ok('block/types-interleaved/cut5', s, every=5))
    for ci in range(8):
        d = min((1 << (ci + 8)) + 1, 32768)
        s = Stream(cinfo=ci)
        s.stored(_rand(8 + ci, d))
        s.fixed([(10, d), 0x61], final=True)
        s.end()
        out.append(ok(f'header/cinfo-{ci}', s))
    s = Stream(fdict=1, dictid=0x12345678)
    s.fixed([0x61], final=True)
    s.end()
    out.append(bad('header/fdict/whole', s, 0))
    s = Stream(fdict=1, dictid=0x12345678)
    s.cuts.append(2)                                        # zlib reads the dictionary id before it refuses
    s.fixed([0x61], final=True)
    s.end()
    out.append(bad('header/fdict/cut-after-flg', s, 1))
    s = Stream(cm=7)
    s.fixed([0x61], final=True)
    s.end()
    out.append(bad('header/cm-7', s, 0))
    s = Stream(fcheck=5)
    s.fixed([0x61], final=True)
    s.end()
    out.append(bad('header/bad-fcheck', s, 0))
    s = Stream()
    s.fixed([0x61, 0x62], final=True)
    s.end(adler=0x01230124)
    out.append(bad('trailer/bad-adler', s, 0))
    return out


# ----------------------------------------------------------------- regions
LADDER_MIX = ([0x41] * 5 + [0x42] * 3 + [0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49],
              [284] * 2 + [281] * 2 + [273, 265, 257, 257, 285], [29] * 4 + [28] * 4 + [0, 27, 1, 20, 2, 10, 3, 16, 4, 22])
LONG_MIX = (list(range(3, 256)), list(range(257, 286)), list(range(6, 30)) * 3 + list(range(6)))


def _region_cases():
    out = []
    s = Stream()
    s.dynamic(random_symbols(random.Random(11), 4200, *LADDER_MIX, p_match=0.25), LADDER_LIT, LADDER_DIST, final=True)
    s.end()
    out.append(ok('region/ladder', s, region=True))
    s = Stream()
    s.dynamic(random_symbols(random.Random(12), 6500, *LONG_MIX, p_match=0.25), LONG_LIT, LONG_DIST, final=True)
    s.end()
    out.append(ok('region/long-codes', s, region=True))
    # literals only until the middle, so that "one byte too far" is still
    # possible there (under 32 KiB of output)
    rng = random.Random(13)
    s = Stream()
    head = random_symbols(rng, 3000, LONG_MIX[0], p_match=0)
    tail = random_symbols(rng, 3000, *LONG_MIX, p_match=0.25, produced=3000)
    s.dynamic(head + [(5, 3001)] + tail, LONG_LIT, LONG_DIST, final=True)
    out.append(Case('region/too-far', s.calls(), Error(0), None, True))
    rng = random.Random(14)
    s = Stream()
    head = random_symbols(rng, 3500, LONG_MIX[0], [257, 258, 270, 285], [0], 0.2)
    s.dynamic(head + [Match(7, None), Raw('1')] + head, LONG_LIT, [1], final=True)
    out.append(Case('region/bad-code', s.calls(), Error(0), None, True))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = (_tree_cases() + _refused_cases() + _run_cases() + _largest_header() + _symbol_cases() + _block_cases()
           + _region_cases())
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected():
    """{name: zlib's [(bytes, status)] per call}, computed once."""
    return {c.name: oracle(c.calls) for c in cases()}
