"""The foreign-stream case list (tests/inflate_cases.py) and the writer that
builds it (tests/deflate_writer.py) against zlib on the CPU: what a case
declares is what zlib does with its cuts, what it decodes to is what its
symbols mean, and random symbol lists through random valid trees decode."""
import random
import zlib

import pytest

from tests.deflate_writer import (DeflateWriter, balanced_lengths, canonical_codes, expand, random_complete_lengths,
                                  random_symbols, run_length_code)
from tests.inflate_cases import Error, cases, expected

PEND_CAP = 1024              # the kernel's carried-input room (xcg_inflate.hip)


@pytest.mark.parametrize('case', cases(), ids=lambda c: c.name)
def test_case_expectation_is_zlibs(case):
    got = expected()[case.name]
    st = [s for _, s in got]
    if isinstance(case.expect, Error):
        k = case.expect.call
        assert len(case.calls) > k
        assert all(s == 0 for s in st[:k]) and all(s == -1 for s in st[k:]), st
        assert case.symbols is None
    else:
        assert -1 not in st and st[-1] == 1, st
        assert b''.join(o for o, _ in got) == case.expect
        assert expand(case.symbols) == case.expect
        # the drop-in driver's output room per call
        for c, (o, _) in zip(case.calls, got):
            assert len(o) <= 8 * len(c) + 4 * 65536 + 4096


def test_case_list_covers_what_it_names():
    names = {c.name for c in cases()}
    for part in ('tree/no-distance-code/ndist1', 'tree/one-distance-code/bad-code/last-nothing',
                 'tree/eob-only/50-blocks', 'tree/ladder/48-bit-symbol', 'refused/cl-one-1bit/cut-after-code-lengths',
                 'refused/hdist31/cut-after-header', 'runs/16-after-17', 'header/largest/bytes',
                 'symbol/fixed-distance-31/last-nothing', 'symbol/distance-32768/straddling',
                 'symbol/too-far/later-call', 'block/stored-at-every-bit-offset', 'block/300-dynamic-blocks',
                 'header/cinfo-0', 'header/fdict/whole', 'region/ladder', 'region/bad-code'):
        assert part in names, part
    for c in cases():
        z = b''.join(c.calls)
        if c.region:
            assert 8192 <= len(z) <= 16384, (c.name, len(z))
            assert len(c.calls) == 1
        if c.name.startswith('header/largest'):
            assert len(z) < PEND_CAP      # a header cut anywhere is carried whole
        if c.name.endswith('/bytes'):
            assert all(len(x) == 1 for x in c.calls if x)
    # the invalid code of a last-bits case sits in its call's last byte: the
    # same stream cut one byte earlier is not refused yet
    for c in cases():
        if '/last' in c.name:
            z = zlib.decompressobj(15)
            z.decompress(c.calls[0][:-1])
            with pytest.raises(zlib.error):
                z.decompress(c.calls[0][-1:])


def test_writer_primitives():
    assert canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]      # RFC 1951 3.2.2's example
    assert run_length_code([0] * 140 + [5] * 8 + [0] * 4) == [(18, 127), (0, 0), (0, 0), (5, 0), (16, 3), (5, 0), (17, 1)]
    for k in range(2, 40):
        assert sum(2.0 ** -n for n in balanced_lengths(k)) == 1
    w = DeflateWriter()
    w.zlib_header()
    assert w.getvalue() == bytes([0x78, 0x9c])
    w.stored(b'hello', final=True)
    w.zlib_trailer(b'hello')
    assert zlib.decompress(w.getvalue()) == b'hello'
    assert expand([1, 2, 3, (5, 2)]) == bytes([1, 2, 3, 2, 3, 2, 3, 2])


@pytest.mark.parametrize('seed', range(6))
def test_random_symbols_through_random_trees(seed):
    """50 streams per seed: a seeded random symbol list, random complete trees
    over exactly the symbols it uses (codes up to 15 bits), a random coding of
    the header's length sequence; zlib decodes each to expand() of the list."""
    from tests.deflate_writer import Match, distance_symbol, length_symbol
    rng = random.Random(1000 + seed)
    for it in range(50):
        lits = rng.sample(range(256), rng.randint(1, 60))
        syms = random_symbols(rng, rng.randint(1, 400), lits, p_match=rng.choice([0, 0.1, 0.5, 0.9]),
                              dist_max=rng.choice([1, 4, 300, 32768]))
        if rng.random() < 0.3:       # far distances need a long output first
            syms = [lits[0], (258, 1)] * 130 + syms + random_symbols(rng, 100, lits, p_match=0.7, produced=33000,
                                                                   dist_min=rng.choice([1, 20000, 32000]))
        ul, ud = {256}, set()
        for s in syms:
            if isinstance(s, int):
                ul.add(s)
            else:
                m = s if isinstance(s, Match) else Match(*s)
                ul.add(m.length_symbol or length_symbol(m.length)[0])
                ud.add(distance_symbol(m.distance)[0])
        while len(ul) < 2:
            ul.add(rng.randrange(256))
        while len(ud) < 2:
            ud.add(rng.randrange(30))
        ll, dl = [0] * 286, [0] * 30
        for s, n in zip(sorted(ul), random_complete_lengths(rng, len(ul))):
            ll[s] = n
        for s, n in zip(sorted(ud), random_complete_lengths(rng, len(ud))):
            dl[s] = n
        w = DeflateWriter()
        w.zlib_header(cinfo=rng.randint(0, 7))
        if rng.random() < 0.5:
            w.stored(b'', final=False)
        w.dynamic(syms, ll, dl, final=True, coding=rng.choice(['single', 'runs']),
                  nlen=rng.randint(max(ul) + 1, 286), ndist=rng.randint(max(ud) + 1, 30))
        data = expand(syms)
        w.zlib_trailer(data)
        assert zlib.decompress(w.getvalue()) == data, (seed, it)
