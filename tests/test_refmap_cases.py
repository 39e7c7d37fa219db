"""The refmap cases and their walker, on the CPU: the walker over an encoder's
output is the reference's own refmap (where oracle/_ref is built), and every
case holds the REFs it is built to hold."""
import numpy as np
import pytest

import refmap_cases as rc
from oracle.lib import MODE_STREAM

SEG = rc.SEG


def encode_batches(orc, batches, oob=False, limit_bytes=0, cache=None):
    """Per batch the chunk encodings of the oracle's stream encoder on one cache."""
    own = cache is None
    c = orc.cache_new(limit_bytes) if own else cache
    out = []
    for parts in batches:
        d, offs, lens = rc.chunked(parts)
        out.append(orc.encode_batch(d, offs, lens, mode=MODE_STREAM, oob=oob, cache=c))
    if own:
        orc.cache_free(c)
    return out


def expected(orc, batches, limit_bytes=0, cache=None):
    """Per batch, per chunk: (encoding, [(hash, pos)], walked) from the in-band oracle."""
    encs = encode_batches(orc, batches, limit_bytes=limit_bytes, cache=cache)
    return [[(e,) + rc.walk(e) for e in b] for b in encs]


def test_the_seeded_segments_are_the_ones_the_cases_name(oracle):
    s = rc.segs()
    hs = [oracle.hash(x) for x in s]
    assert [k for k, h in enumerate(hs) if h & 0xFF == 0xF1][0] == rc.IDX_A
    assert 0xF1 in hs[rc.IDX_B].to_bytes(8, 'big')[1:7]
    assert hs[rc.IDX_C] >> 63 == 1
    assert len(set(hs)) == len(hs)


@pytest.mark.parametrize('name', sorted(rc.stream_cases()))
def test_walker_is_the_reference_refmap(ref_oracle, name):
    """Call by call on one persistent encoder: the same hash set, the same
    segment bytes, ascending order."""
    batches, counts = rc.stream_cases()[name]
    cache = ref_oracle.cache_new(0)
    enc = ref_oracle.encoder_new(cache)
    try:
        for parts, cnt in zip(batches, counts):
            for part, k in zip(parts, cnt):
                out, refs = ref_oracle.encode_refmap(enc, part)
                got, walked = rc.walk(out)
                assert walked == len(out)
                assert [h for h, _ in got] == list(refs) == sorted(refs)
                assert [part[p:p + SEG] for _, p in got] == list(refs.values())
                assert len(got) == k
    finally:
        ref_oracle.encoder_free(enc)
        ref_oracle.cache_free(cache)


@pytest.mark.parametrize('name', sorted(rc.stream_cases()))
def test_cases_hold_what_they_claim(oracle, name):
    batches, counts = rc.stream_cases()[name]
    exp = expected(oracle, batches)
    for b, parts in enumerate(batches):
        for k, part in enumerate(parts):
            e, refs, walked = exp[b][k]
            assert walked == len(e)
            assert len(refs) == counts[b][k], (b, k)
            for h, p in refs:
                assert oracle.hash(part[p:p + SEG]) == h
    assert any(n for cnt in counts for n in cnt) or name == 'edges'


def test_f1_case_byte_for_byte(oracle):
    """The encoding the case is about: 4140 bytes, REF A | 00 02 | REF A, and
    an escaped F1 in front of each first REF."""
    a, b, _ = rc.abc()
    ha, hb = oracle.hash(a).to_bytes(8, 'big'), oracle.hash(b).to_bytes(8, 'big')
    assert ha[-1] == 0xF1
    (e, refs, walked), = expected(oracle, [[rc.f1_input()]])[0]
    assert e == (b'\xf1\x01' + a + b'ab\xf1\x00\xf1\x00' + b'\xf1\x02' + ha + b'\x00\x02' + b'\xf1\x02' + ha +
                 b'\xf1\x01' + b + b'\xf1\x00' + b'\xf1\x02' + hb)
    assert len(e) == 4140 == walked
    assert dict(refs) == {oracle.hash(rc.segs()[k]): p for k, p in rc.F1_REFS.items()}


def test_payload_case_has_ops_inside_its_extract(oracle):
    (e, refs, _), = expected(oracle, [rc.stream_cases()['payload'][0][0]])[0]
    p = rc.payload_segment()
    assert b'\xf1\x01' + p in e and p.count(b'\xf1\x02') > 100 and p.count(b'\xf1\x00') > 100
    assert sorted(pos for _, pos in refs) == [2 * SEG + 1, 3 * SEG + 1]


def test_out_of_band_expectation(oracle):
    """The out-of-band output is the in-band one with its EXTRACTs written as
    F1 02 hash: the parse is the same, so the in-band walk names its REFs."""
    d = rc.oob_input()
    (inb,), = encode_batches(oracle, [[d]])
    (oob,), = encode_batches(oracle, [[d]], oob=True)
    assert oob != inb and oob == rc.extract_to_oob(inb, oracle.hash)
    refs, _ = rc.walk(inb)
    a, b, _ = rc.abc()
    assert dict(refs) == {oracle.hash(a): 2 * SEG + 2, oracle.hash(b): 4 * SEG + 2}
    # the plain walk of the out-of-band bytes takes the declarations for REFs ...
    plain, _ = rc.walk(oob)
    assert len(plain) == 3 and dict(plain)[oracle.hash(a)] == 0
    # ... and the declaration rows put it right
    decls = {(0, oracle.hash(a)), (SEG, oracle.hash(b)), (3 * SEG + 2, oracle.hash(rc.segs()[5]))}
    assert rc.walk(oob, decls=decls)[0] == refs
    assert rc.walk(oob, collect=False) == ([], len(oob))


def test_stops_and_the_257th_hash():
    for name, (enc, n, walked) in rc.stops().items():
        refs, w = rc.walk(enc)
        assert (len(refs), w) == (n, walked), name
    enc, hs = rc.crafted_refs()
    assert len(enc) == 2570
    refs, w = rc.walk(enc)
    assert w == 2560 and [h for h, _ in refs] == sorted(hs[:256])
    assert [p for _, p in refs] == [SEG * hs.index(h) for h, _ in refs]
    assert any(h >> 63 for h in hs) and not all(h >> 63 for h in hs)
    # a repeated hash past the limit is no new entry: the walk goes on
    again = enc[:2560] + enc[:10] + enc[2560:]
    assert rc.walk(again)[1] == 2570


def test_every_prefix_is_walkable(oracle):
    (e, _, _), = expected(oracle, [[rc.f1_input()]])[0]
    counts = [len(rc.walk(e, n)[0]) for n in range(len(e) + 1)]
    assert counts[0] == 0 and counts[-1] == 2 and counts == sorted(counts)
    assert rc.walk(e, 2050 + 6 + 9) == ([], 2056) and rc.walk(e, 2050 + 6 + 10)[1] == 2066
