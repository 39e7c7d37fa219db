"""The expectations of the independent batch decoder's tests, on the CPU: for
every case of tests/indep_decode_cases.py the oracle restatement on a fresh
cache and decoder gives what the compiled reference gives (XCodecDecoder::decode,
xcodec/xcodec_decoder.cc:66-188).  The name-reuse cases are checked against
literal byte strings instead: the reference's XCodecMemoryCache::replace cannot
run in-process on them (see the note at the top of tests/test_gpu_decode_reuse.py)."""
import indep_decode_cases as idc
from indep_decode_cases import R, expect


def both(oracle, ref_oracle, enc, out_cap=None):
    a, b = expect(oracle, enc, out_cap), expect(ref_oracle, enc, out_cap)
    assert a == b, (a[0], a[2], a[3], len(a[1]), b[0], b[2], b[3], len(b[1]))
    return a


def test_probe_values(oracle, ref_oracle):
    S = idc.seg_of(1)
    h = oracle.hash(S)
    assert h == ref_oracle.hash(S)
    assert both(oracle, ref_oracle, b'ab' + R(h) + b'cd') == (1, b'ab', 2, h)
    assert both(oracle, ref_oracle, b'xy\xf1\x07zz') == (-1, b'xy', 2, 0)
    assert both(oracle, ref_oracle, b'xy\xf1') == (3, b'xy', 2, 0)
    assert both(oracle, ref_oracle, b'xy\xf1\x03\x05q') == (-1, b'xy', 5, 0)


def test_round_trip_per_chunk(oracle, ref_oracle):
    for name in ('kat_a', 'magic_heavy'):
        plain, encs = idc.independent_encodings(oracle, name)
        assert len(plain) >= 4
        for p, e in zip(plain, encs):
            assert both(oracle, ref_oracle, e) == (0, p, len(e), 0)


def test_isolation(oracle, ref_oracle):
    chunks, h = idc.isolation(oracle)
    S = idc.seg_of(1)
    got = [both(oracle, ref_oracle, c) for c in chunks]
    assert got == [(0, S, 2050, 0), (1, b'ab', 2, h), (0, S + S, 2060, 0)]


def test_errors(oracle, ref_oracle):
    c = idc.error_chunks(oracle)
    got = {k: both(oracle, ref_oracle, v) for k, v in c.items()}
    assert {k: v[0] for k, v in got.items()} == {
        'good': 0, 'bad_opcode': -1, 'lone_f1': 3, 'extract_cut': 3, 'ref_cut': 3, 'backref_cut': 3,
        'backref_empty': -1, 'backref_empty_after_declares': -1, 'op_byte_only_after_extract': 3}
    assert got['extract_cut'][2] == 1 and got['ref_cut'][2] == 2050 and got['backref_cut'][2] == 2050
    assert got['backref_empty'][1:3] == (b'xy', 5)                      # the BACKREF op has been moved out
    assert got['backref_empty_after_declares'][2] == 2050 + 6


def test_literal_edges_and_ref_order(oracle, ref_oracle):
    for k, v in idc.literal_edges(oracle).items():
        st, out, cons, _ = both(oracle, ref_oracle, v)
        assert (st, cons) == (1 if k == 'esc_then_op_at_1024' else 0, 1024 if k == 'esc_then_op_at_1024' else len(v)), k
    assert both(oracle, ref_oracle, idc.ref_order(oracle))[::2] == (1, 4)


def test_window(oracle, ref_oracle):
    got = {k: both(oracle, ref_oracle, v) for k, v in idc.window_chunks(oracle).items()}
    assert all(got['valid%d' % k][0] == 0 for k in range(3))
    assert got['wrap_live'][0] == 0 and got['wrap_emptied'][0] == -1
    assert len(got['wrap_live'][1]) == (1 + 300 + 3) * 2048 + 3


def test_largest_chunk(oracle, ref_oracle):
    enc, need = idc.largest_chunk(oracle)
    st, out, cons, _ = both(oracle, ref_oracle, enc, out_cap=need + 4096)
    assert (st, len(out), cons) == (0, need, len(enc))


def test_name_reuse_literals(oracle):
    for k, (enc, (st, out, cons)) in idc.reuse_table(oracle).items():
        got = expect(oracle, enc)
        assert got[0] == st and got[2] == cons and got[1] == out and got[3] == 0, (k, got[0], got[2], len(got[1]))
