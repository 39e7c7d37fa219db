"""Name reuse inside one decode() call, on the CPU: the oracle restatement
follows the rule the GPU batch decoder restates -- a REF yields
the bytes of the latest preceding EXTRACT of its hash, else the cache's -- on
the fixed streams of tests/test_gpu_decode_reuse.py, and the generator of
scripts/bench_decode_reuse.py makes the two streams it describes."""
import ctypes
import importlib.util
import os

import pytest

from test_gpu_decode_reuse import BR, LIT, E, R, SEG, case1_ops, case4_batches, family, filler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def fam(oracle):
    a, b, c = family(1)
    h = oracle.hash(a)
    assert h == oracle.hash(b) == oracle.hash(c) and len({a, b, c}) == 3
    f = [filler(k) for k in range(4)]
    return dict(A=a, B=b, C=c, h=h, F=f, fh=[oracle.hash(s) for s in f])


@pytest.fixture
def dec(oracle):
    oc = oracle.cache_new()
    od = oracle.decoder_new(oc)
    yield lambda buf: oracle.decode(buf, oc, decoder=od), oc
    oracle.decoder_free(od)
    oracle.cache_free(oc)


def test_latest_preceding_extract_wins(dec, fam):
    A, B = fam['A'], fam['B']
    ok, out, cons, unk = dec[0](b''.join(case1_ops(fam)))
    assert ok and not unk and cons == 3 * 2050 + 20
    assert out == A + B + B + A + A


def test_cached_then_replaced_then_window(dec, fam):
    A, B, F = fam['A'], fam['B'], fam['F']
    b1, b2, b3 = case4_batches(fam)
    assert dec[0](b1)[1] == A + b'lit'
    assert dec[0](b2)[1] == A + B + B + b'\xf1'
    assert dec[0](b3)[:2] == (True, B + F[0] + B + F[0])


def test_backrefs_behind_a_redeclare(dec, fam):
    A, B, h, F = fam['A'], fam['B'], fam['h'], fam['F']
    buf = (E(A) + E(F[0]) + E(B) + BR(2) + R(h) + BR(3) + LIT(b'x\xf1y') + E(A) + BR(4) + BR(1) + BR(0) + b'tail')
    ok, out, cons, unk = dec[0](buf)
    assert not ok and not unk and cons == len(buf) - 4
    assert out == A + F[0] + B + B + B + B + b'x\xf1y' + A + A + F[0]


@pytest.mark.parametrize('late', ['B', 'A'])
def test_extract_behind_the_stop_is_not_reached(oracle, dec, fam, late):
    A, h, L, U, u = fam['A'], fam['h'], fam[late], fam['F'][3], fam['fh'][3]
    ops = [E(A), R(h), R(u), E(L), R(h)]
    assert dec[0](b''.join(ops)) == (True, A + A, 2060, [u])
    assert oracle.lib.xco_cache_size(dec[1]) == 1
    assert oracle.lib.xco_cache_enter(dec[1], u, (ctypes.c_uint8 * SEG).from_buffer_copy(U)) == 0
    assert dec[0](b''.join(ops[2:])) == (True, U + L + L, 2070, [])


def test_bench_generator_streams(oracle):
    spec = importlib.util.spec_from_file_location('bench_decode_reuse',
                                                  os.path.join(ROOT, 'scripts/bench_decode_reuse.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a, b, decoded, n_fam = mod.build_streams(oracle, 64, 0.1, 8, 7)
    assert n_fam > 8 and decoded == 64 * mod.OPS * SEG
    assert [len(x) for x in a] == [len(x) for x in b]
    for s in (a, b):
        oc = oracle.cache_new()
        ok, out, cons, unk = oracle.decode(b''.join(s), oc, out_cap=decoded + 4096)
        oracle.cache_free(oc)
        assert ok and not unk and len(out) == decoded and cons == sum(map(len, s))
    # the twin holds no two EXTRACTs of one hash (its ops are EXTRACTs and REFs only)
    hs = []
    for c in b:
        j = 0
        while j < len(c):
            if c[j + 1] == 0x01:
                hs.append(oracle.hash(c[j + 2:j + 2 + SEG]))
                j += 2 + SEG
            else:
                j += 10
    assert len(hs) == len(set(hs)) and len(hs) > 500
