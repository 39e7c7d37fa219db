"""The grouped calls' expectations are real and their cases can tell the three
semantics apart (CPU only): the C oracle's per-group streams equal the compiled
reference's, enough groups of the mixed batch differ from the independent
encodings of their chunks and from one whole-batch stream, and every
multi-chunk decode case decodes differently on a fresh decoder per chunk."""
import numpy as np
import pytest

import group_cases as gc


@pytest.fixture(scope='module')
def mixed():
    return gc.mixed_batch()


@pytest.fixture(scope='module')
def mixed_expect(oracle, mixed):
    return gc.expect_groups(oracle, *mixed)


def test_mixed_batch_shape(mixed):
    data, offs, lens, gf = mixed
    assert data.size < 1.1 * (1 << 20) and lens.size == 180
    assert gf[0] == 0 and gf[-1] == 180 and (np.diff(gf.astype(np.int64)) >= 1).all()
    tot = [int(lens[a:b].sum()) for a, b in zip(gf[:-1], gf[1:])]
    assert max(tot) <= gc.SMALL_ENC
    assert len({int(o) % 16 for o in offs}) == 16
    assert {0, 1}.issubset({min(int(n), 1) for n in lens})     # empty chunks and others


def test_mixed_matches_reference(ref_oracle, mixed, mixed_expect):
    data, offs, lens, gf = mixed
    got = []
    for a, b in zip(gf[:-1], gf[1:]):
        c = ref_oracle.cache_new()
        got += ref_oracle.encode_batch(data, offs[a:b], lens[a:b], mode=1, cache=c)
        ref_oracle.cache_free(c)
    assert got == mixed_expect


def test_mixed_tells_semantics_apart(oracle, mixed, mixed_expect):
    data, offs, lens, gf = mixed
    indep = oracle.encode_batch(data, offs, lens, mode=0)
    whole = oracle.encode_batch(data, offs, lens, mode=1)
    multi = [(a, b) for a, b in zip(gf[:-1], gf[1:]) if b - a > 1]
    vs_indep = sum(mixed_expect[a:b] != indep[a:b] for a, b in multi)
    vs_whole = sum(mixed_expect[a:b] != whole[a:b] for a, b in zip(gf[1:-1], gf[2:]))
    print('multi-chunk groups', len(multi), 'differ from independent', vs_indep, 'groups after the first',
          len(gf) - 2, 'differ from one stream', vs_whole)
    assert vs_indep >= 8
    assert vs_whole >= 20


def test_mixed_round_trips(oracle, mixed, mixed_expect):
    data, offs, lens, gf = mixed
    for a, b in zip(gf[:-1], gf[1:]):
        res = gc.decode_expect(oracle, mixed_expect[a:b])
        for i, (st, out, cons, unk) in zip(range(a, b), res):
            assert (st, cons) == (0, len(mixed_expect[i]))
            assert out == data[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes()


def test_class_edge_groups_have_cross_chunk_refs(oracle):
    for name, chunks in gc.class_edge_groups().items():
        data, offs, lens = gc.lay_out(chunks, np.random.default_rng(1))
        exp = gc.expect_groups(oracle, data, offs, lens, np.array([0, len(chunks)], np.uint32))
        ne = sum(gc.op_counts(e)[0] for e in exp)
        nr = sum(gc.op_counts(e)[1] for e in exp)
        if name == '1024x512':
            assert ne == nr == 0
            continue
        assert nr > 0 and exp != oracle.encode_batch(data, offs, lens, mode=0), name
        if name == '512k_256x2k':
            assert ne + nr == 256       # every chunk declares or references: 256 chunks at work


def test_decode_cases_need_the_group(oracle):
    groups = dict(gc.cross_chunk_groups(oracle))
    stops, neighbour = gc.stop_groups(oracle)
    groups.update(stops)
    groups['neighbour'] = neighbour
    groups['capacity'] = gc.capacity_group(oracle)[0]
    groups['room'], groups['room_blocked'] = gc.room_groups(oracle)
    for name, grp in groups.items():
        assert len(grp) > 1
        assert gc.decode_expect(oracle, grp) != gc.decode_expect_fresh(oracle, grp), name


def test_stop_groups_stop_at_chunk_1(oracle):
    stops, _ = gc.stop_groups(oracle)
    for name, grp in stops.items():
        st = [r[0] for r in gc.decode_expect(oracle, grp)]
        if name == 'ref_order_first':
            assert st == [1, 2, 2]
        else:
            assert st[0] == 0 and st[1] in (-1, 3) and st[2:] == [2, 2], (name, st)


def test_capacity_groups(oracle):
    grp, plain = gc.capacity_group(oracle)
    assert len(grp) == 8 and gc.SMALL_DEC < sum(map(len, grp)) <= gc.LARGE_DEC
    assert sum(e.count(b'\xf1\x01') >= 1 for e in grp) == 8
    res = gc.decode_expect(oracle, grp)
    assert all(r[0] == 0 for r in res) and sum(len(r[1]) for r in res) == plain
    over = gc.over_capacity_group()
    assert sum(len(e) // 2050 for e in over) == 512
