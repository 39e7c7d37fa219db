"""The constructed-collision cases (tests/collision_cases.py) on the CPU: the
blocks are related as their tier says, the plain model, the oracle and the
compiled reference agree byte for byte on every case, every case reaches the
branch it is named for, and its output would change under each wrong policy
that can be observed in it.  tests/golden/collisions.json (the reference's
output, tests/golden/make_collision_golden.py) is what the GPU tests check
against on a machine without the reference."""
import importlib.util
import json
import os

import pytest

import collision_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_collision_golden',
                                               os.path.join(HERE, 'golden/make_collision_golden.py'))
mcg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mcg)

SEG = cc.SEG
M32 = cc.M32
CASES = cc.all_cases()
IDS = [c[0] for c in CASES]


@pytest.fixture(scope='module')
def golden_collisions():
    with open(os.path.join(HERE, 'golden/collisions.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def exact():
    """The model's exact run of every case, computed once."""
    return {c[0]: cc.model_case(c) for c in CASES}


def _tier_relations(o):
    for tier in cc.TIERS:
        for at in (cc.AT if tier in ('full', 'lo') else (100,)):
            for nvar in (2, 3):
                tw = cc.twins(31 * at + nvar, tier, at, nvar)
                assert len(tw) == nvar == len(set(tw)) and all(len(t) == SEG for t in tw)
                hs = [o.hash(t) for t in tw]
                ks = [cc.dm_key(t) for t in tw]
                if tier != 'none':          # the blocks differ in the named bytes only
                    lo_, hi_ = (SEG - 2, SEG) if tier == 'key' else (at, at + 3)
                    for t in tw[1:]:
                        diff = [k for k in range(SEG) if t[k] != tw[0][k]]
                        assert diff and lo_ <= diff[0] and diff[-1] < hi_, (tier, at, diff)
                        if tier != 'key':
                            assert diff[0] == at and diff[-1] == at + 2
                if tier == 'full':
                    assert len(set(hs)) == 1, (tier, at)
                elif tier == 'lo':
                    assert len({h & M32 for h in hs}) == 1 and len({h >> 32 for h in hs}) == nvar, (tier, at)
                    assert len({h & 0xFFFFFFFFF for h in hs}) == 1          # (the low 36 bits, in fact)
                elif tier == 'key':
                    assert len(set(ks)) == 1 and len({h & M32 for h in hs}) == nvar
                else:
                    assert len({h & M32 for h in hs}) == nvar and len(set(ks)) == nvar


def test_tier_relations(oracle):
    _tier_relations(oracle)


def test_tier_relations_reference(ref_oracle):
    _tier_relations(ref_oracle)


def test_probe_key_formula():
    """The model derives the probe key of every window from its hash and byte
    sum; dm_key computes it from the definition."""
    x = cc.rnd(5, 3 * SEG)
    cache = cc._Cache()
    cc._encode_one(x, cache, False, 'exact')
    assert [k for _, k in cache.d.values()] == [cc.dm_key(x[c:c + SEG]) for c in (0, SEG, 2 * SEG)]


def test_family_unchanged(oracle):
    """family() moved here from the decoder tests; the digests are those of
    the blocks it gave there (family(1), and pipe_cases' family(7)[:2])."""
    import hashlib
    a, b, c = cc.family(1)
    assert oracle.hash(a) == oracle.hash(b) == oracle.hash(c) and len({a, b, c}) == 3
    assert hashlib.sha256(a + b + c).hexdigest() == \
        'a25f96c30e8e8b5809f3af0edc807301a9e98b9c10c087a7cac2388b1489504c'
    assert hashlib.sha256(b''.join(cc.family(7, 2))).hexdigest() == \
        '5a76ec39aa28f445843ffe37124a0dad0a94283edc30587fdd83d1c86a4bdc3b'


def test_shapes():
    n_large = 0
    for name, data, offs, lens, mode, kw in CASES:
        assert len(offs) <= 64, name
        assert int(offs[-1]) + int(lens[-1]) == data.size, name
        assert {int(o) % 16 for o in offs} <= {0, 9}, name
        for n in lens:
            assert 4096 <= int(n) <= 16384 or int(n) == cc.LARGE, (name, int(n))
        n_large += sum(int(n) == cc.LARGE for n in lens)
        assert sum(kw.get('calls', [len(offs)])) == len(offs), name
    assert n_large == sum(1 for c in CASES if c[5].get('large'))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_model_equals_oracle(oracle, exact, case):
    outs, sizes, _ = cc.oracle_case(oracle, case)
    got = [b for b, _ in exact[case[0]]]
    bad = [i for i in range(len(outs)) if got[i] != outs[i]]
    assert not bad, (case[0], bad)
    if case[4] == 'lru':           # the oracle's final cache_size: the model's LRU holds as many
        m = cc._Cache(case[5]['limit'] // SEG)
        for x in cc.chunks_of_case(case):
            cc._encode_one(x, m, False, 'exact')
        assert sizes[-1] == len(m.d) == cc.LRU_LIMIT


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_oracle_equals_reference(oracle, ref_oracle, case):
    if not mcg.runs_on_reference(case):
        assert case[5]['oob']      # (the reference declares out of band only on its null cache)
        return
    outs, _, st = cc.oracle_case(oracle, case)
    routs, _, rst = cc.oracle_case(ref_oracle, case)
    assert outs == routs, case[0]
    assert st == rst, case[0]


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_reach(exact, case):
    """Every case takes the branch it is named for (counts from the model)."""
    name, _, _, _, mode, kw = case
    colls = [st[2] for _, st in exact[name]]
    if mode == 'independent':
        geoms = kw['geoms']
        for g, n in zip(geoms, colls):
            if kw['tier'] == 'full':
                assert n >= (2 if g in ('abc', 'chain') else 1), (name, g, n)
            else:
                assert n == 0, (name, g, n)
    elif kw['tier'] == 'full' and kw['reach']:
        assert sum(colls) >= 1, name
    else:
        assert sum(colls) == 0, name


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_sensitive(exact, case):
    """The exact output differs from every wrong policy's that applies."""
    name, _, _, _, mode, kw = case
    good = [b for b, _ in exact[name]]
    if mode == 'independent':
        allp = sorted({p for ps in kw['policies'] for p in ps})
        assert allp or kw['tier'] == 'none'
        wrong = {p: [b for b, _ in cc.model_case(case, p)] for p in allp}
        for i, (g, ps) in enumerate(zip(kw['geoms'], kw['policies'])):
            assert ps or kw['tier'] == 'none'
            for p in ps:
                assert wrong[p][i] != good[i], (name, g, p)
        return
    for p in kw['policies']:
        assert [b for b, _ in cc.model_case(case, p)] != good, (name, p)
    if kw.get('round_view'):
        # What the first round sees of the last chunk -- its predecessors
        # parsed without the first chunk's declaration -- is another parse
        # than the sequential one: the collision appears (round_dep) or goes
        # away (mirror) at the fixed point.  For the 'lo' mirror the same holds
        # of a lo match that round 0 would wrongly have taken for one.
        chunks = cc.chunks_of_case(case)
        mirror = name.startswith('stream_mirror')
        if kw['tier'] == 'full':
            r0 = cc.encode_model(chunks[1:])
            assert r0[-1][0] != good[-1], name
            assert (r0[-1][1][2], exact[name][-1][1][2]) == ((1, 0) if mirror else (0, 1)), name
        elif mirror:
            assert cc.encode_model(chunks[1:], policy='lo_is_collision')[-1][0] != good[-1], name
    assert kw['policies'] or kw.get('round_view'), name


def test_pair_case_needs_the_disk(oracle):
    """With the memory level alone, A is gone when B is looked up: the pair
    case's output comes from the disk level."""
    from oracle.lib import MODE_STREAM
    for case in cc.pair_cases():
        _, data, offs, lens, _, kw = case
        outs, _, st = cc.oracle_case(oracle, case)
        c = oracle.cache_new(kw['limit'])
        alone = oracle.encode_batch(data, offs, lens, mode=MODE_STREAM, cache=c)
        oracle.cache_free(c)
        assert alone != outs
        assert st[1] < 204                       # the disk never laps: the unbounded model applies


def test_golden_matches_oracle(oracle, golden_collisions):
    import hashlib
    want = {c[0] for c in CASES if mcg.runs_on_reference(c)}
    assert set(golden_collisions['cases']) == want
    for case in CASES:
        if case[0] not in want:
            continue
        g = golden_collisions['cases'][case[0]]
        outs, _, st = cc.oracle_case(oracle, case)
        assert [len(o) for o in outs] == g['lens'], case[0]
        assert [hashlib.sha256(o).hexdigest()[:32] for o in outs] == g['chunk_sha256'], case[0]
        if st is not None:
            assert list(st) == [g['disk_entries'], g['disk_written']]


def test_golden_regenerates(ref_oracle, golden_collisions):
    assert mcg.generate(ref_oracle) == golden_collisions
