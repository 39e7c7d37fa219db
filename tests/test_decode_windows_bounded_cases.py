"""The cases of decode_windows_bounded_cases on the CPU: the C oracle and
(where oracle/_ref is built) the reference compiled from its own sources agree
on every one, on every kind of cache; the cases keep within the limit they
claim; and each comes out different where it has to -- on one decoder for all
chunks, on an unbounded cache -- so an implementation with one window, or one
that ignored the limit, could not pass it."""
import pytest

import decode_windows_bounded_cases as WB
from backref_bounded_cases import LIMIT_SEGS


@pytest.fixture(scope='module')
def cases(oracle):
    return WB.all_cases(oracle)


def by_name(cases):
    return {c['name']: c for c in cases}


NAME_REUSE = 'refused_name_reuse'


@pytest.mark.parametrize('kind', WB.KINDS)
def test_reference_agrees(oracle, ref_oracle, cases, kind):
    for c in cases:
        if c['name'] == NAME_REUSE:
            continue                     # (test_reference_agrees_on_name_reuse)
        ref, port = WB.run_model(ref_oracle, c, kind), WB.run_model(oracle, c, kind)
        assert WB.without_order(ref) == WB.without_order(port), (c['name'], kind)


_CHILD = '''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import decode_windows_bounded_cases as WB
from oracle.lib import Oracle
port, ref = Oracle(), Oracle(ref=True)
case = [c for c in WB.all_cases(port) if c['name'] == sys.argv[3]][0]
for kind in WB.KINDS:
    assert WB.without_order(WB.run_model(ref, case, kind)) == WB.without_order(WB.run_model(port, case, kind)), kind
print('agree')
'''


def test_reference_agrees_on_name_reuse(ref_oracle):
    """In a child process, as tests/test_backref_bounded_cases.py runs its
    replace case: the reference's replace lets go of a segment a window slot
    may still name (xcodec_cache.h:333-336); only a clean exit counts."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    p = subprocess.run([sys.executable, '-c', _CHILD, here, os.path.dirname(here), NAME_REUSE], capture_output=True,
                       text=True, timeout=120)
    if p.returncode < 0:
        pytest.xfail('reference crashed (signal %d): its replace/window use-after-free' % -p.returncode)
    assert p.returncode == 0 and p.stdout.strip().endswith('agree'), p.stderr[-2000:]


def test_every_batch_is_within_the_limit(cases):
    """EXTRACT + REF ops of a batch: at most LIMIT_SEGS, so the reference alone
    never exceeds the limit; (g) keeps to its own limit and (h) goes over on
    purpose."""
    assert set(WB.OWN_LIMIT) < set(WB.CASE_NAMES)
    for c in cases:
        limit = WB.OWN_LIMIT.get(c['name'], LIMIT_SEGS)
        for step in c['steps']:
            if step[0] == 'batch' and limit is not None:
                assert WB.batch_ops(step) <= limit, (c['name'], WB.batch_ops(step))
    over = by_name(cases)['refused_over_limit']['steps'][0]
    assert WB.batch_ops(over) == LIMIT_SEGS + 1 and WB.refused_on(over, 'bounded')
    wrap = by_name(cases)['slot_wrap']
    assert sum(1 for e, w in zip(*wrap['steps'][0][1:3]) if w == 0 for k, _, _ in WB.walk(e) if k in 'xr') == 260


def test_one_decoder_for_all_chunks_comes_out_different(oracle, cases):
    for name in WB.SINGLE_DIFFERS:
        c = by_name(cases)[name]
        for kind in ('bounded', 'pair'):
            assert WB.run_model(oracle, c, kind, single=True) != WB.run_model(oracle, c, kind), (name, kind)


def test_an_unbounded_cache_comes_out_different(oracle, cases):
    for name in WB.UNBOUNDED_DIFFERS:
        c = by_name(cases)[name]
        a, b = WB.without_order(WB.run_model(oracle, c, 'unbounded')), WB.without_order(WB.run_model(oracle, c, 'bounded'))
        a[-1].pop('found'), b[-1].pop('found')      # (the steps themselves, not the closing lookups)
        assert a != b, name


def batches(case, res):
    return [r for step, r in zip(case['steps'], res) if step[0] in ('batch', 'rest')]


def test_cases_do_what_they_claim(oracle, cases):
    by = by_name(cases)
    run = lambda name, kind: batches(by[name], WB.run_model(oracle, by[name], kind))
    # (a) every chunk decodes, on every cache
    for kind in WB.KINDS:
        assert run('cross_refs', kind)[0]['status'] == [0, 0, 0, 0], kind
    # (b) the REF to what the other window's EXTRACT evicted is the stop; a pair finds it on disk
    assert run('evict_then_ref', 'bounded')[0]['status'] == [0, 1, 2]
    assert run('evict_then_ref', 'pair')[0]['status'] == [0, 0, 0]
    assert run('evict_then_ref', 'unbounded')[0]['status'] == [0, 0, 0]
    r = run('ref_then_evict', 'bounded')[0]
    assert r['status'] == [0, 0, 1, 2] and r['stop'] == 2
    # (c) each window its own bytes at slot 0, window 2's empty slot the stop
    for kind in WB.KINDS:
        r = run('slots_outlive_cache', kind)
        first = r[0]['outs']
        assert r[2]['status'] == [0, 0, -1, 2] and r[2]['stop'] == 2, kind
        assert r[2]['outs'][0].startswith(first[0][:WB.SEG]) and r[2]['outs'][1].endswith(first[1]), kind
        assert first[0][:WB.SEG] != first[1]
    assert run('slots_outlive_cache', 'bounded')[3]['status'] == [1, 2]
    assert run('slots_outlive_cache', 'unbounded')[3]['status'] == [0, 0]
    # (d) the stop leaves the LRU tail alone; the skim of the rest step refreshes it
    r = run('stop_leaves_lru', 'bounded')
    f0 = by['stop_leaves_lru']['expect']['f0']
    assert r[0]['status'] == [0, 1, 2] and r[0]['order'][0] == f0
    assert r[1]['status'] == 1 and r[1]['consumed'] == 0 and r[1]['order'][-1] == f0
    assert r[2]['status'] == [0, 0]
    assert r[4]['status'] == [0, 1] and run('stop_leaves_lru', 'unbounded')[4]['status'] == [0, 0]
    # (e) the pair promotes from disk where the bounded cache stops; after the lap the pair stops too
    assert run('pair_promote', 'bounded')[0]['status'] == [1, 2, 2]
    r = run('pair_promote', 'pair')
    assert r[0]['status'] == [0, 0, 0] and r[-2]['status'] == [0, 1]
    # (f)
    for kind in WB.KINDS:
        assert run('interleave', kind)[0]['status'] == by['interleave']['expect']['status'], kind
        assert run('slot_wrap', kind)[0]['status'] == [0] * 7, kind
    # (h) refused batches are decoded serially by the model, and say so
    for name, kinds in (('refused_name_reuse', ('bounded', 'pair')), ('refused_over_limit', ('bounded',))):
        for kind in WB.KINDS:
            assert ('refused' in run(name, kind)[-1]) == (kind in kinds), (name, kind)
