"""The cases of backref_bounded_cases on the CPU: the C oracle and (where
oracle/_ref is built) the reference compiled from its own sources agree on
every one, on every kind of cache, batch by batch and chunk by chunk; and each
BACKREF case comes out different when its BACKREFs are resolved through the
cache instead of the window, and each error-stop case when a skim runs behind
the error, so a decoder that did either could not pass it."""
import pytest

import backref_bounded_cases as BB


@pytest.fixture(scope='module')
def cases(oracle):
    return BB.all_cases(oracle)


def fuzz(oracle):
    return [c for rate in BB.FUZZ_RATES for bad in BB.FUZZ_BAD for c in BB.fuzz_cases(oracle, rate, bad)]


def same(ref, port):
    """Step by step, and the pair's counters (the LRU order is the C oracle's alone)."""
    return ref[:-1] == port[:-1] and ref[-1]['pair_stats'] == port[-1]['pair_stats']


@pytest.mark.parametrize('split', [False, True], ids=['batch', 'chunk'])
@pytest.mark.parametrize('kind', BB.KINDS)
def test_reference_agrees(oracle, ref_oracle, cases, kind, split):
    for c in cases + fuzz(oracle):
        if c['name'] == BB.REPLACE_CASE:
            continue                     # (test_reference_agrees_on_the_replace_case)
        assert same(BB.run_model(ref_oracle, c, kind, split=split), BB.run_model(oracle, c, kind, split=split)), c['name']


_REPLACE_CHILD = '''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import backref_bounded_cases as BB
from oracle.lib import Oracle
port, ref = Oracle(), Oracle(ref=True)
case = [c for c in BB.all_cases(port) if c['name'] == BB.REPLACE_CASE][0]
for kind in BB.KINDS:
    for split in (False, True):
        a, b = BB.run_model(ref, case, kind, split=split), BB.run_model(port, case, kind, split=split)
        assert a[:-1] == b[:-1] and a[-1]['pair_stats'] == b[-1]['pair_stats'], (kind, split)
print('agree')
'''


def test_reference_agrees_on_the_replace_case(ref_oracle):
    """In a child process: the reference's replace keeps a segment it holds no
    reference to (xcodec_cache.h:333-336), which a later window collision may
    unref after it was freed (xcodec_window.h:77-80); only a clean exit counts."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    p = subprocess.run([sys.executable, '-c', _REPLACE_CHILD, here, os.path.dirname(here)], capture_output=True,
                       text=True, timeout=120)
    if p.returncode < 0:
        pytest.xfail('reference crashed (signal %d): its replace/window use-after-free' % -p.returncode)
    assert p.returncode == 0 and p.stdout.strip().endswith('agree'), p.stderr[-2000:]


# (on the pair a hash that left the memory level is still found, on disk: only the cases in which it left both differ)
PAIR_DIFFERS = ('evicted_across_calls', 'window_larger_than_cache')


@pytest.mark.parametrize('kind', ['bounded', 'pair'])
def test_backrefs_through_the_cache_come_out_different(oracle, cases, kind):
    for c in cases + fuzz(oracle):
        if c['alt'] == 'window' and (kind == 'bounded' or c['name'] in PAIR_DIFFERS):
            assert BB.run_model(oracle, c, kind, via_cache=True) != BB.run_model(oracle, c, kind), (c['name'], kind)


def test_a_skim_behind_the_error_stop_comes_out_different(oracle, cases):
    skim = [c for c in cases if c['alt'] == 'skim']
    assert len(skim) == 3
    for c in skim:
        assert BB.run_model(oracle, c, 'bounded', skim_after_error=True) != BB.run_model(oracle, c, 'bounded'), c['name']


def batches(case, res):
    return [r for step, r in zip(case['steps'], res) if step[0] == 'batch']


def test_cases_do_what_they_claim(oracle, cases):
    by = {c['name']: c for c in cases}
    run = lambda name, kind, **kw: batches(by[name], BB.run_model(oracle, by[name], kind, **kw))
    seg = BB.SEG
    # evicted in the batch: the BACKREF decodes A on every cache; the REF behind it is unknown on the bounded one only
    A = by['evicted_in_batch']['steps'][0][1][0][-seg:]
    for kind, st in (('bounded', [0, 1, 2]), ('pair', [0, 0, 0]), ('unbounded', [0, 0, 0])):
        r = run('evicted_in_batch', kind)
        assert r[1]['status'] == st, kind
        assert A in r[1]['outs'][1], kind
    assert len(run('evicted_in_batch', 'bounded')[1]['unknown']) == 1
    # across calls the pair has lost A from its disk too
    for kind, st in (('bounded', 1), ('pair', 1), ('unbounded', 0)):
        r = run('evicted_across_calls', kind)
        assert r[5]['status'][0] == st, kind
        assert r[5]['outs'][0].count(r[0]['outs'][0][:seg]) >= 1
    for name in ('ghit_then_evicted', 'ghit_run_then_evicted'):
        assert run(name, 'bounded')[-1]['status'] == [0, 1, 2], name
        assert run(name, 'unbounded')[-1]['status'] == [0, 0, 0], name
    fa, fb = BB.family(0x5B)[:2]
    for kind in BB.KINDS:
        assert run('window_larger_than_cache', kind)[-1]['status'] == [0, -1, 2], kind
        # the error stop: nothing behind it looked up, so the follow-up finds p1 and p2 gone from a bounded cache
        r = run('error_stop_no_skim', kind)
        assert r[0]['status'] == [-1, 2, 2] and r[0]['unknown'] == [], kind
        assert (len(r[2]['unknown']) == 2) == (kind == 'bounded'), kind
        # the mirror: the skim refreshed them, so the follow-up evicted fillers instead
        r = run('unknown_stop_skims', kind)
        assert r[0]['status'] == [1, 2, 2] and r[0]['unknown'] == [BB.UNKNOWN], kind
        if kind == 'bounded':
            assert len(r[2]['unknown']) == 1 and r[2]['consumed'] == [40]
        assert run('both_stops_ref_then_bref_chunks', kind)[0]['status'] == [1, 2, 2], kind
        assert run('both_stops_bref_then_ref_chunks', kind)[0]['status'] == [-1, 2, 2], kind
        assert run('both_stops_ref_then_bref', kind)[0]['status'] == [1, 2], kind
        assert run('both_stops_bref_then_ref', kind)[0]['status'] == [-1, 2], kind
        r = run('many_backrefs_few_references', kind)
        assert r[0]['status'] == [0, 0] and len(r[0]['outs'][0]) > 300 * seg, kind
        r = run(BB.REPLACE_CASE, kind)
        assert r[0]['status'] == [0, 0, -1, 2], kind
        s2 = r[0]['outs'][0][-seg:]
        assert r[0]['outs'][0] == fa + fa + s2 and r[0]['outs'][1].endswith(fb + fb + fb + s2) and r[0]['outs'][2] == fb, kind


def test_every_batch_is_within_the_limit(oracle, cases):
    """Enters plus cached entries looked up: at most the EXTRACTs plus the
    distinct REF hashes of a batch."""
    from decode_windows_cases import walk
    for c in cases + fuzz(oracle):
        for step in c['steps']:
            if step[0] == 'batch':
                ops = [(kind, e[a + 2:z]) for e in step[1] for kind, a, z in walk(e)]
                refs = sum(1 for kind, _ in ops if kind == 'x') + len({h for kind, h in ops if kind == 'r'})
                assert refs <= BB.LIMIT_SEGS, (c['name'], refs)


def test_fuzz_streams_hold_backrefs_and_errors(oracle):
    from backref_streams import count_backrefs
    for rate in BB.FUZZ_RATES:
        for bad in BB.FUZZ_BAD:
            errs = 0
            for c in BB.fuzz_cases(oracle, rate, bad):
                chunks = [e for step in c['steps'] if step[0] == 'batch' for e in step[1]]
                assert sum(map(count_backrefs, chunks)) > (5 if rate < 0.1 else 50), c['name']
                res = [r for r in batches(c, BB.run_model(oracle, c, 'bounded')) if r is not None]
                errs += sum(1 for r in res if -1 in r['status'])
                assert not any(r['unknown'] for r in res), c['name']
            assert (errs > 0) == (bad > 0), (rate, bad, errs)
