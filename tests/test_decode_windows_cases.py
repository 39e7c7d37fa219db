"""The cases of decode_windows_cases on the CPU: the C oracle and (where
oracle/_ref is built) the reference agree on every one, and each case does
what it claims -- in particular its BACKREFs come out differently when every
chunk runs on a single decoder, so a one-window implementation cannot pass."""
import pytest

import decode_windows_cases as W


@pytest.fixture(scope='module')
def cases(oracle):
    return W.all_cases(oracle)


@pytest.fixture(scope='module')
def modelled(oracle, cases):
    return {c['name']: W.run_model(oracle, c) for c in cases}


def test_reference_agrees(ref_oracle, cases, modelled):
    for c in cases:
        assert W.run_model(ref_oracle, c) == modelled[c['name']], c['name']


def test_a_single_decoder_decodes_them_differently(oracle, cases, modelled):
    for c in cases:
        if c['name'] in W.BACKREF_CASES:
            assert W.run_model(oracle, c, single=True)[0] != modelled[c['name']][0], c['name']


def test_cases_do_what_they_claim(cases, modelled):
    by = {c['name']: c for c in cases}
    # every batch without a stated stop runs to its end
    for name, (res, held) in modelled.items():
        for k, (step, r) in enumerate(zip(by[name]['steps'], res)):
            if step[0] != 'batch':
                continue
            want = by[name].get('expect', {}).get(k, {})
            assert r['status'] == want.get('status', r['status']), (name, k)
            assert r['stop'] == want.get('stop', len(step[1])), (name, k, r['status'])
            if 'status' not in want:
                assert set(r['status']) == {0}, (name, k, r['status'])
    res, held = modelled['interleave']
    assert [len(W.SEG and [e for e in w if e is not None]) for w in res[1]] == [7, 6, 8]
    res, held = modelled['wrap']
    batch = by['wrap']['steps'][2]
    assert len(batch[1][0]) + len(batch[1][2]) == 3000 and batch[2] == [0, 1, 0]
    # window 0: 7 + 300 declares, the last 300 of one hash -- one live slot, at (307 - 1) mod 256
    assert [k for k, e in enumerate(res[3][0]) if e is not None] == [50]
    # window 1: 4 + 5 declares; the REFs to segments 2 -> slot 3, 15 -> slot 7, 7 -> slot 8 (slot 0 emptied)
    assert [k for k, e in enumerate(res[3][1]) if e is not None] == [1, 2, 3, 4, 5, 6, 7, 8]
    res, held = modelled['stop_ref']
    c = by['stop_ref']
    assert res[0]['consumed'][3] == c['expect'][0]['consumed3']
    # the cache holds the EXTRACTs before the stop only (segments 0..4 of 12), then all but four
    assert len(held) == 9
    live = [[k for k, e in enumerate(w) if e is not None] for w in res[1]]
    assert live == [[0, 1], [0, 1, 2, 3], [0, 1]], live        # (windows 0 and 2: chunks 4 and 5 not reached)
    assert set(res[3]['status']) == {0} and res[3]['stop'] == 3
    res, held = modelled['stop_empty_slot']
    assert res[0]['consumed'][1] == by['stop_empty_slot']['expect'][0]['consumed1']
    assert res[0]['outs'][1].endswith(W.LIT.replace(b'\xf1\x00', b'\xf1'))
    assert res[1][0][2] is not None and res[1][1][2] is None       # live in window 0, empty in window 1
    res, held = modelled['name_reuse']
    assert res[0]['outs'][2] == by['name_reuse']['expect'][0]['out2']
    res, held = modelled['partial_op']
    assert res[0]['consumed'][1] == 2 + W.SEG + 3 and len(by['partial_op']['steps'][0][1][1]) == 2 + W.SEG + 3 + 700
