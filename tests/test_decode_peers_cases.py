"""The xcg_decode_call_many cases hold what they claim (CPU: the oracle alone)."""
import pytest

import decode_peers_cases as P
import decode_windows_cases as W

SEG = 2048


@pytest.fixture(scope='module')
def cases(oracle):
    return {c['name']: c for c in P.all_cases(oracle)}


@pytest.fixture(scope='module')
def modelled(oracle, cases):
    return {name: P.run_model(oracle, c) for name, c in cases.items()}


def test_lengths_case(cases, modelled):
    case = cases['lengths']
    lens = sorted({len(enc) for step in case['steps'] for _, enc, _ in step[1]})
    assert lens == [0, 1, 15, 16, 17, 75999, 76000, 76001, 300000]
    results, final = modelled['lengths']
    for r, step in enumerate(case['steps']):
        for (p, enc, _), res in zip(step[1], results[r]):
            if len(enc) == 1:
                assert res[1] == 3 and res[3] == 0                   # a lone F1
            if len(enc) > 100:
                kinds = [k for k, _, _ in W.walk(enc)]
                assert 'x' in kinds and 'r' in kinds and b'\xf1\x00' in enc
                if (r, p) == (1, 1):                                 # the REF nobody can resolve
                    assert res[1] == 1 and res[4] == [case['missing']]
                else:
                    assert res[1] == 0 and res[3] == len(enc), (r, p)
    # round 2 REFs what round 1 EXTRACTed: peer 0's cache holds less than its EXTRACT ops would add up to
    assert all(len(f[1]) > 0 for f in final[:4])


def test_blocked_case(cases, modelled):
    case = cases['blocked']
    results, final = modelled['blocked']
    first, _, second = results
    assert [r[1] for r in first] == [0, 0, 1, 0, 0]
    assert first[2][3] == case['head'] and first[2][4] == case['unknown']
    assert [r[1] for r in second] == [0] * 5 and not any(r[4] for r in second)


def test_outside_case(cases, modelled):
    case = cases['outside']
    res = modelled['outside'][0][2]
    assert case['outside'] == 7 + 2 and case['calls'] == 11 + 2
    assert [r[1] for r in res] == [0, 0, 0, 1, 0, -1, 3, 1, 0, 0, 0]
    assert len(res[3][4]) == 2049
    assert len(res[4][2]) > P.MIB and len(case['steps'][2][1][4][1]) == P.MIB + 1
    assert len(res[7][4]) == 1                                       # the evicted segment only


def test_wide_case(cases, modelled):
    res = modelled['wide'][0][0]
    assert len(res) == 260 and all(r[1] == 0 for r in res)
    assert all(2500 < len(enc) < 3100 for _, enc, _ in cases['wide']['steps'][0][1])
