"""The reference's XCodecPipePair (oracle/_ref/libppref.so) on the conversations
of tests/pipe_many_cases.py, their `dmany` turns run as the serial loop of
decoder_consume calls: it reproduces the committed transcripts
(tests/golden/pipe_many.json, what tests/test_gpu_pipe_decode_many.py compares
the engine's one-call turns with), and the conversations hold what they
claim."""
import json
import os

import pytest

import pipe_cases as pc
import pipe_many_cases as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def golden_many():
    with open(os.path.join(ROOT, 'tests/golden/pipe_many.json')) as f:
        return json.load(f)['conversations']


@pytest.fixture(scope='module')
def R():
    from oracle import refpipe
    if not refpipe.available('ref'):
        pytest.skip('oracle/_ref/libppref.so not built (needs the reference tree)')
    return pc.RefImpl('ref')


def test_golden_lists_every_conversation(golden_many):
    assert sorted(golden_many) == sorted(pm.NAMES)


@pytest.mark.parametrize('name', pm.NAMES)
def test_reference_reproduces_golden(R, golden_many, name):
    assert pm.record(pm.run(pm.conversation(name), R)) == golden_many[name]


def turns(conv):
    """[(first step, pipes)] of the dmany turns."""
    out, cur = [], []
    for k, st in enumerate(conv.steps):
        if st.op in ('dmany', 'dmany_end'):
            cur.append(st.pipe)
            if st.op == 'dmany_end':
                out.append((k - len(cur) + 1, cur))
                cur = []
    return out


def test_conversations_hold_what_they_claim(golden_many):
    """From the golden alone: the middle pipe blocks and its <LEARN> comes back
    beside the others' frames; exactly one pipe fails on the bad opcode; every
    payload arrives; turns of several receiving pipes exist everywhere."""
    for name in pm.NAMES:
        conv, G = pm.conversation(name), golden_many[name]
        assert len(G) == len(conv.steps)
        assert any(len(p) > 1 and p[0][0] in 'rq' for _, p in turns(conv)), name
        sent = sum(len(st.src) for st in conv.steps if st.op in ('enc', 'many', 'many_end') and st.pipe != 'sx'
                   and st.pipe[0] in 'sa')
        got = sum(g['to_local'][0] for st, g in zip(conv.steps, G) if g and st.pipe[0] in 'rq')
        if name != 'many_bad_opcode':
            assert got == sent and not any(g and g['error'] for g in G), name
    conv, G = pm.conversation('many_middle_blocks'), golden_many['many_middle_blocks']
    t = turns(conv)
    k, pipes = t[2]                                        # the receivers' turn with the unknown hashes
    assert pipes == pm._names('r', 5)
    asked = [i for i in range(5) if G[k + i]['to_peer'][0] > 5]      # more than an <ADVANCE>: <ASK>s
    assert asked == [3, 4]
    assert G[k + 3]['to_local'][0] >= 5000 and G[k + 3]['to_local'][0] < 30_000      # a prefix, then blocked
    k2, pipes2 = t[4]                                      # <LEARN> + FRAME for 3 and 4, FRAMEs for the others
    assert pipes2 == pm._names('r', 5) and all(G[k2 + i]['to_local'][0] > 0 for i in range(5))
    G = golden_many['many_bad_opcode']
    assert sum(1 for g in G if g and g['error']) == 1
    G, conv = golden_many['many_eos'], pm.conversation('many_eos')
    assert any(g and g['local_eos'] for g in G) and any(g and g['peer_eos'] for g in G)
    assert any(st.op.startswith('dmany') and st.src == b'' for st in conv.steps)
