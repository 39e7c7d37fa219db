"""The reference's XCodecPipePair (oracle/_ref/libppref.so) on the hub
conversations of tests/pipe_peers_cases.py, their `dmany` turns run as the
serial loop of decoder_consume calls: it reproduces the committed transcripts
(tests/golden/pipe_peers.json, what tests/test_gpu_pipe_peers.py compares the
engine's one-call turns with), and the conversations hold what they claim."""
import json
import os

import pytest

import pipe_cases as pc
import pipe_peers_cases as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def golden_peers():
    with open(os.path.join(ROOT, 'tests/golden/pipe_peers.json')) as f:
        return json.load(f)['conversations']


@pytest.fixture(scope='module')
def R():
    from oracle import refpipe
    if not refpipe.available('ref'):
        pytest.skip('oracle/_ref/libppref.so not built (needs the reference tree)')
    return pc.RefImpl('ref')


def test_golden_lists_every_conversation(golden_peers):
    assert sorted(golden_peers) == sorted(pp.NAMES)


@pytest.mark.parametrize('name', pp.NAMES)
def test_reference_reproduces_golden(R, golden_peers, name):
    assert pp.record(pp.run(pp.conversation(name), R)) == golden_peers[name]


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


def test_uuids_are_distinct_and_well_formed():
    us = [pp.peer_uuid(i) for i in range(16)] + [pc.UUID_V]
    assert len(set(us)) == len(us) and all(len(u) == 36 for u in us)


def test_conversations_hold_what_they_claim(golden_peers):
    """From the golden alone: every turn of the hub behind the <HELLO>s that
    delivers bytes does so for more than one decoder context; exactly one pipe
    fails in (d); every payload arrives; the blocked pipe asks and learns."""
    for name in pp.NAMES:
        conv, G = pp.conversation(name), golden_peers[name]
        assert len(G) == len(conv.steps)
        hub = [(k, p) for k, p in turns(conv) if p[0][0] == 'r']
        assert len(hub) >= 3, name
        for t in conv.counted:
            k, pipes = hub[t]
            live = {conv.peer_of[p] for i, p in enumerate(pipes) if G[k + i] and G[k + i]['to_local'][0] > 0}
            assert len(live) > 1, (name, t)
        failed = getattr(conv, 'failed', None)
        sent = sum(len(st.src) for st in conv.steps if st.op == 'enc' and st.pipe[0] == 'p' and st.pipe[-1] != 'x')
        got = sum(g['to_local'][0] for st, g in zip(conv.steps, G) if g and st.pipe[0] == 'r')
        assert got == sent, name
        errors = [st.pipe for st, g in zip(conv.steps, G) if g and g['error']]
        assert errors == ([failed] if failed else []), name
    conv, G = pp.conversation('peers_blocks'), golden_peers['peers_blocks']
    assert G[conv.asked]['to_peer'][0] > 5 + 3 and 5_000 <= G[conv.asked]['to_local'][0] < 30_000   # a prefix, then <ASK>
    assert G[conv.learned]['to_peer'][0] > 2048                                                   # the <LEARN>
    G = golden_peers['peers_fail_eos_cut']
    assert any(g and g['local_eos'] for g in G) and any(g and g['peer_eos'] for g in G)
    conv = pp.conversation('peers_fail_eos_cut')
    assert any(st.op.startswith('dmany') and st.src == b'' for st in conv.steps)
    # (e): r1_1 connects to the cache r1_0 decodes on -- one cache size behind the turn
    conv, G = pp.conversation('peers_connecting'), golden_peers['peers_connecting']
    k, pipes = [(k, p) for k, p in turns(conv) if p[0][0] == 'r'][1]
    assert pipes == ['r0_0', 'r1_0', 'r1_1', 'r2_0'] and G[k + 1]['dcache'] == G[k + 2]['dcache'] != G[k]['dcache']
