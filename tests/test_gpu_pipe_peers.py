"""xcg_pipe_decoder_consume_many on a hub's turns -- many peers, a pipe or a few
each: the decode() calls of pipes that stand alone on their peer's cache go up
in one launch (xcg_decode_call_many) -- against the reference XCodecPipePair
serving the same pipes one by one (tests/golden/pipe_peers.json, made by
tests/golden/make_pipe_peers_golden.py; the conversations:
tests/pipe_peers_cases.py).  A serial fallback would pass every transcript:
the counters are what tells the two apart."""
import json
import os

import pytest

import pipe_cases as pc
import pipe_many_cases as pm
import pipe_peers_cases as pp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def golden_peers():
    with open(os.path.join(ROOT, 'tests/golden/pipe_peers.json')) as f:
        return json.load(f)['conversations']


@pytest.fixture(scope='module')
def E():
    from wanproxy_amd.xcgpu import connect_registry_clear
    connect_registry_clear()
    return pp.SmallEngineImpl()


def batches():
    import ctypes as C
    from wanproxy_amd.xcgpu import lib
    out = (C.c_uint64 * 2)()
    lib().xcg_pipe_debug_decode_many(out)
    return out[0], out[1]


@pytest.mark.parametrize('name', pp.NAMES)
def test_engine_reproduces_reference(E, golden_peers, name):
    """Step by step the reference's transcript, and the launches the
    conversation states: (launches, pipes in them)."""
    from wanproxy_amd.xcgpu import pipe_debug_decode_peers
    conv = pp.conversation(name)
    before = pipe_debug_decode_peers()
    got = pp.record(pp.run(conv, E))
    after = pipe_debug_decode_peers()
    exp = golden_peers[name]
    assert len(got) == len(exp)
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g == e, f'{name}: step {k} ({conv.steps[k][:2]}) differs from the reference'
    assert (after[0] - before[0], after[1] - before[1]) == conv.launches, name


def test_one_peer_turns_launch_nothing_new():
    """Conversations whose pipes share one peer cache: the windows batches are
    what they were, and no launch over peers is made."""
    from wanproxy_amd.xcgpu import connect_registry_clear, pipe_debug_decode_peers
    connect_registry_clear()
    impl = pc.EngineImpl()
    peers0 = pipe_debug_decode_peers()
    before = batches()
    pm.run(pm.conversation('many_shared_peer'), impl)
    after = batches()
    assert (after[0] - before[0], after[1] - before[1]) == (2, 16)
    before = after
    pm.run(pm.conversation('many_middle_blocks'), impl)
    after = batches()
    assert after[0] - before[0] >= 2 and after[1] - before[1] >= 5 + 3
    assert pipe_debug_decode_peers() == peers0


def test_two_peers_alternating_is_a_launch():
    """tests/pipe_many_cases.py's many_two_peers: in receive order r0 q0 r1 q1
    nothing was batched; now r0 and q0 go up together, and r1 forces that."""
    import json as _json
    from wanproxy_amd.xcgpu import connect_registry_clear, pipe_debug_decode_peers
    connect_registry_clear()
    with open(os.path.join(ROOT, 'tests/golden/pipe_many.json')) as f:
        exp = _json.load(f)['conversations']['many_two_peers']
    before = pipe_debug_decode_peers()
    got = pm.record(pm.run(pm.conversation('many_two_peers'), pc.EngineImpl()))
    after = pipe_debug_decode_peers()
    assert got == exp
    # turn 3 (r0 q0 r1 q1): {r0, q0} flushed before r1, then {r1, q1} at the end
    assert (after[0] - before[0], after[1] - before[1]) == (2, 4)
