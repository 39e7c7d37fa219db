"""xcg_pipe_decoder_consume_many: the decoder consumes of several pipes in one
call -- the decode() calls of consecutive pipes on one peer cache in one GPU
batch -- against the reference XCodecPipePair serving the same pipes one by one
(tests/golden/pipe_many.json, made by tests/golden/make_pipe_many_golden.py;
the conversations: tests/pipe_many_cases.py)."""
import json
import os

import pytest

import pipe_cases as pc
import pipe_many_cases as pm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def golden_many():
    with open(os.path.join(ROOT, 'tests/golden/pipe_many.json')) as f:
        return json.load(f)['conversations']


@pytest.fixture(scope='module')
def E():
    from wanproxy_amd.xcgpu import connect_registry_clear
    connect_registry_clear()
    return pc.EngineImpl()


def same(conv, T, exp):
    got = pm.record(T)
    assert len(got) == len(exp)
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g == e, f'{conv.name}: step {k} ({conv.steps[k][:2]}) differs from the reference'


@pytest.mark.parametrize('name', pm.NAMES)
def test_engine_reproduces_reference(E, golden_many, name):
    conv = pm.conversation(name)
    same(conv, pm.run(conv, E), golden_many[name])


def test_a_pipe_listed_twice_changes_nothing(E, golden_many):
    """In front of every turn the same call with its first pipe listed again at
    the end: XCG_EINVAL, and the conversation still runs to the reference's
    transcript -- no pipe, window or cache moved."""
    from wanproxy_amd.xcgpu import PipePair, XCGError
    refused = []

    def twice(pairs, datas):
        if len(pairs) > 1:
            with pytest.raises(XCGError, match=r'\(-22\)'):
                PipePair.decoder_consume_many([p.p for p in pairs] + [pairs[0].p], datas + [datas[0]])
            refused.append(len(pairs))

    conv = pm.conversation('many_shared_peer')
    same(conv, pm.run(conv, E, before_dmany=twice), golden_many['many_shared_peer'])
    assert len(refused) == 6


def batches():
    import ctypes as C
    from wanproxy_amd.xcgpu import lib
    out = (C.c_uint64 * 2)()
    lib().xcg_pipe_debug_decode_many(out)
    return out[0], out[1]


def test_the_turns_are_batches(E):
    """The receivers' turns behind the <HELLO>s are one GPU batch each: 8 chunks
    in each of two calls (a serial fallback would pass every transcript)."""
    before = batches()
    pm.run(pm.conversation('many_shared_peer'), E)
    after = batches()
    assert (after[0] - before[0], after[1] - before[1]) == (2, 16)
    # a stop: pipes 0-3 (pipe 3 blocks), then pipe 4 alone by the single call; the <LEARN> turn: pipes 0-2
    before = after
    pm.run(pm.conversation('many_middle_blocks'), E)
    after = batches()
    assert after[0] - before[0] >= 2 and after[1] - before[1] >= 5 + 3


def test_null_arguments():
    from wanproxy_amd.xcgpu import lib
    assert lib().xcg_pipe_decoder_consume_many(None, None, None, 0, None, None) == 0
    assert lib().xcg_pipe_decoder_consume_many(None, None, None, 2, None, None) == -22
