"""The reference's XCodecPipePair itself (oracle/_ref/libppref.so: the reference's
xcodec/xcodec_pipe_pair.cc over its own encoder, decoder and cache) on the
scripted conversations of tests/pipe_cases.py: it reproduces the committed
golden transcripts (tests/golden/pipe.json, what the GPU tests compare with),
oracle/pipe.py's framing restatement equals its outgoing bytes, and two
reference pipe pairs deliver the payloads they were given."""
import json
import os

import pytest

import pipe_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def R():
    from oracle import refpipe
    if not refpipe.available('ref'):
        pytest.skip('oracle/_ref/libppref.so not built (needs the reference tree)')
    return pc.RefImpl('ref')


_transcripts = {}


def transcript(R, name):
    if name not in _transcripts:
        _transcripts[name] = pc.run(pc.conversation(name), R)
    return _transcripts[name]


@pytest.fixture(scope='module')
def golden_pipe():
    with open(os.path.join(ROOT, 'tests/golden/pipe.json')) as f:
        return json.load(f)['conversations']


def test_golden_lists_every_conversation(golden_pipe):
    assert sorted(golden_pipe) == sorted(pc.NAMES)


@pytest.mark.parametrize('name', pc.NAMES)
def test_reference_reproduces_golden(R, golden_pipe, name):
    assert pc.record(transcript(R, name)) == golden_pipe[name]


def test_oracle_framing_equals_reference(R, oracle):
    """oracle/pipe.py's encoder_stream (the restatement tests/test_gpu_pipe.py
    compares the engine's outgoing frames with) on conversation 1."""
    from oracle.pipe import encoder_stream
    T = transcript(R, 'framing')
    cache = oracle.cache_new()
    try:
        exp = encoder_stream(oracle, cache, pc.UUID_A, pc.framing_consumes())
    finally:
        oracle.cache_free(cache)
    assert b''.join(o.to_peer for o in T) == exp
    assert [o.pending for o in T] == [1, 2, 3, 4, 6, 9, 9]
    T = transcript(R, 'framing_eos_first')
    assert T[0].to_peer == pc.hello(pc.UUID_A) + pc.EOS      # <HELLO> and <EOS> in one output


@pytest.mark.parametrize('name', ['roundtrip', 'roundtrip_cut', 'ask_learn', 'ask_learn_cut', 'ask_learn_eos',
                                  'shared_encoder_cache'])
def test_reference_to_reference_delivers_payloads(R, name):
    conv = pc.conversation(name)
    T = transcript(R, conv.name)
    got = pc.locals_of(conv, T)
    for pipe, payload in conv.payloads.items():
        assert got[pipe] == payload
    assert not any(o.error for o in T if o is not None)


def test_ask_learn_shape(R):
    """What conversation 4 is built to reach, read off the reference's
    transcript: three merged frames with the first unknown REF in the second --
    everything before it is delivered, <ADVANCE> 1 and one sorted <ASK> go out,
    a later delivery decodes nothing while hashes are unknown, and the <LEARN>
    completes it with <ADVANCE> for the two frames left and the later one."""
    conv = pc.conversation('ask_learn')
    T = transcript(R, conv.name)
    blocked = T[5]
    kinds = pc.ops(blocked.to_peer)
    assert [k for k, _, _ in kinds] == [0x01, 0xF0]
    assert blocked.to_peer[:5] == pc.advance(1)
    assert pc.FRAME_IN < len(blocked.to_local) < 2 * pc.FRAME_IN
    a, b = kinds[1][1:]
    hs = [int.from_bytes(blocked.to_peer[k:k + 8], 'big') for k in range(a + 3, b, 8)]
    assert hs == sorted(set(hs)) and len(hs) > 100
    assert T[7].to_peer == b'' and T[7].to_local == b''
    assert T[8].to_peer[:1] == b'\xf1' and len(T[8].to_peer) == 3 + pc.SEG * len(hs)
    assert T[9].to_peer == pc.advance(3)
    assert T[10].pending == 0


def test_ask_batching_shape(R):
    for n, nask in ((513, 2), (1025, 3)):
        T = transcript(R, f'ask_batch_{n}')
        asks, learns = pc.ops(T[2].to_peer), pc.ops(T[3].to_peer)
        assert [k for k, _, _ in asks] == [0xF0] * nask and [k for k, _, _ in learns] == [0xF1] * nask
        assert [(b - a - 3) // 8 for _, a, b in asks] == [(b - a - 3) // pc.SEG for _, a, b in learns]
        assert T[2].to_local == b''


def test_eos_ack_waits_for_the_next_consume(R):
    """The quirk of decoder_decode_data: after a <LEARN> unblocks frames that
    ended in <EOS>, the local EOS is raised in that consume; the <EOS_ACK>
    goes out with the next one."""
    T = transcript(R, 'eos_blocked')
    assert T[5].local_eos and T[5].to_peer == pc.advance(1)
    assert T[9].to_peer == pc.EOS_ACK and T[9].peer_eos
    assert T[10].peer_eos


def test_name_reuse_in_learn_replaces(R):
    """Conversation 7: after the second <LEARN> replaced A by B under the same
    hash, REFs on either pipe, and on a fresh pipe of the same peer, read B."""
    A, B = pc.family(7)[:2]
    conv = pc.conversation('shared_peer_cache_reuse')
    T = transcript(R, conv.name)
    assert T[7].to_local[:pc.SEG] == A and T[8].to_local[:pc.SEG] == B
    assert all(b'\xf1\x02' in T[k].to_peer for k in (11, 14, 17))
    assert all(T[k].to_local[:pc.SEG] == B for k in (12, 15, 18))
    T = transcript(R, 'shared_peer_cache')
    assert all(T[k].to_local[:pc.SEG] == A for k in (7, 8, 12, 15, 18))


def test_bounded_conversation_evicts(R):
    T = transcript(R, 'bounded')
    sizes = [o.dcache for o in T if o is not None and o.dcache is not None]
    assert max(sizes) == 600                          # the LRU is full, so it evicts


def test_unknown_hash_capacity(R):
    for n in (65536, 65537):
        T = transcript(R, f'unknown_{n}')
        asks = pc.ops(T[0].to_peer)
        assert len(asks) == -(-n // 512) and all(k == 0xF0 for k, _, _ in asks)
        assert T[0].to_local == b'' and T[0].dcache == 0


@pytest.mark.parametrize('name', pc.ERROR_CASES)
def test_error_cases_fail_on_the_last_step_only(R, name):
    T = transcript(R, 'error_' + name)
    assert [o.error for o in T] == [False] * (len(T) - 1) + [True]
