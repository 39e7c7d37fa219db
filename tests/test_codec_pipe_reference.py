"""The reference's own classes -- XCodecPipePair (oracle/_ref/libppref.so) and
DeflatePipe / InflatePipe (oracle/_ref/libzpref.so) -- chained by the rules of
tests/codec_pipe_cases.py on its scripted conversations: the chain reproduces
the committed transcripts (tests/golden/codec_pipe.json, what
tests/test_gpu_codec_pipe.py holds xcg_codec_* to), delivers the payloads, and
reaches the rules the conversations were built for."""
import json
import os

import pytest

import codec_pipe_cases as cc
import pipe_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def R():
    from oracle import refpipe
    if not refpipe.available('ref') or not os.path.exists(os.path.join(ROOT, 'oracle/_ref/libzpref.so')):
        pytest.skip('oracle/_ref/libppref.so, libzpref.so not built (need the reference tree)')
    return cc.RefChain()


_transcripts = {}


def transcript(R, name):
    if name not in _transcripts:
        _transcripts[name] = cc.run(cc.conversation(name), R)
    return _transcripts[name]


@pytest.fixture(scope='module')
def golden_codec():
    with open(os.path.join(ROOT, 'tests/golden/codec_pipe.json')) as f:
        return json.load(f)['conversations']


def test_golden_lists_every_conversation(golden_codec):
    assert sorted(golden_codec) == sorted(cc.NAMES)


@pytest.mark.parametrize('name', cc.NAMES)
def test_reference_chain_reproduces_golden(R, golden_codec, name):
    assert cc.record(transcript(R, name)) == golden_codec[name]


@pytest.mark.parametrize('name', [n for n in cc.NAMES if cc.conversation(n).payloads])
def test_chain_delivers_payloads(R, name):
    conv = cc.conversation(name)
    T = transcript(R, name)
    got = pc.locals_of(conv, T)
    for pipe, payload in conv.payloads.items():
        assert got[pipe] == payload
    assert not any(o.error for o in T if o is not None)


@pytest.mark.parametrize('level', cc.LEVELS)
def test_second_send_is_ref_dense(R, level):
    """Each size goes out twice: the second wire of 2048 and of 70 000 bytes is
    REFs, a fraction of the first."""
    T = transcript(R, f'sizes_l{level}')
    sends = [o for st, o in zip(cc.conversation(f'sizes_l{level}').steps, T) if st.op.startswith('send')]
    for first, second in ((12, 15), (18, 21)):               # (turns of 3 pipes: 2048 bytes, 70 000 bytes)
        assert len(sends[second].to_peer) * 10 < len(sends[first].to_peer)


@pytest.mark.parametrize('level', cc.LEVELS)
def test_flush_stop_carries(R, level):
    """The first consume produces exactly DeflatePipe's 64 KiB buffer; the 1-byte
    consume behind it delivers the rest first."""
    T = transcript(R, f'flush_stop_l{level}')
    assert len(T[0].to_peer) == 65536
    assert len(T[1].to_peer) > 100 > len(T[2].to_peer)
    assert T[3].to_local == b'' and T[3].to_peer == b''      # (the frame is not complete yet)


def test_big_consume_carries_at_level_1(R):
    T = transcript(R, 'flush_carry_l1')
    assert len(T[0].to_peer) == 16 * 65536 and len(T[1].to_peer) > 1000
    assert T[0].pending == 3                                  # three frames


@pytest.mark.parametrize('level', cc.LEVELS)
def test_eos_trailers(R, level):
    """Both sides reach local_eos and peer_eos; the call that reports peer_eos
    ends with the zlib trailer (the stream's Z_FINISH), so the closing empty
    receives find finished streams."""
    for first in 'ab':
        conv = cc.conversation(f'eos_{first}_first_l{level}')
        T = transcript(R, conv.name)
        for pipe in 'ab':
            mine = [o for st, o in zip(conv.steps, T) if o is not None and st.pipe == pipe]
            assert any(o.local_eos for o in mine) and any(o.peer_eos for o in mine)
            closing = next(o for o in mine if o.peer_eos)
            assert len(closing.to_peer) >= 6                  # empty stored block + adler32 at least


@pytest.mark.parametrize('level', cc.LEVELS)
def test_unfinished_stream_close_reaches_nothing(R, level):
    T = transcript(R, f'close_unfinished_l{level}')
    assert T[2] == T[2]._replace(to_peer=b'', to_local=b'', local_eos=False, peer_eos=False, error=False)


@pytest.mark.parametrize('level', cc.LEVELS)
def test_bad_stream_fails_one_pipe_for_good(R, level):
    conv = cc.conversation(f'bad_stream_l{level}')
    T = transcript(R, conv.name)
    for st, o in zip(conv.steps, T):
        if o is not None and st.op.startswith('recv') and st.pipe == 'r1':
            assert o.error
        elif o is not None and st.pipe in ('r0', 'r2', 's0', 's2'):
            assert not o.error
    assert [o.error for st, o in zip(conv.steps, T) if st.op.startswith('send') and st.pipe == 'r1'] == [True]
    got = pc.locals_of(conv, T)
    assert len(got['r0']) == len(got['r2']) == 18_000 and got['r1'] == b''


def test_no_compressor_equals_the_plain_pair(R):
    conv = cc.conversation('no_compressor')
    plain = cc.plain_transcript(conv, pc.RefImpl('ref'))
    assert cc.record(transcript(R, 'no_compressor')) == pc.record(plain)
