"""xcg_pipe_decoder_consume_many on bounded and pair decoder contexts: the
decode() calls of consecutive pipes on one peer cache go up as one
xcg_decode_host_windows_bounded batch, which may refuse a batch as a whole and
is then presented half of it."""
import ctypes as C
import json
import os

import pytest

import pipe_cases as pc
import pipe_many_cases as pm
from decode_windows_cases import B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 2048
ONE_BLOCK_DISK = (18 + 205) * SEG


def batches():
    from wanproxy_amd.xcgpu import lib
    out = (C.c_uint64 * 2)()
    lib().xcg_pipe_debug_decode_many(out)
    return out[0], out[1]


def receiver_batches(conv):
    """(turns, pipes in them) of the conversation's receiver turns that are one
    batch each: two pipes or more, every one past its <HELLO> (a connecting
    pipe has no decoder context before it and is served alone)."""
    turns, chunks, seen, turn = 0, 0, set(), []
    for st in conv.steps:
        if st.op in ('dmany', 'dmany_end'):
            turn.append(st.pipe)
        if st.op == 'dmany_end':
            if all(p.startswith('r') for p in turn):
                if len(turn) >= 2 and all(p in seen for p in turn):
                    turns += 1
                    chunks += len(turn)
                seen |= set(turn)
            turn = []
    return turns, chunks


def test_many_bounded_is_batched_and_matches_the_reference():
    """The reference's transcript of many_bounded (tests/golden/pipe_many.json),
    and the receivers' turns behind the <HELLO>s were one batch each (the serial
    fallback passes the transcript alone)."""
    from wanproxy_amd.xcgpu import connect_registry_clear
    with open(os.path.join(ROOT, 'tests/golden/pipe_many.json')) as f:
        exp = json.load(f)['conversations']['many_bounded']
    connect_registry_clear()
    conv = pm.conversation('many_bounded')
    want = receiver_batches(conv)
    assert want == (2, 6)
    before = batches()
    got = pm.record(pm.run(conv, pc.EngineImpl()))
    after = batches()
    assert len(got) == len(exp)
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g == e, f'many_bounded: step {k} ({conv.steps[k][:2]}) differs from the reference'
    assert (after[0] - before[0], after[1] - before[1]) == want


# ------------------------------------------------- two set-ups, batch and serial

def bounded_ctx(limit):
    from wanproxy_amd.xcgpu import Context
    return lambda: Context(0, memory_cache_limit=limit)


def pair_ctx(limit, disk):
    from wanproxy_amd.xcgpu import Context
    return lambda: Context(0, memory_cache_limit=limit, disk_bytes=disk)


def one(pipe, data):
    from wanproxy_amd.xcgpu import XCGError
    try:
        return pipe.decoder_consume(data)
    except XCGError as e:
        return str(e)


def state(pipes, pair):
    """pending_frames of every pipe, and of every decoder context (by pipe)
    its size and, on a pair, its pair_stats."""
    from wanproxy_amd.xcgpu import lib
    res = []
    for p in pipes:
        d = p.decoder_ctx()
        st = (C.c_uint64 * 4)()
        if d is not None and pair:
            assert lib().xcg_pair_stats(C.c_void_p(d), st) == 0
        res.append((p.pending_frames(), None if d is None else int(lib().xcg_cache_size(C.c_void_p(d))), tuple(st)))
    return res


def talk(make_ctx, pair, n, rounds, many, before=None):
    """n sender pipes of codec S, n receiver pipes of codec V (all on one peer
    cache), `rounds` lists of messages.  The receivers take each round's wires
    in one turn -- many: one xcg_pipe_decoder_consume_many; else the serial
    loop -- and what they and the senders answer goes back and forth, pipe by
    pipe, until nobody has anything to say.  Returns the transcript: every
    output of every consume (or its error), the state behind every turn, the
    batches counted per receiver turn, and at the end a probe of every
    receiver's window: BACKREFs to every eighth slot, a FRAME each, up to the
    first empty one."""
    from wanproxy_amd.xcgpu import PipePair, connect_registry_clear
    connect_registry_clear()
    S, V = make_ctx(), make_ctx()
    send = [PipePair(S, S, pc.UUID_S, connect=True) for _ in range(n)]
    recv = [PipePair(V, V, pc.UUID_V, connect=True) for _ in range(n)]
    T, counted = [], []
    try:
        for r, msgs in enumerate(rounds):
            wires = PipePair.encoder_consume_many(send, msgs)
            for hop in range(6):
                if not any(wires):
                    break
                live = [k for k in range(n) if wires[k]]
                if many:
                    if before:
                        before(r, hop, [recv[k] for k in live], [wires[k] for k in live])
                    b0 = batches()
                    got = PipePair.decoder_consume_many([recv[k] for k in live], [wires[k] for k in live])
                    b1 = batches()
                    counted.append((b1[0] - b0[0], b1[1] - b0[1]))
                    got = [g if isinstance(g, tuple) else str(g) for g in got]
                else:
                    got = [one(recv[k], wires[k]) for k in live]
                T.append(('recv', r, hop, live, got, state(send + recv, pair)))
                replies = [b''] * n
                for k, g in zip(live, got):
                    replies[k] = g[0] if isinstance(g, tuple) else b''
                back = [one(send[k], replies[k]) if replies[k] else None for k in range(n)]
                T.append(('send', r, hop, back, state(send + recv, pair)))
                wires = [b[0] if isinstance(b, tuple) else b'' for b in back]
        for k, p in enumerate(recv):
            slots = []
            for c in range(0, 256, 8):
                slots.append(one(p, pc.frame(B(c))))
                if not isinstance(slots[-1], tuple):
                    break
            T.append(('probe', k, slots))
    finally:
        for p in send + recv:
            p.close()
        S.close()
        V.close()
        connect_registry_clear()
    return T, counted


def same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x == y, ('step', k, x[:4])


def conversation_rounds(name):
    """The messages of a pipe_many_cases conversation's sender turns, round by round."""
    rounds, turn = [], []
    for st in pm.conversation(name).steps:
        if st.op in ('many', 'many_end', 'enc') and st.pipe.startswith('s'):
            turn.append(st.src)
        if st.op == 'dmany_end' and turn:
            rounds.append(turn)
            turn = []
    return rounds


def test_pair_contexts_like_the_serial_loop():
    """The turns of the many_bounded conversation (its senders' messages, three
    rounds on three pipes) on pair contexts: a memory level of BOUNDED_LIMIT
    over a disk of one index block, connecting pipes.  One consume_many per
    turn against a second, identical set-up served by the serial
    xcg_pipe_decoder_consume loop -- every output and rc, pending_frames,
    pair_stats and a window probe per pipe.  The reference pipe harness has no
    pair codec, so the serial pair path is the yardstick here; it is itself
    pinned to the reference by tests/test_gpu_pair_decode.py.  The first turn
    carries the <HELLO>s (connecting pipes, served one by one); each later
    turn's three pipes are one batch."""
    mk = pair_ctx(pc.BOUNDED_LIMIT, ONE_BLOCK_DISK)
    rounds = conversation_rounds('many_bounded')
    assert [len(r) for r in rounds] == [3, 3, 3]
    serial, _ = talk(mk, True, 3, rounds, many=False)
    many, counted = talk(mk, True, 3, rounds, many=True)
    same(many, serial)
    print('batches per receiver turn:', counted)
    assert counted == [(0, 0), (1, 3), (1, 3)], counted
    assert any(t[0] == 'probe' and len(t[2]) > 1 for t in many)


def small_rounds(n):
    """A round for the <HELLO>s, then one whose 8 frames together enter about
    80 segments: more than a limit of 64, each half fewer."""
    return [[pc.mixed(7000 + i, 3_000) for i in range(n)], [pc.mixed(7100 + i, 10 * SEG + 100) for i in range(n)]]


def test_a_batch_refused_as_a_whole_is_split():
    mk = bounded_ctx(64 * SEG)
    rounds = small_rounds(8)
    serial, _ = talk(mk, False, 8, rounds, many=False)
    many, counted = talk(mk, False, 8, rounds, many=True)
    same(many, serial)
    assert counted[0] == (0, 0)                              # (connecting pipes)
    assert counted[1][0] > 1 and counted[1][1] >= 8, counted  # refused at 8 pipes, taken in parts


def test_a_pipe_listed_twice_changes_nothing_on_a_bounded_context():
    from wanproxy_amd.xcgpu import PipePair, XCGError
    refused = []

    def twice(r, hop, pipes, wires):
        if len(pipes) > 1:
            b0 = batches()
            with pytest.raises(XCGError, match=r'\(-22\)'):
                PipePair.decoder_consume_many(pipes + [pipes[0]], wires + [wires[0]])
            assert batches() == b0
            refused.append((r, hop))

    mk = bounded_ctx(pc.BOUNDED_LIMIT)
    rounds = [[pc.mixed(7200 + (r + i) % 3, 30_000 + 1_001 * i, pool=40, repeat=0.3) for i in range(3)] for r in range(2)]
    serial, _ = talk(mk, False, 3, rounds, many=False)
    many, counted = talk(mk, False, 3, rounds, many=True, before=twice)
    same(many, serial)
    assert len(refused) >= 2 and sum(c[0] for c in counted) >= 1
