"""Scripted pipe-pair conversations whose receiving side serves several pipes
per event-loop turn (test infrastructure, in the style of tests/pipe_cases.py,
whose Conv, payloads and wire helpers these use).

A `dmany` step is the decoder consumes of several pipes in one turn.  The
reference pipe pair (pipe_cases.RefImpl) runs it as the serial loop -- one
XCodecPipePair::decoder_consume per pipe, in order; the engine runs it as ONE
xcg_pipe_decoder_consume_many.  Every pipe's entry of the transcript must be
the same.  (`pending` and `dcache` of a dmany entry are read once the whole
turn is over: a batch has no state in between.)
"""
import pipe_cases as pc
from pipe_cases import (BOUNDED_LIMIT, FAILED, UUID_A, UUID_S, UUID_V, Conv, Out, family, frame, learn, mixed,
                        record)

__all__ = ['NAMES', 'conversation', 'run', 'record']


class ManyConv(Conv):
    def dmany(self, pipes, srcs):
        """The pipes' decoder consumes as one turn; one transcript entry per pipe."""
        for p, s in zip(pipes, srcs):
            k = self._add(p, 'dmany', s, None, False)
        self.steps[k] = self.steps[k]._replace(op='dmany_end')
        return list(range(k - len(pipes) + 1, k + 1))


def _state(pair):
    """(pending, dcache) of an implementation's pair, as its consume reports them."""
    if hasattr(pair, '_state'):
        return pair._state()
    return pair.p.pending_frames(), pair.p.decoder_cache_size()


def dmany(impl, pairs, datas):
    if isinstance(impl, pc.EngineImpl):
        from wanproxy_amd.xcgpu import PipePair, XCGError
        res = PipePair.decoder_consume_many([p.p for p in pairs], datas)
        outs = []
        for r in res:
            if isinstance(r, XCGError):
                if '(-71)' not in str(r):             # only XCG_EPROTO is decoder_error()
                    raise r
                outs.append(FAILED)
            else:
                outs.append(Out(*r, False, None, None))
    else:
        outs = [p.consume('dec', d) for p, d in zip(pairs, datas)]
    return [o if o.error else o._replace(pending=_state(p)[0], dcache=_state(p)[1]) for o, p in zip(outs, pairs)]


class _Cut:
    """A transcript index whose wire is delivered in two pieces (half: 0 or 1;
    cut: the offset of the cut, negative from the end, None = the middle)."""

    def __init__(self, index, cut, half):
        self.index, self.cut, self.half = index, cut, half


def _resolve(src, T):
    if isinstance(src, _Cut):
        wire = pc._resolve(src.index, T)
        at = len(wire) // 2 if src.cut is None else src.cut % len(wire)
        return wire[at:] if src.half else wire[:at]
    if isinstance(src, list):
        return b''.join(_resolve(s, T) for s in src)
    return pc._resolve(src, T)


def run(conv, impl, before_dmany=None):
    """pipe_cases.run with dmany steps (one implementation for every codec).
    A dmany entry whose source is the literal b'' is a len-0 consume (the peer
    closed); one whose source resolves to nothing -- the peer had nothing to
    say -- leaves the turn (None in the transcript).  before_dmany(pairs,
    datas): called in front of every dmany turn."""
    codecs, pipes, T, batch = {}, {}, [], []
    try:
        for name, (uuid, limit) in conv.codecs.items():
            codecs[name] = impl.codec(uuid, limit)
        for name, cname in conv.pipes.items():
            pipes[name] = codecs[cname].pair()
        for st in conv.steps:
            data = _resolve(st.src, T)
            if st.op in ('many', 'many_end', 'dmany', 'dmany_end'):
                if st.op.startswith('d') and not data and st.src != b'':
                    batch.append(None)
                else:
                    batch.append((st.pipe, data))
                if st.op.endswith('_end'):
                    live = [b for b in batch if b is not None]
                    pairs, datas = [pipes[p] for p, _ in live], [d for _, d in live]
                    if st.op == 'many_end':
                        got = impl.consume_many(pairs, datas)
                    else:
                        if before_dmany:
                            before_dmany(pairs, datas)
                        got = dmany(impl, pairs, datas) if pairs else []
                    got = iter(got)
                    T += [None if b is None else next(got) for b in batch]
                    batch = []
                continue
            if st.skip_empty and not data:
                T.append(None)
                continue
            o = pipes[st.pipe].consume(st.op, data)
            T.append(FAILED if o.error else o)
    finally:
        for p in pipes.values():
            p.close()
        for c in codecs.values():
            c.close()
        impl.reset()
    return T


def _names(prefix, n):
    return [f'{prefix}{i}' for i in range(n)]


def _conv(name, n, limit=0):
    """Sender codec S with pipes s0.., receiver codec V with pipes r0..: every
    r connects under S's UUID, so all of them decode on one peer cache."""
    pipes = {**{s: 'S' for s in _names('s', n)}, **{r: 'V' for r in _names('r', n)}, 'sx': 'S'}
    return ManyConv(name, {'S': (UUID_S, limit), 'V': (UUID_V, limit)}, pipes)


def _turn(c, n, msgs, many=True):
    """Every sender encodes its message, the receivers take the wires in one
    turn, the senders the replies in one turn.  Returns the reply indices."""
    S, R = _names('s', n), _names('r', n)
    w = c.many(S, msgs) if many else [c.enc(s, m) for s, m in zip(S, msgs)]
    d = c.dmany(R, w)
    return c.dmany(S, d)


def conv_shared_peer():
    """8 connections on one peer cache, three rounds of ~40 KB per pipe with
    repeats across the connections: a pipe's frame REFs what another pipe's
    frame of the same turn EXTRACTed.  (The first turn carries the <HELLO>s:
    connecting pipes, served one by one.)"""
    n = 8
    c = _conv('many_shared_peer', n)
    base = [mixed(300 + r, 400_000, pool=120) for r in range(3)]
    for r in range(3):
        msgs = [base[r][30_000 * i:30_000 * i + 40_000 + 13 * i] if i % 3 else
                base[(r + 1) % 3][7_000 * i:7_000 * i + 39_000] + base[r][:2048 * 3] for i in range(n)]
        _turn(c, n, msgs, many=r != 1)
    return c


def conv_middle_blocks():
    """The sender's cache knows segments the receiver's does not (declared on
    sx, whose wire is dropped).  Pipe 3 of 5 blocks on them and sends its
    <ASK>; the <LEARN> arrives in a later turn beside the other pipes' FRAMEs
    and ends that turn's run in front of it."""
    n = 5
    c = _conv('many_middle_blocks', n)
    _turn(c, n, [mixed(400 + i, 9_000) for i in range(n)])
    Q = mixed(410, 60_000, pool=30, repeat=0.6)
    c.enc('sx', Q)                                       # (dropped)
    msgs = [mixed(420 + i, 30_000) for i in range(n)]
    msgs[3] = mixed(423, 5_000) + Q[2048:40_000] + mixed(424, 3_000)
    msgs[4] = msgs[3][1000:20_000] + mixed(425, 8_000)   # (REFs what pipe 3's prefix EXTRACTed, and blocks behind it)
    d = _turn(c, n, msgs)                                # d[3]: pipe 3's <LEARN>
    S, R = _names('s', n), _names('r', n)
    w = c.many(S, [mixed(430 + i, 12_000) + Q[:5000] for i in range(n)])
    back = c.dmany(R, [[d[i], w[i]] for i in range(n)])  # <LEARN> + FRAME on the pipes that asked
    back = c.dmany(S, back)
    for _ in range(2):
        back = c.dmany(R, back)
        back = c.dmany(S, back)
    return c


def conv_eos():
    """len-0 entries (the peer closed) and <EOS> / <EOS_ACK> inside turns."""
    n = 4
    c = _conv('many_eos', n)
    _turn(c, n, [mixed(500 + i, 6_000) for i in range(n)])
    S, R = _names('s', n), _names('r', n)
    w0 = c.enc('s0', mixed(510, 20_000))
    w1 = c.enc('s1', b'')                                # <EOS>
    w3 = c.enc('s3', mixed(500, 6_000) + mixed(511, 3_000))
    d = c.dmany(R, [w0, w1, b'', w3])                    # r2: closed
    a = c.dmany(S, d)
    e1 = c.enc('r1', b'')                                # r1 closes its side: <HELLO> <EOS>
    e2 = c.enc('r2', b'')
    k = c.dmany(['s1', 's2', 's0'], [e1, e2, b''])
    w3 = c.enc('s3', mixed(512, 9_000))
    d = c.dmany(['r3', 'r1', 'r2', 'r0'], [w3, k[0], k[1], a[0]])
    c.dmany(['s3', 's1', 's2'], [d[0], d[1], d[2]])
    return c


def conv_cut():
    """The wires cut so that FRAMEs straddle two turns: inside the length, at
    the first payload byte, in the middle, one byte short."""
    n = 4
    c = _conv('many_cut', n)
    _turn(c, n, [mixed(600 + i, 5_000) for i in range(n)])
    S, R = _names('s', n), _names('r', n)
    cuts = [3, 6, None, -1]
    for r in range(2):
        w = c.many(S, [mixed(610 + 2 * r + i % 2, 25_000 + 100 * i) for i in range(n)])
        first = c.dmany(R, [_Cut(k, cut, 0) for k, cut in zip(w, cuts)])
        second = c.dmany(R, [_Cut(k, cut, 1) for k, cut in zip(w, cuts)])
        c.dmany(S, [[a, b] for a, b in zip(first, second)])
    return c


def conv_two_peers():
    """Two peers: r0, r1 decode on S's cache, q0, q1 on A's -- two decoder
    contexts in one turn, in blocks and alternating."""
    pipes = {'s0': 'S', 's1': 'S', 'a0': 'A', 'a1': 'A', 'r0': 'V', 'r1': 'V', 'q0': 'V', 'q1': 'V'}
    c = ManyConv('many_two_peers', {'S': (UUID_S, 0), 'A': (UUID_A, 0), 'V': (UUID_V, 0)}, pipes)
    send, recv = ['s0', 's1', 'a0', 'a1'], ['r0', 'r1', 'q0', 'q1']
    for r, order in enumerate(([0, 1, 2, 3], [0, 1, 2, 3], [0, 2, 1, 3], [2, 3, 0, 1])):
        m = mixed(700 + r, 60_000, pool=40)
        w = [c.enc(send[i], m[5_000 * i:5_000 * i + 30_000]) for i in range(4)]
        d = c.dmany([recv[i] for i in order], [w[i] for i in order])
        c.dmany([send[i] for i in order], d)
    return c


def conv_bounded():
    """Bounded caches on both ends: every pipe takes the serial call."""
    n = 3
    c = _conv('many_bounded', n, BOUNDED_LIMIT)
    for r in range(3):
        _turn(c, n, [mixed(800 + (r + i) % 4, 150_000 + 3_001 * i, pool=300, repeat=0.3) for i in range(n)])
    return c


def conv_bad_opcode():
    """A bad opcode inside one pipe's frame: that pipe fails, the others get
    their bytes."""
    n = 4
    c = _conv('many_bad_opcode', n)
    _turn(c, n, [mixed(900 + i, 5_000) for i in range(n)])
    S, R = _names('s', n), _names('r', n)
    w = c.many(S, [mixed(910 + i, 20_000) for i in range(n)])
    A = family(9)[0]
    bad = frame(b'good bytes' + b'\xf1\x01' + A + b'\xf1\x07 and the rest')
    d = c.dmany(R, [w[0], w[1], bad, w[3]])
    c.dmany([S[0], S[1], S[3]], [d[0], d[1], d[3]])
    w = c.many([S[0], S[1], S[3]], [A + mixed(920, 4_000)] * 3)     # (the failed decode's EXTRACT stays entered)
    c.dmany([R[0], R[1], R[3]], w)
    return c


BUILDERS = {f.__name__[5:]: f for f in (conv_shared_peer, conv_middle_blocks, conv_eos, conv_cut, conv_two_peers,
                                        conv_bounded, conv_bad_opcode)}
NAMES = ['many_' + k for k in BUILDERS]


def conversation(name):
    c = BUILDERS[name[5:]]()
    assert c.name == name
    return c
