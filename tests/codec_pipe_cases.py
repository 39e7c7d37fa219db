"""Scripted conversations of the configured codec -- XCodecPipePair chained with
the zlib pipes, as WANProxyCodecPipePair links them
(programs/wanproxy/wanproxy_codec_pipe_pair.cc:76-196) -- and the interpreter
that runs one on either implementation (test infrastructure, on
tests/pipe_cases.py's Conv, payloads and transcript form):

  R  RefChain()     the reference's own classes, chained here call by call:
                    pipe_cases.RefImpl('ref') pairs (xcodec_pipe_pair.cc) and
                    oracle.zlib_pipe.ReferencePipes('ref') pipes (deflate_pipe.cc,
                    inflate_pipe.cc)
  E  EngineChain()  xcg_codec_* through wanproxy_amd.xcgpu.Codec / CodecPipe

The chain's rules (include/xcgpu.h, xcg_codec_*):
  link     everything one upstream consume() produces is one downstream
           consume() of one Buffer; a produce_eos is that buffer first, if not
           empty, then one empty consume.
  send     W = the pair's encoder_consume; to_peer = DeflatePipe::consume(W).
  receive  InflatePipe::consume(data) -> W, status.  -1: the pipe has failed,
           now and on every later call, and nothing reaches the pair.  data
           not empty: a W that is not empty is the pair's decoder_consume.
           data empty (the peer closed): status 1 hands the pair its bytes, if
           any, then an empty consume; status 0 hands it nothing.
  replies  every to_peer of the pair goes through the pipe's one deflate
           stream; a pair call that reports peer_eos is followed by one empty
           DeflatePipe::consume (Z_FINISH), its bytes appended.
  level None: no compressor, every output is the pair's.

A step is a TURN: `send` or `recv` over several pipes.  R serves the pipes one
after the other; E makes ONE xcg_codec_send_many / xcg_codec_receive_many call.
A recv entry whose source is the literal b'' is an empty receive (the peer
closed); one whose source resolves to nothing leaves the turn (None in the
transcript).  `pending` and `dcache` are read once the turn is over.
tests/golden/codec_pipe.json holds R's transcripts
(tests/golden/make_codec_pipe_golden.py).
"""
from __future__ import annotations

import functools
import random

import pipe_cases as pc
from pipe_cases import FAILED, FRAME_IN, UUID_A, UUID_B, UUID_S, UUID_V, Conv, Out, mixed, record  # noqa: F401

__all__ = ['NAMES', 'conversation', 'run', 'record', 'RefChain', 'EngineChain']


class Cut:
    """Bytes [a, b) of a step's to_peer (b None: to its end; negative: from the
    end; a float: that fraction of the length)."""

    def __init__(self, index, a, b):
        self.index, self.a, self.b = index, a, b


class Flip:
    """A step's to_peer with the byte at `pos` inverted."""

    def __init__(self, index, pos):
        self.index, self.pos = index, pos


class CodecConv(Conv):
    """pipe_cases.Conv with a compressor level (None: no compressor) and turns."""

    def __init__(self, name, codecs, pipes, level):
        super().__init__(name, codecs, pipes)
        self.level = level

    def _turn(self, op, pipes, srcs):
        if isinstance(pipes, str):
            pipes, srcs = [pipes], [srcs]
        for p, s in zip(pipes, srcs):
            k = self._add(p, op, s, None, False)
        self.steps[k] = self.steps[k]._replace(op=op + '_end')
        return list(range(k - len(pipes) + 1, k + 1))

    def send(self, pipes, srcs):
        return self._turn('send', pipes, srcs)

    def recv(self, pipes, srcs):
        return self._turn('recv', pipes, srcs)


def _resolve(src, T):
    if isinstance(src, Cut):
        w = pc._resolve(src.index, T)
        at = [len(w) if x is None else int(len(w) * x) if isinstance(x, float) else x % (len(w) + 1)
              for x in (src.a, src.b)]
        return w[at[0]:at[1]]
    if isinstance(src, Flip):
        w = bytearray(pc._resolve(src.index, T))
        w[src.pos] ^= 0xFF
        return bytes(w)
    if isinstance(src, list):
        return b''.join(_resolve(s, T) for s in src)
    return pc._resolve(src, T)


def run(conv: CodecConv, impl, before_turn=None):
    """The transcript of `conv` on `impl`.  before_turn(op, pipes, datas): called
    in front of every turn with the implementation's pipe objects."""
    codecs, pipes, T, batch = {}, {}, [], []
    try:
        for name, (uuid, limit) in conv.codecs.items():
            codecs[name] = impl.codec(uuid, limit, conv.level)
        for name, cname in conv.pipes.items():
            pipes[name] = codecs[cname].pipe()
        for st in conv.steps:
            data = _resolve(st.src, T)
            closed = isinstance(st.src, (bytes, bytearray)) and not st.src
            batch.append((st.pipe, data, closed))
            if not st.op.endswith('_end'):
                continue
            op = st.op[:-4]
            # (a send of b'' is the local side closing; a receive of nothing is no call at all)
            turn = [(p, d) for p, d, c in batch if d or c or op == 'send']
            outs = []
            if turn:
                ps, ds = [pipes[p] for p, _ in turn], [d for _, d in turn]
                if before_turn:
                    before_turn(op, ps, ds)
                outs = impl.send_many(ps, ds) if op == 'send' else impl.receive_many(ps, ds)
                outs = [o if o.error else o._replace(pending=p.state()[0], dcache=p.state()[1])
                        for o, p in zip(outs, ps)]
            it = iter(outs)
            T += [next(it) if (d or c or op == 'send') else None for _, d, c in batch]
            batch = []
    finally:
        for p in pipes.values():
            p.close()
        for c in codecs.values():
            c.close()
        impl.reset()
    return T


# ---------------------------------------------------------------- conversations

LEVELS = (1, 6)                        # everywhere
BIG_LEVELS = (0, 1, 6, 9)              # the big-consume case


def _exchange(c, senders, receivers, payloads, rounds=2):
    """One send turn, the receive turn, and the replies back and forth."""
    w = c.send(senders, payloads)
    for _ in range(rounds):
        r = c.recv(receivers, w)
        w = c.recv(senders, r)
    return w


def conv_sizes(level):
    """1, 2047, 2048 and 70 000 bytes over 3 pipes, each sent twice: first-sent,
    then REF-dense; the receivers' <ADVANCE>s return through their deflate into
    the senders' inflate."""
    c = CodecConv(f'sizes_l{level}', {'S': (UUID_S, 0), 'V': (UUID_V, 0)},
                  {'s0': 'S', 's1': 'S', 's2': 'S', 'r0': 'V', 'r1': 'V', 'r2': 'V'}, level)
    S, Rv = ['s0', 's1', 's2'], ['r0', 'r1', 'r2']
    got = {r: b'' for r in Rv}
    for i, n in enumerate((1, 2047, 2048, 70_000)):
        pay = [mixed(700 + 10 * i + j, n, pool=12) for j in range(3)]
        for _ in range(2):
            _exchange(c, S, Rv, pay, rounds=1)
            for r, p in zip(Rv, pay):
                got[r] += p
    c.payloads = got
    return c


def conv_ask_learn(level):
    """Q is declared on s0, whose wire is dropped; s1 sends Q as REFs r1 does not
    know: <ASK> and <LEARN> through both zlib directions."""
    c = CodecConv(f'ask_learn_l{level}', {'S': (UUID_S, 0), 'V': (UUID_V, 0)}, {'s0': 'S', 's1': 'S', 'r1': 'V'},
                  level)
    Q = mixed(42, 60_000, pool=20)
    c.send('s0', Q)                                # (dropped)
    w = c.send('s1', Q)
    a = c.recv('r1', w)                            # <ASK>
    l = c.recv('s1', a)                            # <LEARN>
    d = c.recv('r1', l)                            # Q; <ADVANCE>
    c.recv('s1', d)
    c.payloads = {'r1': Q}
    return c


def conv_flush_carry(level):
    """One consume of 2 x 512 KiB + 1 random bytes: three frames whose compressed
    output passes DeflatePipe's 64 KiB flush buffer; the 1-byte consumes behind
    it deliver the rest first."""
    c = CodecConv(f'flush_carry_l{level}', {'A': (UUID_A, 0), 'B': (UUID_B, 0)}, {'a': 'A', 'b': 'B'}, level)
    big = random.Random(91).randbytes(2 * FRAME_IN + 1)
    w1 = c.send('a', big)
    w2 = c.send('a', b'x')
    w3 = c.send('a', b'y')
    for w in (w1, w2, w3):
        r = c.recv('b', w)
        c.recv('a', r)
    c.payloads = {'b': big + b'xy'}
    return c


def conv_flush_stop(level):
    """A consume whose wire is a little over 4 x 16383 incompressible bytes: the
    Z_SYNC_FLUSH call stops at the full 64 KiB buffer (exactly 65536 bytes are
    produced, deflate_pipe.cc:101-105) and the next consume delivers the rest
    first.  (The size comes from a search on the reference chain: every random
    consume of 65456 .. 65696 bytes stops at levels 1 and 6; at levels 6 and 9
    the 1 MiB consume above does not.)"""
    c = CodecConv(f'flush_stop_l{level}', {'A': (UUID_A, 0), 'B': (UUID_B, 0)}, {'a': 'A', 'b': 'B'}, level)
    M = random.Random(92).randbytes(65_500)
    ws = [c.send('a', m) for m in (M, b'x', b'y')]
    for w in ws:
        r = c.recv('b', w)
        c.recv('a', r)
    c.payloads = {'b': M + b'xy'}
    return c


def conv_mixed_send(level):
    """send_many over 8 pipes: pipe 0 new (<HELLO>), pipe 3 closing (len 0), pipe 5
    with three frames -- literal and device pieces next to each other."""
    S, Rv = [f's{j}' for j in range(8)], [f'r{j}' for j in range(8)]
    pipes = {p: 'S' for p in S}
    pipes.update({p: 'V' for p in Rv})
    c = CodecConv(f'mixed_send_l{level}', {'S': (UUID_S, 0), 'V': (UUID_V, 0)}, pipes, level)
    first = [mixed(800 + j, 3000 + 17 * j, pool=8) for j in range(8)]
    _exchange(c, S[1:], Rv[1:], first[1:], rounds=1)
    second = [mixed(820 + j, 5000 + j, pool=8) for j in range(8)]
    second[3] = b''
    second[5] = mixed(830, 2 * FRAME_IN + 1, pool=200)
    _exchange(c, S, Rv, second, rounds=2)
    return c


def conv_eos(level, first):
    """Both sides close, `first` first: <EOS>, <EOS_ACK>, peer_eos and the
    Z_FINISH trailers, then both connections close."""
    second = 'b' if first == 'a' else 'a'
    c = CodecConv(f'eos_{first}_first_l{level}', {'A': (UUID_A, 0), 'B': (UUID_B, 0)}, {'a': 'A', 'b': 'B'}, level)
    M = mixed(62, 30_000, pool=10)
    w = c.send('a', M)
    r = c.recv('b', w)
    c.recv('a', r)
    w = c.send(first, b'')
    r = c.recv(second, w)
    r = c.recv(first, r)
    c.recv(second, r)
    w = c.send(second, b'')
    for _ in range(3):
        w = c.recv(first, w)
        w = c.recv(second, w)
    c.recv(first, b'')
    c.recv(second, b'')
    c.payloads = {'b': M}
    return c


def conv_close_unfinished(level):
    """The peer closes without finishing its zlib stream: nothing reaches the pair."""
    c = CodecConv(f'close_unfinished_l{level}', {'A': (UUID_A, 0), 'B': (UUID_B, 0)}, {'a': 'A', 'b': 'B'}, level)
    w = c.send('a', mixed(63, 20_000, pool=10))
    c.recv('b', w)
    c.recv('b', b'')
    return c


def conv_cut(level):
    """The compressed stream reaches the receiver cut after 1 byte and in the
    middle of a block."""
    c = CodecConv(f'cut_l{level}', {'A': (UUID_A, 0), 'B': (UUID_B, 0)}, {'a': 'A', 'b': 'B'}, level)
    M = mixed(64, 70_000, pool=12)
    w, = c.send('a', M)
    for a, b in ((0, 1), (1, 0.5), (0.5, None)):
        r = c.recv('b', Cut(w, a, b))
        c.recv('a', r)
    c.payloads = {'b': M}
    return c


def conv_bad_stream(level):
    """One flipped byte in r1's stream (its zlib header): r1 has failed from
    then on, in both directions; r0 and r2 go on."""
    c = CodecConv(f'bad_stream_l{level}', {'S': (UUID_S, 0), 'V': (UUID_V, 0)},
                  {'s0': 'S', 's1': 'S', 's2': 'S', 'r0': 'V', 'r1': 'V', 'r2': 'V'}, level)
    S, Rv = ['s0', 's1', 's2'], ['r0', 'r1', 'r2']
    w = c.send(S, [mixed(900 + j, 9000, pool=6) for j in range(3)])
    r = c.recv(Rv, [w[0], Flip(w[1], 1), w[2]])
    c.recv(S, r)
    w = c.send(S, [mixed(910 + j, 9000, pool=6) for j in range(3)])
    r = c.recv(Rv, w)
    c.recv(S, r)
    w = c.send(Rv, [mixed(920 + j, 4000, pool=6) for j in range(3)])
    c.recv(S, w)
    return c


def conv_no_compressor():
    """A codec without compressor: the plain pair's transcript."""
    c = CodecConv('no_compressor', {'A': (UUID_A, 0), 'B': (UUID_B, 0)}, {'a': 'A', 'b': 'B'}, None)
    M = mixed(65, 70_000, pool=12)
    for m in (M, M[1000:50_000], b''):
        w = c.send('a', m)
        r = c.recv('b', w)
        c.recv('a', r)
    c.recv('b', b'')
    c.payloads = {'b': M + M[1000:50_000]}
    return c


BUILDERS = {}
for _l in LEVELS:
    BUILDERS.update({
        f'sizes_l{_l}': functools.partial(conv_sizes, _l),
        f'ask_learn_l{_l}': functools.partial(conv_ask_learn, _l),
        f'flush_stop_l{_l}': functools.partial(conv_flush_stop, _l),
        f'mixed_send_l{_l}': functools.partial(conv_mixed_send, _l),
        f'eos_a_first_l{_l}': functools.partial(conv_eos, _l, 'a'),
        f'eos_b_first_l{_l}': functools.partial(conv_eos, _l, 'b'),
        f'close_unfinished_l{_l}': functools.partial(conv_close_unfinished, _l),
        f'cut_l{_l}': functools.partial(conv_cut, _l),
        f'bad_stream_l{_l}': functools.partial(conv_bad_stream, _l),
    })
BUILDERS.update({f'flush_carry_l{_l}': functools.partial(conv_flush_carry, _l) for _l in BIG_LEVELS})
BUILDERS['no_compressor'] = conv_no_compressor
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def conversation(name: str) -> CodecConv:
    c = BUILDERS[name]()
    assert c.name == name
    return c


def plain_transcript(conv: CodecConv, impl):
    """`conv` (one pipe a turn) on plain pipe pairs of a pipe_cases implementation."""
    p = Conv(conv.name, conv.codecs, conv.pipes)
    for st in conv.steps:
        assert st.op.endswith('_end')
        p._add(st.pipe, 'enc' if st.op == 'send_end' else 'dec', st.src, None, st.op == 'recv_end' and st.src != b'')
    return pc.run(p, impl)


# ---------------------------------------------------------------- implementations

class _RefPipe:
    """One WANProxyCodecPipePair side out of the reference's classes."""

    def __init__(self, pair, zpipes, level):
        self.pair, self.failed = pair, False
        self.zd = zpipes.pipe('deflate', level) if level is not None else None
        self.zi = zpipes.pipe('inflate') if level is not None else None

    def state(self):
        return self.pair.pending_frames(), self.pair.decoder_cache_size()

    def _deflate(self, wire: bytes) -> bytes:
        if self.zd is None or not wire:
            return wire
        return self.zd.consume(wire)[0]

    def _pair(self, which, calls):
        agg = Out(b'', b'', False, False, False, None, None)
        for data in calls:
            o = self.pair.consume(which, data)
            if o.encoder_error or o.decoder_error:
                return FAILED
            peer = self._deflate(o.to_peer)
            if o.encoder_eos and self.zd is not None:     # encoder_produce_eos: Z_FINISH
                peer += self.zd.consume(b'')[0]
            agg = Out(agg.to_peer + peer, agg.to_local + o.to_local, agg.local_eos or o.decoder_eos,
                      agg.peer_eos or o.encoder_eos, False, None, None)
        return agg

    def send(self, data: bytes) -> Out:
        if self.failed:
            return FAILED
        return self._pair(0, [data])

    def receive(self, data: bytes) -> Out:
        if self.failed:
            return FAILED
        if self.zi is None:
            return self._pair(1, [data])
        wire, status = self.zi.consume(data)
        if status == -1:                                  # produce_error
            self.failed = True
            return FAILED
        if data:
            calls = [wire] if wire else []
        else:
            calls = ([wire] if wire else []) + [b''] if status == 1 else []
        return self._pair(1, calls)

    def close(self):
        self.pair.close()
        for z in (self.zd, self.zi):
            if z is not None:
                z.close()


class _RefCodec:
    def __init__(self, codec, zpipes, level):
        self.c, self.zpipes, self.level = codec, zpipes, level

    def pipe(self):
        return _RefPipe(self.c.pair(), self.zpipes, self.level)

    def close(self):
        self.c.close()


class RefChain:
    def __init__(self):
        from oracle.refpipe import RefPipes
        from oracle.zlib_pipe import ReferencePipes
        self.lib, self.z = RefPipes('ref'), ReferencePipes('ref')

    def codec(self, uuid, limit, level):
        return _RefCodec(self.lib.codec(uuid, limit), self.z, level)

    def send_many(self, pipes, datas):
        return [p.send(d) for p, d in zip(pipes, datas)]

    def receive_many(self, pipes, datas):
        return [p.receive(d) for p, d in zip(pipes, datas)]

    def reset(self):
        self.lib.registry_clear()


class _EnginePipe:
    def __init__(self, codec):
        self.p = codec.c.pipe(codec.uuid)

    def state(self):
        from wanproxy_amd.xcgpu import lib
        d = self.p.decoder_ctx()
        return self.p.pending_frames(), (None if d is None else int(lib().xcg_cache_size(d)))

    def close(self):
        self.p.close()


class _EngineCodec:
    def __init__(self, uuid, limit, level, max_pipes):
        from wanproxy_amd.xcgpu import Codec, Context
        self.uuid = uuid
        self.ctx = Context(0, memory_cache_limit=limit) if limit else Context(0, cache_segments=1 << 15)
        # the codec's cache encodes, and is what <HELLO> connects the decoder's from
        self.c = Codec(self.ctx, self.ctx, -1 if level is None else level, max_pipes, connect=True)

    def pipe(self):
        return _EnginePipe(self)

    def close(self):
        self.c.close()
        self.ctx.close()


class EngineChain:
    """E: xcg_codec_* (wanproxy_amd/csrc/xcg_codec.cpp) on the GPU engine."""

    def __init__(self, max_pipes=8):
        self.max_pipes = max_pipes

    def codec(self, uuid, limit, level):
        return _EngineCodec(uuid, limit, level, self.max_pipes)

    @staticmethod
    def _outs(res):
        from wanproxy_amd.xcgpu import XCGError
        outs = []
        for r in res:
            if isinstance(r, XCGError):
                if '(-71)' not in str(r):                 # only XCG_EPROTO is a failed pipe
                    raise r
                outs.append(FAILED)
            else:
                outs.append(Out(*r, False, None, None))
        return outs

    def send_many(self, pipes, datas):
        from wanproxy_amd.xcgpu import CodecPipe
        return self._outs(CodecPipe.send_many([p.p for p in pipes], datas))

    def receive_many(self, pipes, datas):
        from wanproxy_amd.xcgpu import CodecPipe
        return self._outs(CodecPipe.receive_many([p.p for p in pipes], datas))

    def reset(self):
        from wanproxy_amd.xcgpu import connect_registry_clear
        connect_registry_clear()
