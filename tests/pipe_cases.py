"""Scripted XCodecPipePair conversations and the interpreter that runs one on
any implementation of the protocol:

  R  RefImpl('ref')     the reference's xcodec_pipe_pair.cc over the reference
                        codec (oracle/_ref/libppref.so, oracle/refpipe.py)
  D  RefImpl('dropin')  the same pipe pair over the integration/ adapters
                        (oracle/_ref/libppdropin.so)
  E  EngineImpl()       xcg_pipe_* through wanproxy_amd.xcgpu.PipePair

A conversation names its codecs (UUID, memory cache limit) and the pipes on
them, then lists steps: "this pipe's encoder / decoder consumes these bytes",
the bytes being a payload from a seeded generator, a hand-built wire, or what
earlier steps produced for the peer.  A step may be delivered whole or cut
into pieces (`cut`).  `run()` returns the transcript: per step an `Out`
(to_peer, to_local, local_eos, peer_eos, error, pending, dcache) -- outputs
concatenated and flags or-ed over the pieces; `pending` is the acting pipe's
count of frames not yet <ADVANCE>d, `dcache` the size of the cache it connected
at <HELLO>.  A step whose call fails keeps the error flag only (what a failing
call leaves behind is not compared).  tests/golden/pipe.json holds R's
transcripts (tests/golden/make_pipe_golden.py).
"""
from __future__ import annotations

import functools
import hashlib
import random
from collections import namedtuple

from collision_cases import family  # noqa: F401  (segments of one XCodecHash; used below and by importers)

SEG = 2048
FRAME_IN = 512 * 1024                 # XCODEC_PIPE_MAX_FRAME / 2: input bytes per frame

UUID_A = b'0d1f4c8e-95a3-4b2d-8f6e-3c7a9b1d2e4f'
UUID_B = b'a7c3e9f1-2b4d-4e6f-8a0c-1e3f5a7c9e0b'
UUID_S = b'5e2d8b4a-1c3f-4a6e-9b0d-7f1e3c5a8b2d'
UUID_V = b'c41b7d02-6e9a-4f35-b8d1-20a4e6c8f135'

Out = namedtuple('Out', 'to_peer to_local local_eos peer_eos error pending dcache')
FAILED = Out(b'', b'', False, False, True, None, None)


# ---------------------------------------------------------------- payloads

def blocks(seed: int, n: int):
    r = random.Random(seed)
    return [r.randbytes(SEG) for _ in range(n)]


def mixed(seed: int, n: int, pool: int = 150, repeat: float = 0.55) -> bytes:
    """Repeated 2 KiB blocks (aligned, and shifted by the odd-sized runs between
    them), random bytes, runs of 0xF1 and 0xF1-heavy noise: frames of it carry
    EXTRACT, REF, BACKREF and escapes."""
    r = random.Random(seed)
    blk = blocks(seed ^ 0x5EED, pool)
    out = bytearray()
    while len(out) < n:
        x = r.random()
        if x < repeat:
            out += blk[r.randrange(pool)]
        elif x < repeat + 0.25:
            out += r.randbytes(r.randrange(1, 3000))
        elif x < repeat + 0.35:
            out += b'\xf1' * r.randrange(1, 700)
        else:
            out += bytes(0xF1 if b < 128 else b for b in r.randbytes(r.randrange(1, 400)))
    return bytes(out[:n])


# ---------------------------------------------------------------- wire helpers

def hello(uuid: bytes) -> bytes:
    return bytes([0xFF, len(uuid)]) + uuid


def frame(data: bytes) -> bytes:
    return b'\x02' + len(data).to_bytes(4, 'big') + data


def ask(hashes) -> bytes:
    return b'\xf0' + len(hashes).to_bytes(2, 'big') + b''.join(h.to_bytes(8, 'big') for h in hashes)


def learn(segs) -> bytes:
    return b'\xf1' + len(segs).to_bytes(2, 'big') + b''.join(segs)


def advance(n: int) -> bytes:
    return b'\x01' + n.to_bytes(4, 'big')


EOS, EOS_ACK = b'\xfc', b'\xfb'


def ops(wire: bytes):
    """The pipe ops of a well-formed wire buffer: [(opcode, start, end)]."""
    i, out = 0, []
    while i < len(wire):
        op = wire[i]
        if op == 0xFF:
            n = 2 + wire[i + 1]
        elif op == 0x02:
            n = 5 + int.from_bytes(wire[i + 1:i + 5], 'big')
        elif op == 0xF0:
            n = 3 + 8 * int.from_bytes(wire[i + 1:i + 3], 'big')
        elif op == 0xF1:
            n = 3 + SEG * int.from_bytes(wire[i + 1:i + 3], 'big')
        elif op == 0x01:
            n = 5
        else:
            n = 1
        out.append((op, i, i + n))
        i += n
    assert i == len(wire)
    return out


def cut_wire(wire: bytes):
    """Arbitrary segmentation: 1-byte pieces across every op header -- all of a
    <HELLO> and an <ADVANCE>, a <FRAME>'s length, an <ASK>'s count and first
    three hashes, a <LEARN>'s count and the start of its first segment -- and
    777-byte pieces elsewhere."""
    pieces = []
    for op, a, b in ops(wire):
        head = {0xFF: b - a, 0x02: 5, 0xF0: 3 + 24, 0xF1: 3 + 16, 0x01: 5}.get(op, 1)
        h = min(b, a + head)
        pieces += [wire[k:k + 1] for k in range(a, h)]
        pieces += [wire[k:min(k + 777, b)] for k in range(h, b, 777)]
    assert b''.join(pieces) == wire
    return pieces


# ---------------------------------------------------------------- conversations

Step = namedtuple('Step', 'pipe op src cut skip_empty')


class Conv:
    """codecs: {name: (uuid, memory_cache_limit_bytes)}; pipes: {name: codec}.
    enc / dec / many append steps and return their transcript indices."""

    def __init__(self, name, codecs, pipes, cut=None):
        self.name, self.codecs, self.pipes, self.cut = name, codecs, pipes, cut
        self.steps = []
        self.payloads = {}            # what the local sides should have received: {pipe: bytes}

    def _add(self, pipe, op, src, cut, skip_empty):
        self.steps.append(Step(pipe, op, src, cut, skip_empty))
        return len(self.steps) - 1

    def enc(self, pipe, src):
        return self._add(pipe, 'enc', src, None, False)

    def dec(self, pipe, src, skip_empty=False):
        """src: bytes, a transcript index (that step's to_peer), or a list of
        them, concatenated.  skip_empty: no call if that is empty (an empty
        decoder_consume means `connection closed`)."""
        return self._add(pipe, 'dec', src, self.cut, skip_empty)

    def many(self, pipes, srcs):
        """The pipes' encoder consumes as one batch where the implementation has
        one (xcg_pipe_encoder_consume_many); one transcript entry per pipe."""
        for p, s in zip(pipes, srcs):
            k = self._add(p, 'many', s, None, False)
        self.steps[k] = self.steps[k]._replace(op='many_end')
        return list(range(k - len(pipes) + 1, k + 1))


def _resolve(src, T):
    if isinstance(src, (bytes, bytearray)):
        return bytes(src)
    if isinstance(src, int):
        return T[src].to_peer if T[src] is not None else b''
    return b''.join(_resolve(s, T) for s in src)


def run(conv: Conv, impls):
    """Run `conv` on one implementation, or on {codec name: implementation}."""
    by_codec = impls if isinstance(impls, dict) else {c: impls for c in conv.codecs}
    codecs, pipes, T, batch = {}, {}, [], []
    try:
        for name, (uuid, limit) in conv.codecs.items():
            codecs[name] = by_codec[name].codec(uuid, limit)
        for name, cname in conv.pipes.items():
            pipes[name] = codecs[cname].pair()
        for st in conv.steps:
            data = _resolve(st.src, T)
            if st.op in ('many', 'many_end'):
                batch.append((st.pipe, data))
                if st.op == 'many_end':
                    impl = by_codec[conv.pipes[batch[0][0]]]
                    T += impl.consume_many([pipes[p] for p, _ in batch], [d for _, d in batch])
                    batch = []
                continue
            if st.skip_empty and not data:
                T.append(None)
                continue
            pieces = st.cut(data) if st.cut is not None and data else [data]
            agg = Out(b'', b'', False, False, False, None, None)
            for pc in pieces:
                o = pipes[st.pipe].consume(st.op, pc)
                if o.error:
                    agg = FAILED
                    break
                agg = Out(agg.to_peer + o.to_peer, agg.to_local + o.to_local, agg.local_eos or o.local_eos,
                          agg.peer_eos or o.peer_eos, False, o.pending, o.dcache)
            T.append(agg)
    finally:
        for p in pipes.values():
            p.close()
        for c in codecs.values():
            c.close()
        for impl in set(by_codec.values()):
            impl.reset()
    return T


def locals_of(conv: Conv, T):
    """What each pipe's local side received over the conversation."""
    got = {}
    for st, o in zip(conv.steps, T):
        if o is not None:
            got[st.pipe] = got.get(st.pipe, b'') + o.to_local
    return got


def _sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def record(T):
    """The golden form of a transcript: lengths and SHA-256, flags, counts."""
    return [None if o is None else
            {'to_peer': [len(o.to_peer), _sha(o.to_peer)], 'to_local': [len(o.to_local), _sha(o.to_local)],
             'local_eos': o.local_eos, 'peer_eos': o.peer_eos, 'error': o.error, 'pending': o.pending,
             'dcache': o.dcache} for o in T]


# -- 1. framing sizes

FRAMING_SIZES = [1, 2047, 2048, FRAME_IN, FRAME_IN + 1, 2 * FRAME_IN + 1]


def framing_consumes():
    return [mixed(100 + k, n) for k, n in enumerate(FRAMING_SIZES)] + [b'']


def conv_framing():
    c = Conv('framing', {'A': (UUID_A, 0)}, {'a': 'A'})
    for m in framing_consumes():
        c.enc('a', m)
    return c


def conv_framing_eos_first():
    c = Conv('framing_eos_first', {'A': (UUID_A, 0)}, {'a': 'A'})
    c.enc('a', b'')
    return c


# -- 2. round trip with <ADVANCE>  (3: the same, segmented)

def conv_roundtrip(cut=None):
    c = Conv('roundtrip' + ('_cut' if cut else ''), {'A': (UUID_A, 0), 'B': (UUID_B, 0)}, {'a': 'A', 'b': 'B'}, cut)
    m1 = mixed(21, 300_000)
    msgs = [m1, m1[100_000:150_001] + mixed(22, 20_000), mixed(21, 900_000) + mixed(23, 300_000)]
    for m in msgs:
        w = c.enc('a', m)
        r = c.dec('b', w)
        c.dec('a', r)
    w = c.enc('a', b'')
    r = c.dec('b', w)
    c.dec('a', r)
    c.payloads = {'b': b''.join(msgs)}
    return c


# -- 4. <ASK>/<LEARN> with merged frames  (3: the same, segmented)

def _ask_learn_steps(c):
    """Sender codec S (pipes s0, s1), receiver codec V (pipe r1).  r1 learns P
    in-stream; Q is declared on s0, whose wire is dropped; then P + Q goes out on
    s1 as three frames: the first all REFs r1 knows, the second a few such and
    then REFs it does not."""
    P = mixed(41, FRAME_IN)
    Q = P[4096:4096 + 8192] + mixed(42, 1_100_000 - FRAME_IN - 8192, pool=40, repeat=0.3)
    N = mixed(43, 5000)
    w = c.enc('s1', P)
    r = c.dec('r1', w)
    c.dec('s1', r)
    c.enc('s0', Q)                                # (dropped)
    w = c.enc('s1', P + Q)                        # three frames
    r_ask = c.dec('r1', w)                        # P + the start of Q; <ADVANCE> 1; sorted <ASK>
    w = c.enc('s1', N)
    r_none = c.dec('r1', w)                       # buffered: nothing while hashes are unknown
    r_learn = c.dec('s1', [r_ask, r_none])        # <LEARN>
    r = c.dec('r1', r_learn)                      # the rest of Q, N; <ADVANCE> 3
    r = c.dec('s1', r)
    for _ in range(2):                            # (segmented: the frames arrive, and block, one by one)
        r = c.dec('r1', r, skip_empty=True)
        r = c.dec('s1', r, skip_empty=True)
    c.payloads = {'r1': P + P + Q + N}
    return P, Q, N


def conv_ask_learn(cut=None):
    c = Conv('ask_learn' + ('_cut' if cut else ''), {'S': (UUID_S, 0), 'V': (UUID_V, 0)},
             {'s0': 'S', 's1': 'S', 'r1': 'V'}, cut)
    _ask_learn_steps(c)
    return c


# -- 5. <ASK> batching

def conv_ask_batch(n):
    c = Conv(f'ask_batch_{n}', {'S': (UUID_S, 0), 'V': (UUID_V, 0)}, {'s0': 'S', 's1': 'S', 'r1': 'V'})
    M = b''.join(blocks(500 + n, n))
    c.enc('s0', M)                                # (dropped)
    w = c.enc('s1', M)
    r = c.dec('r1', w)                            # ceil(n / 512) <ASK>s in one output
    r = c.dec('s1', r)                            # one <LEARN> per <ASK>, in order
    r = c.dec('r1', r)                            # M; <ADVANCE>
    c.dec('s1', r)
    c.payloads = {'r1': M}
    return c


# -- 6. <EOS> ordering

def _close_both(c, first, second, r):
    """`r`: what `second` sent last (carrying its <EOS_ACK> or not); `second`
    now closes its own side, and the acks go back and forth to peer_eos."""
    c.dec(first, r, skip_empty=True)
    w = c.enc(second, b'')
    r = c.dec(first, w)
    r = c.dec(second, r, skip_empty=True)
    c.dec(first, r, skip_empty=True)


def conv_eos_blocked():
    """<EOS> in the same delivery as frames that block on an <ASK>: the local
    EOS is raised in the consume the <LEARN> completes, the <EOS_ACK> only in
    the next one (decoder_decode_data sends it when it finds no frame data)."""
    c = Conv('eos_blocked', {'S': (UUID_S, 0), 'V': (UUID_V, 0)}, {'s0': 'S', 's1': 'S', 'r1': 'V'})
    M = mixed(61, 200_000)
    c.enc('s0', M)
    w1 = c.enc('s1', M)
    w2 = c.enc('s1', b'')
    r = c.dec('r1', [w1, w2])
    r = c.dec('s1', r)
    r = c.dec('r1', r)
    _close_both(c, 's1', 'r1', r)
    c.payloads = {'r1': M}
    return c


def conv_eos_clean():
    """<EOS> with nothing outstanding, then the other side closes too."""
    c = Conv('eos_clean', {'A': (UUID_A, 0), 'B': (UUID_B, 0)}, {'a': 'A', 'b': 'B'})
    M = mixed(62, 100_000)
    w = c.enc('a', M)
    r = c.dec('b', w)
    c.dec('a', r)
    w = c.enc('a', b'')
    r = c.dec('b', w)
    _close_both(c, 'a', 'b', r)
    c.payloads = {'b': M}
    return c


def conv_eos_closed_before():
    """The connection closes (an empty decoder_consume) before <EOS> arrives."""
    c = Conv('eos_closed_before', {'A': (UUID_A, 0), 'B': (UUID_B, 0)}, {'a': 'A', 'b': 'B'})
    M = mixed(63, 50_000)
    w = c.enc('a', M)
    c.dec('b', w)
    c.dec('b', b'')
    w = c.enc('a', b'')
    c.dec('b', w)
    c.dec('b', b'')
    return c


def conv_eos_closed_after():
    """Frames and <EOS> in one delivery, then the connection closes."""
    c = Conv('eos_closed_after', {'A': (UUID_A, 0), 'B': (UUID_B, 0)}, {'a': 'A', 'b': 'B'})
    M = mixed(64, 50_000)
    w1 = c.enc('a', M)
    w2 = c.enc('a', b'')
    r = c.dec('b', [w1, w2])
    c.dec('b', b'')
    c.dec('a', r)
    return c


# -- 7. two connections, one peer cache

def conv_shared_peer_cache(reuse: bool):
    """r1 and r2 connect under the sender's UUID: one cache.  Both block on the
    hash of A.  r1 learns A; r2's <LEARN> is redundant (the same bytes) or, with
    `reuse`, carries B of the same hash: a replace.  s1, s2 and a fresh s3 then
    send A again, a REF each time, which reads the shared cache."""
    c = Conv('shared_peer_cache' + ('_reuse' if reuse else ''), {'S': (UUID_S, 0), 'V': (UUID_V, 0)},
             {'s0': 'S', 's1': 'S', 's2': 'S', 's3': 'S', 'r1': 'V', 'r2': 'V', 'r3': 'V'})
    A, B = family(7)[:2]
    X = A + random.Random(70).randbytes(100)
    c.enc('s0', X)                                # (dropped)
    w1 = c.enc('s1', X)
    w2 = c.enc('s2', X)
    a1 = c.dec('r1', w1)
    a2 = c.dec('r2', w2)
    l1 = c.dec('s1', a1)
    l2 = c.dec('s2', a2)
    d1 = c.dec('r1', l1)
    d2 = c.dec('r2', learn([B]) if reuse else l2)
    c.dec('s1', d1)
    c.dec('s2', d2)
    for s, r in (('s1', 'r1'), ('s2', 'r2'), ('s3', 'r3')):
        w = c.enc(s, X)
        d = c.dec(r, w)
        c.dec(s, d)
    return c


# -- 8. shared encoder cache

def conv_shared_encoder_cache(many: bool):
    c = Conv('shared_encoder_cache' + ('_many' if many else ''), {'S': (UUID_S, 0), 'V': (UUID_V, 0)},
             {'s1': 'S', 's2': 'S', 'r1': 'V', 'r2': 'V'})
    m1 = mixed(81, 300_000)
    rounds = [(m1, m1[1000:200_000] + mixed(82, 100_000)), (mixed(83, 600_000), m1)]
    for ma, mb in rounds:
        if many:
            w1, w2 = c.many(['s1', 's2'], [ma, mb])
        else:
            w1, w2 = c.enc('s1', ma), c.enc('s2', mb)
        d1 = c.dec('r1', w1)
        d2 = c.dec('r2', w2)
        c.dec('s1', d1)
        c.dec('s2', d2)
    c.payloads = {'r1': rounds[0][0] + rounds[1][0], 'r2': rounds[0][1] + rounds[1][1]}
    return c


# -- 9. bounded caches

BOUNDED_LIMIT = 600 * SEG


def conv_bounded():
    """XCodecMemoryCache(uuid, 600 segments) on both ends, one frame per
    delivery; later messages repeat earlier ones, some of whose segments the
    LRU has evicted by then."""
    c = Conv('bounded', {'A': (UUID_A, BOUNDED_LIMIT), 'B': (UUID_B, BOUNDED_LIMIT)}, {'a': 'A', 'b': 'B'})
    msgs = [mixed(90 + i % 5, 300_000 + 7_001 * i, pool=300, repeat=0.3) for i in range(12)]
    for m in msgs:
        w = c.enc('a', m)
        r = c.dec('b', w)
        r = c.dec('a', r)
        r = c.dec('b', r, skip_empty=True)
        c.dec('a', r, skip_empty=True)
    c.payloads = {'b': b''.join(msgs)}
    return c


# -- 10. errors: one short wire per ERROR branch of decoder_decode

def _error_cases():
    seg = bytes(7 for _ in range(SEG))
    HB = hello(UUID_B)
    # (name, what our encoder consumed first, wires delivered before, the failing wire)
    return [
        ('frame_before_hello', [], [], frame(b'x')),
        ('hello_twice', [], [], HB + HB),
        ('hello_bad_length', [], [], b'\xff\x05hello'),
        ('ask_before_our_hello', [], [], ask([0])),
        ('advance_before_our_hello', [], [], advance(1)),
        ('ask_count_0', [b'x'], [], b'\xf0\x00\x00'),
        ('ask_count_513', [b'x'], [], b'\xf0\x02\x01'),
        ('learn_count_0', [], [], HB + b'\xf1\x00\x00'),
        ('learn_count_513', [], [], HB + b'\xf1\x02\x01'),
        ('ask_hash_in_no_frame', [mixed(10, 9000)], [], ask([0x1234])),
        ('ask_after_all_advanced', [mixed(10, 9000)], [advance(1)], ask([0x1234])),
        ('learn_before_hello', [], [], learn([seg])),
        ('learn_gratuitous', [], [], HB + learn([seg])),
        ('frame_length_0', [], [], HB + b'\x02\x00\x00\x00\x00'),
        ('frame_length_1mib_1', [], [], HB + b'\x02\x00\x10\x00\x01'),
        ('advance_0', [mixed(10, 9000)], [], advance(0)),
        ('advance_above_pending', [mixed(10, 9000)], [], advance(2)),
        ('eos_twice', [], [], EOS + EOS),
        ('eos_ack_before_our_eos', [], [], EOS_ACK),
        ('eos_ack_twice', [b''], [], EOS_ACK + EOS_ACK),
        ('unknown_op', [], [], b'\x55'),
        ('frame_bad_opcode', [], [], HB + frame(b'abc\xf1\x00' + b'\xf1\x01' + seg + b'\xf1\x07zz')),
    ]


ERROR_CASES = [e[0] for e in _error_cases()]


def conv_error(name):
    _, encs, before, wire = next(e for e in _error_cases() if e[0] == name)
    c = Conv('error_' + name, {'A': (UUID_A, 0)}, {'a': 'A'})
    for m in encs:
        c.enc('a', m)
    for w in before:
        c.dec('a', w)
    c.dec('a', wire)
    return c


# -- 11. unknown-hash capacity

def conv_unknown(n):
    """One hand-built frame of n distinct REFs no cache holds: ceil(n / 512)
    sorted <ASK> ops."""
    c = Conv(f'unknown_{n}', {'V': (UUID_V, 0)}, {'r': 'V'})
    r = random.Random(1100 + n)
    hs = set()
    while len(hs) < n:
        hs.add(r.getrandbits(64))
    hs = list(hs)
    r.shuffle(hs)
    c.dec('r', hello(UUID_S) + frame(b''.join(b'\xf1\x02' + h.to_bytes(8, 'big') for h in hs)))
    return c


# -- 4 and 6 joined: both directions carry a payload, both sides close

def conv_ask_learn_eos():
    c = Conv('ask_learn_eos', {'S': (UUID_S, 0), 'V': (UUID_V, 0)}, {'s0': 'S', 's1': 'S', 'r1': 'V'})
    P, Q, N = _ask_learn_steps(c)
    back = mixed(44, 150_000)
    w = c.enc('r1', back)
    r = c.dec('s1', w)
    c.dec('r1', r)
    tail = mixed(41, 60_000)                      # (the start of P again: REFs r1 knows)
    w1 = c.enc('s1', tail)
    w2 = c.enc('s1', b'')
    r = c.dec('r1', [w1, w2])
    _close_both(c, 's1', 'r1', r)
    c.payloads = {'r1': P + P + Q + N + tail, 's1': back}
    return c


BUILDERS = {
    'framing': conv_framing,
    'framing_eos_first': conv_framing_eos_first,
    'roundtrip': conv_roundtrip,
    'roundtrip_cut': functools.partial(conv_roundtrip, cut_wire),
    'ask_learn': conv_ask_learn,
    'ask_learn_cut': functools.partial(conv_ask_learn, cut_wire),
    'ask_batch_513': functools.partial(conv_ask_batch, 513),
    'ask_batch_1025': functools.partial(conv_ask_batch, 1025),
    'eos_blocked': conv_eos_blocked,
    'eos_clean': conv_eos_clean,
    'eos_closed_before': conv_eos_closed_before,
    'eos_closed_after': conv_eos_closed_after,
    'shared_peer_cache': functools.partial(conv_shared_peer_cache, False),
    'shared_peer_cache_reuse': functools.partial(conv_shared_peer_cache, True),
    'shared_encoder_cache': functools.partial(conv_shared_encoder_cache, False),
    'shared_encoder_cache_many': functools.partial(conv_shared_encoder_cache, True),
    'bounded': conv_bounded,
    'unknown_65536': functools.partial(conv_unknown, 65536),
    'unknown_65537': functools.partial(conv_unknown, 65537),
    'ask_learn_eos': conv_ask_learn_eos,
}
BUILDERS.update({'error_' + n: functools.partial(conv_error, n) for n in ERROR_CASES})
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def conversation(name: str) -> Conv:
    c = BUILDERS[name]()
    assert c.name == name
    return c


# ---------------------------------------------------------------- implementations

class _RefPair:
    def __init__(self, pair):
        self.p = pair

    def consume(self, op, data):
        o = self.p.consume(0 if op == 'enc' else 1, data)
        if o.encoder_error or o.decoder_error:
            return FAILED
        return Out(o.to_peer, o.to_local, o.decoder_eos, o.encoder_eos, False, self.p.pending_frames(),
                   self.p.decoder_cache_size())

    def close(self):
        self.p.close()


class _RefCodec:
    def __init__(self, codec):
        self.c = codec

    def pair(self):
        return _RefPair(self.c.pair())

    def close(self):
        self.c.close()


class RefImpl:
    """R ('ref') or D ('dropin'): the reference's XCodecPipePair class."""

    def __init__(self, which='ref'):
        from oracle.refpipe import RefPipes
        self.lib = RefPipes(which)

    def codec(self, uuid, limit=0):
        return _RefCodec(self.lib.codec(uuid, limit))

    def consume_many(self, pairs, datas):
        return [p.consume('enc', d) for p, d in zip(pairs, datas)]

    def reset(self):
        self.lib.registry_clear()


class _EnginePair:
    def __init__(self, ctx, uuid):
        from wanproxy_amd.xcgpu import PipePair
        # the codec's cache encodes, and is what <HELLO> connects the decoder's from
        self.p = PipePair(ctx, ctx, uuid, connect=True)

    def _state(self):
        from wanproxy_amd.xcgpu import lib
        d = self.p.decoder_ctx()
        return self.p.pending_frames(), (None if d is None else int(lib().xcg_cache_size(d)))

    def consume(self, op, data):
        from wanproxy_amd.xcgpu import XCGError
        try:
            if op == 'enc':
                o = (self.p.encoder_consume(data), b'', False, False)
            else:
                o = self.p.decoder_consume(data)
        except XCGError as e:
            if '(-71)' not in str(e):             # only XCG_EPROTO is decoder_error()
                raise
            return FAILED
        return Out(*o, False, *self._state())

    def close(self):
        self.p.close()


class _EngineCodec:
    def __init__(self, uuid, limit):
        from wanproxy_amd.xcgpu import Context
        self.uuid = uuid
        self.ctx = Context(0, memory_cache_limit=limit) if limit else Context(0, cache_segments=1 << 15)

    def pair(self):
        return _EnginePair(self.ctx, self.uuid)

    def close(self):
        self.ctx.close()


class EngineImpl:
    """E: xcg_pipe_* (wanproxy_amd/csrc/xcg_pipe.cpp) on the GPU engine."""

    def codec(self, uuid, limit=0):
        return _EngineCodec(uuid, limit)

    def consume_many(self, pairs, datas):
        from wanproxy_amd.xcgpu import PipePair
        wires = PipePair.encoder_consume_many([p.p for p in pairs], datas)
        return [Out(w, b'', False, False, False, *p._state()) for w, p in zip(wires, pairs)]

    def reset(self):
        from wanproxy_amd.xcgpu import connect_registry_clear
        connect_registry_clear()
