"""Scripted pipe-pair conversations of a hub: a receiving codec V whose pipes
come from MANY peers, a pipe or a few each (test infrastructure, on the
machinery of tests/pipe_many_cases.py).  Every peer is a sender codec with a
UUID of its own, so XCodecCache::connect gives each of V's receiving pipes the
cache of its peer: a `dmany` turn of V is decode() calls on several decoder
contexts.  The reference runs such a turn as the serial loop; the engine as ONE
xcg_pipe_decoder_consume_many, which puts the calls of pipes that stand alone
on their context into one launch (xcg_decode_call_many).

Each conversation carries what the test needs beside the transcript:
  conv.peer_of   {receiving pipe: its peer's codec}
  conv.launches  (launches, pipes in them) xcg_pipe_debug_decode_peers moves by,
                 worked out from the rule of xcg_pipe_decoder_consume_many: a
                 plain pipe that is a run of one is held if its ops leave frame
                 bytes to decode; the held set goes up before a later pipe of a
                 held context, before a pipe with no context yet and at the end
                 of the turn; a held set of one is the single call (no launch).
  conv.counted   which of V's turns (0: the <HELLO>s) hold those launches
"""
import pipe_cases as pc
from pipe_cases import UUID_V, family, frame, mixed
from pipe_many_cases import ManyConv, _Cut, record, run  # noqa: F401  (run, record: for the importers)

SEGMENTS = 1 << 12                       # an engine codec's cache: many codecs stay small


def peer_uuid(i: int) -> bytes:
    return b'%08x-7b1e-4c2a-9d3f-5a6b7c8d9e0f' % (0xA0000000 + i)


class _SmallCodec(pc._EngineCodec):
    def __init__(self, uuid, limit):
        from wanproxy_amd.xcgpu import Context
        assert not limit
        self.uuid = uuid
        self.ctx = Context(0, cache_segments=SEGMENTS)


class SmallEngineImpl(pc.EngineImpl):
    """EngineImpl whose codecs hold small caches."""

    def codec(self, uuid, limit=0):
        return _SmallCodec(uuid, limit)


def _hub(name, pipes_per_peer):
    """Peer i is codec P<i> with sending pipes p<i>_<j>; V receives each on r<i>_<j>."""
    codecs = {'V': (UUID_V, 0)}
    pipes, peer_of = {}, {}
    for i, m in enumerate(pipes_per_peer):
        codecs[f'P{i}'] = (peer_uuid(i), 0)
        for j in range(m):
            pipes[f'p{i}_{j}'] = f'P{i}'
            pipes[f'r{i}_{j}'] = 'V'
            peer_of[f'r{i}_{j}'] = f'P{i}'
    c = ManyConv(name, codecs, pipes)
    c.peer_of = peer_of
    return c


def _recv(p):
    return 'r' + p[1:]


def _turn(c, senders, msgs, order=None):
    """The senders encode, V takes the wires in one turn (in `order`), the
    senders the replies in one turn.  Returns (wire indices, V's indices in sender order)."""
    w = [c.enc(s, m) for s, m in zip(senders, msgs)]
    order = list(range(len(senders))) if order is None else order
    d = c.dmany([_recv(senders[i]) for i in order], [w[i] for i in order])
    c.dmany([senders[i] for i in order], d)
    back = [None] * len(senders)
    for k, i in enumerate(order):
        back[i] = d[k]
    return w, back


def conv_hub():
    """(a) 8 peers, a pipe each, three turns of ~40 KB per pipe, each turn
    repeating half of the one before.  The <HELLO> turn is served serially
    (connecting pipes); every later turn is one launch of 8."""
    n = 8
    c = _hub('peers_hub', [1] * n)
    S = [f'p{i}_0' for i in range(n)]
    base = [mixed(1000 + i, 120_000, pool=60) for i in range(n)]
    for r in range(3):
        _turn(c, S, [base[i][20_000 * r:20_000 * r + 40_000 + 13 * i] for i in range(n)])
    c.launches, c.counted = (2, 16), [1, 2]
    return c


def conv_mixed():
    """(b) 3 peers with 1, 2 and 3 pipes.  In blocks: peer 0's pipe is held, the
    others are windows batches.  Interleaved (r1_0 r0_0 r2_0 r1_1 r2_1 r2_2):
    three pipes are held, r1_1 -- whose frame REFs what r1_0's EXTRACTed --
    forces the flush, r2_1 r2_2 are a windows batch behind it."""
    c = _hub('peers_mixed', [1, 2, 3])
    S = ['p0_0', 'p1_0', 'p1_1', 'p2_0', 'p2_1', 'p2_2']
    shared = [mixed(1100 + i, 90_000, pool=40) for i in range(3)]

    def msgs(r):
        out = []
        for k, s in enumerate(S):
            i = int(s[1])
            out.append(shared[i][7_000 * k + 9_000 * r:7_000 * k + 9_000 * r + 30_000] + mixed(1120 + 10 * r + k, 2_000))
        return out
    _turn(c, S, msgs(0))                                   # <HELLO>s
    _turn(c, S, msgs(1))                                   # held: r0_0 alone (the single call)
    _turn(c, S, msgs(2), order=[1, 0, 3, 2, 4, 5])         # held: r1_0 r0_0 r2_0, flushed before r1_1; then r1_1 alone
    c.launches, c.counted = (1, 3), [2]
    return c


def conv_blocks():
    """(c) 4 peers.  Peer 1's cache knows segments V's does not (declared on
    p1_x, whose wire is dropped): r1_0 blocks inside the launch and sends its
    <ASK>; the <LEARN> comes back beside the other peers' frames, and r1_0 is
    not plain that turn."""
    c = _hub('peers_blocks', [1] * 4)
    c.pipes['p1_x'] = 'P1'
    S = [f'p{i}_0' for i in range(4)]
    _turn(c, S, [mixed(1200 + i, 9_000) for i in range(4)])
    Q = mixed(1210, 60_000, pool=30, repeat=0.6)
    c.enc('p1_x', Q)                                       # (dropped)
    m = [mixed(1220 + i, 30_000) for i in range(4)]
    m[1] = mixed(1223, 5_000) + Q[2048:40_000] + mixed(1224, 3_000)
    w = [c.enc(s, x) for s, x in zip(S, m)]
    R = [_recv(s) for s in S]
    d = c.dmany(R, w)                                      # one launch of 4; r1_0: a prefix and its <ASK>
    a = c.dmany(S, d)                                      # a[1]: the <LEARN>
    w = [c.enc(s, mixed(1230 + i, 12_000) + Q[:5000]) for i, s in enumerate(S)]
    back = c.dmany(R, [[a[i], w[i]] for i in range(4)])    # r1_0 serial (<LEARN>), the others one launch of 3
    back = c.dmany(S, back)
    back = c.dmany(R, back)
    c.dmany(S, back)
    c.asked, c.learned = d[1], a[1]
    c.launches, c.counted = (2, 7), [1, 2]
    return c


def conv_fail_eos_cut():
    """(d) A bad opcode on one peer, a frame cut across two turns, <EOS> /
    <EOS_ACK> and a len-0 entry."""
    c = _hub('peers_fail_eos_cut', [1] * 4)
    S = [f'p{i}_0' for i in range(4)]
    R = [_recv(s) for s in S]
    _turn(c, S, [mixed(1300 + i, 6_000) for i in range(4)])
    w = [c.enc(S[i], mixed(1310 + i, 25_000 + 100 * i)) for i in range(3)]
    bad = frame(b'good bytes' + b'\xf1\x01' + family(9)[0] + b'\xf1\x07 and the rest')
    d = c.dmany(R, [w[0], _Cut(w[1], 6, 0), w[2], bad])    # held: r0 r2 r3 (r1's frame is not whole); r3 fails
    c.dmany(S[:3], d[:3])
    e2 = c.enc(S[2], b'')                                  # <EOS>
    w0 = c.enc(S[0], mixed(1310, 12_000) + mixed(1320, 5_000))
    d = c.dmany(R[:3], [w0, _Cut(w[1], 6, 1), e2])         # held: r0 r1; r2: <EOS> alone
    a = c.dmany(S[:3], d)
    e = c.enc(R[2], b'')                                   # r2 closes its side: <HELLO> <EOS>
    k = c.dmany([S[2], S[0]], [e, b''])                    # p0: the peer closed
    w1 = c.enc(S[1], mixed(1311, 9_000))
    d = c.dmany([R[1], R[2], R[0]], [w1, k[0], a[0]])      # held: r1 alone
    c.dmany([S[1], S[2]], d[:2])
    c.failed = R[3]
    c.launches, c.counted = (2, 5), [1, 2]
    return c


def conv_connecting():
    """(e) Peer 1 has a second pipe whose receiver is still before its <HELLO>
    in the middle of a turn: it may connect to a held context (it does), so the
    held calls go up first -- its frame REFs what r1_0's EXTRACTs."""
    c = _hub('peers_connecting', [1, 2, 1])
    S = ['p0_0', 'p1_0', 'p2_0']
    both = mixed(1400, 80_000, pool=30)
    _turn(c, S, [mixed(1410 + i, 7_000) for i in range(3)])
    w = [c.enc('p0_0', mixed(1420, 20_000)), c.enc('p1_0', both[:30_000]), c.enc('p1_1', both[10_000:45_000]),
         c.enc('p2_0', mixed(1422, 20_000))]
    d = c.dmany(['r0_0', 'r1_0', 'r1_1', 'r2_0'], w)       # held: r0_0 r1_0 | r1_1 connects | r2_0 alone
    c.dmany(['p0_0', 'p1_0', 'p1_1', 'p2_0'], d)
    w = [c.enc('p0_0', mixed(1420, 9_000) + mixed(1430, 6_000)), c.enc('p1_1', both[40_000:70_000]),
         c.enc('p2_0', mixed(1432, 15_000)), c.enc('p1_0', both[50_000:80_000])]
    d = c.dmany(['r0_0', 'r1_1', 'r2_0', 'r1_0'], w)       # held: r0_0 r1_1 r2_0, flushed before r1_0; r1_0 alone
    c.dmany(['p0_0', 'p1_1', 'p2_0', 'p1_0'], d)
    c.launches, c.counted = (2, 5), [1, 2]
    return c


BUILDERS = {f.__name__[5:]: f for f in (conv_hub, conv_mixed, conv_blocks, conv_fail_eos_cut, conv_connecting)}
NAMES = ['peers_' + k for k in BUILDERS]


def conversation(name):
    c = BUILDERS[name[6:]]()
    assert c.name == name
    return c
