"""xcg_decode_call_many: one decode() call per peer cache, the calls of many
peers in one launch, against the oracle serving the same calls one by one
(decode_peers_cases.run_model: a cache_new() cache and a decoder_new decoder
per peer)."""
import ctypes as C
import gc

import numpy as np
import pytest

import decode_peers_cases as P
import decode_windows_cases as W

pytestmark = pytest.mark.gpu

SEG = 2048
XCG_EINVAL, XCG_EOVERFLOW = -22, -75
SEGMENTS = 4096                          # a peer's cache: small, so that many peers stay small


@pytest.fixture(scope='module')
def cases(oracle):
    return {c['name']: c for c in P.all_cases(oracle)}


@pytest.fixture(scope='module')
def modelled(oracle, cases):
    return {name: P.run_model(oracle, c) for name, c in cases.items()}


def make_ctx(kind):
    from wanproxy_amd.xcgpu import Context
    if kind == 'bounded':
        return Context(0, memory_cache_limit=P.LIMIT)
    if kind == 'pair':
        return Context(0, memory_cache_limit=P.LIMIT, disk_bytes=P.DISK)
    if kind == 'null':
        return Context(0, null_cache=True, cache_segments=SEGMENTS)
    return Context(0, cache_segments=SEGMENTS)


class Peers:
    """The engine's side of a case: a context per peer; every second plain peer
    decodes on a window of its own, the others on their context's."""

    def __init__(self, kinds):
        from wanproxy_amd.xcgpu import Window
        self.kinds = kinds
        self.ctx = [make_ctx(k) for k in kinds]
        self.win = [Window(c) if p % 2 == 0 else None for p, c in enumerate(self.ctx)]

    def calls(self, step, caps=None):
        return [(self.ctx[p], self.win[p], enc) + ((caps[k],) if caps else ()) for k, (p, enc, _) in enumerate(step)]

    def probe(self, p):
        def decode1(chunk):
            outs, st, cons, _ = self.ctx[p].decode_chunks([chunk], window=self.win[p])
            return int(st[0]), outs[0], int(cons[0])
        return W.probe_window(decode1)

    def export(self, p):
        hs, segs = self.ctx[p].cache_export()
        return {int(h): bytes(segs[k * SEG:(k + 1) * SEG]) for k, h in enumerate(hs)}

    def check_final(self, final, name):
        for p, (slots, cache) in enumerate(final):
            assert self.probe(p) == slots, (name, 'window of peer', p)
            if self.kinds[p] == 'plain':
                assert self.export(p) == cache, (name, 'cache of peer', p)
            elif self.kinds[p] == 'bounded':
                assert self.ctx[p].cache_size() == len(cache), (name, 'cache of peer', p)

    def close(self):
        for w in self.win:
            if w is not None:
                w.close()
        for c in self.ctx:
            c.close()


def run_case(case, want):
    """The case's steps on the engine, each call list in one function call,
    compared call by call; (peers, launches, finished, outside) -- the counters' moves."""
    from wanproxy_amd.xcgpu import debug_decode_call_many, decode_call_many
    peers = Peers(case['kinds'])
    before = debug_decode_call_many()
    for k, step in enumerate(case['steps']):
        if step[0] == 'learn':
            peers.ctx[step[1]].cache_learn(b''.join(step[2]))
            continue
        got = decode_call_many(peers.calls(step[1]))
        for j, (g, e) in enumerate(zip(got, want[k])):
            assert g == e, (case['name'], 'step', k, 'call', j, 'peer', step[1][j][0], g[:2], e[:2])
    after = debug_decode_call_many()
    return (peers,) + tuple(a - b for a, b in zip(after, before))


def test_lengths(cases, modelled):
    """Case 1: every call length that takes another path through the kernel's
    staging; the kernel finishes every non-empty call."""
    case = cases['lengths']
    want, final = modelled['lengths']
    peers, launches, finished, outside = run_case(case, want)
    nonempty = sum(1 for step in case['steps'] for _, enc, _ in step[1] if enc)
    assert (launches, finished, outside) == (3, nonempty, 0)
    peers.check_final(final, 'lengths')
    peers.close()


def test_blocked_peer(cases, modelled):
    """Case 2: one peer blocks mid-call -- status 1, the consumed prefix, the
    skim's set -- and the others are complete; then the <LEARN> and the rest."""
    case = cases['blocked']
    want, final = modelled['blocked']
    peers, launches, finished, outside = run_case(case, want)
    assert (launches, finished, outside) == (2, 10, 0)
    peers.check_final(final, 'blocked')
    peers.close()


def test_declined_and_ineligible_calls(cases, modelled):
    """Case 3: what the kernel declines and what it never takes, in one list
    with plain calls; each equals its oracle, the others are untouched."""
    case = cases['outside']
    want, final = modelled['outside']
    peers, launches, finished, outside = run_case(case, want)
    assert (launches, finished, outside) == (1, case['calls'] - case['outside'], case['outside'])
    peers.check_final(final, 'outside')
    peers.close()


def test_too_little_room(cases, modelled):
    """Case 4: one call of the list gets too little room: -75 and the size it
    needs, its cache and window untouched, the others done; again with room it
    equals the oracle."""
    from wanproxy_amd.xcgpu import decode_call_many
    case = cases['blocked']
    step = case['steps'][0][1]
    want, _ = modelled['blocked']
    peers = Peers(case['kinds'])
    short = 3
    caps = [None] * len(step)
    caps[short] = len(want[0][short][2]) - 1
    need = []
    got = decode_call_many(peers.calls(step, caps), out_lens=need)
    assert got[short][0] == XCG_EOVERFLOW and need[short] == len(want[0][short][2])
    for j, (g, e) in enumerate(zip(got, want[0])):
        assert j == short or g == e, j
    assert peers.ctx[short].cache_size() == 0 and peers.probe(short) == [None] * 256
    again = decode_call_many(peers.calls([step[short]]))
    assert again == [want[0][short]]
    peers.close()


def raw_many(ctxs, wins, encs, null=(), n=None):
    """xcg_decode_call_many on sentinel-filled outputs: (rc, buffers)."""
    from wanproxy_amd.xcgpu import lib
    m = len(ctxs)
    arr = lambda hs: (C.c_void_p * len(hs))(*[(h.h.value if h is not None else None) for h in hs])
    outs = [np.full(len(e) * 2 + 3 * SEG, 0x5A, np.uint8) for e in encs]
    unk = [np.full(64, 0x5A5A, np.uint64) for _ in encs]
    b = {'ol': np.full(m, 77, np.uint64), 'cons': np.full(m, 77, np.uint64), 'st': np.full(m, 77, np.int32),
         'nunk': np.full(m, 77, np.uint32), 'rc': np.full(m, 77, np.int32)}
    a = {'ctx': arr(ctxs), 'win': arr(wins), 'in': (C.c_char_p * m)(*encs),
         'len': (C.c_uint32 * m)(*[len(e) for e in encs]), 'out': (C.c_void_p * m)(*[o.ctypes.data for o in outs]),
         'cap': (C.c_uint64 * m)(*[o.size for o in outs]), 'unk': (C.c_void_p * m)(*[u.ctypes.data for u in unk]),
         'ucap': (C.c_uint32 * m)(*[u.size for u in unk])}
    p = lambda k: None if k in null else (a[k] if k in a else b[k].ctypes.data)
    rc = lib().xcg_decode_call_many(p('ctx'), p('win'), p('in'), p('len'), p('out'), p('cap'), m if n is None else n,
                                    p('ol'), p('cons'), p('st'), p('unk'), p('ucap'), p('nunk'), None, None, None,
                                    p('rc'))
    b['out'], b['unk'] = outs, unk
    return rc, b


def untouched(b):
    return (all((o == 0x5A).all() for o in b['out']) and all((u == 0x5A5A).all() for u in b['unk']) and
            all((b[k] == 77).all() for k in ('ol', 'cons', 'st', 'nunk', 'rc')))


def test_refusals_change_nothing(oracle, cases, modelled):
    """Case 5: every XCG_EINVAL behind the blocked case's first call list:
    outputs untouched, probes and exports afterwards the model's."""
    import torch
    from wanproxy_amd.xcgpu import Context, Window, decode_call_many
    case = cases['blocked']
    want, _ = modelled['blocked']
    peers = Peers(case['kinds'])
    step = case['steps'][0][1]
    assert decode_call_many(peers.calls(step)) == want[0]
    encs = [enc for _, enc, _ in case['steps'][2][1]]
    cs, ws = peers.ctx, peers.win
    for null in ('ctx', 'in', 'len', 'out', 'cap', 'ol', 'cons', 'st', 'unk', 'ucap', 'nunk', 'rc'):
        rc, b = raw_many(cs, ws, encs, null=(null,))
        assert rc == XCG_EINVAL and untouched(b), null
    spare = Window(cs[1])
    refused = {
        'a context twice': ([cs[0], cs[1], cs[0], cs[3], cs[4]], ws),
        'a window twice': (cs, [ws[0], None, ws[0], None, ws[4]]),
        'a null context': ([cs[0], None, cs[2], cs[3], cs[4]], ws),
    }
    if torch.cuda.device_count() > 1:
        other = Context(1, cache_segments=SEGMENTS)
        refused['contexts across devices'] = ([cs[0], other, cs[2], cs[3], cs[4]], [ws[0], None, ws[2], None, ws[4]])
        refused['a window of another device'] = (cs, [ws[0], Window(other), ws[2], None, ws[4]])
    for why, (c, w) in refused.items():
        rc, b = raw_many(c, w, encs)
        assert rc == XCG_EINVAL and untouched(b), why
    # n == 0 is fine, with or without arrays
    rc, b = raw_many(cs, ws, encs, n=0)
    assert rc == 0 and untouched(b)
    assert decode_call_many([]) == []
    spare.close()
    # nothing moved: the model after the first call list alone
    first_only = dict(case, steps=case['steps'][:1])
    _, final = P.run_model(oracle, first_only)
    peers.check_final(final, 'refusals')
    peers.close()


def test_one_call_is_decode_call(cases):
    """n == 1 is xcg_decode_call on a twin context."""
    from wanproxy_amd.xcgpu import Context, decode_call_many
    a, b = Context(0, cache_segments=SEGMENTS), Context(0, cache_segments=SEGMENTS)
    for _, enc, _ in cases['blocked']['steps'][0][1] + cases['lengths']['steps'][0][1][3:]:
        got = decode_call_many([(a, None, enc)])[0]
        assert got[0] == 0 and got[1:] == b.decode_call(enc)
    ha, sa = a.cache_export()
    hb, sb = b.cache_export()
    assert list(ha) == list(hb) and bytes(sa) == bytes(sb) and len(ha) > 0
    a.close()
    b.close()


def test_more_calls_than_compute_units(cases, modelled):
    """Case 6: 260 peers, one 3 KB call each, one function call, one launch."""
    want, final = modelled['wide']
    peers, launches, finished, outside = run_case(cases['wide'], want)
    assert (launches, finished, outside) == (1, 260, 0)
    for p in (0, 1, 128, 258, 259):
        assert peers.probe(p) == final[p][0] and peers.export(p) == final[p][1], p
    peers.close()


def mem_live():
    from wanproxy_amd.xcgpu import lib
    gc.collect()
    out = (C.c_uint64 * 4)()
    lib().xcg_debug_mem_live.restype = None
    lib().xcg_debug_mem_live.argtypes = [C.c_void_p]
    lib().xcg_debug_mem_live(out)
    return tuple(int(v) for v in out)


def test_memory_goes_with_its_owner(cases, modelled):
    """Case 7: the call's staging belongs to the first listed context; with the
    contexts and windows gone, nothing is held."""
    from wanproxy_amd.xcgpu import decode_call_many
    case = cases['blocked']
    for _ in range(2):
        before = mem_live()
        peers = Peers(case['kinds'])
        assert decode_call_many(peers.calls(case['steps'][0][1])) == modelled['blocked'][0][0]
        held = mem_live()
        assert held[0] > before[0] and held[1] > before[1]
        peers.close()
        del peers
        assert mem_live() == before
