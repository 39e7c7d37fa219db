"""xcg_decode_batch_windows_bounded / xcg_decode_host_windows_bounded: the chunks
of several decoders, one BACKREF window each, in one batch on a bounded cache or
a pair -- against the yardstick of tests/decode_windows_bounded_cases.py, which
tests/test_decode_windows_bounded_cases.py pins to the compiled reference:
outputs, statuses, consumed bytes and the stop chunk of every batch, the rest of
a stopped chunk through xcg_decode_batch, every window slot by slot, and the
cache -- the bounded cache's LRU order behind every step, the pair's disk
counters, and a lookup of every hash a case names.

65 distinct EXTRACTs on a limit of 64 are refused on the bounded context only: a
pair's disk level takes what the memory level lets go of, xcg_decode_batch
declines nothing there, and the batch has to come out as the model's."""
import ctypes as C

import numpy as np
import pytest

import decode_windows_bounded_cases as WB
from decode_windows_cases import R, X, probe_window

pytestmark = pytest.mark.gpu

SEG = WB.SEG
XCG_EINVAL = -22


@pytest.fixture(scope='module')
def cases(oracle):
    return {c['name']: c for c in WB.all_cases(oracle)}


@pytest.fixture(scope='module')
def modelled(oracle, cases):
    """run_model of (name, kind), made once."""
    memo = {}

    def get(name, kind):
        if (name, kind) not in memo:
            memo[name, kind] = WB.run_model(oracle, cases[name], kind)
        return memo[name, kind]
    return get


def make_ctx(case, kind):
    from wanproxy_amd.xcgpu import Context
    limit, disk = WB.geometry(case)
    if kind == 'bounded':
        return Context(0, memory_cache_limit=limit)
    if kind == 'pair':
        return Context(0, memory_cache_limit=limit, disk_bytes=disk)
    return Context(0, cache_segments=1 << 12)


def order(ctx, kind):
    return [int(h) for h in ctx.cache_export()[0]] if kind == 'bounded' else None


def probes(ctx, wins):
    def one(win):
        def decode1(chunk):
            outs, st, cons, _ = ctx.decode_chunks([chunk], window=win)
            return int(st[0]), outs[0], int(cons[0])
        return decode1
    return [probe_window(one(w)) for w in wins]


def serial(ctx, e, win):
    outs, st, cons, unk = ctx.decode_chunks([e], window=win)
    return int(st[0]), outs[0], int(cons[0]), sorted(unk)


def run_gpu(oracle, case, kind, host):
    """run_model's steps on a context of `kind`, batches through
    Context.decode_chunks_windows_bounded."""
    from wanproxy_amd.xcgpu import Window, XCGError
    ctx = make_ctx(case, kind)
    wins = [Window(ctx) for _ in range(case['n_windows'])]
    learner = Window(ctx)
    results, rest = [], None
    try:
        for step in case['steps']:
            if step[0] == 'learn':                   # (a decoder of their own: no window of the case moves)
                for a in range(0, len(step[1]), 32):
                    _, st, _, _ = ctx.decode_chunks([X(s) for s in step[1][a:a + 32]], window=learner)
                    assert not st.any()
                results.append(None)
            elif step[0] == 'probe':
                results.append(probes(ctx, wins))
            elif step[0] == 'rest':
                if rest is None:
                    results.append(None)
                    continue
                w, e = rest
                rest = None
                st, out, cons, unk = serial(ctx, e, wins[w])
                results.append({'status': st, 'out': out, 'consumed': cons, 'unknown': unk, 'order': order(ctx, kind)})
            elif WB.refused_on(step, kind):
                before = order(ctx, kind), ctx.pair_stats() if kind == 'pair' else None, probes(ctx, wins), ctx.cache_size()
                with pytest.raises(XCGError, match=r'\(-95\)'):
                    ctx.decode_chunks_windows_bounded(step[1], wins, step[2], host=host)
                after = order(ctx, kind), ctx.pair_stats() if kind == 'pair' else None, probes(ctx, wins), ctx.cache_size()
                assert after == before, (case['name'], kind, 'a refused batch changed something')
                rest = None
                results.append({'refused': True, 'serial': [serial(ctx, e, wins[w]) for e, w in zip(step[1], step[2])],
                                'order': order(ctx, kind)})
            else:
                outs, st, cons, stop = ctx.decode_chunks_windows_bounded(step[1], wins, step[2], host=host)
                st, cons = [int(s) for s in st], [int(c) for c in cons]
                rest = (step[2][stop], step[1][stop][cons[stop]:]) if stop < len(st) and st[stop] == 1 else None
                results.append({'outs': outs, 'status': st, 'consumed': cons, 'stop': stop, 'order': order(ctx, kind)})
        found = [serial(ctx, R(h), learner)[0] == 0 for h in WB.hashes_of(oracle, case)]
        ps = ctx.pair_stats() if kind == 'pair' else None
        results.append({'order': order(ctx, kind), 'pair_stats': (ps[1], ps[2]) if ps else None, 'found': found})
    finally:
        for w in wins + [learner]:
            w.close()
        ctx.close()
    return results


def check(got, want, name):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, dict):
            assert sorted(g) == sorted(w), (name, k)
            for key in w:
                if key == 'outs':
                    for i, (a, b) in enumerate(zip(g['outs'], w['outs'])):
                        assert a == b, (name, k, 'output of chunk', i, len(a), len(b))
                elif key == 'serial':
                    for i, (a, b) in enumerate(zip(g['serial'], w['serial'])):
                        assert a == b, (name, k, 'serial chunk', i, a[0], b[0], a[2], b[2])
                elif key == 'out':
                    assert g['out'] == w['out'], (name, k, 'rest output', len(g['out']), len(w['out']))
                else:
                    assert g[key] == w[key], (name, k, key, g[key], w[key])
        else:
            assert g == w, (name, k)


@pytest.mark.parametrize('host', [False, True], ids=['device', 'host'])
@pytest.mark.parametrize('kind', ['bounded', 'pair'])
@pytest.mark.parametrize('name', WB.CASE_NAMES)
def test_case_matches_the_model(oracle, cases, modelled, name, kind, host):
    check(run_gpu(oracle, cases[name], kind, host), modelled(name, kind), (name, kind, host))


def test_an_unbounded_context_is_not_supported(cases):
    from wanproxy_amd.xcgpu import Context, Window, XCGError
    ctx = Context(0, cache_segments=1 << 12)
    wins = [Window(ctx) for _ in range(2)]
    step = cases['cross_refs']['steps'][0]
    for host in (False, True):
        with pytest.raises(XCGError, match=r'\(-95\)'):
            ctx.decode_chunks_windows_bounded(step[1], wins, step[2], host=host)
    assert ctx.cache_size() == 0
    outs, st, _, stop = ctx.decode_chunks_windows(step[1], wins, step[2])     # (its own call takes the batch)
    assert not any(st) and stop == len(step[1])
    ctx.close()


def raw_call(ctx, chunks, wins, n_windows, cw, null=(), max_len=None):
    """xcg_decode_batch_windows_bounded on device buffers filled with a
    sentinel.  Returns (rc, every output buffer as numpy)."""
    import torch
    from wanproxy_amd.xcgpu import _stream_ptr, lib
    dev = torch.device('cuda', ctx.device)
    n = len(chunks)
    lens = np.array([len(e) for e in chunks], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
    t = {'enc': torch.from_numpy(np.frombuffer(b''.join(chunks), np.uint8).copy()).to(dev),
         'off': torch.from_numpy(offs.view(np.int64)).to(dev), 'len': torch.from_numpy(lens.view(np.int32)).to(dev)}
    cap = int(lens.sum()) * 205 + 4096
    o = {'out': torch.full((cap,), 0x5A, dtype=torch.uint8, device=dev),
         'oo': torch.full((n,), -7, dtype=torch.int64, device=dev), 'ol': torch.full((n,), -7, dtype=torch.int64, device=dev),
         'st': torch.full((n,), -7, dtype=torch.int32, device=dev), 'cons': torch.full((n,), -7, dtype=torch.int64, device=dev)}
    p = lambda name, d: None if name in null else C.c_void_p(d[name].data_ptr())
    cwa = np.ascontiguousarray(cw, dtype=np.uint32)
    stop, total = np.full(1, 77, np.uint32), np.full(1, 77, np.uint64)
    rc = lib().xcg_decode_batch_windows_bounded(
        ctx.h, p('enc', t), p('off', t), p('len', t), n, int(lens.max()) if max_len is None else max_len,
        None if 'windows' in null else wins, n_windows, None if 'cw' in null else cwa.ctypes.data, p('out', o), cap,
        p('oo', o), p('ol', o), p('st', o), p('cons', o), stop.ctypes.data, total.ctypes.data, _stream_ptr(None))
    torch.cuda.synchronize(dev)
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def untouched(bufs):
    return (bufs['out'] == 0x5A).all() and all((bufs[k] == -7).all() for k in ('oo', 'ol', 'st', 'cons'))


@pytest.mark.parametrize('kind', ['bounded', 'pair'])
def test_argument_errors_change_nothing(oracle, cases, modelled, kind):
    """Each XCG_EINVAL of the header behind the cross_refs batch: outputs
    untouched, and the probe and the account that follow are the model's."""
    from wanproxy_amd.xcgpu import Window
    case = cases['cross_refs']
    chunks, cw = case['steps'][0][1], case['steps'][0][2]
    want = modelled('cross_refs', kind)
    ctx = make_ctx(case, kind)
    wins = [Window(ctx) for _ in range(2)]
    outs, st, cons, stop = ctx.decode_chunks_windows_bounded(chunks, wins, cw)
    assert outs == want[0]['outs'] and stop == want[0]['stop']
    arr = lambda ws: (C.c_void_p * len(ws))(*[w.h if w is not None else None for w in ws])
    for null in ('enc', 'off', 'len', 'oo', 'ol', 'st', 'cons', 'windows', 'cw'):
        rc, bufs = raw_call(ctx, chunks, arr(wins), 2, cw, null=(null,))
        assert rc == XCG_EINVAL and untouched(bufs), null
    refused = {
        'window index out of range': (arr(wins), 2, [0, 1, 0, 2], None),
        'fewer windows than named': (arr(wins), 1, cw, None),
        'a null window': (arr([wins[0], None]), 2, cw, None),
        'a window listed twice': (arr([wins[0], wins[0]]), 2, cw, None),
        'no window': (arr(wins), 0, cw, None),
        'chunks of 2 MiB': (arr(wins), 2, cw, 1 << 21),
    }
    for why, (wa, nw, cwk, max_len) in refused.items():
        rc, bufs = raw_call(ctx, chunks, wa, nw, cwk, max_len=max_len)
        assert rc == XCG_EINVAL and untouched(bufs), why
    assert probes(ctx, wins) == want[1]
    assert order(ctx, kind) == want[0]['order']
    for w in wins:
        w.close()
    ctx.close()


def mem_live():
    from wanproxy_amd.xcgpu import lib
    out = (C.c_uint64 * 4)()
    lib().xcg_debug_mem_live.restype = None
    lib().xcg_debug_mem_live.argtypes = [C.c_void_p]
    lib().xcg_debug_mem_live(out)
    return list(out)


@pytest.mark.parametrize('kind', ['bounded', 'pair'])
def test_no_chunk_is_ok_and_nothing_stays_allocated(cases, kind):
    from wanproxy_amd.xcgpu import Window, lib
    live0 = mem_live()
    case = cases['cross_refs']
    ctx = make_ctx(case, kind)
    wins = [Window(ctx) for _ in range(2)]
    stop, total = np.full(1, 77, np.uint32), np.full(1, 77, np.uint64)
    assert lib().xcg_decode_batch_windows_bounded(ctx.h, None, None, None, 0, 0, None, 0, None, None, 0, None, None,
                                                  None, None, stop.ctypes.data, total.ctypes.data, None) == 0
    assert (int(stop[0]), int(total[0])) == (0, 0)
    assert lib().xcg_decode_host_windows_bounded(ctx.h, None, 0, None, None, 0, None, 0, None, None, 0, None, None,
                                                 None, None, stop.ctypes.data, total.ctypes.data) == 0
    outs, st, cons, stop_chunk = ctx.decode_chunks_windows_bounded([], wins, [])
    assert outs == [] and stop_chunk == 0 and ctx.cache_size() == 0
    for host in (False, True):
        ctx.decode_chunks_windows_bounded(case['steps'][0][1], wins, case['steps'][0][2], host=host)
    for w in wins:
        w.close()
    ctx.close()
    assert mem_live() == live0
