"""xcg_decode_batch_windows / xcg_decode_host_windows: the chunks of several
decoders -- one BACKREF window each, one cache -- in one GPU batch, against the
oracle's own model of that (decode_windows_cases.run_model: several
Oracle.decoder_new decoders on one cache, chunk by chunk)."""
import ctypes as C
import struct

import numpy as np
import pytest

import decode_windows_cases as W
from backref_streams import stream_with_backrefs
from wanproxy_amd import synth

pytestmark = pytest.mark.gpu

SEG = 2048
XCG_EINVAL, XCG_ENOTSUP = -22, -95


@pytest.fixture(scope='module')
def cases(oracle):
    return {c['name']: c for c in W.all_cases(oracle)}


@pytest.fixture(scope='module')
def modelled(oracle, cases):
    return {name: W.run_model(oracle, c) for name, c in cases.items()}


def batch_result(r):
    outs, st, cons, stop = r
    return {'outs': outs, 'status': [int(s) for s in st], 'consumed': [int(c) for c in cons], 'stop': stop}


def probe(ctx, wins, w, host):
    def decode1(chunk):
        outs, st, cons, _ = ctx.decode_chunks_windows([chunk], wins, [w], host=host)
        return int(st[0]), outs[0], int(cons[0])
    return W.probe_window(decode1)


def exported(ctx):
    hs, segs = ctx.cache_export()
    assert list(hs) == sorted(hs)                              # (an unbounded cache: ascending hash)
    return {int(h): bytes(segs[k * SEG:(k + 1) * SEG]) for k, h in enumerate(hs)}


def run_gpu(case, host, upto=None):
    from wanproxy_amd.xcgpu import Context, Window
    ctx = Context(0)
    wins = [Window(ctx) for _ in range(case['n_windows'])]
    results = []
    for step in case['steps'][:upto]:
        if step[0] == 'learn':
            ctx.cache_learn(b''.join(step[1]))
            results.append(None)
        elif step[0] == 'batch':
            results.append(batch_result(ctx.decode_chunks_windows(step[1], wins, step[2], host=host)))
        else:
            results.append([probe(ctx, wins, w, host) for w in range(case['n_windows'])])
    return ctx, wins, results


NAMES = [f.__name__[5:] for f in W.BUILDERS]


@pytest.mark.parametrize('host', [False, True], ids=['device', 'host'])
@pytest.mark.parametrize('name', NAMES)
def test_case_matches_the_model(cases, modelled, name, host):
    ctx, wins, results = run_gpu(cases[name], host)
    want, held = modelled[name]
    for k, (got, exp) in enumerate(zip(results, want)):
        assert got == exp, (name, 'step', k, cases[name]['steps'][k][0])
    assert exported(ctx) == held, name
    ctx.close()


@pytest.mark.parametrize('rate,bad,nbytes,chunk', [(0.4, 0.03, 1 << 18, 16384), (0.4, 0.0, 1 << 18, 16384),
                                                   (0.0, 0.0, 1 << 20, 65536)],
                         ids=['backrefs-stop', 'backrefs', 'tail'])
def test_one_window_is_decode_batch(oracle, rate, bad, nbytes, chunk):
    """n_windows == 1: xcg_decode_batch's outputs, statuses, consumed, window
    and cache on the same input (full records with BACKREFs, the 256-record
    tail of more than 256 declares without)."""
    from wanproxy_amd.xcgpu import Context, Window
    data = synth.stream(23, nbytes, 70, 1)
    encs = stream_with_backrefs(oracle, data, chunk, 23, rate, bad)
    a, b = Context(0), Context(0)
    wa, wb = Window(a), Window(b)
    outs, st, cons, _ = a.decode_chunks(encs, window=wa)
    got = b.decode_chunks_windows(encs, [wb], [0] * len(encs))
    assert got[0] == outs and list(got[1]) == list(st) and list(got[2]) == list(cons)
    stops = [k for k, s in enumerate(st) if s in (1, -1)]
    assert got[3] == (stops[0] if stops else len(encs)) and bool(stops) == bool(bad)

    def slots_a(chunk):
        o, s, c, _ = a.decode_chunks([chunk], window=wa)
        return int(s[0]), o[0], int(c[0])
    assert probe(b, [wb], 0, False) == W.probe_window(slots_a)
    assert exported(a) == exported(b)
    a.close()
    b.close()


def raw_call(ctx, chunks, wins, n_windows, cw, null=(), out_cap=None):
    """xcg_decode_batch_windows on device buffers filled with a sentinel.
    Returns (rc, stop, total, every output buffer as numpy)."""
    import torch
    from wanproxy_amd.xcgpu import _stream_ptr, lib
    dev = torch.device('cuda', ctx.device)
    n = len(chunks)
    lens = np.array([len(e) for e in chunks], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
    t = {'enc': torch.from_numpy(np.frombuffer(b''.join(chunks), np.uint8).copy()).to(dev),
         'off': torch.from_numpy(offs.view(np.int64)).to(dev), 'len': torch.from_numpy(lens.view(np.int32)).to(dev)}
    cap = int(lens.sum()) * 205 + 4096 if out_cap is None else out_cap
    o = {'out': torch.full((max(cap, 1),), 0x5A, dtype=torch.uint8, device=dev),
         'oo': torch.full((n,), -7, dtype=torch.int64, device=dev), 'ol': torch.full((n,), -7, dtype=torch.int64, device=dev),
         'st': torch.full((n,), -7, dtype=torch.int32, device=dev), 'cons': torch.full((n,), -7, dtype=torch.int64, device=dev)}
    p = lambda name, d: None if name in null else C.c_void_p(d[name].data_ptr())
    cwa = np.ascontiguousarray(cw, dtype=np.uint32)
    stop, total = np.full(1, 77, np.uint32), np.full(1, 77, np.uint64)
    rc = lib().xcg_decode_batch_windows(
        ctx.h, p('enc', t), p('off', t), p('len', t), n, int(lens.max()), None if 'windows' in null else wins,
        n_windows, None if 'cw' in null else cwa.ctypes.data, p('out', o), cap, p('oo', o), p('ol', o), p('st', o),
        p('cons', o), stop.ctypes.data, total.ctypes.data, _stream_ptr(None))
    torch.cuda.synchronize(dev)
    return rc, int(stop[0]), int(total[0]), {k: v.cpu().numpy() for k, v in o.items()}


def untouched(bufs):
    return (bufs['out'] == 0x5A).all() and all((bufs[k] == -7).all() for k in ('oo', 'ol', 'st', 'cons'))


def test_refusals_change_nothing(cases, modelled):
    """Each XCG_EINVAL of the call, and XCG_EOVERFLOW, behind the interleave
    batch: outputs untouched, and the probe and the export that follow are the
    model's -- windows and cache as the batch left them.  A window no chunk
    names keeps its bytes."""
    import torch
    from wanproxy_amd.xcgpu import Context, Window
    case = cases['interleave']
    ctx, wins, results = run_gpu(case, False, upto=1)
    want, held = modelled['interleave']
    assert results[0] == want[0]
    chunks, cw = case['steps'][0][1], case['steps'][0][2]
    arr = lambda ws: (C.c_void_p * len(ws))(*[w.h if w is not None else None for w in ws])
    for null in ('enc', 'off', 'len', 'oo', 'ol', 'st', 'cons', 'windows', 'cw'):
        rc, _, _, bufs = raw_call(ctx, chunks, arr(wins), 3, cw, null=(null,))
        assert rc == XCG_EINVAL and untouched(bufs), null
    refused = {
        'window index out of range': (arr(wins), 3, [0, 1, 0, 3, 1, 0, 2]),
        'fewer windows than named': (arr(wins), 2, cw),
        'a null window': (arr([wins[0], None, wins[2]]), 3, cw),
        'a window listed twice': (arr([wins[0], wins[1], wins[0]]), 3, cw),
        'no window': (arr(wins), 0, cw),
        'above the cap': ((C.c_void_p * 65537)(*([wins[0].h] * 65537)), 65537, cw),
    }
    if torch.cuda.device_count() > 1:
        other = Context(1)
        refused['a window of another device'] = (arr([wins[0], Window(other), wins[2]]), 3, cw)
    for why, (wa, nw, cwk) in refused.items():
        rc, _, _, bufs = raw_call(ctx, chunks, wa, nw, cwk)
        assert rc == XCG_EINVAL and untouched(bufs), why
    # too little room: the size needed comes back, nothing is written or committed
    rc, _, total, bufs = raw_call(ctx, chunks, arr(wins), 3, cw, out_cap=4096)
    assert rc == -75 and (bufs['out'] == 0x5A).all()
    assert total == sum(len(o) for o in want[0]['outs'])
    # a batch that names windows 0 and 2 only: window 1 is not touched (probe below)
    spare = Window(ctx)
    rc, stop, _, bufs = raw_call(ctx, [W.B(0), W.B(0)], arr([wins[0], spare, wins[2]]), 3, [0, 2])
    assert rc == 0 and stop == 2 and list(bufs['st']) == [0, 0]
    assert probe(ctx, [spare], 0, False) == [None] * 256
    assert [probe(ctx, wins, w, False) for w in range(3)] == want[1]
    assert exported(ctx) == held
    ctx.close()


def test_no_chunk_is_ok():
    from wanproxy_amd.xcgpu import Context, Window, lib
    ctx = Context(0)
    win = Window(ctx)
    stop, total = np.full(1, 77, np.uint32), np.full(1, 77, np.uint64)
    assert lib().xcg_decode_batch_windows(ctx.h, None, None, None, 0, 0, None, 0, None, None, 0, None, None, None,
                                          None, stop.ctypes.data, total.ctypes.data, None) == 0
    assert (int(stop[0]), int(total[0])) == (0, 0)
    assert lib().xcg_decode_host_windows(ctx.h, None, 0, None, None, 0, None, 0, None, None, 0, None, None, None,
                                         None, stop.ctypes.data, total.ctypes.data) == 0
    outs, st, cons, stop_chunk = ctx.decode_chunks_windows([], [win], [])
    assert outs == [] and stop_chunk == 0
    assert ctx.cache_size() == 0
    ctx.close()


@pytest.mark.parametrize('kind', ['bounded', 'pair'])
def test_bounded_and_pair_contexts_are_not_supported(kind, cases):
    from wanproxy_amd.xcgpu import Context, Window, XCGError
    kw = {'memory_cache_limit': 64 * SEG}
    if kind == 'pair':
        kw['disk_bytes'] = (18 + 205) * SEG
    ctx = Context(0, **kw)
    wins = [Window(ctx) for _ in range(3)]
    step = cases['interleave']['steps'][0]
    for host in (False, True):
        with pytest.raises(XCGError, match=r'\(-95\)'):
            ctx.decode_chunks_windows(step[1], wins, step[2], host=host)
    assert ctx.cache_size() == 0
    # (the serial calls such a context is served by still work, on an untouched window)
    outs, st, _, _ = ctx.decode_chunks([W.X(bytes(SEG)) + W.R(0x1234)], window=wins[0])
    assert int(st[0]) == 1 and outs[0] == bytes(SEG)
    ctx.close()


def test_many_unknown_hashes_behind_a_stop_do_not_fail_the_call():
    """65,537 REFs to distinct unknown hashes (more than the unknown set of
    xcg_decode_batch holds): the first is the stop point, the call is fine."""
    from wanproxy_amd.xcgpu import Context, Window
    seg = W.rnd_segs(9, 1)[0]
    hs = np.unique(np.random.default_rng(0x65537).integers(1 << 40, 1 << 62, 70000, dtype=np.uint64))[:65537]
    assert hs.size == 65537
    refs = b''.join(b'\xf1\x02' + struct.pack('>Q', int(h)) for h in hs)
    ctx = Context(0)
    wins = [Window(ctx), Window(ctx)]
    outs, st, cons, stop = ctx.decode_chunks_windows([W.X(seg) + b'ab', b'cd' + refs, W.X(seg)], wins, [0, 1, 0])
    assert [int(s) for s in st] == [0, 1, 2] and stop == 1
    assert outs[0] == seg + b'ab' and outs[1] == b'cd' and int(cons[1]) == 2
    assert ctx.cache_size() == 1
    ctx.close()
