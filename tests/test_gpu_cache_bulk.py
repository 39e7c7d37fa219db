"""GPU tests of the bulk cache learn and export (xcg_cache_learn_batch /
xcg_cache_export and their host forms): a learn equals n single-segment enters
in order, an export lists the cache in its fixed order and changes nothing.
Expected states come from the C restatement's sequential result
(tests/test_cache_bulk_cases.py pins the closed form to it) and, where it is
built, from the reference's own classes."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

import cache_bulk_cases as cb
from collision_cases import LRU_LIMIT, PAIR_DISK, PAIR_LIMIT
from oracle.lib import MODE_STREAM
from test_cache_bulk_cases import oracle_export, oracle_learn

pytestmark = pytest.mark.gpu
SEG = 2048
XCG_EOVERFLOW, XCG_ENOTSUP = -75, -95


def learn_at(ctx, segs, offset=0, sync=True):
    """xcg_cache_learn_batch with d_segs at byte `offset` of its buffer (a torch
    allocation is 256-byte aligned).  Returns the hashes (sync) or the tensors."""
    import torch
    dev = torch.device('cuda', ctx.device)
    n = len(segs)
    buf = torch.zeros(n * SEG + 64, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    buf[offset:offset + n * SEG] = torch.from_numpy(np.frombuffer(b''.join(segs), np.uint8).copy()).to(dev)
    d_hash = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    ctx.cache_learn_device(buf[offset:], n, d_hash)
    if not sync:
        return buf, d_hash
    return d_hash.cpu().numpy().view(np.uint64)[:n]


def export_of(ctx):
    hs, segs = ctx.cache_export()
    return [int(h) for h in hs], [segs[k * SEG:(k + 1) * SEG] for k in range(len(hs))]


def chunks8k(d):
    offs = np.arange(0, d.size, 8192, dtype=np.uint64)
    return offs, np.minimum(8192, d.size - offs).astype(np.uint32)


def mem_live():
    from wanproxy_amd.xcgpu import lib
    gc.collect()
    out = (C.c_uint64 * 4)()
    lib().xcg_debug_mem_live.restype = None
    lib().xcg_debug_mem_live.argtypes = [C.c_void_p]
    lib().xcg_debug_mem_live(out)
    return tuple(int(v) for v in out)


# -------------------------------------------------- equivalence with n enters

_ENTERED = {}


def entered(oracle, n):
    """Per n, once: the segment set, its hashes, and the state of a context
    that took it through n cache_enter calls -- size, export, every lookup."""
    if n not in _ENTERED:
        from wanproxy_amd.xcgpu import Context
        segs = cb.segment_set(n, n)
        hs = [oracle.hash(s) for s in segs]
        ctx = Context(0, cache_segments=1024)
        for h, s in zip(hs, segs):
            ctx.cache_enter(h, s)
        _ENTERED[n] = (segs, hs, ctx.cache_size(), export_of(ctx), {h: ctx.cache_lookup(h) for h in set(hs)})
        ctx.close()
    return _ENTERED[n]


@pytest.mark.parametrize('offset', cb.OFFSETS)
@pytest.mark.parametrize('n', cb.SIZES)
def test_learn_equals_enter_calls(oracle, n, offset):
    from wanproxy_amd.xcgpu import Context
    segs, hs, size, exp, looked = entered(oracle, n)
    ctx = Context(0, cache_segments=1024)
    try:
        got_h = learn_at(ctx, segs, offset)
        assert [int(h) for h in got_h] == hs
        assert ctx.cache_size() == size == len(set(hs))
        assert export_of(ctx) == exp
        assert exp[0] == sorted(exp[0])                   # unbounded: ascending hash
        for h, s in looked.items():
            assert ctx.cache_lookup(h) == s, hex(h)
        if n > 1:                                         # the last of a family won; both lo twins are held
            last = {h: s for h, s in zip(hs, segs)}
            assert dict(zip(*exp)) == last
        ctx.status()
    finally:
        ctx.close()


def test_learn_on_a_filled_cache_and_the_host_form(oracle):
    """A second learn meets hashes the cache holds (overwritten in place) and
    new ones; xcg_cache_learn_host is the same call from host memory."""
    from wanproxy_amd.xcgpu import Context
    first, second = cb.segment_set(64, 64), cb.segment_set(65, 64)
    a, b = Context(0, cache_segments=256), Context(0, cache_segments=256)
    try:
        learn_at(a, first, 3)
        learn_at(a, second, 1)
        for s in first + second:
            b.cache_enter(oracle.hash(s), s)
        assert export_of(a) == export_of(b)
        c = Context(0, cache_segments=256)
        hs = c.cache_learn(b''.join(first))
        assert [int(h) for h in hs] == [oracle.hash(s) for s in first]
        assert [int(h) for h in c.cache_learn(np.frombuffer(b''.join(second), np.uint8))] == \
            [oracle.hash(s) for s in second]
        assert export_of(c) == export_of(b)
        assert len(c.cache_learn(b'')) == 0
        c.close()
    finally:
        a.close()
        b.close()


# ------------------------------------------------------ behaviour after a load

def test_stream_encode_after_a_learn_inband(oracle, ref_oracle):
    """No synchronisation between the learn and the batch: the encode is
    ordered behind it by the context.  Against the reference's classes (name
    reuse taken out, see cache_bulk_cases.without_reuse)."""
    from wanproxy_amd.xcgpu import XCG_SEM_STREAM, Context
    (batch,) = cb.without_reuse(oracle.hash, cb.segment_set(300, 300))
    rc = ref_oracle.cache_new(0)
    for s in batch:
        ref_oracle.cache_learn(rc, s)
    d = cb.later_stream(batch)
    offs, lens = chunks8k(d)
    exp = ref_oracle.encode_batch(d, offs, lens, mode=MODE_STREAM, cache=rc)
    ref_oracle.cache_free(rc)
    ctx = Context(0, cache_segments=1024)
    try:
        keep = learn_at(ctx, batch, 1, sync=False)
        got = ctx.encode_chunks(d, offs, lens, semantics=XCG_SEM_STREAM)
        del keep
        assert got == exp
        assert sum(e.count(b'\xf1\x02') for e in got) >= 12
    finally:
        ctx.close()


def test_tack_p_flow_out_of_band(oracle, tmp_path):
    """cache_save / cache_load are tack -p's file (the segments back to back):
    a second out-of-band context loads what the first learned, and encodes and
    decodes as the restatement does on its learned cache."""
    from wanproxy_amd.xcgpu import XCG_SEM_STREAM, Context
    batch = cb.segment_set(300, 300)
    c = oracle.cache_new(0)
    oracle_learn(oracle, c, batch)
    d = cb.later_stream(batch)
    offs, lens = chunks8k(d)
    exp = oracle.encode_batch(d, offs, lens, mode=MODE_STREAM, oob=True, cache=c)
    oracle.cache_free(c)
    path = os.path.join(tmp_path, 'tack.cache')
    a = Context(0, out_of_band=True, cache_segments=1024)
    b = Context(0, out_of_band=True, cache_segments=1024)
    try:
        learn_at(a, batch, 16)
        a.cache_save(path)
        hs, segs = a.cache_export()
        assert os.path.getsize(path) == len(hs) * SEG == len(segs)
        got_h = b.cache_load(path)
        assert [int(h) for h in got_h] == [int(h) for h in hs]
        assert export_of(b) == export_of(a)
        assert b.encode_chunks(d, offs, lens, semantics=XCG_SEM_STREAM) == exp
        # a REF-only stream decodes from the loaded cache
        last = {oracle.hash(s): s for s in batch}
        names = list(last)[:40]
        enc = b''.join(b'\xf1\x02' + h.to_bytes(8, 'big') for h in names)
        outs, st, cons, unk = b.decode_chunks([enc])
        assert outs == [b''.join(last[h] for h in names)] and not st.any() and not unk and cons[0] == len(enc)
    finally:
        a.close()
        b.close()


# --------------------------------------------------------------------- bounded

@pytest.mark.parametrize('full', [False, True], ids=['empty', 'full'])
def test_bounded_learn_is_the_sequential_lru(oracle, full):
    """Limit 24: the 100-segment batch over 40 hashes, on an empty cache and on
    24 earlier entries, as one call and cut in two at every third position.
    The export is xco_cache_export's exactly -- hashes, bytes and order -- and a
    stream encode that goes on to evict equals the oracle's."""
    from wanproxy_amd.xcgpu import XCG_SEM_STREAM, Context
    earlier, batch = (cb.lru_earlier() if full else []), cb.lru_batch()
    c = oracle.cache_new(LRU_LIMIT * SEG)
    oracle_learn(oracle, c, earlier)
    oracle_learn(oracle, c, batch)
    exp = oracle_export(oracle, c)
    assert len(exp[0]) == LRU_LIMIT
    d = cb.later_stream(batch)
    offs, lens = chunks8k(d)
    exp_enc = oracle.encode_batch(d, offs, lens, mode=MODE_STREAM, cache=c)
    exp_after = oracle_export(oracle, c)
    oracle.cache_free(c)
    assert exp_after != exp
    for cut in cb.splits(len(batch)):
        ctx = Context(0, memory_cache_limit=LRU_LIMIT * SEG)
        try:
            if earlier:
                learn_at(ctx, earlier, 1)
            if cut is None:
                learn_at(ctx, batch, 3)
            else:
                learn_at(ctx, batch[:cut], 0, sync=False)
                learn_at(ctx, batch[cut:], 1)
            assert export_of(ctx) == exp, cut
            assert ctx.cache_size() == LRU_LIMIT
            assert export_of(ctx) == exp, cut             # an export refreshes nothing
            if cut in (None, 48):
                assert ctx.encode_chunks(d, offs, lens, semantics=XCG_SEM_STREAM) == exp_enc, cut
                assert export_of(ctx) == exp_after, cut
            ctx.status()
        finally:
            ctx.close()


@pytest.mark.parametrize('name', ['lru_set300', 'lru_limit1'])
def test_bounded_learn_past_the_limit(oracle, name):
    """n many times the limit in one call, between single-segment calls that
    share the LRU clock."""
    from wanproxy_amd.xcgpu import Context
    _, limit, _, batch = next(c for c in cb.cases() if c[0] == name)
    c = oracle.cache_new(limit * SEG)
    oracle_learn(oracle, c, batch[:5] + batch + batch[7:9])
    exp = oracle_export(oracle, c)
    oracle.cache_free(c)
    ctx = Context(0, memory_cache_limit=limit * SEG)
    try:
        for s in batch[:5]:
            ctx.cache_enter(oracle.hash(s), s)
        learn_at(ctx, batch, 3)
        for s in batch[7:9]:
            ctx.cache_enter(oracle.hash(s), s)
        assert export_of(ctx) == exp
    finally:
        ctx.close()


# -------------------------------------------------------------------- capacity

def test_capacity_is_all_or_nothing():
    from wanproxy_amd.xcgpu import Context, XCGError, lib
    segs = [cb.rnd([0xCA9, k], SEG) for k in range(24)]
    ctx = Context(0, cache_segments=16)
    try:
        with pytest.raises(XCGError, match=str(XCG_EOVERFLOW)):
            learn_at(ctx, segs[:17])                                # 17 distinct segments
        assert ctx.cache_size() == 0 and export_of(ctx) == ([], [])
        learn_at(ctx, segs[:5])
        before = export_of(ctx)
        with pytest.raises(XCGError, match=str(XCG_EOVERFLOW)):
            learn_at(ctx, segs[3:5] + segs[7:24] + segs[:2])      # 17 distinct, 12 of them new
        assert ctx.cache_size() == 5 and export_of(ctx) == before
        learn_at(ctx, segs[:16] + segs[2:9] + [segs[15]], 3)        # 16 distinct and duplicates
        assert ctx.cache_size() == 16
        hs, _ = ctx.cache_export()
        with pytest.raises(XCGError, match=str(XCG_EOVERFLOW)):
            learn_at(ctx, [segs[16]])
        assert ctx.cache_size() == 16
        # an export with room for one segment too few
        buf = np.full(15 * SEG, 0xAA, np.uint8)
        hb = np.full(15, 0xAAAAAAAAAAAAAAAA, np.uint64)
        cnt = C.c_uint64(0)
        rc = lib().xcg_cache_export_host(ctx.h, buf.ctypes.data, hb.ctypes.data, 15, C.byref(cnt))
        assert rc == XCG_EOVERFLOW and cnt.value == 16
        assert (buf == 0xAA).all() and (hb == 0xAAAAAAAAAAAAAAAA).all()
        import torch
        dbuf = torch.full((15 * SEG,), 0xAA, dtype=torch.uint8, device='cuda:0')
        rc = lib().xcg_cache_export(ctx.h, C.c_void_p(dbuf.data_ptr()), None, 15, C.byref(cnt), None)
        torch.cuda.synchronize()
        assert rc == XCG_EOVERFLOW and cnt.value == 16 and bool((dbuf == 0xAA).all())
        ctx.status()
    finally:
        ctx.close()


# ------------------------------------------------------------------ round trip

@pytest.mark.parametrize('limit', [0, LRU_LIMIT], ids=['unbounded', 'bounded'])
def test_export_learn_round_trip(oracle, limit):
    """Learning A's export, in export order, into a fresh B of the same kind
    and limit reproduces the cache: byte-identical exports, and the same
    behaviour afterwards."""
    from wanproxy_amd.xcgpu import XCG_SEM_STREAM, Context
    kw = dict(memory_cache_limit=limit * SEG) if limit else dict(cache_segments=1024)
    a, b = Context(0, **kw), Context(0, **kw)
    try:
        batch = cb.lru_batch() if limit else cb.segment_set(300, 300)
        if limit:
            learn_at(a, cb.lru_earlier())
        learn_at(a, batch, 1)
        hs, segs = a.cache_export()
        assert len(hs) == (limit or len({oracle.hash(s) for s in batch}))
        got = b.cache_learn(segs)
        assert (got == hs).all()
        hb, sb = b.cache_export()
        assert (hb == hs).all() and sb == segs
        d = cb.later_stream(batch)
        offs, lens = chunks8k(d)
        assert a.encode_chunks(d, offs, lens, semantics=XCG_SEM_STREAM) == \
            b.encode_chunks(d, offs, lens, semantics=XCG_SEM_STREAM)
        assert a.cache_export()[1] == b.cache_export()[1]
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------ pair

def test_pair_context_is_refused(oracle):
    import torch
    from wanproxy_amd.xcgpu import Context, lib
    ctx = Context(0, memory_cache_limit=PAIR_LIMIT * SEG, disk_bytes=PAIR_DISK)
    try:
        seg = cb.rnd([0x9A1, 0], SEG)
        ctx.cache_enter(oracle.hash(seg), seg)
        st = ctx.pair_stats()
        assert st[0] == 1
        d = torch.zeros(4 * SEG, dtype=torch.uint8, device='cuda:0')
        h = np.zeros(4 * SEG, np.uint8)
        cnt = C.c_uint64(7)
        L = lib()
        assert L.xcg_cache_learn_batch(ctx.h, C.c_void_p(d.data_ptr()), 4, None, None) == XCG_ENOTSUP
        assert L.xcg_cache_learn_host(ctx.h, h.ctypes.data, 4, None) == XCG_ENOTSUP
        assert L.xcg_cache_export(ctx.h, C.c_void_p(d.data_ptr()), None, 4, C.byref(cnt), None) == XCG_ENOTSUP
        assert L.xcg_cache_export_host(ctx.h, h.ctypes.data, None, 4, C.byref(cnt)) == XCG_ENOTSUP
        assert ctx.pair_stats() == st
    finally:
        ctx.close()


# ---------------------------------------------------------------------- memory

def test_memory_returns_to_its_earlier_values():
    from wanproxy_amd.xcgpu import Context
    segs = cb.segment_set(65, 65)
    warm = Context(0, cache_segments=64)                          # (the runtime's pools exist before the count)
    learn_at(warm, segs[:3])
    warm.close()
    live0 = mem_live()
    for kw in (dict(cache_segments=256), dict(memory_cache_limit=LRU_LIMIT * SEG)):
        ctx = Context(0, **kw)
        learn_at(ctx, segs[:1])
        held = mem_live()
        learn_at(ctx, segs, 3)
        ctx.cache_size()                                          # (the context's work is done)
        assert mem_live() == held
        ctx.cache_export()
        ctx.cache_learn(b''.join(segs[:9]))
        assert mem_live() == held
        ctx.close()
        assert mem_live() == live0
