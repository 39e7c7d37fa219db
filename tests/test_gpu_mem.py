"""Nothing leaks: every GPU buffer the library allocates goes through one owner
per host object (wanproxy_amd/csrc/xcg_devmem.h), and xcg_debug_mem_live counts
what is held.  Make every kind of object, drive each through the calls that
allocate and regrow its buffers (round trips checked, so the code still
works), destroy everything: the four counts are back where they started --
twice in one process."""
import ctypes as C
import gc
import importlib.util
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_pair_golden', os.path.join(HERE, 'golden/make_pair_golden.py'))
mpg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mpg)

SEG = 2048


def mem_live():
    """(device bytes, pinned bytes, device allocations, pinned allocations)"""
    from wanproxy_amd.xcgpu import lib
    gc.collect()
    out = (C.c_uint64 * 4)()
    lib().xcg_debug_mem_live.restype = None
    lib().xcg_debug_mem_live.argtypes = [C.c_void_p]
    lib().xcg_debug_mem_live(out)
    return tuple(int(v) for v in out)


def encode_call(ctx, data):
    """One xcg_encode_call (the context's kept staging); the encoded bytes."""
    from wanproxy_amd.xcgpu import _check, encode_bound, lib
    cap = encode_bound(len(data))
    out = np.zeros(cap, np.uint8)
    ol = np.zeros(1, np.uint64)
    dh, dp, nd = np.zeros(64, np.uint64), np.zeros(64, np.uint32), np.zeros(1, np.uint32)
    rh, rk, ri, nr = np.zeros(256, np.uint64), np.zeros(256, np.uint32), np.zeros(256, np.uint32), np.zeros(1, np.uint32)
    f = lib().xcg_encode_call
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                  C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    _check(f(ctx.h, data, len(data), out.ctypes.data, cap, ol.ctypes.data, dh.ctypes.data, dp.ctypes.data, dh.size,
             nd.ctypes.data, rh.ctypes.data, rk.ctypes.data, ri.ctypes.data, rh.size, nr.ctypes.data))
    return out[:int(ol[0])].tobytes()


def codec_sequence(oracle, enc, dec, data, whole):
    """The calls that allocate and regrow a codec context's buffers, on an
    encoder context and the decoder context that mirrors it (whole: each
    batch is decoded in one call)."""
    from wanproxy_amd import synth
    from wanproxy_amd.xcgpu import XCG_SEM_STREAM
    small, big, call = data[:2 * 4096], data[8192:8192 + 8 * 65536], data[-8192:]
    # 2 chunks of 4 KiB (the screen's queues), then 8 of 64 KiB (every scratch regrows)
    for part, chunk in ((small, 4096), (big, 65536)):
        offs, lens = synth.chunks_of(part, chunk)
        e = enc.encode_chunks(part, offs, lens, semantics=XCG_SEM_STREAM)
        # (a limited cache decodes what one batch may enter: a 64 KiB chunk's 32 segments per call)
        calls = [e] if whole else [[x] for x in e]
        outs = []
        for call_chunks in calls:
            o, st, _, unk = dec.decode_chunks(call_chunks)
            assert not (st != 0).any() and not unk
            outs += o
        assert b''.join(outs) == part
    # one host call each way (the kept staging, the zero-copy block)
    st, out, cons, unk, _ = dec.decode_call(encode_call(enc, call))
    assert (st, out, unk) == (0, call, [])
    # single-segment host calls (their short-lived blocks)
    seg = bytes(np.random.default_rng(7).integers(0, 256, SEG, dtype=np.uint8))
    h = oracle.hash(seg)
    enc.cache_enter(h, seg)
    assert enc.cache_lookup(h) == seg


def zlib_sequence(data):
    """One 1 KiB and one 64 KiB consume on every zlib object (and the empty
    consume that ends the stream, so that it can be checked)."""
    from wanproxy_amd.zpipe import DeflatePipes, InflatePipes
    parts = [data[:1024], data[4096:4096 + 65536], b'']
    made = {}
    for level in (0, 1, 6):
        z = DeflatePipes(level=level, nstreams=2)
        made[level] = [z.consume_many([(1, p)])[0] for p in parts]
        z.close()
        assert zlib.decompress(b''.join(made[level])) == b''.join(parts), level
    zi = InflatePipes(nstreams=2)
    got = [zi.consume_many([(0, made[0][i]), (1, made[6][i])]) for i in range(3)]   # stream 0 stored, 1 level 6
    zi.close()
    for s in range(2):
        assert b''.join(g[s][0] for g in got) == b''.join(parts) and all(g[s][1] >= 0 for g in got), s


def one_round(oracle, data):
    from wanproxy_amd.xcgpu import Context, Disk, Window
    limit, disk_bytes = 64 * SEG, mpg.disk_bytes(1)
    made = []

    def keep(x):
        made.append(x)
        return x
    # unbounded (1,024 segments), bounded (64 segments), pair (64 segments over the smallest disk)
    codecs = [(keep(Context(0, cache_segments=1024)), keep(Context(0, cache_segments=1024))),
              (keep(Context(0, memory_cache_limit=limit)), keep(Context(0, memory_cache_limit=limit)))]
    K = Disk(disk_bytes)
    front = keep(Context(0, memory_cache_limit=limit, disk=K))
    second = keep(Context(0, memory_cache_limit=limit, disk=K))      # a second front on that disk
    codecs.append((front, keep(Context(0, memory_cache_limit=limit, disk_bytes=disk_bytes))))
    extra = keep(Window(codecs[0][1]))                                # an extra window
    held = mem_live()
    for k, (enc, dec) in enumerate(codecs):
        print('codec', k, flush=True)
        codec_sequence(oracle, enc, dec, data, whole=k == 0)
    outs, st, _, unk = codecs[0][1].decode_chunks(
        codecs[0][0].encode_chunks(data[:4096], np.array([0]), np.array([4096]), semantics=1), window=extra)
    assert outs == [data[:4096]] and not (st != 0).any() and not unk
    seg = data[:SEG]
    second.cache_enter(oracle.hash(seg), seg)
    assert second.cache_lookup(oracle.hash(seg)) == seg
    zlib_sequence(data)
    grown = mem_live()
    for x in reversed(made):
        x.close()
    K.close()
    return held, grown


def test_everything_is_freed(oracle):
    from wanproxy_amd import synth
    data = synth.stream(0xA110C, 8192 + 8 * 65536 + 8192, 50, 2)
    start = mem_live()
    for rnd in range(2):
        held, grown = one_round(oracle, data)
        print('round', rnd, 'start', start, 'created', held, 'after the calls', grown, 'end', mem_live(), flush=True)
        # (the counters do count: creating holds memory, the calls grow it)
        assert held[0] > start[0] and held[2] > start[2]
        assert all(g > h for g, h in zip(grown, held))
        assert mem_live() == start, rnd
