"""xcg_encode_call and the inspection calls report the same rows.  A call's
declarations (hash, input offset) and, on a bounded or pair cache, its cache
references in stream order (hash, kind, index) come back from xcg_encode_call
itself and, afterwards, from xcg_last_declarations / xcg_last_references on
chunk 0: both unpack the same device rows (wanproxy_amd/csrc/xcg_api_host.h),
so they agree element for element, truncate alike and leave the entries past
the cap alone.  Two calls on a bounded, a pair and an unbounded context:
s0 s1 s2 s3 s4 + 100 tail bytes, then s4 s0 s5 s2 (2,048-byte random segments,
s5 new)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_pair_golden', os.path.join(HERE, 'golden/make_pair_golden.py'))
mpg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mpg)

SEG = 2048
LIMIT = 16 * SEG
XCG_ENOTSUP = -95
XCG_NO_REFERENCES = 0xFFFFFFFF
SENTINEL64, SENTINEL32 = 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5


def calls():
    rng = np.random.default_rng(0xCA11)
    s = [bytes(rng.integers(0, 256, SEG, dtype=np.uint8)) for _ in range(6)]
    tail = bytes(rng.integers(0, 256, 100, dtype=np.uint8))
    return [s[0] + s[1] + s[2] + s[3] + s[4] + tail, s[4] + s[0] + s[5] + s[2]]


def encode_call(ctx, data):
    """One xcg_encode_call: (declarations [(hash, pos)], references [(hash, kind, idx)] or None)."""
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
    n, m = int(nd[0]), int(nr[0])
    assert n <= dh.size
    decls = [(int(dh[i]), int(dp[i])) for i in range(n)]
    if m == XCG_NO_REFERENCES:
        return decls, None
    assert m <= rh.size
    return decls, [(int(rh[i]), int(rk[i]), int(ri[i])) for i in range(m)]


def last_declarations(ctx, cap):
    """xcg_last_declarations(c, 0, ...) into sentinel-filled arrays of cap + 1: (status, count, hashes, positions)."""
    from wanproxy_amd.xcgpu import lib
    h, p = np.full(cap + 1, SENTINEL64, np.uint64), np.full(cap + 1, SENTINEL32, np.uint32)
    cnt = np.zeros(1, np.uint32)
    f = lib().xcg_last_declarations
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    rc = f(ctx.h, 0, h.ctypes.data, p.ctypes.data, cap, cnt.ctypes.data)
    return rc, int(cnt[0]), h, p


def last_references(ctx, cap):
    """xcg_last_references(c, 0, ...) likewise: (status, count, hashes, kinds, indices)."""
    from wanproxy_amd.xcgpu import lib
    h, k, r = (np.full(cap + 1, SENTINEL64, np.uint64), np.full(cap + 1, SENTINEL32, np.uint32),
               np.full(cap + 1, SENTINEL32, np.uint32))
    cnt = np.zeros(1, np.uint32)
    f = lib().xcg_last_references
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    rc = f(ctx.h, 0, h.ctypes.data, k.ctypes.data, r.ctypes.data, cap, cnt.ctypes.data)
    return rc, int(cnt[0]), h, k, r


def check_declarations(ctx, decls):
    """Agreement at a cap above the count; truncation at cap 1.  True if the truncation was exercised."""
    rc, n, h, p = last_declarations(ctx, 64)
    assert rc == 0 and n == len(decls)
    assert [(int(h[i]), int(p[i])) for i in range(n)] == decls
    assert int(h[n]) == SENTINEL64 and int(p[n]) == SENTINEL32
    if n < 2:
        return False
    rc, n1, h, p = last_declarations(ctx, 1)
    assert rc == 0 and n1 == n                                           # the full count
    assert (int(h[0]), int(p[0])) == decls[0]
    assert int(h[1]) == SENTINEL64 and int(p[1]) == SENTINEL32           # untouched
    return True


def check_references(ctx, refs):
    rc, n, h, k, r = last_references(ctx, 256)
    assert rc == 0 and n == len(refs)
    assert [(int(h[i]), int(k[i]), int(r[i])) for i in range(n)] == refs
    assert int(h[n]) == SENTINEL64 and int(k[n]) == SENTINEL32 and int(r[n]) == SENTINEL32
    if n < 2:
        return False
    rc, n1, h, k, r = last_references(ctx, 1)
    assert rc == 0 and n1 == n
    assert (int(h[0]), int(k[0]), int(r[0])) == refs[0]
    assert int(h[1]) == SENTINEL64 and int(k[1]) == SENTINEL32 and int(r[1]) == SENTINEL32
    return True


def make_ctx(kind):
    from wanproxy_amd.xcgpu import Context
    if kind == 'bounded':
        return Context(0, memory_cache_limit=LIMIT)
    if kind == 'pair':
        return Context(0, memory_cache_limit=LIMIT, disk_bytes=mpg.disk_bytes(1))
    return Context(0, cache_segments=1024)


@pytest.mark.parametrize('kind', ['bounded', 'pair'])
def test_call_rows_agree_with_references(kind):
    ctx = make_ctx(kind)
    try:
        truncated_d = truncated_r = False
        for i, data in enumerate(calls()):
            decls, refs = encode_call(ctx, data)
            print(kind, 'call', i + 1, 'declarations', [(hex(h), p) for h, p in decls], flush=True)
            print(kind, 'call', i + 1, 'references', [(hex(h), k, r) for h, k, r in refs], flush=True)
            assert refs is not None
            truncated_d |= check_declarations(ctx, decls)
            truncated_r |= check_references(ctx, refs)
        # call 1 declares s0..s4; call 2 declares s5 alone (kind 0, an enter) among lookups that hit entries
        # cached by call 1 (kind 2: kind 1 is a hit on a declaration of the same call, and no segment of
        # call 2 repeats within it)
        assert truncated_d and truncated_r
        assert [p for _, p in decls] == [2 * SEG]
        kinds = [k for _, k, _ in refs]
        assert 0 in kinds and 2 in kinds, kinds
    finally:
        ctx.close()


def test_call_rows_unbounded():
    ctx = make_ctx('unbounded')
    try:
        truncated = False
        for i, data in enumerate(calls()):
            decls, refs = encode_call(ctx, data)
            print('unbounded call', i + 1, 'declarations', [(hex(h), p) for h, p in decls], flush=True)
            assert refs is None                                          # *h_nref == XCG_NO_REFERENCES
            assert last_references(ctx, 4)[0] == XCG_ENOTSUP
            truncated |= check_declarations(ctx, decls)
        assert truncated
        assert [p for _, p in decls] == [2 * SEG]
    finally:
        ctx.close()
