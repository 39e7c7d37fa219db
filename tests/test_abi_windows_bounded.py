"""xcg_decode_batch_windows_bounded / xcg_decode_host_windows_bounded are part of
the C ABI: declared in include/xcgpu.h with the arguments of their unbounded
counterparts, exported by libxcgpu.so, and their null-argument returns need no
device."""
import ctypes as C
import os
import re

from test_abi import ROOT, declared_functions

PAIRS = (('xcg_decode_batch_windows_bounded', 'xcg_decode_batch_windows'),
         ('xcg_decode_host_windows_bounded', 'xcg_decode_host_windows'))


def prototype(name):
    """(return type, [parameter declarations]) of `name` in the header."""
    src = open(os.path.join(ROOT, 'include/xcgpu.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'(\w[\w \*]*?)\b%s\s*\(([^)]*)\)\s*;' % name, src)
    assert m, name
    return m.group(1).strip(), [' '.join(p.split()) for p in m.group(2).split(',')]


def test_header_declares_them_with_the_unbounded_calls_arguments():
    names = declared_functions()
    for new, old in PAIRS:
        assert new in names
        assert prototype(new) == prototype(old), new
    ret, params = prototype('xcg_decode_batch_windows_bounded')
    assert ret == 'int' and len(params) == 18 and params[0] == 'xcg_ctx *ctx' and params[-1] == 'void *stream'
    assert len(prototype('xcg_decode_host_windows_bounded')[1]) == 17


def library():
    from wanproxy_amd.build import OUT, build_lib
    if not os.path.exists(OUT):
        build_lib()
    import torch  # noqa: F401  (shares its HIP runtime with the library)
    return C.CDLL(OUT)


def test_library_exports_them():
    lib = library()
    assert [new for new, _ in PAIRS if not hasattr(lib, new)] == []


def test_null_context_is_invalid_whatever_n():
    lib = library()
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    dev = lib.xcg_decode_batch_windows_bounded
    dev.argtypes = [vp, vp, vp, vp, u32, u32, vp, u32, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp]
    dev.restype = C.c_int
    host = lib.xcg_decode_host_windows_bounded
    host.argtypes = [vp, vp, u64, vp, vp, u32, vp, u32, vp, vp, u64, vp, vp, vp, vp, vp, vp]
    host.restype = C.c_int
    stop, total = u32(77), u64(77)
    for n in (0, 2):
        assert dev(None, None, None, None, n, 0, None, 0, None, None, 0, None, None, None, None, C.byref(stop),
                   C.byref(total), None) == -22
        assert host(None, None, 0, None, None, n, None, 0, None, None, 0, None, None, None, None, C.byref(stop),
                    C.byref(total)) == -22
    assert (stop.value, total.value) == (77, 77)            # (refused before anything is written)
