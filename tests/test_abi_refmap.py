"""The encoder refmap entry points are part of the C ABI: declared in
include/xcgpu.h and exported by libxcgpu.so (no GPU needed)."""
import ctypes as C
import os
import re

from test_abi import ROOT, declared_functions

REFMAP = ('xcg_encode_refmap_batch', 'xcg_encode_host_refmap')


def test_header_declares_the_refmap_calls():
    names = declared_functions()
    assert [n for n in REFMAP if n not in names] == []
    src = open(os.path.join(ROOT, 'include/xcgpu.h')).read()
    assert re.search(r'#define\s+XCG_REFMAP_MAX\s+256u', src)


def test_library_exports_the_refmap_calls():
    from wanproxy_amd.build import OUT, build_lib
    if not os.path.exists(OUT):
        build_lib()
    import torch  # noqa: F401  (shares its HIP runtime with the library)
    lib = C.CDLL(OUT)
    assert [n for n in REFMAP if not hasattr(lib, n)] == []


def test_python_binding_knows_the_limit():
    from wanproxy_amd import xcgpu
    assert xcgpu.XCG_REFMAP_MAX == 256
    assert hasattr(xcgpu.Context, 'encode_refmap_device') and hasattr(xcgpu.Context, 'encode_chunks_refmap')
