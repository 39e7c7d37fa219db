"""The bulk cache learn / export entry points are part of the C ABI: declared
in include/xcgpu.h and exported by libxcgpu.so (no GPU needed)."""
import ctypes as C
import os

from test_abi import declared_functions

BULK = ('xcg_cache_learn_batch', 'xcg_cache_learn_host', 'xcg_cache_export', 'xcg_cache_export_host')


def test_header_declares_the_bulk_calls():
    names = declared_functions()
    assert [n for n in BULK if n not in names] == []


def test_library_exports_the_bulk_calls():
    from wanproxy_amd.build import OUT, build_lib
    if not os.path.exists(OUT):
        build_lib()
    import torch  # noqa: F401  (shares its HIP runtime with the library)
    lib = C.CDLL(OUT)
    assert [n for n in BULK if not hasattr(lib, n)] == []
