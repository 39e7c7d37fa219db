"""ctypes binding of libxcgpu.so (include/xcgpu.h) plus a host-side mirror of
the reference's XCodec encoder interface.

The product path is the HIP library; this module only moves buffers (torch is
used for device memory and streams) and never falls back to a CPU codec: if
the library or a GPU is missing, every entry point raises.

Reference interface mirrored (wanproxy tree):
  XCodecEncoder(XCodecCache*) / encode(Buffer*, Buffer*)   xcodec/xcodec_encoder.h:40-43
  XCodecMemoryCache / TackNullCache / out_of_band()         xcodec/xcodec_cache.h:245-365,
                                                            programs/tack/tack.cc:70-101
  XCodecHash::hash / mix                                    xcodec/xcodec_hash.h:155-174
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# XCGPU_LIB selects a diagnostic build of the same library (scripts/dev).
LIB_PATH = os.environ.get('XCGPU_LIB') or os.path.join(HERE, 'libxcgpu.so')
SEG = 2048

XCG_FLAG_OOB = 0x1
XCG_FLAG_NULLCACHE = 0x2
XCG_SEM_INDEPENDENT = 0
XCG_SEM_STREAM = 1
XCG_EOVERFLOW = -75
XCG_REFMAP_MAX = 256    # entries of one encode() call's refmap (what 512 KiB of input can reference)
XCG_CHUNK_NOROOM = 4   # per-chunk status of xcg_decode_batch_independent: the output slot is too small

_lib = None


XCG_ENOENT = -2


class XCGError(RuntimeError):
    pass


class _PipeOut(C.Structure):
    _fields_ = [('to_peer', C.c_void_p), ('to_peer_len', C.c_uint64), ('to_local', C.c_void_p),
                ('to_local_len', C.c_uint64), ('local_eos', C.c_int), ('peer_eos', C.c_int)]

    def peer(self) -> bytes:
        return C.string_at(self.to_peer, self.to_peer_len) if self.to_peer_len else b''

    def local(self) -> bytes:
        return C.string_at(self.to_local, self.to_local_len) if self.to_local_len else b''


def lib():
    """Load libxcgpu.so (after torch, so both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  -- load torch's libamdhip64 first
    if not os.path.exists(LIB_PATH):
        raise XCGError(f'{LIB_PATH} missing: run `python -c "import __graft_entry__ as g; g.build()"`')
    L = C.CDLL(LIB_PATH)
    vp, u8p, u32p, u64p = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p
    L.xcg_version.restype = C.c_char_p
    L.xcg_strerror.restype = C.c_char_p
    L.xcg_strerror.argtypes = [C.c_int]
    L.xcg_encode_bound.restype = C.c_uint64
    L.xcg_encode_bound.argtypes = [C.c_uint32]
    L.xcg_ctx_create.argtypes = [C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
    L.xcg_ctx_create.restype = C.c_int
    L.xcg_ctx_create_ex.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.POINTER(C.c_void_p)]
    L.xcg_ctx_create_ex.restype = C.c_int
    L.xcg_ctx_create_bounded.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.POINTER(C.c_void_p)]
    L.xcg_ctx_create_bounded.restype = C.c_int
    L.xcg_ctx_create_pair.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]
    L.xcg_ctx_create_pair.restype = C.c_int
    L.xcg_disk_create.argtypes = [C.c_uint64, C.POINTER(C.c_void_p)]
    L.xcg_disk_create.restype = C.c_int
    L.xcg_disk_destroy.argtypes = [vp]
    L.xcg_disk_destroy.restype = None
    L.xcg_disk_stats.argtypes = [vp, vp]
    L.xcg_disk_stats.restype = C.c_int
    L.xcg_disk_create_ex.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
    L.xcg_disk_create_ex.restype = C.c_int
    L.xcg_disk_tier.argtypes = [vp]
    L.xcg_disk_tier.restype = C.c_int
    L.xcg_disk_open.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
    L.xcg_disk_open.restype = C.c_int
    L.xcg_disk_save.argtypes = [vp, C.c_char_p]
    L.xcg_disk_save.restype = C.c_int
    L.xcg_ctx_create_pair_uuid.argtypes = [C.c_int, C.c_uint32, C.c_uint64, vp, C.c_char_p, C.POINTER(C.c_void_p)]
    L.xcg_ctx_create_pair_uuid.restype = C.c_int
    L.xcg_ctx_create_pair_on.argtypes = [C.c_int, C.c_uint32, C.c_uint64, vp, C.POINTER(C.c_void_p)]
    L.xcg_ctx_create_pair_on.restype = C.c_int
    L.xcg_ctx_create_pair_xuid.argtypes = [C.c_int, C.c_uint32, C.c_uint64, vp, C.c_char_p, C.c_int,
                                           C.POINTER(C.c_void_p)]
    L.xcg_ctx_create_pair_xuid.restype = C.c_int
    L.xcg_disk_open_fd.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
    L.xcg_disk_open_fd.restype = C.c_int
    L.xcg_disk_head.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.xcg_disk_head.restype = C.c_int
    L.xcg_pair_xuid.argtypes = [vp]
    L.xcg_pair_xuid.restype = C.c_int
    L.xcg_pair_stats.argtypes = [vp, vp]
    L.xcg_pair_stats.restype = C.c_int
    L.xcg_ctx_flags.argtypes = [vp, vp]
    L.xcg_ctx_flags.restype = C.c_int
    L.xcg_cache_size.argtypes = [vp]
    L.xcg_cache_size.restype = C.c_uint64
    L.xcg_cache_clear.argtypes = [vp]
    L.xcg_cache_clear.restype = C.c_int
    L.xcg_cache_learn_batch.argtypes = [vp, u8p, C.c_uint64, u64p, vp]
    L.xcg_cache_learn_batch.restype = C.c_int
    L.xcg_cache_learn_host.argtypes = [vp, u8p, C.c_uint64, u64p]
    L.xcg_cache_learn_host.restype = C.c_int
    L.xcg_cache_export.argtypes = [vp, u8p, u64p, C.c_uint64, C.POINTER(C.c_uint64), vp]
    L.xcg_cache_export.restype = C.c_int
    L.xcg_cache_export_host.argtypes = [vp, u8p, u64p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.xcg_cache_export_host.restype = C.c_int
    L.xcg_last_rounds.argtypes = [vp]
    L.xcg_last_rounds.restype = C.c_int
    L.xcg_ctx_destroy.argtypes = [vp]
    L.xcg_ctx_status.argtypes = [vp]
    L.xcg_ctx_status.restype = C.c_int
    L.xcg_encode_batch.argtypes = [vp, C.c_int, u8p, u64p, u32p, C.c_uint32, C.c_uint32, u8p, u64p, u64p, u32p, vp]
    L.xcg_encode_batch.restype = C.c_int
    L.xcg_encode_host.argtypes = [vp, C.c_int, u8p, C.c_uint64, u64p, u32p, C.c_uint32, u8p, C.c_uint64, u64p, u64p]
    L.xcg_encode_host.restype = C.c_int
    if hasattr(L, 'xcg_encode_refmap_batch'):   # (an XCGPU_LIB build from before the refmap: calling them raises)
        L.xcg_encode_refmap_batch.argtypes = [vp, u8p, u64p, u64p, C.c_uint32, C.c_uint32, C.c_uint32, u64p, u32p,
                                              C.c_uint32, u32p, u64p, vp]
        L.xcg_encode_refmap_batch.restype = C.c_int
        L.xcg_encode_host_refmap.argtypes = [vp, C.c_int, u8p, C.c_uint64, u64p, u32p, C.c_uint32, u8p, C.c_uint64,
                                             u64p, u64p, u64p, u32p, C.c_uint32, u32p]
        L.xcg_encode_host_refmap.restype = C.c_int
    L.xcg_decode_batch.argtypes = [vp, u8p, u64p, u32p, C.c_uint32, C.c_uint32, u8p, C.c_uint64, u64p, u64p, vp, u64p,
                                   u64p, C.c_uint32, vp, u64p, vp]
    L.xcg_decode_batch.restype = C.c_int
    if hasattr(L, 'xcg_decode_batch_windows'):   # (an XCGPU_LIB build from before the windows call: calling it raises)
        L.xcg_decode_batch_windows.argtypes = [vp, u8p, u64p, u32p, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, u8p,
                                               C.c_uint64, u64p, u64p, vp, u64p, vp, vp, vp]
        L.xcg_decode_batch_windows.restype = C.c_int
        L.xcg_decode_host_windows.argtypes = [vp, u8p, C.c_uint64, u64p, u32p, C.c_uint32, vp, C.c_uint32, vp, u8p,
                                              C.c_uint64, u64p, u64p, vp, u64p, vp, vp]
        L.xcg_decode_host_windows.restype = C.c_int
    if hasattr(L, 'xcg_decode_batch_windows_bounded'):   # (likewise: a build from before the bounded windows call)
        L.xcg_decode_batch_windows_bounded.argtypes = L.xcg_decode_batch_windows.argtypes
        L.xcg_decode_batch_windows_bounded.restype = C.c_int
        L.xcg_decode_host_windows_bounded.argtypes = L.xcg_decode_host_windows.argtypes
        L.xcg_decode_host_windows_bounded.restype = C.c_int
    L.xcg_decode_batch_independent.argtypes = [vp, u8p, u64p, u32p, C.c_uint32, C.c_uint32, u8p, u64p, u64p, u64p, vp,
                                               u64p, u64p, vp]
    L.xcg_decode_batch_independent.restype = C.c_int
    L.xcg_encode_batch_grouped.argtypes = [vp, u8p, u64p, u32p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, u8p, u64p,
                                           u64p, u32p, vp]
    L.xcg_encode_batch_grouped.restype = C.c_int
    L.xcg_decode_batch_grouped.argtypes = [vp, u8p, u64p, u32p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, u8p, u64p,
                                           u64p, u64p, vp, u64p, u64p, vp]
    L.xcg_decode_batch_grouped.restype = C.c_int
    L.xcg_window_create.argtypes = [vp, C.POINTER(C.c_void_p)]
    L.xcg_window_create.restype = C.c_int
    L.xcg_window_destroy.argtypes = [vp]
    L.xcg_window_destroy.restype = None
    L.xcg_decode_set_window.argtypes = [vp, vp]
    L.xcg_decode_set_window.restype = C.c_int
    L.xcg_decode_call.argtypes = [vp, C.c_char_p, C.c_uint32, vp, C.c_uint64, vp, vp, vp, vp, C.c_uint32, vp, vp,
                                  C.c_uint32, vp]
    L.xcg_decode_call.restype = C.c_int
    L.xcg_pack_outputs.argtypes = [vp, u8p, u64p, u64p, C.c_uint32, u8p, u64p, u64p, vp]
    L.xcg_pack_outputs.restype = C.c_int
    L.xcg_window_hashes.argtypes = [vp, u8p, C.c_uint64, u64p, vp]
    L.xcg_window_hashes.restype = C.c_int
    L.xcg_segment_hashes.argtypes = [vp, u8p, C.c_uint64, u64p, vp]
    L.xcg_segment_hashes.restype = C.c_int
    L.xcg_pipe_create.argtypes = [vp, vp, C.c_char_p, C.POINTER(C.c_void_p)]
    L.xcg_pipe_create.restype = C.c_int
    L.xcg_pipe_destroy.argtypes = [vp]
    L.xcg_pipe_destroy.restype = None
    L.xcg_pipe_create_connect.argtypes = [vp, vp, C.c_char_p, C.POINTER(C.c_void_p)]
    L.xcg_pipe_create_connect.restype = C.c_int
    L.xcg_pipe_decoder_ctx.argtypes = [vp]
    L.xcg_pipe_decoder_ctx.restype = vp
    L.xcg_ctx_connect.argtypes = [vp, C.c_char_p, C.POINTER(C.c_void_p)]
    L.xcg_ctx_connect.restype = C.c_int
    L.xcg_ctx_register.argtypes = [vp, C.c_char_p]
    L.xcg_ctx_register.restype = C.c_int
    L.xcg_ctx_lookup.argtypes = [C.c_char_p]
    L.xcg_ctx_lookup.restype = vp
    L.xcg_connect_registry_clear.argtypes = []
    L.xcg_connect_registry_clear.restype = None
    L.xcg_pipe_encoder_consume.argtypes = [vp, C.c_char_p, C.c_uint64, C.POINTER(_PipeOut)]
    L.xcg_pipe_encoder_consume.restype = C.c_int
    L.xcg_pipe_encoder_consume_many.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_char_p), C.POINTER(C.c_uint64),
                                                C.c_uint32, C.POINTER(_PipeOut)]
    L.xcg_pipe_encoder_consume_many.restype = C.c_int
    L.xcg_pipe_decoder_consume.argtypes = [vp, C.c_char_p, C.c_uint64, C.POINTER(_PipeOut)]
    if hasattr(L, 'xcg_pipe_decoder_consume_many'):
        L.xcg_pipe_decoder_consume_many.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_char_p),
                                                    C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(_PipeOut),
                                                    C.POINTER(C.c_int)]
        L.xcg_pipe_decoder_consume_many.restype = C.c_int
    L.xcg_pipe_decoder_consume.restype = C.c_int
    if hasattr(L, 'xcg_decode_call_many'):
        L.xcg_decode_call_many.argtypes = [vp, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.xcg_decode_call_many.restype = C.c_int
        L.xcg_debug_decode_call_many.argtypes = [C.POINTER(C.c_uint64)]
        L.xcg_debug_decode_call_many.restype = None
        L.xcg_pipe_debug_decode_peers.argtypes = [C.POINTER(C.c_uint64)]
        L.xcg_pipe_debug_decode_peers.restype = None
    L.xcg_pipe_pending_frames.argtypes = [vp]
    L.xcg_pipe_pending_frames.restype = C.c_uint32
    if hasattr(L, 'xcg_codec_create'):   # (an XCGPU_LIB build from before the codec layer: calling them raises)
        many = [C.POINTER(C.c_void_p), C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(_PipeOut),
                C.POINTER(C.c_int)]
        L.xcg_codec_create.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
        L.xcg_codec_create.restype = C.c_int
        L.xcg_codec_destroy.argtypes = [vp]
        L.xcg_codec_destroy.restype = None
        L.xcg_codec_pipe_create.argtypes = [vp, C.c_char_p, C.POINTER(C.c_void_p)]
        L.xcg_codec_pipe_create.restype = C.c_int
        L.xcg_codec_pipe_destroy.argtypes = [vp]
        L.xcg_codec_pipe_destroy.restype = None
        L.xcg_codec_pipe_pair.argtypes = [vp]
        L.xcg_codec_pipe_pair.restype = vp
        L.xcg_codec_send_many.argtypes = many
        L.xcg_codec_send_many.restype = C.c_int
        L.xcg_codec_receive_many.argtypes = many
        L.xcg_codec_receive_many.restype = C.c_int
        L.xcg_codec_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.xcg_codec_stats.restype = C.c_int
        L.xcg_debug_set_codec_fused.argtypes = [C.c_int]
        L.xcg_debug_set_codec_fused.restype = C.c_int
        L.xcg_codec_debug_counts.argtypes = [C.POINTER(C.c_uint64)]
        L.xcg_codec_debug_counts.restype = None
        L.xcg_gather_pieces.argtypes = [vp, u8p, u64p, u64p, u32p, C.c_uint32, C.c_uint32, u8p, vp]
        L.xcg_gather_pieces.restype = C.c_int
    L.xcg_debug_set_stream_seed.argtypes = [C.c_int]
    L.xcg_debug_set_stream_seed.restype = C.c_int
    L.xcg_debug_stream_kernel_timing.argtypes = [C.c_int]
    L.xcg_debug_stream_kernel_timing.restype = C.c_int
    L.xcg_debug_stream_kernel_time.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.xcg_debug_stream_kernel_time.restype = C.c_int
    L.xcg_debug_restart_counts.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.xcg_debug_restart_counts.restype = C.c_int
    L.xcg_debug_set_lds_filter_keys.argtypes = [C.c_uint32]
    L.xcg_debug_set_lds_filter_keys.restype = C.c_uint32
    L.xcg_debug_set_lds_prefilter_keys.argtypes = [C.c_uint32]
    L.xcg_debug_set_lds_prefilter_keys.restype = C.c_uint32
    L.xcg_debug_decode_kernel_timing.argtypes = [C.c_int]
    L.xcg_debug_decode_kernel_timing.restype = C.c_int
    L.xcg_debug_decode_kernel_time.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.xcg_debug_decode_kernel_time.restype = C.c_int
    L.xcg_debug_decode_reuse.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.xcg_debug_decode_reuse.restype = C.c_int
    L.xcg_debug_set_screen.argtypes = [C.c_int]
    L.xcg_debug_set_screen.restype = C.c_int
    L.xcg_debug_screen_counts.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.xcg_debug_screen_counts.restype = C.c_int
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise XCGError(f'xcgpu: {lib().xcg_strerror(rc).decode()} ({rc})')


def _stream_ptr(stream):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def stream_kernel_time():
    """(milliseconds, launches) of the stream-parse kernel since the last call,
    timed by HIP events on its launch stream while xcg_debug_stream_kernel_timing
    is on (bench.py's roofline for stream semantics)."""
    ms, k = C.c_double(), C.c_uint32()
    _check(lib().xcg_debug_stream_kernel_time(C.byref(ms), C.byref(k)))
    return float(ms.value), int(k.value)


def encode_bound(n: int) -> int:
    return 2 * int(n) + 16


class Disk:
    """One XCodecDisk shared by several pair contexts (xcg_disk_create): the
    local cache's front and each peer front XCodecCache::connect makes append
    to one FIFO ring (xcodec/xcodec_cache_disk.h:33-69)."""

    HOST, DEVICE = 1, 2          # XCG_DISK_HOST / XCG_DISK_DEVICE: force the blocks' tier

    def __init__(self, disk_bytes: int, tier: int = 0, path: str = None):
        """With `path`: the volume file there (xcg_disk_open: reopened when it
        holds one, else fresh)."""
        h = C.c_void_p()
        if path is not None:
            _check(lib().xcg_disk_open(path.encode(), int(disk_bytes), int(tier), C.byref(h)))
        else:
            _check(lib().xcg_disk_create_ex(int(disk_bytes), int(tier), C.byref(h)))
        self.h = h

    def save(self, path: str):
        """Write the volume as the reference's file stands now (xcg_disk_save)."""
        _check(lib().xcg_disk_save(self.h, path.encode()))

    def head(self):
        """The write head: (index block, next entry) -- XCodecDisk's
        current_index_block_ / index_block_next_."""
        b, n = C.c_uint64(), C.c_uint64()
        _check(lib().xcg_disk_head(self.h, C.byref(b), C.byref(n)))
        return int(b.value), int(n.value)

    def tier(self) -> int:
        """Where the data blocks live: 0 HBM, 1 pinned host memory (-1: no front yet)."""
        return int(lib().xcg_disk_tier(self.h))

    def stats(self):
        """(live index entries of every front, entries written, index blocks, fronts)."""
        st = (C.c_uint64 * 4)()
        _check(lib().xcg_disk_stats(self.h, st))
        return tuple(int(v) for v in st)

    def close(self):
        if getattr(self, 'h', None):
            lib().xcg_disk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """An XCodecEncoder + cache configuration bound to one GPU."""

    def __init__(self, device: int = 0, out_of_band: bool = False, null_cache: bool = False,
                 cache_segments: int = 1 << 19, memory_cache_limit: int = 0, disk_bytes: int = 0,
                 disk: Disk = None, uuid: str = None, xuid: int = None):
        """memory_cache_limit (bytes): the bounded, LRU-evicting cache
        XCodecMemoryCache(uuid, memory_cache_limit) (xcodec/xcodec_cache.h:277)
        instead of an unbounded one of cache_segments capacity.  With
        disk_bytes too: wanproxy.conf's XCodecCachePair of that memory cache
        and a disk of disk_bytes (xcodec/xcodec_cache.h:140-237); with `disk`
        instead, the pair's secondary is the next front of that shared disk
        (with `uuid`, that UUID's front: XCodecDisk::connect; with `xuid`, that
        front of the disk)."""
        import torch
        if not torch.cuda.is_available():
            raise XCGError('no GPU: the XCodec engine has no CPU path')
        self.device = device
        self.flags = (XCG_FLAG_OOB if out_of_band else 0) | (XCG_FLAG_NULLCACHE if null_cache else 0)
        h = C.c_void_p()
        if disk is not None and xuid is not None:
            _check(lib().xcg_ctx_create_pair_xuid(device, self.flags, int(memory_cache_limit), disk.h,
                                                  uuid.encode() if uuid else None, int(xuid), C.byref(h)))
        elif disk is not None and uuid is not None:
            _check(lib().xcg_ctx_create_pair_uuid(device, self.flags, int(memory_cache_limit), disk.h, uuid.encode(),
                                                  C.byref(h)))
        elif disk is not None:
            _check(lib().xcg_ctx_create_pair_on(device, self.flags, int(memory_cache_limit), disk.h, C.byref(h)))
        elif disk_bytes:
            _check(lib().xcg_ctx_create_pair(device, self.flags, int(memory_cache_limit), int(disk_bytes), C.byref(h)))
        elif memory_cache_limit:
            _check(lib().xcg_ctx_create_bounded(device, self.flags, int(memory_cache_limit), C.byref(h)))
        else:
            _check(lib().xcg_ctx_create_ex(device, self.flags, int(cache_segments), C.byref(h)))
        self.h = h

    # The persistent cache (XCG_SEM_STREAM): XCodecMemoryCache of the encoder.
    def cache_size(self) -> int:
        return int(lib().xcg_cache_size(self.h))

    def cache_lookup(self, h: int):
        """XCodecCache::lookup of one hash: its 2048 bytes, or None (a hit
        refreshes a bounded cache's LRU order)."""
        buf = (C.c_uint8 * 2048)()
        rc = lib().xcg_cache_lookup_host(self.h, C.c_uint64(h), buf)
        if rc == XCG_ENOENT:
            return None
        _check(rc)
        return bytes(buf)

    def cache_enter(self, h: int, seg: bytes):
        """enter (or replace the bytes of) one segment -- XCodecPipePair's <LEARN>."""
        assert len(seg) == 2048
        _check(lib().xcg_cache_enter_host(self.h, C.c_uint64(h), (C.c_uint8 * 2048).from_buffer_copy(seg)))

    def cache_learn_device(self, d_segs, n: int, d_hash=None, stream=None):
        """xcg_cache_learn_batch on device tensors: the n segments at
        d_segs.data_ptr() (any alignment), their hashes into d_hash (int64
        tensor, or None).  Ordered on `stream`; no synchronisation is needed
        before the context's next batch."""
        _check(lib().xcg_cache_learn_batch(
            self.h, C.c_void_p(d_segs.data_ptr()), int(n),
            C.c_void_p(d_hash.data_ptr()) if d_hash is not None else None, _stream_ptr(stream)))

    def cache_learn(self, segs) -> np.ndarray:
        """Learn whole 2048-byte segments (bytes / np.uint8, back to back) in
        order, as n <LEARN>s (xcg_cache_learn_host).  Returns their XCodecHash
        values (np.uint64)."""
        a = np.frombuffer(segs, dtype=np.uint8) if not isinstance(segs, np.ndarray) else np.ascontiguousarray(segs)
        if a.size % SEG:
            raise ValueError('segments are 2048 bytes each')
        n = a.size // SEG
        hs = np.zeros(n, dtype=np.uint64)
        if n:
            _check(lib().xcg_cache_learn_host(self.h, a.ctypes.data, n, hs.ctypes.data))
        return hs

    def cache_export(self):
        """Every live (hash, segment) of a memory cache, nothing changed: a
        bounded cache least recently used first, an unbounded one by ascending
        hash (xcg_cache_export_host).  Returns (hashes np.uint64, bytes)."""
        cnt = C.c_uint64()
        rc = lib().xcg_cache_export_host(self.h, None, None, 0, C.byref(cnt))
        if rc != XCG_EOVERFLOW:
            _check(rc)
        n = int(cnt.value)
        hs = np.zeros(n, dtype=np.uint64)
        segs = np.zeros(n * SEG, dtype=np.uint8)
        if n:
            _check(lib().xcg_cache_export_host(self.h, segs.ctypes.data, hs.ctypes.data, n, C.byref(cnt)))
        return hs, segs.tobytes()

    def cache_save(self, path: str):
        """Write the cache as `tack -p`'s persistent cache file: the segments
        back to back, in export order (programs/tack/tack.cc:103-127)."""
        _, segs = self.cache_export()
        with open(path, 'wb') as f:
            f.write(segs)

    def cache_load(self, path: str) -> np.ndarray:
        """Learn every segment of a `tack -p` file, in file order."""
        with open(path, 'rb') as f:
            data = f.read()
        if len(data) % SEG:
            raise ValueError('Corrupt persistent cache')
        return self.cache_learn(data)

    def pair_stats(self):
        """(primary entries, this front's disk index entries, disk entries
        written by every front, disk index blocks) of a pair context."""
        st = (C.c_uint64 * 4)()
        _check(lib().xcg_pair_stats(self.h, st))
        return tuple(int(v) for v in st)

    def xuid(self) -> int:
        """The disk front (xuid) of a pair context."""
        x = lib().xcg_pair_xuid(self.h)
        _check(min(x, 0))
        return x

    def restart_counts(self):
        """(chunks resumed from their rows, chunks that rejoined their old parse)
        in this context's bounded / pair re-parse passes so far."""
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib().xcg_debug_restart_counts(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def decode_reuse_stats(self):
        """(duplicate EXTRACTs, hashes whose EXTRACTs differ in bytes, whether
        the name-reuse resolver ran) of this context's last decode batch."""
        st = (C.c_uint64 * 3)()
        _check(lib().xcg_debug_decode_reuse(self.h, st))
        return int(st[0]), int(st[1]), bool(st[2])

    def cache_clear(self):
        _check(lib().xcg_cache_clear(self.h))

    def last_rounds(self) -> int:
        return int(lib().xcg_last_rounds(self.h))

    def close(self):
        if getattr(self, 'h', None):
            lib().xcg_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def status(self):
        _check(lib().xcg_ctx_status(self.h))

    # ------------------------------------------------------------- device API
    def encode_batch_device(self, d_in, d_off, d_len, n, max_len, d_out, d_out_off, d_out_len,
                            d_stats=None, stream=None, semantics=XCG_SEM_INDEPENDENT):
        """Raw launch on device tensors (all torch tensors on this device)."""
        _check(lib().xcg_encode_batch(
            self.h, semantics, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_off.data_ptr()),
            C.c_void_p(d_len.data_ptr()), int(n), int(max_len), C.c_void_p(d_out.data_ptr()),
            C.c_void_p(d_out_off.data_ptr()), C.c_void_p(d_out_len.data_ptr()),
            C.c_void_p(d_stats.data_ptr()) if d_stats is not None else None, _stream_ptr(stream)))

    def encode_chunks(self, data, offs, lens, with_stats=False, semantics=XCG_SEM_INDEPENDENT):
        """Encode chunks of host `data` (bytes / np.uint8) on the GPU; returns a
        list of encoded bytes objects (and per-chunk stats if asked)."""
        import torch
        dev = torch.device('cuda', self.device)
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        n = int(offs.size)
        if n == 0:
            return ([], np.zeros((0, 4), np.uint32)) if with_stats else []
        bounds = 2 * lens.astype(np.uint64) + 16
        oo = np.zeros(n, dtype=np.uint64)
        oo[1:] = np.cumsum(bounds)[:-1]
        d_in = torch.from_numpy(a.copy() if a.size else np.zeros(1, np.uint8)).to(dev)
        d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
        d_oo = torch.from_numpy(oo.view(np.int64)).to(dev)
        d_out = torch.zeros(int(bounds.sum()), dtype=torch.uint8, device=dev)
        d_ol = torch.zeros(n, dtype=torch.int64, device=dev)
        d_st = torch.zeros(4 * n, dtype=torch.int32, device=dev)
        self.encode_batch_device(d_in, d_off, d_len, n, int(lens.max()), d_out, d_oo, d_ol, d_st,
                                 semantics=semantics)
        torch.cuda.synchronize(dev)
        self.status()
        out = d_out.cpu().numpy()
        ol = d_ol.cpu().numpy().astype(np.uint64)
        res = [out[int(oo[i]):int(oo[i] + ol[i])].tobytes() for i in range(n)]
        if with_stats:
            return res, d_st.cpu().numpy().view(np.uint32).reshape(n, 4)
        return res

    def encode_refmap_device(self, d_enc, d_enc_off, d_enc_len, n, max_enc_len, d_ref_hash, d_ref_pos, ref_cap,
                             d_ref_count, d_ref_walked=None, first_chunk=0, stream=None):
        """Raw launch of xcg_encode_refmap_batch on device tensors: the refmap
        rows of the encoder outputs d_enc / d_enc_off / d_enc_len (what
        encode_batch_device just wrote); asynchronous on `stream`."""
        _check(lib().xcg_encode_refmap_batch(
            self.h, C.c_void_p(d_enc.data_ptr()), C.c_void_p(d_enc_off.data_ptr()), C.c_void_p(d_enc_len.data_ptr()),
            int(n), int(max_enc_len), int(first_chunk), C.c_void_p(d_ref_hash.data_ptr()),
            C.c_void_p(d_ref_pos.data_ptr()), int(ref_cap), C.c_void_p(d_ref_count.data_ptr()),
            C.c_void_p(d_ref_walked.data_ptr()) if d_ref_walked is not None else None, _stream_ptr(stream)))

    def encode_chunks_refmap(self, data, offs, lens, semantics=XCG_SEM_STREAM):
        """encode_chunks with each call's refmap (xcg_encode_host_refmap), the
        third parameter of XCodecEncoder::encode: returns (encs, refmaps), one
        ordered {hash: segment bytes} per chunk, ascending by hash as std::map
        iterates, the segments cut from `data` at the reported positions."""
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        n = int(offs.size)
        if n == 0:
            return [], []
        bounds = 2 * lens.astype(np.uint64) + 16
        oo = np.zeros(n, dtype=np.uint64)
        oo[1:] = np.cumsum(bounds)[:-1]
        out = np.zeros(int(bounds.sum()), dtype=np.uint8)
        ol = np.zeros(n, dtype=np.uint64)
        cap = XCG_REFMAP_MAX
        rh = np.zeros(n * cap, dtype=np.uint64)
        rp = np.zeros(n * cap, dtype=np.uint32)
        rn = np.zeros(n, dtype=np.uint32)
        src = a if a.size else np.zeros(1, np.uint8)
        _check(lib().xcg_encode_host_refmap(self.h, semantics, src.ctypes.data, a.size, offs.ctypes.data,
                                            lens.ctypes.data, n, out.ctypes.data, out.size, oo.ctypes.data,
                                            ol.ctypes.data, rh.ctypes.data, rp.ctypes.data, cap, rn.ctypes.data))
        encs = [out[int(oo[i]):int(oo[i] + ol[i])].tobytes() for i in range(n)]
        refmaps = []
        for i in range(n):
            m = {}
            for k in range(int(rn[i])):
                at = int(offs[i]) + int(rp[i * cap + k])
                m[int(rh[i * cap + k])] = a[at:at + SEG].tobytes()
            refmaps.append(m)
        return encs, refmaps

    def decode_chunks(self, encs, window: 'Window' = None):
        """Decode encoded chunks (one stream, this context's cache) on the GPU,
        with `window` as the decoder's BACKREF window (default: the context's).
        Returns (outs, status, consumed, unknown) -- see xcg_decode_batch."""
        import torch
        dev = torch.device('cuda', self.device)
        n = len(encs)
        lens = np.array([len(e) for e in encs], dtype=np.uint32)
        offs = np.zeros(n, dtype=np.uint64)
        if n > 1:
            offs[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
        blob = np.frombuffer(b''.join(encs) or b'\0', dtype=np.uint8)
        d_in = torch.from_numpy(blob.copy()).to(dev)
        d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
        d_oo = torch.zeros(n, dtype=torch.int64, device=dev)
        d_ol = torch.zeros(n, dtype=torch.int64, device=dev)
        d_st = torch.zeros(n, dtype=torch.int32, device=dev)
        d_cons = torch.zeros(n, dtype=torch.int64, device=dev)
        cap = int(lens.astype(np.uint64).sum()) * 205 + 4096   # a 10-byte REF expands to 2048
        unk = np.zeros(1 << 16, dtype=np.uint64)
        nunk = np.zeros(1, dtype=np.uint32)
        total = np.zeros(1, dtype=np.uint64)
        if window is not None:
            _check(lib().xcg_decode_set_window(self.h, window.h))
        try:
            for _ in range(2):
                d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
                rc = lib().xcg_decode_batch(
                    self.h, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_off.data_ptr()), C.c_void_p(d_len.data_ptr()),
                    n, int(lens.max()) if n else 0, C.c_void_p(d_out.data_ptr()), cap, C.c_void_p(d_oo.data_ptr()),
                    C.c_void_p(d_ol.data_ptr()), C.c_void_p(d_st.data_ptr()), C.c_void_p(d_cons.data_ptr()),
                    unk.ctypes.data, unk.size, nunk.ctypes.data, total.ctypes.data, _stream_ptr(None))
                if rc != XCG_EOVERFLOW:
                    break
                cap = int(total[0])            # BACKREF-dense: 3 bytes -> 2048; nothing was committed
            _check(rc)
        finally:
            if window is not None:
                lib().xcg_decode_set_window(self.h, None)
        torch.cuda.synchronize(dev)
        oo = d_oo.cpu().numpy()
        ol = d_ol.cpu().numpy()
        st = d_st.cpu().numpy()
        cons = d_cons.cpu().numpy()
        out = d_out.cpu().numpy()
        outs = [out[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes() if st[i] != 2 else b'' for i in range(n)]
        return outs, st, cons, [int(u) for u in unk[:int(nunk[0])]]

    def decode_chunks_windows(self, chunks, windows, chunk_window, host: bool = False):
        """Decode encoded chunks that are successive decode() calls of several
        decoders on this context's cache, in one batch: chunk i declares into
        and BACKREFs from windows[chunk_window[i]] (Window objects).  Returns
        (outs, status, consumed, stop_chunk) -- see xcg_decode_batch_windows;
        host=True goes through xcg_decode_host_windows."""
        return self._decode_chunks_windows(chunks, windows, chunk_window, host, False)

    def decode_chunks_windows_bounded(self, chunks, windows, chunk_window, host: bool = False):
        """decode_chunks_windows on a bounded or pair context
        (xcg_decode_batch_windows_bounded / xcg_decode_host_windows_bounded):
        the same arguments and return shape; XcgError(-95) when the batch is
        refused as a whole (nothing has changed: split it)."""
        return self._decode_chunks_windows(chunks, windows, chunk_window, host, True)

    def _decode_chunks_windows(self, chunks, windows, chunk_window, host, bounded):
        host_call = lib().xcg_decode_host_windows_bounded if bounded else lib().xcg_decode_host_windows
        batch_call = lib().xcg_decode_batch_windows_bounded if bounded else lib().xcg_decode_batch_windows
        n = len(chunks)
        lens = np.array([len(e) for e in chunks], dtype=np.uint32)
        offs = np.zeros(n, dtype=np.uint64)
        if n > 1:
            offs[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
        blob = np.frombuffer(b''.join(chunks) or b'\0', dtype=np.uint8).copy()
        wins = (C.c_void_p * max(len(windows), 1))(*[w.h if w is not None else None for w in windows])
        cw = np.ascontiguousarray(chunk_window, dtype=np.uint32)
        if cw.size != n:
            raise ValueError('chunk_window: one entry per chunk')
        cap = int(lens.astype(np.uint64).sum()) * 205 + 4096   # a 10-byte REF expands to 2048
        stop = np.zeros(1, dtype=np.uint32)
        total = np.zeros(1, dtype=np.uint64)
        if host:
            oo, ol, cons = (np.zeros(n, dtype=np.uint64) for _ in range(3))
            st = np.zeros(n, dtype=np.int32)
            for _ in range(2):
                out = np.zeros(cap, dtype=np.uint8)
                rc = host_call(
                    self.h, blob.ctypes.data, sum(len(e) for e in chunks), offs.ctypes.data, lens.ctypes.data, n,
                    wins, len(windows), cw.ctypes.data, out.ctypes.data, cap, oo.ctypes.data, ol.ctypes.data,
                    st.ctypes.data, cons.ctypes.data, stop.ctypes.data, total.ctypes.data)
                if rc != XCG_EOVERFLOW:
                    break
                cap = int(total[0])            # BACKREF-dense: 3 bytes -> 2048; nothing was committed
            _check(rc)
        else:
            import torch
            dev = torch.device('cuda', self.device)
            d_in = torch.from_numpy(blob).to(dev)
            d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
            d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
            d_oo = torch.zeros(n, dtype=torch.int64, device=dev)
            d_ol = torch.zeros(n, dtype=torch.int64, device=dev)
            d_st = torch.zeros(n, dtype=torch.int32, device=dev)
            d_cons = torch.zeros(n, dtype=torch.int64, device=dev)
            for _ in range(2):
                d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
                rc = batch_call(
                    self.h, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_off.data_ptr()), C.c_void_p(d_len.data_ptr()),
                    n, int(lens.max()) if n else 0, wins, len(windows), cw.ctypes.data,
                    C.c_void_p(d_out.data_ptr()), cap, C.c_void_p(d_oo.data_ptr()), C.c_void_p(d_ol.data_ptr()),
                    C.c_void_p(d_st.data_ptr()), C.c_void_p(d_cons.data_ptr()), stop.ctypes.data, total.ctypes.data,
                    _stream_ptr(None))
                if rc != XCG_EOVERFLOW:
                    break
                cap = int(total[0])
            _check(rc)
            torch.cuda.synchronize(dev)
            oo, ol, st, cons, out = (t.cpu().numpy() for t in (d_oo, d_ol, d_st, d_cons, d_out))
        outs = [out[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes() if st[i] != 2 else b'' for i in range(n)]
        return outs, st, cons, int(stop[0])

    def decode_batch_independent_device(self, d_enc, d_off, d_len, n, max_len, d_out, d_out_off, d_out_cap,
                                        d_out_len, d_status, d_consumed, d_first_unknown=None, stream=None):
        """Raw launch of xcg_decode_batch_independent on device tensors (all torch
        tensors on this device); asynchronous on `stream`."""
        _check(lib().xcg_decode_batch_independent(
            self.h, C.c_void_p(d_enc.data_ptr()), C.c_void_p(d_off.data_ptr()), C.c_void_p(d_len.data_ptr()),
            int(n), int(max_len), C.c_void_p(d_out.data_ptr()), C.c_void_p(d_out_off.data_ptr()),
            C.c_void_p(d_out_cap.data_ptr()), C.c_void_p(d_out_len.data_ptr()), C.c_void_p(d_status.data_ptr()),
            C.c_void_p(d_consumed.data_ptr()),
            C.c_void_p(d_first_unknown.data_ptr()) if d_first_unknown is not None else None, _stream_ptr(stream)))

    def decode_chunks_independent(self, encs, out_caps=None):
        """Decode encoded chunks on the GPU, each on a fresh decoder of its own
        (empty cache, empty window): the inverse of encode_chunks' independent
        semantics.  out_caps: per-chunk slot sizes (default len * 205 + 4096, as
        decode_chunks sizes its buffer); chunks whose slot was too small are
        run once more with the size the kernel reported.  Returns (outs, status,
        consumed, first_unknown) -- see xcg_decode_batch_independent."""
        import torch
        dev = torch.device('cuda', self.device)
        n = len(encs)
        st = np.zeros(n, dtype=np.int32)
        cons = np.zeros(n, dtype=np.uint64)
        unk = np.zeros(n, dtype=np.uint64)
        outs = [b''] * n
        if n == 0:
            return outs, st, cons, unk
        caps = (np.array([len(e) * 205 + 4096 for e in encs], dtype=np.uint64) if out_caps is None
                else np.ascontiguousarray(out_caps, dtype=np.uint64))
        todo = np.arange(n)
        for attempt in range(2):
            sub = [encs[i] for i in todo]
            m = len(sub)
            lens = np.array([len(e) for e in sub], dtype=np.uint32)
            offs = np.zeros(m, dtype=np.uint64)
            offs[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
            oo = np.zeros(m, dtype=np.uint64)
            oo[1:] = np.cumsum(caps[todo])[:-1]
            d_in = torch.from_numpy(np.frombuffer(b''.join(sub) or b'\0', dtype=np.uint8).copy()).to(dev)
            d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
            d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
            d_oo = torch.from_numpy(oo.view(np.int64)).to(dev)
            d_cap = torch.from_numpy(caps[todo].view(np.int64)).to(dev)
            d_out = torch.zeros(max(int(caps[todo].sum()), 1), dtype=torch.uint8, device=dev)
            d_ol = torch.zeros(m, dtype=torch.int64, device=dev)
            d_st = torch.zeros(m, dtype=torch.int32, device=dev)
            d_cons = torch.zeros(m, dtype=torch.int64, device=dev)
            d_unk = torch.zeros(m, dtype=torch.int64, device=dev)
            self.decode_batch_independent_device(d_in, d_off, d_len, m, int(lens.max()), d_out, d_oo, d_cap, d_ol,
                                                 d_st, d_cons, d_unk)
            torch.cuda.synchronize(dev)
            self.status()
            out = d_out.cpu().numpy()
            ol = d_ol.cpu().numpy().view(np.uint64)
            st[todo] = d_st.cpu().numpy()
            cons[todo] = d_cons.cpu().numpy().view(np.uint64)
            unk[todo] = d_unk.cpu().numpy().view(np.uint64)
            for k, i in enumerate(todo):
                if st[i] != XCG_CHUNK_NOROOM:
                    outs[i] = out[int(oo[k]):int(oo[k]) + int(ol[k])].tobytes()
            again = st[todo] == XCG_CHUNK_NOROOM
            if attempt or not again.any():
                break
            caps = caps.copy()
            caps[todo[again]] = ol[again]
            todo = todo[again]
        return outs, st, cons, unk

    # ------------------------------------------------- grouped (short streams)
    def encode_batch_grouped_device(self, d_in, d_off, d_len, n, d_group_first, n_groups, max_group_len, d_out,
                                    d_out_off, d_out_len, d_stats=None, stream=None):
        """Raw launch of xcg_encode_batch_grouped on device tensors (all torch
        tensors on this device); asynchronous on `stream`."""
        _check(lib().xcg_encode_batch_grouped(
            self.h, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_off.data_ptr()), C.c_void_p(d_len.data_ptr()), int(n),
            C.c_void_p(d_group_first.data_ptr()), int(n_groups), int(max_group_len), C.c_void_p(d_out.data_ptr()),
            C.c_void_p(d_out_off.data_ptr()), C.c_void_p(d_out_len.data_ptr()),
            C.c_void_p(d_stats.data_ptr()) if d_stats is not None else None, _stream_ptr(stream)))

    def decode_batch_grouped_device(self, d_enc, d_off, d_len, n, d_group_first, n_groups, max_group_len, d_out,
                                    d_out_off, d_out_cap, d_out_len, d_status, d_consumed, d_first_unknown=None,
                                    stream=None):
        """Raw launch of xcg_decode_batch_grouped on device tensors; asynchronous
        on `stream`."""
        _check(lib().xcg_decode_batch_grouped(
            self.h, C.c_void_p(d_enc.data_ptr()), C.c_void_p(d_off.data_ptr()), C.c_void_p(d_len.data_ptr()), int(n),
            C.c_void_p(d_group_first.data_ptr()), int(n_groups), int(max_group_len), C.c_void_p(d_out.data_ptr()),
            C.c_void_p(d_out_off.data_ptr()), C.c_void_p(d_out_cap.data_ptr()), C.c_void_p(d_out_len.data_ptr()),
            C.c_void_p(d_status.data_ptr()), C.c_void_p(d_consumed.data_ptr()),
            C.c_void_p(d_first_unknown.data_ptr()) if d_first_unknown is not None else None, _stream_ptr(stream)))

    def encode_groups(self, data, offs, lens, group_first, with_stats=False, max_group_len=None, check=True):
        """Encode chunks of host `data` as many short streams: group g is the
        chunks [group_first[g], group_first[g + 1]), successive encode() calls on
        one fresh cache of its own (xcg_encode_batch_grouped).  Returns one
        encoding per chunk (and the per-chunk stats if asked).  max_group_len
        defaults to the largest group's total; check=False leaves the context's
        status word to the caller (a refused group then shows as empty outputs)."""
        import torch
        dev = torch.device('cuda', self.device)
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        gf = np.ascontiguousarray(group_first, dtype=np.uint32)
        n, ng = int(offs.size), int(gf.size) - 1
        if n == 0 or ng <= 0:
            return ([b''] * n, np.zeros((n, 4), np.uint32)) if with_stats else [b''] * n
        if max_group_len is None:
            cs = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))]).astype(np.uint64)
            g0, g1 = np.minimum(gf[:-1], n), np.minimum(gf[1:], n)
            max_group_len = int(max(0, (cs[g1].astype(np.int64) - cs[g0].astype(np.int64)).max()))
        bounds = 2 * lens.astype(np.uint64) + 16
        oo = np.zeros(n, dtype=np.uint64)
        oo[1:] = np.cumsum(bounds)[:-1]
        d_in = torch.from_numpy(a.copy() if a.size else np.zeros(1, np.uint8)).to(dev)
        d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
        d_gf = torch.from_numpy(gf.view(np.int32)).to(dev)
        d_oo = torch.from_numpy(oo.view(np.int64)).to(dev)
        d_out = torch.zeros(int(bounds.sum()), dtype=torch.uint8, device=dev)
        d_ol = torch.zeros(n, dtype=torch.int64, device=dev)
        d_st = torch.zeros(4 * n, dtype=torch.int32, device=dev)
        self.encode_batch_grouped_device(d_in, d_off, d_len, n, d_gf, ng, max_group_len, d_out, d_oo, d_ol, d_st)
        torch.cuda.synchronize(dev)
        if check:
            self.status()
        out = d_out.cpu().numpy()
        ol = d_ol.cpu().numpy().astype(np.uint64)
        res = [out[int(oo[i]):int(oo[i] + ol[i])].tobytes() for i in range(n)]
        if with_stats:
            return res, d_st.cpu().numpy().view(np.uint32).reshape(n, 4)
        return res

    def decode_groups(self, groups, out_caps=None, max_group_len=None, check=True):
        """Decode many short streams: groups[g] is the list of one stream's
        encoded chunks, decoded in order on one fresh decoder of its own
        (xcg_decode_batch_grouped).  out_caps: per-chunk slot sizes, flat in
        chunk order (default len * 205 + 4096); the groups that hold a chunk
        whose slot was too small are run once more with the sizes the kernel
        reported.  Returns, flat in chunk order, a list of (status, out,
        consumed, first_unknown)."""
        import torch
        dev = torch.device('cuda', self.device)
        encs = [e for grp in groups for e in grp]
        n = len(encs)
        gsz = np.array([len(grp) for grp in groups], dtype=np.int64)
        gfirst = np.concatenate([[0], np.cumsum(gsz)]).astype(np.int64)
        st = np.zeros(n, dtype=np.int32)
        cons = np.zeros(n, dtype=np.uint64)
        unk = np.zeros(n, dtype=np.uint64)
        outs = [b''] * n
        if n == 0:
            return []
        caps = (np.array([len(e) * 205 + 4096 for e in encs], dtype=np.uint64) if out_caps is None
                else np.ascontiguousarray(out_caps, dtype=np.uint64).copy())
        todo_g = np.arange(len(groups))
        for attempt in range(2):
            idx = np.concatenate([np.arange(gfirst[g], gfirst[g + 1]) for g in todo_g]).astype(np.int64)
            m = int(idx.size)
            if m == 0:
                break
            sub = [encs[i] for i in idx]
            lens = np.array([len(e) for e in sub], dtype=np.uint32)
            offs = np.zeros(m, dtype=np.uint64)
            offs[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
            gf = np.concatenate([[0], np.cumsum(gsz[todo_g])]).astype(np.uint32)
            cs = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))]).astype(np.int64)
            mgl = int((cs[gf[1:]] - cs[gf[:-1]]).max()) if max_group_len is None else int(max_group_len)
            oo = np.zeros(m, dtype=np.uint64)
            oo[1:] = np.cumsum(caps[idx])[:-1]
            d_in = torch.from_numpy(np.frombuffer(b''.join(sub) or b'\0', dtype=np.uint8).copy()).to(dev)
            d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
            d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
            d_gf = torch.from_numpy(gf.view(np.int32)).to(dev)
            d_oo = torch.from_numpy(oo.view(np.int64)).to(dev)
            d_cap = torch.from_numpy(caps[idx].view(np.int64)).to(dev)
            d_out = torch.zeros(max(int(caps[idx].sum()), 1), dtype=torch.uint8, device=dev)
            d_ol = torch.zeros(m, dtype=torch.int64, device=dev)
            d_st = torch.zeros(m, dtype=torch.int32, device=dev)
            d_cons = torch.zeros(m, dtype=torch.int64, device=dev)
            d_unk = torch.zeros(m, dtype=torch.int64, device=dev)
            self.decode_batch_grouped_device(d_in, d_off, d_len, m, d_gf, int(gf.size) - 1, mgl, d_out, d_oo, d_cap,
                                             d_ol, d_st, d_cons, d_unk)
            torch.cuda.synchronize(dev)
            if check:
                self.status()
            out = d_out.cpu().numpy()
            ol = d_ol.cpu().numpy().view(np.uint64)
            st[idx] = d_st.cpu().numpy()
            cons[idx] = d_cons.cpu().numpy().view(np.uint64)
            unk[idx] = d_unk.cpu().numpy().view(np.uint64)
            for k, i in enumerate(idx):
                outs[i] = b'' if st[i] == XCG_CHUNK_NOROOM else out[int(oo[k]):int(oo[k]) + int(ol[k])].tobytes()
            again = st[idx] == XCG_CHUNK_NOROOM
            if attempt or not again.any():
                break
            caps[idx[again]] = ol[again]
            chunk_group = np.searchsorted(gfirst, idx[again], side='right') - 1
            todo_g = np.unique(chunk_group)
        return [(int(st[i]), outs[i], int(cons[i]), int(unk[i])) for i in range(n)]

    def decode_call(self, data: bytes, out_cap: int = None):
        """One XCodecDecoder::decode(output, input, unknown) call from host memory
        (xcg_decode_call: one launch, one synchronisation on an unbounded cache).
        Returns (status, out, consumed, unknown, extract_hashes or None)."""
        n = len(data)
        if out_cap is None:
            out_cap = (n // 10 + 1) * 2048 + n
        out = np.zeros(max(1, out_cap), np.uint8)
        ol, cons = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
        st = np.zeros(1, np.int32)
        unk = np.zeros(1 << 16, np.uint64)
        nunk, ne = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
        ext = np.zeros(1024, np.uint64)
        _check(lib().xcg_decode_call(self.h, data, n, out.ctypes.data, out_cap, ol.ctypes.data, cons.ctypes.data,
                                     st.ctypes.data, unk.ctypes.data, unk.size, nunk.ctypes.data, ext.ctypes.data,
                                     ext.size, ne.ctypes.data))
        hashes = None if int(ne[0]) == 0xFFFFFFFF else [int(h) for h in ext[:int(ne[0])]]
        return (int(st[0]), out[:int(ol[0])].tobytes(), int(cons[0]), [int(u) for u in unk[:int(nunk[0])]], hashes)

    def window_hashes(self, data) -> np.ndarray:
        import torch
        dev = torch.device('cuda', self.device)
        a = np.frombuffer(data, dtype=np.uint8)
        n = max(0, a.size - SEG + 1)
        if n == 0:
            return np.zeros(0, np.uint64)
        d_x = torch.from_numpy(a.copy()).to(dev)
        d_h = torch.zeros(n, dtype=torch.int64, device=dev)
        _check(lib().xcg_window_hashes(self.h, C.c_void_p(d_x.data_ptr()), a.size, C.c_void_p(d_h.data_ptr()),
                                       _stream_ptr(None)))
        torch.cuda.synchronize(dev)
        return d_h.cpu().numpy().view(np.uint64)

    def segment_hashes_be(self, data) -> bytes:
        import torch
        dev = torch.device('cuda', self.device)
        a = np.frombuffer(data, dtype=np.uint8)
        n = a.size // SEG
        if n == 0:
            return b''
        d_x = torch.from_numpy(a.copy()).to(dev)
        d_h = torch.zeros(n, dtype=torch.int64, device=dev)
        _check(lib().xcg_segment_hashes(self.h, C.c_void_p(d_x.data_ptr()), a.size, C.c_void_p(d_h.data_ptr()),
                                        _stream_ptr(None)))
        torch.cuda.synchronize(dev)
        return d_h.cpu().numpy().tobytes()


class Window:
    """A decoder's BACKREF window (XCodecWindow, xcodec/xcodec_window.h)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        h = C.c_void_p()
        _check(lib().xcg_window_create(ctx.h, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, 'h', None):
            lib().xcg_window_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class XCodecEncoder:
    """Mirror of XCodecEncoder(XCodecCache*) (xcodec/xcodec_encoder.h:40-43):
    successive encode() calls share the context's cache, exactly like tack's
    loop (programs/tack/tack.cc:301-321)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def encode(self, data: bytes, refmap: dict = None) -> bytes:
        """encode(output, input, refmap): with a dict, every hash the call REF'd
        and not yet in it is added with its segment, in ascending hash order
        (xcodec/xcodec_encoder.cc:364-371)."""
        if not data:
            return b''
        if refmap is not None:
            encs, maps = self.ctx.encode_chunks_refmap(data, np.array([0]), np.array([len(data)]))
            for h, seg in maps[0].items():
                refmap.setdefault(h, seg)
            return encs[0]
        return self.ctx.encode_chunks(data, np.array([0]), np.array([len(data)]), semantics=XCG_SEM_STREAM)[0]


class XCodecDecoder:
    """Mirror of XCodecDecoder(XCodecCache*) (xcodec/xcodec_decoder.h:35-45):
    decode(input) -> (ok, output, consumed, unknown_hashes), where `consumed`
    is how much of `input` decode() removed (a partial op stays) and
    `unknown_hashes` the sorted set an ASK would request."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.window = Window(ctx)      # XCodecDecoder::window_, one per decoder

    def decode(self, data: bytes):
        if not data:
            return True, b'', 0, []
        outs, st, cons, unk = self.ctx.decode_chunks([data], window=self.window)
        return int(st[0]) >= 0, outs[0], int(cons[0]), unk


class PipePair:
    """Mirror of XCodecPipePair (xcodec/xcodec_pipe_pair.h:41-212) over
    xcg_pipe_*: encoder_consume(data) -> bytes for the peer (b'' input = EOS);
    decoder_consume(data) -> (to_peer, to_local, local_eos, peer_eos).  `enc`
    is the codec's context (cache shared by its pipes), `dec` the context of the
    peer's cache; `uuid` the 36-byte UUID string sent in <HELLO>."""

    def __init__(self, enc: Context, dec: Context, uuid: bytes, connect: bool = False):
        """connect=True: `dec` is the codec's cache (codec_->cache()) and the
        decoder context is connected at the peer's <HELLO>
        (xcg_pipe_create_connect: XCodecCache::connect(uuid, parent))."""
        self.enc, self.dec = enc, dec
        h = C.c_void_p()
        fn = lib().xcg_pipe_create_connect if connect else lib().xcg_pipe_create
        _check(fn(enc.h, dec.h, uuid, C.byref(h)))
        self.h = h

    def decoder_ctx(self):
        """Handle (int) of the context this pipe decodes on, None before <HELLO>."""
        return lib().xcg_pipe_decoder_ctx(self.h)

    def close(self):
        if getattr(self, 'h', None):
            lib().xcg_pipe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encoder_consume(self, data: bytes) -> bytes:
        o = _PipeOut()
        _check(lib().xcg_pipe_encoder_consume(self.h, data, len(data), C.byref(o)))
        return o.peer()

    @staticmethod
    def encoder_consume_many(pipes, datas):
        n = len(pipes)
        hs = (C.c_void_p * n)(*[p.h.value for p in pipes])
        ds = (C.c_char_p * n)(*datas)
        ls = (C.c_uint64 * n)(*[len(d) for d in datas])
        outs = (_PipeOut * n)()
        _check(lib().xcg_pipe_encoder_consume_many(hs, ds, ls, n, outs))
        return [o.peer() for o in outs]

    def decoder_consume(self, data: bytes):
        o = _PipeOut()
        rc = lib().xcg_pipe_decoder_consume(self.h, data, len(data), C.byref(o))
        _check(rc)
        return o.peer(), o.local(), bool(o.local_eos), bool(o.peer_eos)

    @staticmethod
    def decoder_consume_many(pipes, datas):
        """decoder_consume(datas[k]) of every pipe in order, the decode() calls of
        consecutive pipes on one decoder context in one GPU batch and those of
        pipes that each stand alone on a context of their own (many peers, a
        pipe each) in one launch (xcg_pipe_decoder_consume_many:
        xcg_decode_host_windows / _bounded, xcg_decode_call_many).  One (to_peer, to_local, local_eos,
        peer_eos) per pipe, or the XCGError its serial call would have raised;
        bad arguments (a pipe listed twice) and engine failures raise."""
        n = len(pipes)
        hs = (C.c_void_p * n)(*[p.h.value for p in pipes])
        ds = (C.c_char_p * n)(*datas)
        ls = (C.c_uint64 * n)(*[len(d) for d in datas])
        outs = (_PipeOut * n)()
        rcs = (C.c_int * n)(*([1] * n))                  # (1: not reached)
        rc = lib().xcg_pipe_decoder_consume_many(hs, ds, ls, n, outs, rcs)
        if rc != 0 and (rc not in list(rcs) or 1 in list(rcs)):
            _check(rc)
        res = []
        for k, o in enumerate(outs):
            if rcs[k] != 0:
                res.append(XCGError(f'xcgpu: {lib().xcg_strerror(rcs[k]).decode()} ({rcs[k]})'))
            else:
                res.append((o.peer(), o.local(), bool(o.local_eos), bool(o.peer_eos)))
        return res

    def pending_frames(self) -> int:
        return int(lib().xcg_pipe_pending_frames(self.h))


class Codec:
    """One WANProxyCodec (wanproxy.conf: `codec XCodec` + `compressor zlib` /
    `compressor_level N`) over xcg_codec_*: `enc` the codec's encoder context;
    `dec` the decoder context, or with connect=True the context its pipes'
    decoder contexts connect from at <HELLO>; level 0-9, or -1 for no
    compressor; at most `max_pipes` pipes alive at a time."""

    def __init__(self, enc: Context, dec: Context, level: int = 6, max_pipes: int = 64, connect: bool = False):
        self.enc, self.dec, self.level = enc, dec, level
        h = C.c_void_p()
        _check(lib().xcg_codec_create(enc.h, dec.h, int(connect), level, max_pipes, C.byref(h)))
        self.h = h

    def pipe(self, uuid: bytes) -> 'CodecPipe':
        return CodecPipe(self, uuid)

    def stats(self):
        """PipeByteCount's counters: (local bytes in, bytes to the peer after
        deflate, bytes from the peer before inflate, bytes to the local side)."""
        st = (C.c_uint64 * 4)()
        _check(lib().xcg_codec_stats(self.h, st))
        return tuple(int(x) for x in st)

    def close(self):
        if getattr(self, 'h', None):
            lib().xcg_codec_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def set_codec_fused(on: bool) -> bool:
    """xcg_debug_set_codec_fused: the send path that keeps the wire on the
    device (True) or the host composition (False, the default); returns the
    previous setting."""
    return bool(lib().xcg_debug_set_codec_fused(int(bool(on))))


def codec_debug_counts():
    """(fused send batches, host-composed send batches, inflate batches,
    decode batches) the codec layer has made in this process."""
    st = (C.c_uint64 * 4)()
    lib().xcg_codec_debug_counts(st)
    return tuple(int(x) for x in st)


class CodecPipe:
    """One side of a WANProxyCodecPipePair on a Codec: send(data) -> bytes for
    the peer (b'' = the local side closed); receive(data) -> (to_peer,
    to_local, local_eos, peer_eos) (b'' = the peer closed).  Close the pipes
    before their codec."""

    def __init__(self, codec: Codec, uuid: bytes):
        self.codec = codec
        h = C.c_void_p()
        _check(lib().xcg_codec_pipe_create(codec.h, uuid, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, 'h', None):
            lib().xcg_codec_pipe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def pending_frames(self) -> int:
        return int(lib().xcg_pipe_pending_frames(lib().xcg_codec_pipe_pair(self.h)))

    def decoder_ctx(self):
        return lib().xcg_pipe_decoder_ctx(lib().xcg_codec_pipe_pair(self.h))

    @staticmethod
    def _many(fn, pipes, datas):
        n = len(pipes)
        hs = (C.c_void_p * n)(*[p.h.value for p in pipes])
        ds = (C.c_char_p * n)(*datas)
        ls = (C.c_uint64 * n)(*[len(d) for d in datas])
        outs = (_PipeOut * n)()
        rcs = (C.c_int * n)(*([1] * n))                  # (1: not reached)
        rc = fn(hs, ds, ls, n, outs, rcs)
        if rc != 0 and (rc not in list(rcs) or 1 in list(rcs)):
            _check(rc)                                   # refused, or an engine failure
        res = []
        for k, o in enumerate(outs):
            if rcs[k] != 0:
                res.append(XCGError(f'xcgpu: {lib().xcg_strerror(rcs[k]).decode()} ({rcs[k]})'))
            else:
                res.append((o.peer(), o.local(), bool(o.local_eos), bool(o.peer_eos)))
        return res

    @staticmethod
    def send_many(pipes, datas):
        """xcg_codec_send_many: per pipe (to_peer, b'', False, False), or the
        XCGError of a pipe that has failed; refused calls raise."""
        return CodecPipe._many(lib().xcg_codec_send_many, pipes, datas)

    @staticmethod
    def receive_many(pipes, datas):
        """xcg_codec_receive_many: per pipe (to_peer, to_local, local_eos,
        peer_eos), or the XCGError (XCG_EPROTO) of that pipe."""
        return CodecPipe._many(lib().xcg_codec_receive_many, pipes, datas)

    def send(self, data: bytes) -> bytes:
        r = CodecPipe.send_many([self], [data])[0]
        if isinstance(r, XCGError):
            raise r
        return r[0]

    def receive(self, data: bytes):
        r = CodecPipe.receive_many([self], [data])[0]
        if isinstance(r, XCGError):
            raise r
        return r


def decode_call_many(calls, want_extracts: bool = True, out_lens: list = None):
    """xcg_decode_call_many: one decode() call per entry of `calls`, each
    (Context, Window or None, bytes[, out_cap]) on a context (and window) of its
    own, the calls an unbounded cache decodes in one launch all in ONE launch.
    Returns per call (rc, status, out, consumed, unknown, extract_hashes or
    None); bad arguments (a context or window listed twice, more than one
    device) and engine failures raise.  out_lens (a list) receives every call's
    out_len: with rc -75 for too little room, the size that call needs."""
    n = len(calls)
    if n == 0:
        _check(lib().xcg_decode_call_many(None, None, None, None, None, None, 0, None, None, None, None, None, None,
                                          None, None, None, None))
        return []
    UCAP, ECAP = 1 << 16, 1024
    datas = [bytes(c[2]) for c in calls]
    caps = [(c[3] if len(c) > 3 and c[3] is not None else (len(d) // 10 + 1) * 2048 + len(d))
            for c, d in zip(calls, datas)]
    cs = (C.c_void_p * n)(*[c[0].h.value for c in calls])
    ws = (C.c_void_p * n)(*[(c[1].h.value if c[1] is not None else None) for c in calls])
    ins = (C.c_char_p * n)(*datas)
    lens = (C.c_uint32 * n)(*[len(d) for d in datas])
    outs = [np.zeros(max(1, cap), np.uint8) for cap in caps]
    ops = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    ocap = (C.c_uint64 * n)(*caps)
    ol, cons = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    st = np.zeros(n, np.int32)
    unk = np.empty((n, UCAP), np.uint64)
    ups = (C.c_void_p * n)(*[unk[i].ctypes.data for i in range(n)])
    ucap = (C.c_uint32 * n)(*([UCAP] * n))
    nunk, ne = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    ext = np.zeros((n, ECAP), np.uint64)
    eps = (C.c_void_p * n)(*[ext[i].ctypes.data for i in range(n)])
    ecap = (C.c_uint32 * n)(*([ECAP] * n))
    rcs = (C.c_int * n)()
    _check(lib().xcg_decode_call_many(cs, ws, ins, lens, ops, ocap, n, ol.ctypes.data, cons.ctypes.data,
                                      st.ctypes.data, ups, ucap, nunk.ctypes.data,
                                      eps if want_extracts else None, ecap if want_extracts else None,
                                      ne.ctypes.data if want_extracts else None, rcs))
    res = []
    for i in range(n):
        hashes = None
        if want_extracts and int(ne[i]) != 0xFFFFFFFF:
            hashes = [int(h) for h in ext[i, :int(ne[i])]]
        k = min(int(ol[i]), caps[i]) if rcs[i] == 0 else 0
        res.append((int(rcs[i]), int(st[i]), outs[i][:k].tobytes(), int(cons[i]),
                    [int(u) for u in unk[i, :int(nunk[i])]], hashes))
    if out_lens is not None:
        out_lens[:] = [int(v) for v in ol]
    return res


def debug_decode_call_many():
    """(launches, calls the kernel finished, calls served outside the launch) of
    xcg_decode_call_many in this process."""
    o = (C.c_uint64 * 3)()
    lib().xcg_debug_decode_call_many(o)
    return int(o[0]), int(o[1]), int(o[2])


def pipe_debug_decode_peers():
    """(launches, pipes in them): the xcg_decode_call_many calls
    xcg_pipe_decoder_consume_many has made in this process."""
    o = (C.c_uint64 * 2)()
    lib().xcg_pipe_debug_decode_peers(o)
    return int(o[0]), int(o[1])


def ctx_connect(parent: Context, uuid: bytes):
    """xcg_ctx_connect: handle (int) of the registry's context for `uuid`."""
    h = C.c_void_p()
    _check(lib().xcg_ctx_connect(parent.h, uuid, C.byref(h)))
    return h.value


def ctx_register(ctx: Context, uuid: bytes):
    _check(lib().xcg_ctx_register(ctx.h, uuid))


def ctx_lookup(uuid: bytes):
    return lib().xcg_ctx_lookup(uuid)


def connect_registry_clear():
    lib().xcg_connect_registry_clear()
