"""wanproxy's XCodecPipePair itself -- TEST INFRASTRUCTURE ONLY.

`RefPipes('ref')` loads oracle/_ref/libppref.so: the reference's
xcodec/xcodec_pipe_pair.cc over its own XCodecEncoder, XCodecDecoder and
XCodecCache, compiled from the reference tree by oracle/Makefile and driven through
oracle/pipe_driver.cc.  `RefPipes('dropin')` loads oracle/_ref/libppdropin.so:
the same pipe pair over the integration/ adapters on libxcgpu.so.

A codec is an XCodec over XCodecMemoryCache(uuid[, limit]); a pair is one
XCodecPipePair on a codec.  consume() is one encoder_consume / decoder_consume
under the pair's mutex and returns what the call produced for the peer and for
the local side, and the flags it raised.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = {'ref': 'libppref.so', 'dropin': 'libppdropin.so'}

Consumed = namedtuple('Consumed', 'to_peer to_local encoder_eos decoder_eos encoder_error decoder_error')


class _Out(C.Structure):
    _fields_ = [('to_peer', C.c_void_p), ('to_peer_len', C.c_uint64), ('to_local', C.c_void_p),
                ('to_local_len', C.c_uint64), ('encoder_eos', C.c_int32), ('decoder_eos', C.c_int32),
                ('encoder_error', C.c_int32), ('decoder_error', C.c_int32)]


def path(which: str = 'ref') -> str:
    return os.path.join(HERE, '_ref', LIBS[which])


def available(which: str = 'ref') -> bool:
    return os.path.exists(path(which))


class RefPipes:
    _libs = {}

    def __init__(self, which: str = 'ref'):
        if which not in self._libs:
            if which == 'dropin':
                import torch  # noqa: F401  (one HIP runtime shared with libxcgpu.so)
            L = C.CDLL(path(which))
            L.pp_codec_new.restype = C.c_void_p
            L.pp_codec_new.argtypes = [C.c_char_p, C.c_uint64]
            L.pp_codec_free.argtypes = [C.c_void_p]
            L.pp_codec_cache_size.restype = C.c_uint64
            L.pp_codec_cache_size.argtypes = [C.c_void_p]
            L.pp_pair_new.restype = C.c_void_p
            L.pp_pair_new.argtypes = [C.c_void_p]
            L.pp_pair_free.argtypes = [C.c_void_p]
            L.pp_consume.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_uint64, C.POINTER(_Out)]
            L.pp_consume.restype = None
            L.pp_pending_frames.restype = C.c_uint64
            L.pp_pending_frames.argtypes = [C.c_void_p]
            L.pp_decoder_cache_size.restype = C.c_uint64
            L.pp_decoder_cache_size.argtypes = [C.c_void_p]
            L.pp_registry_clear.restype = None
            self._libs[which] = L
        self.L = self._libs[which]

    def codec(self, uuid: bytes, limit_bytes: int = 0) -> 'RefCodec':
        return RefCodec(self.L, uuid, limit_bytes)

    def registry_clear(self):
        """Empty XCodecCache::connect's registry (no pair may be alive)."""
        self.L.pp_registry_clear()


class RefCodec:
    def __init__(self, L, uuid: bytes, limit_bytes: int):
        self.L = L
        self.h = L.pp_codec_new(uuid, limit_bytes)
        if not self.h:
            raise ValueError('a codec needs a 36-byte UUID string')

    def pair(self) -> 'RefPair':
        return RefPair(self.L, self)

    def cache_size(self) -> int:
        return int(self.L.pp_codec_cache_size(self.h))

    def close(self):
        if getattr(self, 'h', None):
            self.L.pp_codec_free(self.h)
            self.h = None


class RefPair:
    ENCODER, DECODER = 0, 1

    def __init__(self, L, codec: RefCodec):
        self.L, self.codec = L, codec
        self.h = L.pp_pair_new(codec.h)

    def consume(self, which: int, data: bytes) -> Consumed:
        o = _Out()
        self.L.pp_consume(self.h, which, data, len(data), C.byref(o))
        return Consumed(C.string_at(o.to_peer, o.to_peer_len) if o.to_peer_len else b'',
                        C.string_at(o.to_local, o.to_local_len) if o.to_local_len else b'',
                        bool(o.encoder_eos), bool(o.decoder_eos), bool(o.encoder_error), bool(o.decoder_error))

    def encoder_consume(self, data: bytes) -> Consumed:
        return self.consume(self.ENCODER, data)

    def decoder_consume(self, data: bytes) -> Consumed:
        return self.consume(self.DECODER, data)

    def pending_frames(self) -> int:
        return int(self.L.pp_pending_frames(self.h))

    def decoder_cache_size(self):
        """Entries of the cache connected at <HELLO>; None before it."""
        n = int(self.L.pp_decoder_cache_size(self.h))
        return None if n == 2 ** 64 - 1 else n

    def close(self):
        if getattr(self, 'h', None):
            self.L.pp_pair_free(self.h)
            self.h = None
