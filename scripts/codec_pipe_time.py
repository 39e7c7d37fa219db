#!/usr/bin/env python3
"""Time the configured codec (XCodec pipe pair + zlib level 6) over N pipes, one
64 KiB consume each, in both directions.  Writes profiles/codec_pipe.txt.

Variants, all fed the same payloads:
  (a) chain, many     the chain as it could be written before xcg_codec_*:
                      xcg_pipe_encoder_consume_many then ONE xcg_zdeflate_host
                      over all pipes; ONE xcg_zinflate_host then
                      xcg_pipe_decoder_consume_many.  On --parent-lib (a build
                      of the parent commit) when given, else on this build.
  (b) chain, serial   the same served one pipe at a time.
  (c) codec, host     xcg_codec_send_many / xcg_codec_receive_many with
                      xcg_debug_set_codec_fused(0).
  (d) codec, fused    the same with the wire kept on the device.

Shape: N in {1, 8, 64} pipes on one unbounded codec pair.  Two rounds of
pipe_cases.mixed data per repetition: the payloads sent for the first time
(EXTRACT-dense wires) and sent again (REF-dense wires).  Per repetition the
variants run alternately, in rotating order; the figures are medians over the
repetitions with the spread (min .. max).  The clock is the host's around calls
that return host memory (each ends in a stream synchronisation).  The replies
to the senders are delivered, untimed; (c) and (d) compress them inside the
timed receive call (the layer's rule), (a) and (b) hand them back as they are.

    python scripts/codec_pipe_time.py [--parent-lib wanproxy_amd/libxcgpu.parent.so]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

UUID = b'5e2d8b4a-1c3f-4a6e-9b0d-7f1e3c5a8b2d'
FRAME = 64 * 1024
LEVEL = 6
vp = C.c_void_p


class PipeOut(C.Structure):
    _fields_ = [('to_peer', vp), ('to_peer_len', C.c_uint64), ('to_local', vp), ('to_local_len', C.c_uint64),
                ('local_eos', C.c_int), ('peer_eos', C.c_int)]


def ok(rc):
    if rc != 0:
        raise RuntimeError(f'xcgpu call failed ({rc})')


def load(path):
    L = C.CDLL(path)
    many = [C.POINTER(vp), C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(PipeOut)]
    L.xcg_ctx_create_ex.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.POINTER(vp)]
    L.xcg_ctx_destroy.argtypes = [vp]
    L.xcg_pipe_create.argtypes = [vp, vp, C.c_char_p, C.POINTER(vp)]
    L.xcg_pipe_destroy.argtypes = [vp]
    L.xcg_pipe_encoder_consume_many.argtypes = many
    L.xcg_pipe_decoder_consume_many.argtypes = many + [C.POINTER(C.c_int)]
    L.xcg_pipe_encoder_consume.argtypes = [vp, C.c_char_p, C.c_uint64, C.POINTER(PipeOut)]
    L.xcg_pipe_decoder_consume.argtypes = [vp, C.c_char_p, C.c_uint64, C.POINTER(PipeOut)]
    L.xcg_zdeflate_bound.argtypes = [C.c_uint32]
    L.xcg_zdeflate_bound.restype = C.c_uint64
    L.xcg_zdeflate_create.argtypes = [C.c_int, C.c_int, C.c_uint32, C.POINTER(vp)]
    L.xcg_zdeflate_destroy.argtypes = [vp]
    L.xcg_zdeflate_host.argtypes = [vp] * 5 + [C.c_uint32] + [vp] * 6
    L.xcg_zinflate_create.argtypes = [C.c_int, C.c_uint32, C.POINTER(vp)]
    L.xcg_zinflate_destroy.argtypes = [vp]
    L.xcg_zinflate_host.argtypes = [vp] * 5 + [C.c_uint32] + [vp] * 5
    if hasattr(L, 'xcg_codec_create'):
        L.xcg_codec_create.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32, C.POINTER(vp)]
        L.xcg_codec_destroy.argtypes = [vp]
        L.xcg_codec_pipe_create.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
        L.xcg_codec_pipe_destroy.argtypes = [vp]
        L.xcg_codec_send_many.argtypes = many + [C.POINTER(C.c_int)]
        L.xcg_codec_receive_many.argtypes = many + [C.POINTER(C.c_int)]
    return L


def arrays(items):
    n = len(items)
    return (C.c_char_p * n)(*items), (C.c_uint64 * n)(*[len(x) for x in items])


class Chain:
    """(a), (b): pipe pairs and zlib objects driven by this script."""

    def __init__(self, path, n, serial):
        import numpy as np
        self.np, self.L, self.n, self.serial = np, load(path), n, serial
        L = self.L
        self.ctx = [vp() for _ in range(3)]               # sender codec, receiver codec, the peer's cache there
        for c in self.ctx:
            ok(L.xcg_ctx_create_ex(0, 0, 1 << 19, C.byref(c)))
        self.send, self.recv = (vp * n)(), (vp * n)()
        for i in range(n):
            s, r = vp(), vp()
            ok(L.xcg_pipe_create(self.ctx[0], self.ctx[0], UUID, C.byref(s)))
            ok(L.xcg_pipe_create(self.ctx[1], self.ctx[2], UUID, C.byref(r)))
            self.send[i], self.recv[i] = s.value, r.value
        self.zd, self.zi = vp(), vp()
        ok(L.xcg_zdeflate_create(0, LEVEL, n, C.byref(self.zd)))
        ok(L.xcg_zinflate_create(0, n, C.byref(self.zi)))
        self.und = [b''] * n
        self.outs = (PipeOut * n)()

    def _deflate(self, streams, wires):
        np, m = self.np, len(wires)
        lens = np.array([len(w) for w in wires], dtype=np.uint32)
        in_off = np.zeros(m, dtype=np.uint64)
        in_off[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
        room = np.array([(int(self.L.xcg_zdeflate_bound(int(x))) + 3) & ~3 for x in lens], dtype=np.uint64)
        out_off = np.zeros(m, dtype=np.uint64)
        out_off[1:] = np.cumsum(room)[:-1]
        out = np.empty(int(room.sum()), dtype=np.uint8)
        made, dl = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint64)
        st = np.array(streams, dtype=np.uint32)
        blob = b''.join(wires)
        ok(self.L.xcg_zdeflate_host(self.zd, blob, in_off.ctypes.data, lens.ctypes.data, st.ctypes.data, m, None, None,
                                    out.ctypes.data, out_off.ctypes.data, made.ctypes.data, dl.ctypes.data))
        res = []
        for i, s in enumerate(streams):       # DeflatePipe's undelivered bytes first
            q = self.und[s] + out[int(out_off[i]):int(out_off[i]) + int(made[i])].tobytes()
            res.append(q[:int(dl[i])])
            self.und[s] = q[int(dl[i]):]
        return res

    def _inflate(self, streams, datas):
        np, m = self.np, len(datas)
        lens = np.array([len(w) for w in datas], dtype=np.uint32)
        in_off = np.zeros(m, dtype=np.uint64)
        in_off[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
        cap = np.array([4 * int(x) + 65536 for x in lens], dtype=np.uint32)
        out_off = np.zeros(m, dtype=np.uint64)
        out_off[1:] = np.cumsum(cap.astype(np.uint64))[:-1]
        out = np.empty(int(cap.sum()), dtype=np.uint8)
        ol, stt = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.int32)
        st = np.array(streams, dtype=np.uint32)
        ok(self.L.xcg_zinflate_host(self.zi, b''.join(datas), in_off.ctypes.data, lens.ctypes.data, st.ctypes.data, m,
                                    out.ctypes.data, out_off.ctypes.data, cap.ctypes.data, ol.ctypes.data,
                                    stt.ctypes.data))
        assert (stt >= 0).all()
        return [out[int(out_off[i]):int(out_off[i]) + int(ol[i])].tobytes() for i in range(m)]

    def send_turn(self, payloads):
        n, L = self.n, self.L
        t0 = time.perf_counter()
        if self.serial:
            res = []
            for i in range(n):
                ok(L.xcg_pipe_encoder_consume(self.send[i], payloads[i], len(payloads[i]), C.byref(self.outs[i])))
                w = C.string_at(self.outs[i].to_peer, self.outs[i].to_peer_len)
                res += self._deflate([i], [w])
        else:
            ds, ls = arrays(payloads)
            ok(L.xcg_pipe_encoder_consume_many(self.send, ds, ls, n, self.outs))
            res = self._deflate(list(range(n)), [C.string_at(o.to_peer, o.to_peer_len) for o in self.outs])
        return time.perf_counter() - t0, res

    def recv_turn(self, datas):
        n, L = self.n, self.L
        t0 = time.perf_counter()
        if self.serial:
            for i in range(n):
                w = self._inflate([i], [datas[i]])[0]
                if w:
                    ok(L.xcg_pipe_decoder_consume(self.recv[i], w, len(w), C.byref(self.outs[i])))
                else:
                    self.outs[i] = PipeOut()
        else:
            wires = self._inflate(list(range(n)), datas)
            live = [i for i in range(n) if wires[i]]
            for i in range(n):
                self.outs[i] = PipeOut()
            if live:
                hs = (vp * len(live))(*[self.recv[i] for i in live])
                ds, ls = arrays([wires[i] for i in live])
                po = (PipeOut * len(live))()
                ok(L.xcg_pipe_decoder_consume_many(hs, ds, ls, len(live), po, None))
                for i, o in zip(live, po):
                    self.outs[i] = o
        dt = time.perf_counter() - t0
        got = sum(o.to_local_len for o in self.outs)
        for i, o in enumerate(self.outs):     # the replies (<ADVANCE>), untimed and outside zlib
            if o.to_peer_len:
                r = C.string_at(o.to_peer, o.to_peer_len)
                ok(L.xcg_pipe_decoder_consume(self.send[i], r, len(r), C.byref(PipeOut())))
        return dt, got

    def close(self):
        for i in range(self.n):
            self.L.xcg_pipe_destroy(self.send[i])
            self.L.xcg_pipe_destroy(self.recv[i])
        self.L.xcg_zdeflate_destroy(self.zd)
        self.L.xcg_zinflate_destroy(self.zi)
        for c in self.ctx:
            self.L.xcg_ctx_destroy(c)


class Layer:
    """(c), (d): xcg_codec_*."""

    def __init__(self, path, n, fused):
        self.L, self.n, self.fused = load(path), n, fused
        L = self.L
        self.ctx = [vp() for _ in range(3)]
        for c in self.ctx:
            ok(L.xcg_ctx_create_ex(0, 0, 1 << 19, C.byref(c)))
        self.cs, self.cr = vp(), vp()
        ok(L.xcg_codec_create(self.ctx[0], self.ctx[0], 0, LEVEL, n, C.byref(self.cs)))
        ok(L.xcg_codec_create(self.ctx[1], self.ctx[2], 0, LEVEL, n, C.byref(self.cr)))
        self.send, self.recv = (vp * n)(), (vp * n)()
        for i in range(n):
            s, r = vp(), vp()
            ok(L.xcg_codec_pipe_create(self.cs, UUID, C.byref(s)))
            ok(L.xcg_codec_pipe_create(self.cr, UUID, C.byref(r)))
            self.send[i], self.recv[i] = s.value, r.value
        self.outs = (PipeOut * n)()

    def send_turn(self, payloads):
        self.L.xcg_debug_set_codec_fused(int(self.fused))
        ds, ls = arrays(payloads)
        t0 = time.perf_counter()
        ok(self.L.xcg_codec_send_many(self.send, ds, ls, self.n, self.outs, None))
        dt = time.perf_counter() - t0
        return dt, [C.string_at(o.to_peer, o.to_peer_len) for o in self.outs]

    def recv_turn(self, datas):
        ds, ls = arrays(datas)
        t0 = time.perf_counter()
        ok(self.L.xcg_codec_receive_many(self.recv, ds, ls, self.n, self.outs, None))
        dt = time.perf_counter() - t0
        got = sum(o.to_local_len for o in self.outs)
        back = [(i, C.string_at(o.to_peer, o.to_peer_len)) for i, o in enumerate(self.outs) if o.to_peer_len]
        if back:                              # the replies, untimed, through the senders' inflate
            hs = (vp * len(back))(*[self.send[i] for i, _ in back])
            rs, rl = arrays([r for _, r in back])
            ok(self.L.xcg_codec_receive_many(hs, rs, rl, len(back), (PipeOut * len(back))(), None))
        return dt, got

    def close(self):
        for i in range(self.n):
            self.L.xcg_codec_pipe_destroy(self.send[i])
            self.L.xcg_codec_pipe_destroy(self.recv[i])
        self.L.xcg_codec_destroy(self.cs)
        self.L.xcg_codec_destroy(self.cr)
        for c in self.ctx:
            self.L.xcg_ctx_destroy(c)


def measure(n, variants, reps, warm):
    from pipe_cases import mixed
    sides = [(lab, make(n)) for lab, make in variants]
    times = {lab: {(rnd, d): [] for rnd in ('extract', 'ref') for d in ('send', 'recv')} for lab, _ in variants}
    try:
        for rep in range(warm + reps):
            payloads = [mixed(1000 * rep + i, FRAME) for i in range(n)]
            for rnd in ('extract', 'ref'):
                order = sides[rep % len(sides):] + sides[:rep % len(sides)]
                seen = set()
                for lab, side in order:
                    ts, wires = side.send_turn(payloads)
                    tr, got = side.recv_turn(wires)
                    seen.add((sum(map(len, wires)), got))
                    if rep >= warm:
                        times[lab][(rnd, 'send')].append(ts)
                        times[lab][(rnd, 'recv')].append(tr)
                assert len(seen) == 1, (n, rep, rnd, seen)     # every variant made and delivered the same bytes
    finally:
        for _, side in sides:
            side.close()
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help="the parent commit's libxcgpu.so, for (a) and (b)")
    ap.add_argument('--sizes', default='1,8,64')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles/codec_pipe.txt'))
    a = ap.parse_args()
    import torch  # noqa: F401  -- load torch's HIP runtime first, as wanproxy_amd.xcgpu does
    here = os.path.join(ROOT, 'wanproxy_amd/libxcgpu.so')
    chain = os.path.abspath(a.parent_lib) if a.parent_lib else here
    on = 'parent build' if a.parent_lib else 'this build'
    variants = [(f'(a) chain, many ({on})', lambda n: Chain(chain, n, False)),
                (f'(b) chain, serial ({on})', lambda n: Chain(chain, n, True)),
                ('(c) codec, host composed', lambda n: Layer(here, n, False)),
                ('(d) codec, fused send', lambda n: Layer(here, n, True))]
    lines = [f'configured codec (XCodec pipe pair + zlib level {LEVEL}), N pipes, one 64 KiB consume each (MI355X)',
             'scripts/codec_pipe_time.py: per repetition every variant serves the same payloads, alternately;',
             f'median of {a.reps} repetitions [min .. max], microseconds per turn and per pipe',
             '(c) and (d) differ in the send path only; their receive paths are the same code, and their receive turns',
             "include the deflate batch of the pair's replies (<ADVANCE>), which (a) and (b) hand back uncompressed", '']
    for n in [int(s) for s in a.sizes.split(',')]:
        T = measure(n, variants, a.reps, a.warmup)
        for rnd, what in (('extract', 'first send (EXTRACT-dense)'), ('ref', 'sent again (REF-dense)')):
            for d, dname in (('send', 'send turn'), ('recv', 'receive turn')):
                lines.append(f'N = {n}, {what}, {dname}')
                for lab, _ in variants:
                    v = [1e6 * t for t in T[lab][(rnd, d)]]
                    med = statistics.median(v)
                    lines.append(f'  {lab:34s} {med:11.1f} us [{min(v):.1f} .. {max(v):.1f}]   {med / n:9.1f} us per pipe')
                lines.append('')
        print('\n'.join(lines[-28:]), flush=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines).rstrip('\n') + '\n')


if __name__ == '__main__':
    main()
