#!/usr/bin/env python3
"""Time a hub's receive turn: N peers, one pipe each, one 64 KiB input frame per
pipe and turn -- the serial loop of xcg_pipe_decoder_consume against one
xcg_pipe_decoder_consume_many (which puts the N decode() calls, each on its own
peer cache, into one launch), and (with --parent-lib, a build of the parent
commit's library; N = 64 only) the parent's consume_many and serial loop.
Writes profiles/pipe_peers.txt.

Shape: N in {1, 2, 4, 8, 64, 256}; every peer has a sender codec and, on the
hub, a decoder context of its own.  Two rounds of pipe_cases.mixed data per
repetition: the payloads sent for the first time (EXTRACT-dense wires) and the
same payloads sent again (REF-dense wires).  Every variant has its own codecs,
caches and pipes and is fed the same payloads, so all do the same work; per
repetition the variants run alternately, in rotating order, and the figures
are the median over the repetitions with the spread (min .. max).  The clock
is the host's around calls that end in a stream synchronisation (the pipe
calls return host memory).  Encoding and the replies to the senders are not
timed.

    python scripts/pipe_peers_time.py [--parent-lib wanproxy_amd/libxcgpu.parent.so] [--bench-ab FILE]
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

FRAME = 64 * 1024
SEGMENTS = 1 << 12                       # a cache per peer and side: small


def uuid_of(i):
    return b'%08x-1c3f-4a6e-9b0d-7f1e3c5a8b2d' % (0xB0000000 + i)


class PipeOut(C.Structure):
    _fields_ = [('to_peer', C.c_void_p), ('to_peer_len', C.c_uint64), ('to_local', C.c_void_p),
                ('to_local_len', C.c_uint64), ('local_eos', C.c_int), ('peer_eos', C.c_int)]


def ok(rc):
    if rc != 0:
        raise RuntimeError(f'xcgpu call failed ({rc})')


class Side:
    """One variant: a library, the hub's codec, and per peer a sender codec, the
    peer's cache on the hub and a pipe pair."""

    def __init__(self, path, n):
        self.L = L = C.CDLL(path)
        self.n = n
        vp = C.c_void_p
        L.xcg_ctx_create_ex.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.POINTER(vp)]
        L.xcg_pipe_create.argtypes = [vp, vp, C.c_char_p, C.POINTER(vp)]
        L.xcg_pipe_encoder_consume.argtypes = [vp, C.c_char_p, C.c_uint64, C.POINTER(PipeOut)]
        L.xcg_pipe_decoder_consume.argtypes = [vp, C.c_char_p, C.c_uint64, C.POINTER(PipeOut)]
        L.xcg_pipe_decoder_consume_many.argtypes = [C.POINTER(vp), C.POINTER(C.c_char_p), C.POINTER(C.c_uint64),
                                                    C.c_uint32, C.POINTER(PipeOut), C.POINTER(C.c_int)]
        L.xcg_pipe_destroy.argtypes = [vp]
        L.xcg_ctx_destroy.argtypes = [vp]
        self.hub = C.c_void_p()
        ok(L.xcg_ctx_create_ex(0, 0, SEGMENTS, C.byref(self.hub)))
        self.ctx = []
        self.send = (C.c_void_p * n)()
        self.recv = (C.c_void_p * n)()
        for i in range(n):
            sc, dc, s, r = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
            ok(L.xcg_ctx_create_ex(0, 0, SEGMENTS, C.byref(sc)))
            ok(L.xcg_ctx_create_ex(0, 0, SEGMENTS, C.byref(dc)))
            ok(L.xcg_pipe_create(sc, sc, uuid_of(i), C.byref(s)))
            ok(L.xcg_pipe_create(self.hub, dc, uuid_of(i), C.byref(r)))
            self.ctx += [sc, dc]
            self.send[i], self.recv[i] = s.value, r.value
        self.outs = (PipeOut * n)()

    def encode(self, payloads):
        wires = []
        for i, p in enumerate(payloads):
            ok(self.L.xcg_pipe_encoder_consume(self.send[i], p, len(p), C.byref(self.outs[i])))
            wires.append(C.string_at(self.outs[i].to_peer, self.outs[i].to_peer_len))
        return wires

    def decode(self, wires, many):
        """The timed part.  Returns (seconds, delivered bytes, replies)."""
        n = self.n
        ds = (C.c_char_p * n)(*wires)
        ls = (C.c_uint64 * n)(*[len(w) for w in wires])
        t0 = time.perf_counter()
        if many:
            ok(self.L.xcg_pipe_decoder_consume_many(self.recv, ds, ls, n, self.outs, None))
        else:
            for i in range(n):
                ok(self.L.xcg_pipe_decoder_consume(self.recv[i], wires[i], len(wires[i]), C.byref(self.outs[i])))
        dt = time.perf_counter() - t0
        return dt, sum(o.to_local_len for o in self.outs), [C.string_at(o.to_peer, o.to_peer_len) for o in self.outs]

    def reply(self, replies):
        for i, r in enumerate(replies):
            if r:
                ok(self.L.xcg_pipe_decoder_consume(self.send[i], r, len(r), C.byref(self.outs[i])))

    def close(self):
        for i in range(self.n):
            self.L.xcg_pipe_destroy(self.send[i])
            self.L.xcg_pipe_destroy(self.recv[i])
        for c in self.ctx + [self.hub]:
            self.L.xcg_ctx_destroy(c)


def measure(n, variants, reps, warm):
    """variants: [(label, library path, many)].  Returns {label: {round: [seconds]}}."""
    from pipe_cases import mixed
    sides = [(lab, Side(path, n), many) for lab, path, many in variants]
    times = {lab: {'extract': [], 'ref': []} for lab, _, _ in variants}
    try:
        for rep in range(warm + reps):
            payloads = [mixed(1000 * rep + i, FRAME) for i in range(n)]
            for rnd in ('extract', 'ref'):
                order = sides[rep % len(sides):] + sides[:rep % len(sides)]
                for lab, side, many in order:
                    wires = side.encode(payloads)
                    dt, got, replies = side.decode(wires, many)
                    assert got == n * FRAME, (lab, rnd, got)
                    side.reply(replies)
                    if rep >= warm:
                        times[lab][rnd].append(dt)
    finally:
        for _, side, _ in sides:
            side.close()
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help="the parent commit's libxcgpu.so (N = 64 only)")
    ap.add_argument('--sizes', default='1,2,4,8,64,256')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--bench-ab', default=None, help='a text file with the bench.py --full A/B to append')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles/pipe_peers.txt'))
    a = ap.parse_args()
    import torch  # noqa: F401  -- load torch's HIP runtime first, as wanproxy_amd.xcgpu does
    here = os.path.join(ROOT, 'wanproxy_amd/libxcgpu.so')
    lines = ['pipe decode on a hub, N peers with a decoder context each, one pipe and one 64 KiB input frame per peer (MI355X)',
             'scripts/pipe_peers_time.py: per repetition every variant decodes the same wires, alternately;',
             f'median of {a.reps} repetitions [min .. max], microseconds per turn and per pipe', '']
    for n in [int(s) for s in a.sizes.split(',')]:
        variants = [('serial', here, False), ('many', here, True)]
        if a.parent_lib and n == 64:
            variants = [('serial, parent', os.path.abspath(a.parent_lib), False),
                        ('many, parent', os.path.abspath(a.parent_lib), True)] + variants
        T = measure(n, variants, a.reps, a.warmup)
        for rnd, what in (('extract', 'first send (EXTRACT-dense)'), ('ref', 'sent again (REF-dense)')):
            lines.append(f'N = {n}, {what}')
            for lab, _, _ in variants:
                v = [1e6 * t for t in T[lab][rnd]]
                med = statistics.median(v)
                lines.append(f'  {lab:16s} {med:11.1f} us [{min(v):.1f} .. {max(v):.1f}]   {med / n:9.1f} us per pipe')
            lines.append('')
        print('\n'.join(lines[-2 * (len(variants) + 2):]), flush=True)
    if a.bench_ab and os.path.exists(a.bench_ab):
        lines += ['bench.py --full, `decode` and `tack_loop`, this commit against its parent, runs alternated:', '']
        lines += open(a.bench_ab).read().rstrip('\n').split('\n')
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines).rstrip('\n') + '\n')


if __name__ == '__main__':
    main()
