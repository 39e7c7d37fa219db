#!/usr/bin/env python3
"""Time the receiving side of N pipes from one peer: the serial loop of
xcg_pipe_decoder_consume against one xcg_pipe_decoder_consume_many, and (with
--parent-lib, a build of the parent commit's library) the same serial loop on
the parent.  Writes profiles/pipe_decode_many.txt.

--cache bounded|pair puts the peer cache (and both codecs) on a bounded context
of LIMIT bytes, or on a pair of that over a disk of DISK bytes; the parent's
library then also runs its consume_many (which serves these contexts pipe by
pipe), xcg_pipe_debug_set_run_min(2) makes this library take the batch at every
N >= 2 whatever run length the pipe layer takes by default, and the output goes to
profiles/pipe_decode_many_bounded.txt (appended per cache kind).

Shape: N in {1, 8, 64, 512} pipes on one unbounded decoder context, one 64 KiB
input frame each.  Two rounds of pipe_cases.mixed data per repetition: the
payloads sent for the first time (EXTRACT-dense wires) and the same payloads
sent again (REF-dense wires).  Every variant has its own sender codec, peer
cache and pipes and is fed the same payloads, so all do the same work; per
repetition the variants run alternately, in rotating order, and the figures
are the median over the repetitions with the spread (min .. max).  The clock
is the host's around calls that end in a stream synchronisation (the pipe
calls return host memory).  Encoding and the replies to the senders are not
timed.

    python scripts/pipe_decode_many_time.py [--parent-lib wanproxy_amd/libxcgpu.parent.so] [--bench-ab FILE]
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
LIMIT = 128 << 20                  # wanproxy.conf's memory cache
DISK = 256 << 20                   # (its disk is 1 GB; the FIFO does not lap in a run either way)


class PipeOut(C.Structure):
    _fields_ = [('to_peer', C.c_void_p), ('to_peer_len', C.c_uint64), ('to_local', C.c_void_p),
                ('to_local_len', C.c_uint64), ('local_eos', C.c_int), ('peer_eos', C.c_int)]


def ok(rc):
    if rc != 0:
        raise RuntimeError(f'xcgpu call failed ({rc})')


class Side:
    """One variant: a library, a sender codec, the peer cache and n pipe pairs."""

    def __init__(self, path, n, cache='unbounded'):
        self.L = L = C.CDLL(path)
        self.n = n
        vp = C.c_void_p
        L.xcg_ctx_create_ex.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.POINTER(vp)]
        L.xcg_ctx_create_bounded.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.POINTER(vp)]
        L.xcg_ctx_create_pair.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(vp)]
        L.xcg_pipe_create.argtypes = [vp, vp, C.c_char_p, C.POINTER(vp)]
        L.xcg_pipe_encoder_consume_many.argtypes = [C.POINTER(vp), C.POINTER(C.c_char_p), C.POINTER(C.c_uint64),
                                                    C.c_uint32, C.POINTER(PipeOut)]
        L.xcg_pipe_decoder_consume.argtypes = [vp, C.c_char_p, C.c_uint64, C.POINTER(PipeOut)]
        if hasattr(L, 'xcg_pipe_decoder_consume_many'):
            L.xcg_pipe_decoder_consume_many.argtypes = [C.POINTER(vp), C.POINTER(C.c_char_p), C.POINTER(C.c_uint64),
                                                        C.c_uint32, C.POINTER(PipeOut), C.POINTER(C.c_int)]
        L.xcg_pipe_destroy.argtypes = [vp]
        L.xcg_ctx_destroy.argtypes = [vp]
        self.ctx = [C.c_void_p() for _ in range(3)]       # sender codec, receiver codec, the peer's cache there
        for c in self.ctx:
            if cache == 'bounded':
                ok(L.xcg_ctx_create_bounded(0, 0, LIMIT, C.byref(c)))
            elif cache == 'pair':
                ok(L.xcg_ctx_create_pair(0, 0, LIMIT, DISK, C.byref(c)))
            else:
                ok(L.xcg_ctx_create_ex(0, 0, 1 << 19, C.byref(c)))
        self.send = (C.c_void_p * n)()
        self.recv = (C.c_void_p * n)()
        for i in range(n):
            s, r = C.c_void_p(), C.c_void_p()
            ok(L.xcg_pipe_create(self.ctx[0], self.ctx[0], UUID, C.byref(s)))
            ok(L.xcg_pipe_create(self.ctx[1], self.ctx[2], UUID, C.byref(r)))
            self.send[i], self.recv[i] = s.value, r.value
        self.outs = (PipeOut * n)()

    def encode(self, payloads):
        ds = (C.c_char_p * self.n)(*payloads)
        ls = (C.c_uint64 * self.n)(*[len(p) for p in payloads])
        ok(self.L.xcg_pipe_encoder_consume_many(self.send, ds, ls, self.n, self.outs))
        return [C.string_at(o.to_peer, o.to_peer_len) for o in self.outs]

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
        for c in self.ctx:
            self.L.xcg_ctx_destroy(c)


def measure(n, variants, reps, warm, cache='unbounded'):
    """variants: [(label, library path, many)].  Returns {label: {round: [seconds]}}."""
    from pipe_cases import mixed
    sides = [(lab, Side(path, n, cache), many) for lab, path, many in variants]
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
    ap.add_argument('--parent-lib', default=None, help="the parent commit's libxcgpu.so (serial loop only)")
    ap.add_argument('--sizes', default='1,8,64,512')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--bench-ab', default=None, help='a text file with the bench.py --full decode A/B to append')
    ap.add_argument('--cache', default='unbounded', choices=('unbounded', 'bounded', 'pair'))
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    classified = a.cache != 'unbounded'
    out = a.out or os.path.join(ROOT, 'profiles/pipe_decode_many_bounded.txt' if classified else
                                'profiles/pipe_decode_many.txt')
    import torch  # noqa: F401  -- load torch's HIP runtime first, as wanproxy_amd.xcgpu does
    here = os.path.join(ROOT, 'wanproxy_amd/libxcgpu.so')
    if classified:
        C.CDLL(here).xcg_pipe_debug_set_run_min(2)     # (process-wide: every Side of this library)
    variants = [('serial', here, False), ('many', here, True)]
    if a.parent_lib:
        variants.insert(0, ('serial, parent', os.path.abspath(a.parent_lib), False))
        if classified:
            variants.append(('many, parent', os.path.abspath(a.parent_lib), True))
    what = {'unbounded': 'unbounded', 'bounded': 'bounded (%d MiB)' % (LIMIT >> 20),
            'pair': 'pair (%d MiB over a %d MiB disk)' % (LIMIT >> 20, DISK >> 20)}[a.cache]
    big = f' (N = 512: {max(3, a.reps // 2)})' if '512' in a.sizes.split(',') else ''
    lines = [f'pipe decode, N pipes on one {what} decoder context, one 64 KiB input frame each (MI355X)',
             'scripts/pipe_decode_many_time.py: per repetition every variant decodes the same wires, alternately;',
             f'median of {a.reps} repetitions{big} [min .. max], microseconds per turn and per pipe', '']
    for n in [int(s) for s in a.sizes.split(',')]:
        reps = a.reps if n < 512 else max(3, a.reps // 2)
        T = measure(n, variants, reps, a.warmup, a.cache)
        for rnd, what in (('extract', 'first send (EXTRACT-dense)'), ('ref', 'sent again (REF-dense)')):
            lines.append(f'N = {n}, {what}')
            for lab, _, _ in variants:
                v = [1e6 * t for t in T[lab][rnd]]
                med = statistics.median(v)
                lines.append(f'  {lab:16s} {med:11.1f} us [{min(v):.1f} .. {max(v):.1f}]   {med / n:9.1f} us per pipe')
            lines.append('')
        print('\n'.join(lines[-8:]), flush=True)
    if a.bench_ab and os.path.exists(a.bench_ab):
        lines += ['bench.py --full, `decode` (xcg_decode_batch), this commit against its parent, runs alternated:', '']
        lines += open(a.bench_ab).read().rstrip('\n').split('\n')
    with open(out, 'a' if classified else 'w') as f:
        f.write('\n'.join(lines).rstrip('\n') + '\n' + ('\n' if classified else ''))


if __name__ == '__main__':
    main()
