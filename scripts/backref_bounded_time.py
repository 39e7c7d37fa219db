#!/usr/bin/env python3
"""Time xcg_decode_batch on bounded and pair contexts, with and without
<BACKREF> ops in the stream, this build against a build of the parent commit's
library (--parent-lib).  Writes profiles/backref_bounded.txt.

Shape: --chunks (4096) x 64 KiB of synth.stream(dup 50), encoded as one stream
on a fresh cache, decoded in ONE call.  The contexts: bounded with a memory
limit of --limit-mib (512: the call's enters must fit the limit), a pair of
that memory cache over a disk of --disk-mib (1024: under a lap of writes), and
an unbounded one.  Two streams: the encoder's own (no BACKREF: the path that
must cost what it cost) and the same with BACKREFs inserted behind 30% of the
ops, each to a live slot of the decoder's window (the path this adds on
bounded and pair contexts; the parent declines it there, so the parent's
figure for it is the unbounded context's).

Per repetition every variant decodes the same stream on a cleared cache and a
fresh window, alternately, in rotating order; the figures are medians over the
repetitions with the spread [min .. max].  The clock is the host's around the
call, which ends in a stream synchronisation.

    python scripts/backref_bounded_time.py --parent-lib PATH/libxcgpu.so
"""
import argparse
import ctypes as C
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEG, MiB = 2048, 1 << 20
XCG_ENOTSUP = -95


def insert_backrefs(encs, oracle, rate, seed):
    """backref_streams.with_backrefs for long streams (a BACKREF to a live slot
    behind `rate` of the ops), with the window model kept as a hash -> slot map."""
    rng = random.Random(seed)
    slot, where, cursor, out, count = [0] * 256, {}, 0, [], 0
    for enc in encs:
        parts, i, n = [], 0, len(enc)
        while True:
            j = enc.find(b'\xf1', i)
            if j < 0 or j + 1 >= n:
                parts.append(enc[i:])
                break
            op = enc[j + 1]
            if op == 0:
                parts.append(enc[i:j + 2])
                i = j + 2
                continue
            size = 2 + SEG if op == 1 else 10
            h = oracle.hash(enc[j + 2:j + size]) if op == 1 else int.from_bytes(enc[j + 2:j + 10], 'big')
            old = where.pop(h, None)
            if old is not None:
                slot[old] = 0
            if slot[cursor]:
                where.pop(slot[cursor], None)
            slot[cursor], where[h] = h, cursor
            cursor = (cursor + 1) % 256
            parts.append(enc[i:j + size])
            i = j + size
            if rng.random() < rate:
                parts.append(bytes([0xF1, 0x03, rng.choice(list(where.values()))]))
                count += 1
        out.append(b''.join(parts))
    return out, count


class Side:
    """One variant: a library and a context of one kind."""

    def __init__(self, path, kind, limit, disk):
        self.L = L = C.CDLL(path)
        vp = C.c_void_p
        L.xcg_ctx_create_ex.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.POINTER(vp)]
        L.xcg_ctx_create_bounded.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.POINTER(vp)]
        L.xcg_ctx_create_pair.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(vp)]
        L.xcg_ctx_destroy.argtypes = [vp]
        L.xcg_cache_clear.argtypes = [vp]
        L.xcg_window_create.argtypes = [vp, C.POINTER(vp)]
        L.xcg_window_destroy.argtypes = [vp]
        L.xcg_decode_set_window.argtypes = [vp, vp]
        L.xcg_decode_batch.argtypes = [vp] * 4 + [C.c_uint32, C.c_uint32, vp, C.c_uint64] + [vp] * 5 + [C.c_uint32, vp, vp, vp]
        self.kind, self.limit, self.disk = kind, limit, disk
        self.ctx = None
        self.fresh()

    def fresh(self):
        L = self.L
        if self.ctx is not None and self.kind != 'pair' and L.xcg_cache_clear(self.ctx) == 0:
            return
        if self.ctx is not None:
            L.xcg_ctx_destroy(self.ctx)
        self.ctx = C.c_void_p()
        if self.kind == 'bounded':
            rc = L.xcg_ctx_create_bounded(0, 0, self.limit, C.byref(self.ctx))
        elif self.kind == 'pair':
            rc = L.xcg_ctx_create_pair(0, 0, self.limit, self.disk, C.byref(self.ctx))
        else:
            rc = L.xcg_ctx_create_ex(0, 0, 1 << 19, C.byref(self.ctx))
        if rc != 0:
            raise RuntimeError(f'context ({self.kind}): {rc}')

    def decode(self, S):
        """One timed call on a cleared cache and a fresh window: seconds, or None when declined."""
        L = self.L
        self.fresh()
        win = C.c_void_p()
        assert L.xcg_window_create(self.ctx, C.byref(win)) == 0 and L.xcg_decode_set_window(self.ctx, win) == 0
        nunk, total = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
        p = lambda t: C.c_void_p(t.data_ptr())
        import torch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = L.xcg_decode_batch(self.ctx, p(S['enc']), p(S['off']), p(S['len']), S['n'], S['maxlen'], p(S['out']),
                                S['cap'], p(S['oo']), p(S['ol']), p(S['st']), p(S['cons']), S['unk'].ctypes.data,
                                S['unk'].size, nunk.ctypes.data, total.ctypes.data, None)
        dt = time.perf_counter() - t0
        L.xcg_decode_set_window(self.ctx, None)
        L.xcg_window_destroy(win)
        if rc == XCG_ENOTSUP:
            return None
        if rc != 0 or int(nunk[0]) or int(S['st'].abs().max()) or int(total[0]) != S['decoded']:
            raise RuntimeError(f'{self.kind}: rc {rc}, unknown {int(nunk[0])}, decoded {int(total[0])} of {S["decoded"]}')
        return dt

    def close(self):
        self.L.xcg_ctx_destroy(self.ctx)


def device_stream(encs, decoded):
    import torch
    dev = torch.device('cuda', 0)
    lens = np.array([len(e) for e in encs], dtype=np.uint32)
    offs = np.zeros(len(encs), dtype=np.uint64)
    offs[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
    n = len(encs)
    z = lambda dt: torch.zeros(n, dtype=dt, device=dev)
    return {'enc': torch.from_numpy(np.frombuffer(b''.join(encs), dtype=np.uint8).copy()).to(dev),
            'off': torch.from_numpy(offs.view(np.int64)).to(dev), 'len': torch.from_numpy(lens.view(np.int32)).to(dev),
            'n': n, 'maxlen': int(lens.max()), 'cap': decoded + 4096,
            'out': torch.zeros(decoded + 4096, dtype=torch.uint8, device=dev), 'oo': z(torch.int64), 'ol': z(torch.int64),
            'st': z(torch.int32), 'cons': z(torch.int64), 'unk': np.zeros(1 << 16, np.uint64), 'decoded': decoded}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help="the parent commit's libxcgpu.so")
    ap.add_argument('--chunks', type=int, default=4096)
    ap.add_argument('--limit-mib', type=int, default=512)
    ap.add_argument('--disk-mib', type=int, default=1024)
    ap.add_argument('--kinds', default='bounded,pair,unbounded')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles/backref_bounded.txt'))
    a = ap.parse_args()
    import torch  # noqa: F401  -- load torch's HIP runtime first, as wanproxy_amd.xcgpu does
    from oracle.lib import MODE_STREAM, Oracle
    from wanproxy_amd import synth
    o = Oracle()
    chunk = 64 * 1024
    data = synth.stream(0xBB0, a.chunks * chunk, 50, 0)
    offs, lens = synth.chunks_of(data, chunk)
    plain = o.encode_batch(data, offs, lens, mode=MODE_STREAM)
    withb, nb = insert_backrefs(plain, o, 0.3, 0xBB0)
    streams = {'plain': device_stream(plain, len(data)), 'backref': device_stream(withb, len(data) + nb * SEG)}
    here = os.path.join(ROOT, 'wanproxy_amd/libxcgpu.so')
    builds = [('this', here)] + ([('parent', os.path.abspath(a.parent_lib))] if a.parent_lib else [])
    limit, disk = a.limit_mib * MiB, a.disk_mib * MiB
    kinds = a.kinds.split(',')
    sides = [(f'{kind}, {lab}', Side(path, kind, limit, disk)) for kind in kinds for lab, path in builds]
    T = {name: {lab: [] for lab, _ in sides} for name in streams}
    for rep in range(a.warmup + a.reps):
        for name, S in streams.items():
            for lab, side in sides[rep % len(sides):] + sides[:rep % len(sides)]:
                dt = side.decode(S)
                if rep >= a.warmup:
                    T[name][lab].append(dt)
    for _, side in sides:
        side.close()
    enc_mib = {name: sum(S['len'].cpu().numpy().view(np.uint32).astype(np.uint64)) / MiB for name, S in streams.items()}
    lines = [f'xcg_decode_batch, {a.chunks} x 64 KiB of synth.stream(dup 50) in one call (MI355X)',
             f'scripts/backref_bounded_time.py --chunks {a.chunks} --limit-mib {a.limit_mib} --disk-mib {a.disk_mib}'
             f' --reps {a.reps} --parent-lib <the parent commit\'s build>',
             f'bounded: {a.limit_mib} MiB memory limit; pair: that over a {a.disk_mib} MiB disk; every call on a cleared cache',
             'and a fresh window; variants alternate within a repetition, in rotating order;',
             f'median of {a.reps} repetitions [min .. max], milliseconds per call', '']
    med = {}
    for name, what in (('plain', f'no BACKREF ({enc_mib["plain"]:.1f} MiB encoded, {len(data) / MiB:.0f} MiB decoded)'),
                       ('backref', f'{nb} BACKREFs, rate 0.3 ({enc_mib["backref"]:.1f} MiB encoded, '
                                   f'{(len(data) + nb * SEG) / MiB:.0f} MiB decoded)')):
        lines.append(what)
        for lab, _ in sides:
            v = T[name][lab]
            if any(t is None for t in v):
                lines.append(f'  {lab:20s} declined (XCG_ENOTSUP)')
                continue
            v = [1e3 * t for t in v]
            med[name, lab] = (statistics.median(v), min(v), max(v))
            lines.append(f'  {lab:20s} {med[name, lab][0]:9.3f} ms [{min(v):.3f} .. {max(v):.3f}]')
        lines.append('')
    if a.parent_lib:
        lines.append('no BACKREF, this build\'s median against the parent\'s own min .. max:')
        for kind in kinds:
            m, (_, lo, hi) = med['plain', f'{kind}, this'][0], med['plain', f'{kind}, parent']
            verdict = 'within' if lo <= m <= hi else 'below the parent\'s fastest' if m < lo else 'ABOVE the parent\'s slowest'
            lines.append(f'  {kind:10s} {m:.3f} ms, parent [{lo:.3f} .. {hi:.3f}]: {verdict}')
        lines.append('')
    if a.parent_lib and 'unbounded' in kinds:
        lines.append('BACKREFs at rate 0.3, this build on the context against the parent on the unbounded context:')
        base = med['backref', 'unbounded, parent'][0]
        for kind in [k for k in kinds if k != 'unbounded']:
            m = med['backref', f'{kind}, this'][0]
            lines.append(f'  {kind:10s} {m:.3f} ms / {base:.3f} ms = {m / base:.2f}x')
    print('\n'.join(lines), flush=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines).rstrip('\n') + '\n')


if __name__ == '__main__':
    main()
