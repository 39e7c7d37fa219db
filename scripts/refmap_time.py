#!/usr/bin/env python
"""What the encoder refmap costs (needs a GPU; reads nothing but this repository).

1. Kernel time beside its encode batch: HIP-event time of xcg_encode_refmap_batch
   over the outputs of a 4096 x 64 KiB XCG_SEM_STREAM batch, beside that batch's
   own event time in the same run -- cold (few REFs), then the same data again
   (REF-dense).

2. xcg_pipe_encoder_consume_many, 64 pipes x 512 KiB, cold and REF-dense, wall
   time: this build against another build of the library (--other-lib, e.g. the
   parent commit's), in fresh child processes that alternate between the two.

    python scripts/refmap_time.py [--other-lib PATH] [--out profiles/refmap.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEG = 2048


def med(v):
    return statistics.median(v)


def kernel_part(chunks=4096, chunk=65536, reps=5, rounds=2):
    import torch
    from wanproxy_amd import synth
    from wanproxy_amd.xcgpu import XCG_SEM_STREAM, Context
    dev = torch.device('cuda', 0)
    d = np.frombuffer(synth.stream(0x7EF, chunks * chunk, 50, 2), np.uint8)
    offs, lens = synth.chunks_of(d, chunk)
    n = len(offs)
    bounds = 2 * lens.astype(np.uint64) + 16
    oo = np.zeros(n, np.uint64)
    oo[1:] = np.cumsum(bounds)[:-1]
    d_in = torch.from_numpy(d.copy()).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_oo = torch.from_numpy(oo.view(np.int64)).to(dev)
    d_out = torch.zeros(int(bounds.sum()), dtype=torch.uint8, device=dev)
    d_ol = torch.zeros(n, dtype=torch.int64, device=dev)
    cap = 32                                            # a 64 KiB chunk references at most 32 segments
    d_h = torch.zeros(n * cap, dtype=torch.int64, device=dev)
    d_p = torch.zeros(n * cap, dtype=torch.int32, device=dev)
    d_c = torch.zeros(n, dtype=torch.int32, device=dev)
    d_w = torch.zeros(n, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b)

    rows = {'cold': [], 'dense': []}
    for _ in range(rounds):
        ctx = Context(0)
        for phase in ('cold', 'dense'):
            t_enc = timed(lambda: ctx.encode_batch_device(d_in, d_off, d_len, n, chunk, d_out, d_oo, d_ol,
                                                          semantics=XCG_SEM_STREAM))
            t_ref = [timed(lambda: ctx.encode_refmap_device(d_out, d_oo, d_ol, n, 2 * chunk + 16, d_h, d_p, cap,
                                                            d_c, d_w)) for _ in range(reps)]
            ctx.status()
            assert bool((d_w == d_ol).all()), 'the walk did not cover every output'
            rows[phase].append(dict(encode_ms=t_enc, refmap_ms=t_ref, entries=int(d_c.sum()),
                                    enc_bytes=int(d_ol.sum())))
        ctx.close()
    return dict(chunks=n, chunk=chunk, in_bytes=int(d.size), rows=rows)


UUID = b'0d1f4c8e-95a3-4b2d-8f6e-3c7a9b1d2e4f'


def pipe_child(pipes=64, per=512 * 1024, reps=3, dense_reps=4):
    """One process, one library (XCGPU_LIB): per repeat a fresh codec context and
    its pipes, one cold consume_many, then REF-dense ones over the same data."""
    from wanproxy_amd.xcgpu import Context, PipePair
    rng = np.random.default_rng(0x7EF)
    datas = [rng.integers(0, 256, per, dtype=np.uint8).tobytes() for _ in range(pipes)]
    warm = Context(0, cache_segments=1 << 10)            # (the runtime and the library are up before a timing)
    wp = PipePair(warm, warm, UUID)
    wp.encoder_consume(datas[0][:8 * SEG])
    wp.close()
    warm.close()
    cold, dense, nbytes = [], [], []
    for _ in range(reps):
        enc, dec = Context(0, cache_segments=1 << 16), Context(0, cache_segments=1 << 10)
        ps = [PipePair(enc, dec, UUID) for _ in range(pipes)]
        t0 = time.perf_counter()
        out = PipePair.encoder_consume_many(ps, datas)
        cold.append((time.perf_counter() - t0) * 1e3)
        nbytes.append(sum(map(len, out)))
        for _ in range(dense_reps):
            t0 = time.perf_counter()
            out = PipePair.encoder_consume_many(ps, datas)
            dense.append((time.perf_counter() - t0) * 1e3)
        nbytes.append(sum(map(len, out)))
        for p in ps:
            p.close()
        enc.close()
        dec.close()
    print(json.dumps(dict(cold_ms=cold, dense_ms=dense, wire_bytes=nbytes[:2])))


def pipe_part(other_lib, sessions=3):
    libs = [('this', None)] + ([('other', other_lib)] if other_lib else [])
    res = {name: dict(cold_ms=[], dense_ms=[], wire_bytes=None) for name, _ in libs}
    for _ in range(sessions):
        for name, path in libs:                           # the two alternate
            env = dict(os.environ)
            env.pop('XCGPU_LIB', None)
            if path:
                env['XCGPU_LIB'] = os.path.abspath(path)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--pipe-child'], env=env, cwd=ROOT,
                               capture_output=True, text=True, timeout=240)
            if r.returncode != 0:
                raise SystemExit(f'pipe child ({name}) failed with {r.returncode}:\n{r.stderr[-2000:]}')
            j = json.loads(r.stdout.strip().splitlines()[-1])
            res[name]['cold_ms'] += j['cold_ms']
            res[name]['dense_ms'] += j['dense_ms']
            res[name]['wire_bytes'] = j['wire_bytes']
    return res


def fmt(v):
    return f'median {med(v):8.2f} ms   min {min(v):8.2f}   max {max(v):8.2f}   n {len(v)}'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--other-lib', default=None, help="another build of libxcgpu.so to alternate with (the parent's)")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles/refmap.txt'))
    ap.add_argument('--pipe-child', action='store_true')
    a = ap.parse_args()
    if a.pipe_child:
        return pipe_child()
    # (the pipe part first: its child processes start before this one opens the GPU)
    p = pipe_part(a.other_lib)
    k = kernel_part()
    lines = ['encoder refmap: what the by-product costs  (scripts/refmap_time.py)', '']
    lines.append(f"1. xcg_encode_refmap_batch beside its XCG_SEM_STREAM batch: {k['chunks']} x {k['chunk']} B, "
                 f"{k['in_bytes'] >> 20} MiB, HIP events, one stream")
    for phase in ('cold', 'dense'):
        for r in k['rows'][phase]:
            m = med(r['refmap_ms'])
            lines.append(f"   {phase:5s}  encode batch {r['encode_ms']:9.2f} ms   refmap {m:7.3f} ms "
                         f"(min {min(r['refmap_ms']):.3f}, max {max(r['refmap_ms']):.3f}, n {len(r['refmap_ms'])})   "
                         f"ratio {m / r['encode_ms']:.4f}   entries {r['entries']}   encoded {r['enc_bytes']} B")
    lines.append('')
    lines.append('2. xcg_pipe_encoder_consume_many, 64 pipes x 512 KiB, wall time per call; fresh processes, the '
                 'builds alternating')
    for name in p:
        lines.append(f"   {name:5s} cold   {fmt(p[name]['cold_ms'])}")
        lines.append(f"   {name:5s} dense  {fmt(p[name]['dense_ms'])}   (wire bytes cold / dense {p[name]['wire_bytes']})")
    if 'other' in p:
        lines.append(f"   wire bytes equal in both builds: {p['this']['wire_bytes'] == p['other']['wire_bytes']}")
        for ph in ('cold_ms', 'dense_ms'):
            t, o = p['this'][ph], p['other'][ph]
            spread = max(o) - min(o)
            ok = med(t) <= med(o) + spread
            lines.append(f"   {ph[:-3]:5s}  this - other = {med(t) - med(o):+.2f} ms; the other build's own spread "
                         f"{spread:.2f} ms: {'within it' if ok else 'SLOWER than the other build by more than that'}")
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
