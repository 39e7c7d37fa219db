#!/usr/bin/env python3
"""Decode rate with name reuse inside the batch (xcodec_decoder.cc:106-136)
beside the same stream's collision-free twin, on one build.

The stream has the shape of an S2 (stream-semantics) encoding of C2-like data:
chunks of 32 ops, EXTRACTs of new segments and REFs of earlier ones.  A stated
share of the EXTRACTs carries a variant of one of a few collision families
(three distinct segments of one XCodecHash each: +2, -4, +2 on three odd
bytes), so later EXTRACTs of a family's hash replace its bytes and the REFs of
that hash resolve by position (the name-reuse resolver).  In the twin every
family EXTRACT carries a fresh segment of its own hash and the family's REFs
name the latest of those: the same ops, sizes and offsets without any
duplicate EXTRACT (the path bench.py's decode figure takes).

Every step decodes the whole batch on an empty decoder cache (as bench.py's
decode does); both outputs are checked against the oracle restatement.  Prints
one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEG = 2048
OPS = 32


def odd_segments(rng, n):
    return (rng.integers(3, 101, size=(n, SEG), dtype=np.uint8) * 2 + 1).astype(np.uint8)


def build_streams(oracle, chunks, share, families, seed):
    """(reuse chunks, twin chunks, decoded bytes, family EXTRACTs)."""
    rng = np.random.default_rng(seed)
    fam = []
    for base in odd_segments(rng, families):
        vs = []
        for j in range(3):
            v = base.copy()
            o = 100 + 40 * j
            v[o] += 2
            v[o + 1] -= 4
            v[o + 2] += 2
            vs.append(v.tobytes())
        h = oracle.hash(vs[0])
        assert all(oracle.hash(v) == h for v in vs) and len(set(vs)) == 3
        fam.append((h, vs))
    n_ops = chunks * OPS
    # ordinary segments: any bytes, each of a hash of its own (XCodecHash is a pair of sums: chance collisions
    # among 10^5 random segments are rare but not impossible, and the twin must not hold a single one)
    fresh = rng.integers(0, 256, size=(2 * n_ops, SEG), dtype=np.uint8)
    nfresh = 0
    seen = {h for h, _ in fam}

    def new_seg():
        nonlocal nfresh
        while True:
            s = fresh[nfresh].tobytes()
            nfresh += 1
            h = oracle.hash(s)
            if h not in seen:
                seen.add(h)
                return s, h

    ext = lambda s: b'\xf1\x01' + s
    ref = lambda h: b'\xf1\x02' + int(h).to_bytes(8, 'big')
    plain = []                                                # hashes of the ordinary EXTRACTs so far
    twin_of = {}                                              # family -> hash of its latest EXTRACT in the twin
    a_chunks, b_chunks, n_fam = [], [], 0
    for _ in range(chunks):
        a, b = [], []
        for _ in range(OPS):
            is_ref = plain and rng.random() < 0.5
            in_fam = rng.random() < share
            if in_fam and (not is_ref or twin_of):
                if is_ref:
                    f = list(twin_of)[int(rng.integers(len(twin_of)))]
                    a.append(ref(fam[f][0]))
                    b.append(ref(twin_of[f]))
                else:
                    f = int(rng.integers(families))
                    a.append(ext(fam[f][1][int(rng.integers(3))]))
                    s, h = new_seg()
                    b.append(ext(s))
                    twin_of[f] = h
                    n_fam += 1
            elif is_ref:
                op = ref(plain[int(rng.integers(len(plain)))])
                a.append(op)
                b.append(op)
            else:
                s, h = new_seg()
                plain.append(h)
                a.append(ext(s))
                b.append(ext(s))
        a_chunks.append(b''.join(a))
        b_chunks.append(b''.join(b))
    return a_chunks, b_chunks, n_ops * SEG, n_fam


def measure(oracle, encs, decoded, steps, warmup, dev):
    import torch
    from wanproxy_amd.xcgpu import Context, _check, lib
    n = len(encs)
    lens = np.array([len(e) for e in encs], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
    blob = b''.join(encs)
    d_enc = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_out = torch.empty(decoded + 4096, dtype=torch.uint8, device=dev)
    d_oo = torch.zeros(n, dtype=torch.int64, device=dev)
    d_ol = torch.zeros(n, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    d_cons = torch.zeros(n, dtype=torch.int64, device=dev)
    unk = np.zeros(16, np.uint64)
    nunk = np.zeros(1, np.uint32)
    tot = np.zeros(1, np.uint64)
    ctx = Context(dev.index, cache_segments=1 << 17)
    stream = torch.cuda.current_stream(dev)

    def dec():
        ctx.cache_clear()
        _check(lib().xcg_decode_batch(ctx.h, C.c_void_p(d_enc.data_ptr()), C.c_void_p(d_off.data_ptr()),
                                      C.c_void_p(d_len.data_ptr()), n, int(lens.max()), C.c_void_p(d_out.data_ptr()),
                                      d_out.numel(), C.c_void_p(d_oo.data_ptr()), C.c_void_p(d_ol.data_ptr()),
                                      C.c_void_p(d_st.data_ptr()), C.c_void_p(d_cons.data_ptr()), unk.ctypes.data,
                                      unk.size, nunk.ctypes.data, tot.ctypes.data, C.c_void_p(stream.cuda_stream)))
    for _ in range(warmup):
        dec()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        dec()
    torch.cuda.synchronize(dev)
    wall = (time.perf_counter() - t0) / steps
    stats = ctx.decode_reuse_stats()
    got = d_out[:decoded].cpu().numpy().tobytes()
    ctx.close()
    oc = oracle.cache_new()
    ok, exp, cons, ounk = oracle.decode(blob, oc, out_cap=decoded + 4096)
    oracle.cache_free(oc)
    if not ok or ounk or cons != len(blob) or int(tot[0]) != decoded or int(nunk[0]) or got != exp:
        raise SystemExit('PARITY FAILURE (decode vs the oracle restatement)')
    return {'GiBps': round(decoded / 2**30 / wall, 3), 'ms_per_step': round(wall * 1e3, 3),
            'encoded_bytes': len(blob),
            'reuse_stats': {'duplicates': stats[0], 'conflicted_hashes': stats[1], 'resolver_ran': stats[2]}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--chunks', type=int, default=4096)
    ap.add_argument('--share', type=float, default=0.05, help='share of ops that belong to a collision family')
    ap.add_argument('--families', type=int, default=64)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0x2E05E)
    args = ap.parse_args()
    import torch
    from oracle.lib import Oracle
    if not torch.cuda.is_available():
        raise SystemExit('no GPU')
    dev = torch.device('cuda', 0)
    oracle = Oracle()
    a, b, decoded, n_fam = build_streams(oracle, args.chunks, args.share, args.families, args.seed)
    reuse = measure(oracle, a, decoded, args.steps, args.warmup, dev)
    twin = measure(oracle, b, decoded, args.steps, args.warmup, dev)
    if not reuse['reuse_stats']['resolver_ran'] or twin['reuse_stats']['duplicates']:
        raise SystemExit('the streams did not take the paths they are built for')
    print(json.dumps({
        'metric': 'XCodec decode GiB/s of decoded bytes, whole batch on an empty decoder cache',
        'chunks': args.chunks, 'ops_per_chunk': OPS, 'decoded_bytes': decoded, 'family_share': args.share,
        'families': args.families, 'family_extracts': n_fam, 'steps': args.steps,
        'name_reuse': reuse, 'collision_free_twin': twin,
        'ratio': round(reuse['GiBps'] / twin['GiBps'], 4),
        'checked': 'both outputs equal the oracle restatement byte for byte'}))


if __name__ == '__main__':
    main()
