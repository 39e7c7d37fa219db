"""Time of the grouped batch calls (xcg_encode_batch_grouped /
xcg_decode_batch_grouped) on synth.stream(0xC2, ...) bytes, 256 MiB per shape:
  (A) 4096 groups x 8 x  8 KiB   small class, one resident wave per group
  (B)  512 groups x 8 x 64 KiB   large class, 512 waves: a latency-bound launch

    group_time.py [--out FILE] [--rounds N] [--shapes AB]

Before anything is timed, a 64-group prefix of each shape is checked against
the oracle (one stream per group on a fresh cache) and every group by GPU round
trip.  Timed with HIP events in blocks of 20 launches after 3 warm-ups, five
blocks of each alternating (the median block, with the blocks' range):
  (g) xcg_encode_batch_grouped
  (d) xcg_decode_batch_grouped of (g)'s output
  (i) xcg_encode_batch XCG_SEM_INDEPENDENT on the same chunks: another output,
      the floor the carried cache is measured against
  (s) what a caller does without the grouped call: per group, clear an
      unbounded context and run one XCG_SEM_STREAM batch (the call synchronises
      itself); clear + batch timed per group over a 32-group sample, scaled to
      the shape's group count."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from wanproxy_amd import synth  # noqa: E402
from wanproxy_amd.xcgpu import XCG_SEM_STREAM, Context  # noqa: E402

LAUNCHES, WARM, ROUNDS, PER_GROUP, CHECK_GROUPS, SAMPLE = 20, 3, 5, 8, 64, 32
SHAPES = {'A': (4096, 8 << 10), 'B': (512, 64 << 10)}


def run_shape(name, rounds, oracle):
    ng, ch = SHAPES[name]
    n, glen = ng * PER_GROUP, PER_GROUP * ch
    dev = torch.device('cuda', 0)
    s = torch.cuda.current_stream(dev)
    data = np.frombuffer(synth.stream(0xC2, n * ch, 50, 0), dtype=np.uint8)
    d_plain = torch.from_numpy(data.copy()).to(dev)
    d_len = torch.full((n,), ch, dtype=torch.int32, device=dev)
    d_off = torch.arange(n, dtype=torch.int64, device=dev) * ch
    d_gf = (torch.arange(ng + 1, dtype=torch.int32, device=dev) * PER_GROUP).contiguous()
    bound = 2 * ch + 16
    d_eoff = torch.arange(n, dtype=torch.int64, device=dev) * bound
    d_enc = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    d_elen64 = torch.zeros(n, dtype=torch.int64, device=dev)
    d_ienc = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    d_ilen64 = torch.zeros(n, dtype=torch.int64, device=dev)
    ctx = Context(0)

    def enc_g():
        ctx.encode_batch_grouped_device(d_plain, d_off, d_len, n, d_gf, ng, glen, d_enc, d_eoff, d_elen64, stream=s)

    def enc_i():
        ctx.encode_batch_device(d_plain, d_off, d_len, n, ch, d_ienc, d_eoff, d_ilen64, stream=s)

    enc_g()
    enc_i()
    torch.cuda.synchronize()
    ctx.status()
    enc_bytes, ind_bytes = int(d_elen64.sum()), int(d_ilen64.sum())
    # a prefix against the oracle: one stream per group on a fresh cache
    m = CHECK_GROUPS * PER_GROUP
    offs = np.arange(m, dtype=np.uint64) * ch
    lens = np.full(m, ch, np.uint32)
    el = d_elen64[:m].cpu().numpy()
    enc_host = d_enc[:m * bound].cpu().numpy()
    for g in range(CHECK_GROUPS):
        a = g * PER_GROUP
        exp = oracle.encode_batch(data, offs[a:a + PER_GROUP], lens[a:a + PER_GROUP], mode=1)
        for k, e in enumerate(exp):
            got = enc_host[(a + k) * bound:(a + k) * bound + int(el[a + k])].tobytes()
            assert got == e, 'shape %s: group %d chunk %d differs from the oracle' % (name, g, k)

    d_elen = d_elen64.to(torch.int32)
    glen_enc = int(d_elen64.view(ng, PER_GROUP).sum(1).max())
    d_out = torch.zeros(n * ch, dtype=torch.uint8, device=dev)
    d_cap = torch.full((n,), ch, dtype=torch.int64, device=dev)
    d_ol = torch.zeros(n, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    d_cons = torch.zeros(n, dtype=torch.int64, device=dev)

    def dec_g():
        ctx.decode_batch_grouped_device(d_enc, d_eoff, d_elen, n, d_gf, ng, glen_enc, d_out, d_off, d_cap, d_ol, d_st,
                                        d_cons, stream=s)

    dec_g()
    torch.cuda.synchronize()
    ctx.status()
    assert not bool(d_st.any()) and torch.equal(d_ol, d_cap) and torch.equal(d_cons, d_elen64)
    assert torch.equal(d_out, d_plain), 'shape %s: the grouped decode does not give the input back' % name

    sctx = Context(0)
    d_senc = torch.empty(PER_GROUP * bound, dtype=torch.uint8, device=dev)
    d_slen = torch.zeros(PER_GROUP, dtype=torch.int64, device=dev)

    def stream_group(g):
        a = g * PER_GROUP
        sctx.cache_clear()
        sctx.encode_batch_device(d_plain, d_off[a:a + PER_GROUP], d_len[a:a + PER_GROUP], PER_GROUP, ch, d_senc,
                                 d_eoff[:PER_GROUP], d_slen, stream=s, semantics=XCG_SEM_STREAM)

    stream_group(0)
    torch.cuda.synchronize()
    assert torch.equal(d_slen, d_elen64[:PER_GROUP]), 'the per-group stream batch gives other lengths'

    def timed(fn):
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(LAUNCHES):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / LAUNCHES * 1e3

    def timed_sample():
        """us for all the shape's groups done one by one, from a SAMPLE-group sample."""
        stream_group(0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for g in range(SAMPLE):
            stream_group(g)
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 * ng / SAMPLE

    blocks = {'g': [], 'd': [], 'i': [], 's': []}
    for _ in range(rounds):
        blocks['g'].append(timed(enc_g))
        blocks['d'].append(timed(dec_g))
        blocks['i'].append(timed(enc_i))
        blocks['s'].append(timed_sample())
    ctx.status()
    t = {k: sorted(v)[rounds // 2] for k, v in blocks.items()}
    plain = n * ch
    gib = lambda us: plain / (us * 1e-6) / 2 ** 30   # noqa: E731
    row = lambda k, what: ('  (%s) %-46s %10.1f us (blocks %.1f .. %.1f)  %7.1f GiB/s' %   # noqa: E731
                           (k, what, t[k], min(blocks[k]), max(blocks[k]), gib(t[k])))
    lines = [
        '(%s) %d groups x %d x %d KiB, seed 0xC2, %d plain bytes; grouped out/in %.3f, independent out/in %.3f'
        % (name, ng, PER_GROUP, ch >> 10, plain, enc_bytes / plain, ind_bytes / plain),
        row('g', 'xcg_encode_batch_grouped'),
        row('d', 'xcg_decode_batch_grouped'),
        row('i', 'xcg_encode_batch independent, same chunks'),
        row('s', 'clear + XCG_SEM_STREAM batch per group (scaled)'),
        '  time ratios: (g)/(i) %.3f  (d)/(g) %.3f  (s)/(g) %.1f' % (t['g'] / t['i'], t['d'] / t['g'], t['s'] / t['g']),
    ]
    ctx.close()
    sctx.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=ROUNDS)
    ap.add_argument('--shapes', default='AB')
    args = ap.parse_args()
    from oracle.lib import Oracle
    oracle = Oracle()
    lines = ['median of %d alternating blocks, each %d launches after %d warm-ups; GiB/s of plain bytes; a %d-group '
             'prefix checked against the oracle, every group by round trip'
             % (max(1, args.rounds), LAUNCHES, WARM, CHECK_GROUPS)]
    for name in args.shapes:
        lines += run_shape(name, max(1, args.rounds), oracle)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
