"""Time of the independent batch decode (xcg_decode_batch_independent) on the C2
workload as bench.py builds it: 4096 x 64 KiB chunks, seed 0xC2, encoded
independently on the device; every decoded chunk is checked against its input
before anything is timed.

    indep_decode_time.py [--out FILE] [--rounds N]

Timed with HIP events in blocks of 20 launches after 3 warm-ups, five blocks of
each alternating (the median block is reported, with the blocks' range):
  (e) the independent encode of the same chunks (the launch the decode inverts)
  (a) xcg_decode_batch_independent, the 20 launches back to back
  (b) the stream decoder on the same bytes: xcg_decode_batch on a cleared
      unbounded context, each launch bracketed by its own event pair with the
      cache clear outside it (that call synchronises its stream itself)
Printed (and written to FILE): us per launch and GiB/s of decoded bytes for
each, and (a)'s algorithmic bytes (encoded in + decoded out) per second."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from wanproxy_amd import synth  # noqa: E402
from wanproxy_amd.xcgpu import Context, _check, _stream_ptr, lib  # noqa: E402

CH, N, LAUNCHES, WARM, ROUNDS = 65536, 4096, 20, 3, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=ROUNDS, help='blocks of each (1: a short run for a counter pass)')
    args = ap.parse_args()
    rounds = max(1, args.rounds)
    dev = torch.device('cuda', 0)
    s = torch.cuda.current_stream(dev)
    data = np.frombuffer(synth.stream(0xC2, N * CH, 50, 0), dtype=np.uint8)
    d_plain = torch.from_numpy(data.copy()).to(dev)
    d_len = torch.full((N,), CH, dtype=torch.int32, device=dev)
    d_off = torch.arange(N, dtype=torch.int64, device=dev) * CH
    bound = 2 * CH + 16
    d_eoff = torch.arange(N, dtype=torch.int64, device=dev) * bound
    d_enc = torch.empty(N * bound, dtype=torch.uint8, device=dev)
    d_elen64 = torch.zeros(N, dtype=torch.int64, device=dev)
    ctx = Context(0)

    def encode():
        ctx.encode_batch_device(d_plain, d_off, d_len, N, CH, d_enc, d_eoff, d_elen64, stream=s)

    encode()
    torch.cuda.synchronize()
    ctx.status()
    d_elen = d_elen64.to(torch.int32)
    enc_bytes, max_len = int(d_elen64.sum()), int(d_elen64.max())

    d_out = torch.zeros(N * CH, dtype=torch.uint8, device=dev)
    d_cap = torch.full((N,), CH, dtype=torch.int64, device=dev)
    d_ol = torch.zeros(N, dtype=torch.int64, device=dev)
    d_st = torch.zeros(N, dtype=torch.int32, device=dev)
    d_cons = torch.zeros(N, dtype=torch.int64, device=dev)

    def decode_a():
        ctx.decode_batch_independent_device(d_enc, d_eoff, d_elen, N, max_len, d_out, d_off, d_cap, d_ol, d_st, d_cons,
                                            stream=s)

    decode_a()
    torch.cuda.synchronize()
    ctx.status()
    assert not bool(d_st.any()) and torch.equal(d_ol, d_cap) and torch.equal(d_cons, d_elen64)
    assert torch.equal(d_out, d_plain), 'independent decode does not give the input back'

    sctx = Context(0)
    d_soff = torch.zeros(N, dtype=torch.int64, device=dev)
    unk, nunk, total = np.zeros(16, np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.uint64)

    def decode_b():
        _check(lib().xcg_decode_batch(
            sctx.h, C.c_void_p(d_enc.data_ptr()), C.c_void_p(d_eoff.data_ptr()), C.c_void_p(d_elen.data_ptr()), N,
            max_len, C.c_void_p(d_out.data_ptr()), N * CH, C.c_void_p(d_soff.data_ptr()), C.c_void_p(d_ol.data_ptr()),
            C.c_void_p(d_st.data_ptr()), C.c_void_p(d_cons.data_ptr()), unk.ctypes.data, unk.size, nunk.ctypes.data,
            total.ctypes.data, _stream_ptr(s)))

    d_out.zero_()
    decode_b()
    torch.cuda.synchronize()
    assert not bool(d_st.any()) and int(total[0]) == N * CH and torch.equal(d_out, d_plain)

    def timed(fn, before=None):
        """us per launch: back to back between two events, or (with `before`
        run untimed ahead of every launch) the sum of per-launch event pairs."""
        for _ in range(WARM):
            if before:
                before()
            fn()
        torch.cuda.synchronize()
        if before is None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(LAUNCHES):
                fn()
            e1.record(s)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / LAUNCHES * 1e3
        tot = 0.0
        for _ in range(LAUNCHES):
            before()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            torch.cuda.synchronize()
            tot += e0.elapsed_time(e1)
        return tot / LAUNCHES * 1e3

    # `rounds` blocks of each, alternating, so that the three share the device's minutes
    blocks = {'e': [], 'a': [], 'b': []}
    for _ in range(rounds):
        blocks['e'].append(timed(encode))
        blocks['a'].append(timed(decode_a))
        blocks['b'].append(timed(decode_b, before=sctx.cache_clear))
    ctx.status()
    t_e, t_a, t_b = (sorted(blocks[k])[rounds // 2] for k in 'eab')
    dec_bytes = N * CH
    gib = lambda us: dec_bytes / (us * 1e-6) / 2 ** 30   # noqa: E731
    row = lambda k, name, t, what: ('(%s) %-37s %8.1f us/launch (blocks %.1f .. %.1f)  %7.1f GiB/s %s' %   # noqa: E731
                                    (k, name, t, min(blocks[k]), max(blocks[k]), gib(t), what))
    lines = [
        'C2: %d x %d KiB chunks, seed 0xC2; %d encoded bytes -> %d decoded bytes' % (N, CH >> 10, enc_bytes, dec_bytes),
        'median of %d alternating blocks, each %d launches after %d warm-ups' % (rounds, LAUNCHES, WARM),
        row('e', 'xcg_encode_batch independent', t_e, 'of input'),
        row('a', 'xcg_decode_batch_independent', t_a, 'decoded'),
        row('b', 'xcg_decode_batch, cleared context', t_b, 'decoded'),
        '(a) algorithmic bytes (encoded in + decoded out) %d = %.2f TB/s; (a)/(b) time %.3f; (a)/(e) time %.3f'
        % (enc_bytes + dec_bytes, (enc_bytes + dec_bytes) / (t_a * 1e-6) / 1e12, t_a / t_b, t_a / t_e),
    ]
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    ctx.close()
    sctx.close()


if __name__ == '__main__':
    main()
