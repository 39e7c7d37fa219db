"""Kernel time of the C2 independent (headline) encode, no parity check
(diagnostics: timing-experiment builds whose output is wrong).

    indep_time.py                 the library XCGPU_LIB names (or the in-tree one)
    indep_time.py A.so B.so [N]   both libraries in this one process, alternating
                                  A B A B ... for N rounds (default 5): parent and
                                  change timed on the same device minutes apart

Every block is 20 back-to-back launches between two events; a line gives the
block's time per launch and the spread of the single launches in it.  The
device's clock settles only after ~60 launches (the first blocks of either
build run 5-10 % slower), so WARM untimed launches per library come first."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', '..'))
import numpy as np
import torch

from wanproxy_amd import synth
from wanproxy_amd import xcgpu

CH, N, LAUNCHES, WARM = 65536, 4096, 20, 100
args = sys.argv[1:]
rounds = int(args.pop()) if args and args[-1].isdigit() else (5 if len(args) > 1 else 3)
paths = [os.path.abspath(a) for a in args] or [xcgpu.LIB_PATH]

dev = torch.device('cuda', 0)
data = np.frombuffer(synth.stream(0xC2, N * CH, 50, 0), dtype=np.uint8)
d_in = torch.from_numpy(data.copy()).to(dev)
d_len = torch.full((N,), CH, dtype=torch.int32, device=dev)
d_off = torch.arange(N, dtype=torch.int64, device=dev) * CH
bound = 2 * CH + 16
d_oo = torch.arange(N, dtype=torch.int64, device=dev) * bound
d_out = torch.empty(N * bound, dtype=torch.uint8, device=dev)
d_ol = torch.zeros(N, dtype=torch.int64, device=dev)
d_st = torch.zeros(4 * N, dtype=torch.int32, device=dev)
s = torch.cuda.current_stream(dev)


def launch(ctx):
    ctx.encode_batch_device(d_in, d_off, d_len, N, CH, d_out, d_oo, d_ol, d_st, stream=s)


# one loaded library + context per path; xcgpu calls go through its module-level handle
loaded = []
for p in paths:
    xcgpu.LIB_PATH, xcgpu._lib = p, None
    handle = xcgpu.lib()
    ctx = xcgpu.Context(0)
    for _ in range(3):
        launch(ctx)
    torch.cuda.synchronize()
    loaded.append((p, handle, ctx))

for i in range(WARM * len(loaded)):
    p, handle, ctx = loaded[(i // LAUNCHES) % len(loaded)]
    xcgpu._lib = handle
    launch(ctx)
torch.cuda.synchronize()
blocks = {p: [] for p in paths}
for rep in range(rounds):
    for p, handle, ctx in loaded:
        xcgpu._lib = handle
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(LAUNCHES + 1)]
        ev[0].record(s)
        for i in range(LAUNCHES):
            launch(ctx)
            ev[i + 1].record(s)
        torch.cuda.synchronize()
        per = ev[0].elapsed_time(ev[LAUNCHES]) / LAUNCHES * 1e3
        one = [ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(LAUNCHES)]
        blocks[p].append(per)
        print('round %d %-36s per launch %6.1f us (single launches %.1f .. %.1f)'
              % (rep, os.path.basename(p), per, min(one), max(one)), flush=True)
for p in paths:
    b = blocks[p]
    print('%-36s per launch %6.1f us (blocks %s)' % (os.path.basename(p), min(b), ' '.join('%.1f' % v for v in b)))
if len(paths) == 2:
    a, b = (sorted(blocks[p]) for p in paths)
    print('median ratio %s / %s = %.4f; ranges %s' % (os.path.basename(paths[1]), os.path.basename(paths[0]),
                                                     b[len(b) // 2] / a[len(a) // 2],
                                                     'disjoint' if max(b) < min(a) or max(a) < min(b) else 'overlap'))
