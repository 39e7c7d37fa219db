"""Time of warming and reading back a memory cache: xcg_cache_learn_batch and
xcg_cache_export against a device-to-device copy of the same bytes, and the
per-segment path (xcg_cache_enter_host) they replace.

    cache_load_time.py [--out FILE] [--reps N] [--parent-lib LIBXCGPU_OF_THE_PARENT_COMMIT]

Timed with HIP events around each call, the median of --reps (>= 20) after 3
warm-ups, the cache cleared before each learn outside the timed region:
  (l) xcg_cache_learn_batch of 2^18 distinct device-resident segments (512 MiB)
      into an empty default context (2^19 segments)
  (b) the same into a bounded context of 2^16 segments (three quarters of the
      batch is evicted by the rest: only the last 2^16 are written)
  (e) xcg_cache_export of each into a device buffer
  (c) a device-to-device copy of the 512 MiB in the same process: the yardstick
Reported: milliseconds, segments per second, GiB/s of segment bytes (learned or
exported) and the ratio to the copy's time for the same bytes.

The per-segment baseline is xcg_cache_enter_host over 4096 segments, host
clock around the loop, in a child process on --parent-lib: a build of the
commit before the batched calls (the calls themselves are unchanged since, so
without --parent-lib the current library is timed and the line says so)."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from wanproxy_amd.xcgpu import SEG, Context, _check, lib  # noqa: E402

N_LEARN, N_BOUNDED, N_ENTER, WARM = 1 << 18, 1 << 16, 4096, 3


def timed(fn, reps, before=None):
    ms = []
    for k in range(WARM + reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= WARM:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def enter_host_only():
    """Child process: seconds per xcg_cache_enter_host call over N_ENTER segments."""
    rng = np.random.default_rng(0xCAC4E)
    segs = rng.integers(0, 256, N_ENTER * SEG, dtype=np.uint8)
    from oracle.lib import Oracle
    o = Oracle()
    hs = [o.hash(segs[k * SEG:(k + 1) * SEG].tobytes()) for k in range(N_ENTER)]
    bufs = [(C.c_uint8 * SEG).from_buffer_copy(segs[k * SEG:(k + 1) * SEG].tobytes()) for k in range(N_ENTER)]
    # (the library by its path and plain ctypes: the parent's build has no batched calls to bind)
    L = C.CDLL(os.environ.get('XCGPU_LIB') or os.path.join(ROOT, 'wanproxy_amd', 'libxcgpu.so'))
    L.xcg_ctx_create.argtypes = [C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
    L.xcg_cache_enter_host.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    L.xcg_cache_clear.argtypes = [C.c_void_p]
    L.xcg_cache_size.argtypes = [C.c_void_p]
    L.xcg_cache_size.restype = C.c_uint64
    L.xcg_ctx_destroy.argtypes = [C.c_void_p]
    L.xcg_ctx_destroy.restype = None
    h = C.c_void_p()
    assert L.xcg_ctx_create(0, 0, C.byref(h)) == 0
    for k in range(64):                                  # warm-up (and the cache's allocation)
        assert L.xcg_cache_enter_host(h, hs[k], bufs[k]) == 0
    assert L.xcg_cache_clear(h) == 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(N_ENTER):
        rc = L.xcg_cache_enter_host(h, hs[k], bufs[k])
        if rc != 0:
            raise RuntimeError('xcg_cache_enter_host: %d' % rc)
    dt = time.perf_counter() - t0
    assert L.xcg_cache_size(h) == len(set(hs))
    L.xcg_ctx_destroy(h)
    print('ENTER_HOST_SECONDS_PER_SEGMENT %.9f' % (dt / N_ENTER))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cache_load.txt'))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--enter-host-only', action='store_true')
    a = ap.parse_args()
    if a.enter_host_only:
        return enter_host_only()
    reps = max(20, a.reps)
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0xCAC4E)
    d_segs = torch.randint(0, 256, (N_LEARN * SEG,), dtype=torch.uint8, device=dev, generator=gen)
    d_hash = torch.zeros(N_LEARN, dtype=torch.int64, device=dev)
    d_out = torch.empty(N_LEARN * SEG, dtype=torch.uint8, device=dev)
    d_ohash = torch.zeros(N_LEARN, dtype=torch.int64, device=dev)
    nbytes = N_LEARN * SEG
    lines = ['cache_load_time.py: %s, %d reps after %d warm-ups, HIP events, median (min .. max)'
             % (torch.cuda.get_device_name(0), reps, WARM)]

    def row(tag, t, segs, copy_ms):
        med, lo, hi = t
        gib = segs * SEG / 2.0 ** 30
        lines.append('%-46s %8.3f ms (%.3f .. %.3f)  %7.1f Mseg/s  %7.1f GiB/s  %5.2f x copy'
                     % (tag, med, lo, hi, segs / med / 1e3, gib / (med / 1e3), med / copy_ms))
        print(lines[-1], flush=True)

    copy = timed(lambda: d_out.copy_(d_segs), reps)
    copy_ms = copy[0]
    row('(c) device-to-device copy, 2^18 segments', copy, N_LEARN, copy_ms)
    copy_b = timed(lambda: d_out[:N_BOUNDED * SEG].copy_(d_segs[:N_BOUNDED * SEG]), reps)
    row('(c) device-to-device copy, 2^16 segments', copy_b, N_BOUNDED, copy_b[0])

    cnt = C.c_uint64()
    for tag, ctx, held in (('default context (2^19)', Context(0), N_LEARN),
                           ('bounded context (2^16)', Context(0, memory_cache_limit=N_BOUNDED * SEG), N_BOUNDED)):
        learn = timed(lambda: ctx.cache_learn_device(d_segs, N_LEARN, d_hash), reps, before=ctx.cache_clear)
        size = ctx.cache_size()
        row('(l) learn 2^18 segments, %s' % tag, learn, N_LEARN, copy_ms)
        lines.append('    cache holds %d segments afterwards (%d expected at most)' % (size, held))

        def export():
            _check(lib().xcg_cache_export(ctx.h, C.c_void_p(d_out.data_ptr()), C.c_void_p(d_ohash.data_ptr()),
                                          N_LEARN, C.byref(cnt), None))
        exp = timed(export, reps)
        row('(e) export %d segments, %s' % (size, tag), exp, size, copy_ms * size / N_LEARN)
        ctx.close()

    # the per-segment path, in a process of its own on the parent commit's build
    env = dict(os.environ)
    which = 'this build (no --parent-lib given)'
    if a.parent_lib:
        env['XCGPU_LIB'] = os.path.abspath(a.parent_lib)
        which = "the parent commit's build"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--enter-host-only'], env=env, capture_output=True,
                       text=True, timeout=300)
    per = [ln for ln in r.stdout.splitlines() if ln.startswith('ENTER_HOST_SECONDS_PER_SEGMENT')]
    if r.returncode != 0 or not per:
        lines.append('(p) xcg_cache_enter_host baseline failed: %s' % r.stderr[-300:])
    else:
        s = float(per[0].split()[1])
        lines.append('(p) xcg_cache_enter_host x %d on %s: %.1f us per segment (host clock), %.4f Mseg/s;'
                     % (N_ENTER, which, s * 1e6, 1e-6 / s))
        lines.append('    extrapolated to 2^18 segments: %.1f s' % (s * N_LEARN))
    print('\n'.join(lines[-2:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
