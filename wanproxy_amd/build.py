"""Build libxcgpu.so in-tree for gfx950 (hipcc; no JIT cache, so the .so
travels with the repository snapshot to the GPU box).

Each source compiles to its own object in parallel (objects are reused while
they are newer than the source and every header), then one link."""
from __future__ import annotations

import glob
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
# (the encoder's units first: the two stream units are the longest compiles)
SRCS = ['csrc/xcg_encode_stream.hip', 'csrc/xcg_encode_stream_lru.hip', 'csrc/xcg_encode_indep.hip',
        'csrc/xcg_encode_group.hip', 'csrc/xcg_encode_screen.hip', 'csrc/xcg_ctx.hip', 'csrc/xcg_api_cache.hip',
        'csrc/xcg_encode_refmap.hip', 'csrc/xcg_api_encode.hip', 'csrc/xcg_api_decode.hip', 'csrc/xcg_decode.hip',
        'csrc/xcg_decode_bounded.hip', 'csrc/xcg_decode_small.hip', 'csrc/xcg_decode_windows.hip',
        'csrc/xcg_decode_indep.hip', 'csrc/xcg_decode_group.hip', 'csrc/xcg_hash.hip', 'csrc/xcg_lru.hip',
        'csrc/xcg_pair.hip', 'csrc/xcg_cache_bulk.hip', 'csrc/xcg_cache_point.hip', 'csrc/xcg_pipe.cpp',
        'csrc/xcg_codec.cpp', 'csrc/xcg_wire.hip',
        'csrc/xcg_zdeflate.hip', 'csrc/xcg_zdeflate_match.hip', 'csrc/xcg_zdeflate_parse.hip',
        'csrc/xcg_zdeflate_huff.hip', 'csrc/xcg_inflate.hip',
        'csrc/xcg_pair_state.hip', 'csrc/xcg_volume.cpp']
HDRS = sorted(glob.glob(os.path.join(HERE, 'csrc', '*.h'))) + ['../include/xcgpu.h']   # every object depends on all
OUT = os.path.join(HERE, 'libxcgpu.so')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
# Units whose kernels keep their whole parse state in registers: a compiler that spills it
# to scratch still builds a correct library, several times slower, and no test would notice -- so the build reads
# these units' resource-usage remarks and refuses a kernel with scratch.
NO_SCRATCH = ('csrc/xcg_encode_indep.hip', 'csrc/xcg_encode_group.hip', 'csrc/xcg_wire.hip')
REMARKS = '-Rpass-analysis=kernel-resource-usage'
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wall'] + os.environ.get('XCG_EXTRA_FLAGS', '').split()


def _newer(out: str, deps) -> bool:
    return os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)


def scratch_of(remarks: str) -> dict:
    """kernel name -> scratch bytes per lane, from hipcc's kernel-resource-usage remarks."""
    out, name = {}, None
    for line in remarks.splitlines():
        m = re.search(r'remark: +Function Name: (\S+)', line)
        if m:
            name = m.group(1)
        m = re.search(r'remark: +ScratchSize \[bytes/lane\]: (\d+)', line)
        if m and name is not None:
            out[name] = int(m.group(1))
    return out


def build_lib(force: bool = False, verbose: bool = False, out: str = OUT, defines=()) -> str:
    """Build the library (or, for diagnostics, a variant at `out` with extra
    -D `defines`, e.g. XCG_TIMING: per-wave timestamps in the stats words)."""
    out = os.path.abspath(out)
    srcs = [os.path.join(HERE, s) for s in SRCS]
    hdrs = [os.path.join(HERE, h) for h in HDRS]
    if not force and _newer(out, srcs + hdrs):
        return out
    tag = '' if not defines else '.' + '_'.join(defines)
    objdir = os.path.join(HERE, 'build')
    os.makedirs(objdir, exist_ok=True)
    dflags = ['-D' + d for d in defines]

    def compile_one(src):
        obj = os.path.join(objdir, os.path.basename(src) + tag + '.o')
        if not force and _newer(obj, [src] + hdrs):
            return obj
        checked = os.path.relpath(src, HERE) in NO_SCRATCH
        cmd = [HIPCC] + FLAGS + ([REMARKS] if checked else []) + dflags + ['-c', '-o', obj + '.tmp', src]
        if verbose:
            print(' '.join(cmd))
        if checked:
            r = subprocess.run(cmd, check=True, cwd=HERE, stderr=subprocess.PIPE, text=True)
            sys.stderr.write(''.join(ln + '\n' for ln in r.stderr.splitlines() if 'remark:' not in ln))
            usage = scratch_of(r.stderr)
            spilled = {k: v for k, v in usage.items() if v}
            if not usage or spilled:
                raise RuntimeError('%s: kernels with scratch (or no remarks at all): %s' % (src, spilled))
        else:
            subprocess.run(cmd, check=True, cwd=HERE)
        os.replace(obj + '.tmp', obj)
        return obj

    with ThreadPoolExecutor(min(len(srcs), os.cpu_count() or 1, 16)) as ex:
        objs = list(ex.map(compile_one, srcs))
    # -z defs: a function one unit declares and none defines fails here, not at its first call
    cmd = [HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-Wl,-z,defs', '-o', out + '.tmp'] + objs
    if verbose:
        print(' '.join(cmd))
    subprocess.run(cmd, check=True, cwd=HERE)
    os.replace(out + '.tmp', out)
    return out


SYNTH_SRC = os.path.join(HERE, 'csrc/xcg_synth.c')
SYNTH_OUT = os.path.join(HERE, 'libxcsynth.so')


def build_synth(force: bool = False) -> str:
    """The workload generator (csrc/xcg_synth.c: bench / test inputs, no GPU)."""
    if force or not _newer(SYNTH_OUT, [SYNTH_SRC]):
        subprocess.run(['gcc', '-O2', '-shared', '-fPIC', '-o', SYNTH_OUT + '.tmp', SYNTH_SRC], check=True)
        os.replace(SYNTH_OUT + '.tmp', SYNTH_OUT)
    return SYNTH_OUT


NATIVE_SRC = os.path.join(HERE, '..', 'tests', 'native', 'disk_tier_driver.c')
NATIVE_OUT = os.path.join(HERE, '..', 'tests', 'native', 'disk_tier_driver')


def build_native_tests(force: bool = False) -> str:
    """C drivers of the ABI that GPU tests run in processes without PyTorch
    (tests/native: test infrastructure, linked against the in-tree library)."""
    if force or not _newer(NATIVE_OUT, [NATIVE_SRC, OUT]):
        subprocess.run(['gcc', '-O2', '-Wall', '-o', NATIVE_OUT + '.tmp', NATIVE_SRC, '-L' + HERE, '-l:libxcgpu.so',
                        '-Wl,-rpath,$ORIGIN/../../wanproxy_amd'], check=True)
        os.replace(NATIVE_OUT + '.tmp', NATIVE_OUT)
    return NATIVE_OUT


if __name__ == '__main__':
    print(build_lib(force=True, verbose=True))
    print(build_synth(force=True))
