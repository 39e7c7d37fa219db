#!/usr/bin/env python3
"""Regenerate tests/golden/codec_pipe.json from the reference's own classes:
XCodecPipePair (oracle/_ref/libppref.so) chained with DeflatePipe and
InflatePipe (oracle/_ref/libzpref.so) by the rules of
tests/codec_pipe_cases.py.

Run in the build container only (needs `make -C oracle` with the reference
tree).  The conversations are regenerated on any machine (seeded); the JSON
holds, per conversation and step, what pipe_cases.record() keeps: lengths and
SHA-256 of the bytes for the peer and for the local side, the flags, the acting
pipe's pending frame count and its connected decoder cache's size -- or null
for a pipe that had nothing delivered in its turn.  Data only.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import codec_pipe_cases as cc  # noqa: E402


def main():
    R = cc.RefChain()
    out = {'generator': 'tests/golden/make_codec_pipe_golden.py', 'conversations': {}}
    for name in cc.NAMES:
        T = cc.run(cc.conversation(name), R)
        out['conversations'][name] = cc.record(T)
        print(name, len(T), 'steps,', sum(len(o.to_peer) for o in T if o), 'bytes to the peer,',
              sum(len(o.to_local) for o in T if o), 'delivered', 'FAILED' if any(o and o.error for o in T) else '')
    with open(os.path.join(HERE, 'codec_pipe.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
