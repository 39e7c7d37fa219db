#!/usr/bin/env python3
"""Regenerate tests/golden/pipe.json from the REAL reference XCodecPipePair
(oracle/_ref/libppref.so: xcodec/xcodec_pipe_pair.cc over the reference's own
encoder, decoder and cache, through oracle/pipe_driver.cc).

Run in the build container only (needs `make -C oracle` with the reference
tree).  The conversations are tests/pipe_cases.py's, regenerated on any machine
(seeded); the JSON holds, per conversation and step, the lengths and SHA-256 of
what the call produced for the peer and for the local side, the flags it
raised, the acting pipe's pending frame count and its connected decoder
cache's size -- or null for a step that was skipped because nothing was there
to deliver.  Data only.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import pipe_cases as pc  # noqa: E402


def main():
    R = pc.RefImpl('ref')
    out = {'generator': 'tests/golden/make_pipe_golden.py', 'conversations': {}}
    for name in pc.NAMES:
        T = pc.run(pc.conversation(name), R)
        out['conversations'][name] = pc.record(T)
        print(name, len(T), 'steps,', sum(len(o.to_peer) for o in T if o), 'wire bytes,',
              sum(len(o.to_local) for o in T if o), 'delivered', 'ERROR' if any(o and o.error for o in T) else '')
    with open(os.path.join(HERE, 'pipe.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
