#!/usr/bin/env python3
"""Regenerate tests/golden/pipe_peers.json from the REAL reference
XCodecPipePair (oracle/_ref/libppref.so, through oracle/pipe_driver.cc): the
conversations of tests/pipe_peers_cases.py -- a hub that receives from many
peers -- whose `dmany` turns the reference runs as the serial loop of
decoder_consume calls.

Run in the build container only (needs `make -C oracle` with the reference
tree).  The JSON holds what tests/golden/pipe.json holds per step (see
make_pipe_golden.py): lengths and hashes.  Data only.
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
import pipe_peers_cases as pp  # noqa: E402


def main():
    R = pc.RefImpl('ref')
    out = {'generator': 'tests/golden/make_pipe_peers_golden.py', 'conversations': {}}
    for name in pp.NAMES:
        T = pp.run(pp.conversation(name), R)
        out['conversations'][name] = pp.record(T)
        print(name, len(T), 'steps,', sum(len(o.to_peer) for o in T if o), 'wire bytes,',
              sum(len(o.to_local) for o in T if o), 'delivered,', sum(1 for o in T if o and o.error), 'errors')
    with open(os.path.join(HERE, 'pipe_peers.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
