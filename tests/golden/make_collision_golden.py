#!/usr/bin/env python3
"""Regenerate tests/golden/collisions.json from the REAL reference encoder
(oracle/_ref/libxcref.so, compiled from the reference sources by
oracle/Makefile) over the constructed-collision cases of
tests/collision_cases.py.

Run in the build container only.  The cases are regenerated deterministically
by collision_cases.all_cases(); per case the JSON holds the per-encode()
lengths and SHA-256 prefixes of the reference's output, and for the pair case
its disk counters.  The reference runs every mode but out-of-band declarations
on a real cache (its out-of-band mode is the null cache), so those cases have
no entry.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import collision_cases as cc  # noqa: E402


def sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def runs_on_reference(case) -> bool:
    return not case[5].get('oob', False)


def generate(ref) -> dict:
    out = {'generator': 'tests/golden/make_collision_golden.py', 'cases': {}}
    for case in cc.all_cases():
        if not runs_on_reference(case):
            continue
        encs, _, st = cc.oracle_case(ref, case)
        e = {'lens': [len(x) for x in encs], 'chunk_sha256': [sha(x)[:32] for x in encs]}
        if st is not None:
            e['disk_entries'], e['disk_written'] = st
        out['cases'][case[0]] = e
    return out


def main():
    from oracle.lib import Oracle
    out = generate(Oracle(ref=True))
    with open(os.path.join(HERE, 'collisions.json'), 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(len(out['cases']), 'cases')


if __name__ == '__main__':
    main()
