"""The closed form of a bulk learn (cache_bulk_cases.model_learn) against the
sequential definition: the C restatement's decode of `F1 01 <segment>` ops is
exactly <LEARN>'s lookup / replace / enter per segment
(xcodec/xcodec_pipe_pair.cc:311-327, xcodec/xcodec_decoder.cc:106-136), and
where the reference is built, its own classes.  No GPU."""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import pytest

import cache_bulk_cases as cb
from collision_cases import LRU_LIMIT, family, twins
from oracle.lib import MODE_STREAM

SEG = 2048
CASES = cb.cases()
IDS = [c[0] for c in CASES]


def oracle_export(o, c):
    n = int(o.lib.xco_cache_size(c))
    keys = np.zeros(max(n, 1), np.uint64)
    segs = np.zeros(max(n, 1) * SEG, np.uint8)
    got = int(o.lib.xco_cache_export(c, keys.ctypes.data_as(C.POINTER(C.c_uint64)),
                                     segs.ctypes.data_as(C.POINTER(C.c_uint8)), n))
    assert got == n
    return [int(k) for k in keys[:n]], [segs[k * SEG:(k + 1) * SEG].tobytes() for k in range(n)]


def oracle_learn(o, c, segs):
    """The learn sequence on the restatement's cache `c`."""
    if not segs:
        return
    enc = b''.join(b'\xf1\x01' + s for s in segs)
    ok, out, cons, unk = o.decode(enc, c, out_cap=len(enc))
    assert ok and cons == len(enc) and not unk and out == b''.join(segs)


def model_of(o, limit, earlier, batch):
    m = OrderedDict()
    for part in (earlier, batch):
        cb.model_learn(m, limit, [o.hash(s) for s in part], part)
    return m


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_model_is_the_sequential_result(oracle, case):
    _, limit, earlier, batch = case
    for cut in cb.splits(len(batch)) if limit == LRU_LIMIT and len(batch) == 100 else [None, len(batch) // 2]:
        c = oracle.cache_new(limit * SEG)
        m = OrderedDict()
        for part in [earlier] + ([batch] if cut is None else [batch[:cut], batch[cut:]]):
            oracle_learn(oracle, c, part)
            cb.model_learn(m, limit, [oracle.hash(s) for s in part], part)
        keys, segs = oracle_export(oracle, c)
        oracle.cache_free(c)
        if limit:                                       # exactly: hashes, bytes and order
            assert keys == list(m.keys()), cut
            assert segs == list(m.values()), cut
        else:
            assert sorted(zip(keys, segs)) == sorted(m.items()), cut


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_model_is_the_python_sequence(oracle, case):
    _, limit, earlier, batch = case
    a, b = OrderedDict(), OrderedDict()
    for part in (earlier, batch):
        hs = [oracle.hash(s) for s in part]
        cb.model_learn(a, limit, hs, part)
        cb.sequential_learn(b, limit, hs, part)
    assert list(a.items()) == list(b.items()) if limit else dict(a) == dict(b)


def test_segment_sets_hold_what_they_promise(oracle):
    for n in cb.SIZES[1:]:
        s = cb.segment_set(n, n)
        assert len(s) == n
        h = [oracle.hash(x) for x in s]
        fam = family(0xB01C + n)
        lo = twins(0xB01C + n, 'lo')
        where = [s.index(f) for f in fam]
        assert where == sorted(where) and len({h[i] for i in where}) == 1 and len(set(fam)) == 3
        ha, hb = oracle.hash(lo[0]), oracle.hash(lo[1])
        assert ha != hb and ha & 0xFFFFFFFF == hb & 0xFFFFFFFF and lo[0] in s and lo[1] in s
        assert s[-1] == s[0] and all(x in s for x in (bytes(SEG), b'\xff' * SEG, b'\xf1' * SEG))
        assert len(set(h)) == n - 3                     # the duplicate and the family's two other variants


def test_lru_batch_holds_what_it_promises(oracle):
    batch = cb.lru_batch()
    hs = [oracle.hash(s) for s in batch]
    assert len(batch) == 100 and len(set(hs)) == 40
    for earlier in ([], cb.lru_earlier()):
        c, trace = OrderedDict(), []
        cb.sequential_learn(c, LRU_LIMIT, [oracle.hash(s) for s in earlier], earlier)
        assert len(c) == len(earlier)
        cb.sequential_learn(c, LRU_LIMIT, hs, batch, trace)
        kinds = [k for k, _ in trace]
        assert 'hit' in kinds and 'replace' in kinds and 'evict' in kinds
        # an eviction followed by the re-entry of that hash with other bytes
        first = {}
        for i, h in enumerate(hs):
            first.setdefault(h, i)
        gone = {}
        reentered = False
        for k, h in trace:
            if k == 'evict':
                gone[h] = True
            elif k == 'enter' and gone.pop(h, False):
                reentered = reentered or h == hs[0]
        assert reentered and batch[30] != batch[0] and hs[30] == hs[0]
        # name reuse between two live occurrences: a replace
        assert ('replace', hs[34]) in trace and batch[34] != batch[20] and hs[34] == hs[20]


def test_model_against_the_reference(oracle, ref_oracle):
    """The reference's own <LEARN> on its own cache, then the same later stream
    encoded on it and on a restatement cache filled from the model.  Every case
    runs with its name reuse taken out (cache_bulk_cases.without_reuse: the
    reference's replace leaves a freed pointer); hits, evictions and re-entries
    stay, and the reuse itself is pinned by the restatement above."""
    for name, limit, earlier, batch in CASES:
        earlier, batch = cb.without_reuse(oracle.hash, earlier, batch)
        rc = ref_oracle.cache_new(limit * SEG)
        for s in earlier + batch:
            ref_oracle.cache_learn(rc, s)
        m = model_of(oracle, limit, earlier, batch)
        oc = oracle.cache_new(limit * SEG)
        for h, s in m.items():                          # least recently used first
            a = np.frombuffer(s, np.uint8)
            assert oracle.lib.xco_cache_enter(oc, h, a.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
        d = cb.later_stream(batch)
        offs = np.arange(0, d.size, 8192, dtype=np.uint64)
        lens = np.minimum(8192, d.size - offs).astype(np.uint32)
        exp = ref_oracle.encode_batch(d, offs, lens, mode=MODE_STREAM, cache=rc)
        got = oracle.encode_batch(d, offs, lens, mode=MODE_STREAM, cache=oc)
        ref_oracle.cache_free(rc)
        oracle.cache_free(oc)
        assert got == exp, name


def test_cache_load_refuses_a_cut_file(tmp_path):
    """A file that is not whole segments is tack -p's 'Corrupt persistent
    cache' (programs/tack/tack.cc:119-120), raised before any GPU call: the
    context here has no engine behind it at all."""
    from wanproxy_amd.xcgpu import Context
    p = os.path.join(tmp_path, 'cut.cache')
    with open(p, 'wb') as f:
        f.write(bytes(3 * SEG + 5))
    ctx = object.__new__(Context)
    with pytest.raises(ValueError, match='Corrupt persistent cache'):
        ctx.cache_load(p)
