"""GPU: the grouped batch calls (xcg_encode_batch_grouped /
xcg_decode_batch_grouped) against the oracle -- per group one stream of
encode() calls on a fresh cache, one decoder per group (run on MI355X)."""
import numpy as np
import pytest

import collision_cases as cc
import group_cases as gc
from golden_cases import data as golden_data
from indep_decode_cases import seg_of
from test_gpu_decode_reuse import SEG
from test_gpu_mem import mem_live

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from wanproxy_amd.xcgpu import Context
    c = Context(0)
    yield c
    c.status()
    c.close()


@pytest.fixture(scope='module')
def mixed():
    return gc.mixed_batch()


@pytest.fixture(scope='module')
def mixed_expect(oracle, mixed):
    return gc.expect_groups(oracle, *mixed)


def check_encode(got, stats, exp):
    bad = [i for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, (bad[:10], [len(got[i]) for i in bad[:5]], [len(exp[i]) for i in bad[:5]])
    if stats is not None:
        want = np.array([gc.op_counts(e) for e in exp], np.uint32).reshape(len(exp), 2)
        assert np.array_equal(stats[:, :2], want)


def status_word(c, capfd):
    """The context's sticky status word: xcg_ctx_status folds every non-zero
    word into one error code, and prints the word itself under XCG_STATUS_DEBUG."""
    import os
    import re
    from wanproxy_amd.xcgpu import lib
    capfd.readouterr()
    old = os.environ.get('XCG_STATUS_DEBUG')
    os.environ['XCG_STATUS_DEBUG'] = '1'
    try:
        rc = int(lib().xcg_ctx_status(c.h))
    finally:
        if old is None:
            del os.environ['XCG_STATUS_DEBUG']
        else:
            os.environ['XCG_STATUS_DEBUG'] = old
    m = re.search(r'context status word (0x[0-9a-f]+)', capfd.readouterr().err)
    assert (rc != 0) == (m is not None)
    return int(m.group(1), 16) if m else 0


# ---------------------------------------------------------------- encode

def test_mixed_batch(ctx, oracle, mixed, mixed_expect):
    data, offs, lens, gf = mixed
    got, st = ctx.encode_groups(data, offs, lens, gf, with_stats=True)
    check_encode(got, st, mixed_expect)
    # the groups in reversed order: the outputs permute with the groups
    order = [np.arange(a, b) for a, b in zip(gf[:-1], gf[1:])][::-1]
    perm = np.concatenate(order)
    got_r = ctx.encode_groups(data, offs[perm], lens[perm], gc.group_first_of([len(o) for o in order]))
    assert got_r == [mixed_expect[i] for i in perm]
    # one group placed twice in a batch (around another): identical outputs
    g = next(k for k in range(len(gf) - 1) if gf[k + 1] - gf[k] >= 4)
    a, b = int(gf[g]), int(gf[g + 1])
    idx = np.concatenate([np.arange(a, b), np.arange(0, int(gf[1])), np.arange(a, b)])
    got_t = ctx.encode_groups(data, offs[idx], lens[idx], gc.group_first_of([b - a, int(gf[1]), b - a]))
    assert got_t[:b - a] == got_t[-(b - a):] == mixed_expect[a:b]
    assert got_t[b - a:-(b - a)] == mixed_expect[:int(gf[1])]


def test_every_group_one_chunk_is_independent(ctx, mixed):
    data, offs, lens, _ = mixed
    n = lens.size
    got, st = ctx.encode_groups(data, offs, lens, np.arange(n + 1), with_stats=True)
    ind, st_i = ctx.encode_chunks(data, offs, lens, with_stats=True)
    assert got == ind
    full = lens >= SEG                                   # (the independent call leaves short chunks' stats alone)
    assert np.array_equal(st[full], st_i[full]) and not st[~full].any()


def test_one_group_is_a_stream(oracle):
    from wanproxy_amd.synth import chunks_of
    from wanproxy_amd.xcgpu import XCG_SEM_STREAM, Context
    d = golden_data('c2_small')[:512 << 10]
    offs, lens = chunks_of(d, 65536)
    c = Context(0, cache_segments=1 << 12)
    got = c.encode_groups(d, offs, lens, [0, len(lens)])
    c.cache_clear()
    assert got == c.encode_chunks(d, offs, lens, semantics=XCG_SEM_STREAM)
    assert got == oracle.encode_batch(d, offs, lens, mode=1)
    c.status()
    c.close()


def test_degenerate_partitions(ctx, oracle, mixed, mixed_expect):
    import torch
    data, offs, lens, gf = mixed
    # empty groups at the start, in the middle and at the end
    gfe = np.concatenate([[0, 0], gf[:5], [gf[4], gf[4]], gf[5:], [gf[-1], gf[-1]]]).astype(np.uint32)
    got, st = ctx.encode_groups(data, offs, lens, gfe, with_stats=True)
    check_encode(got, st, mixed_expect)
    # n_groups == 0 and n == 0: XCG_OK, nothing launched
    dev = torch.device('cuda', 0)
    z8 = torch.zeros(64, dtype=torch.uint8, device=dev)
    z64 = torch.zeros(8, dtype=torch.int64, device=dev)
    z32 = torch.zeros(8, dtype=torch.int32, device=dev)
    assert ctx.encode_batch_grouped_device(z8, z64, z32, 1, z32, 0, 4096, z8, z64, z64) is None
    assert ctx.encode_batch_grouped_device(z8, z64, z32, 0, z32, 1, 4096, z8, z64, z64) is None
    assert ctx.decode_batch_grouped_device(z8, z64, z32, 1, z32, 0, 4096, z8, z64, z64, z64, z32, z64) is None
    assert ctx.encode_groups(b'abc', [0], [3], [0]) == [b'']
    # a zero-length chunk and chunks of 1, 2047 and 2048 bytes between declaring chunks
    rng = np.random.default_rng(77)
    P, Q = (rng.integers(0, 256, SEG, dtype=np.uint8).tobytes() for _ in range(2))
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()     # noqa: E731
    chunks = [P + rb(700) + Q, b'', rb(1), Q + rb(3000), rb(2047), P[:2047], P, rb(2048), rb(100) + P + Q + rb(50)]
    d, o, n = gc.lay_out(chunks, rng)
    exp = gc.expect_groups(oracle, d, o, n, [0, len(chunks)])
    assert sum(gc.op_counts(e)[1] for e in exp) >= 3
    got, st = ctx.encode_groups(d, o, n, [0, len(chunks)], with_stats=True)
    check_encode(got, st, exp)


@pytest.mark.parametrize('large', [False, True], ids=['small', 'large'])
def test_collisions_across_chunks(ctx, oracle, large):
    """Every stream case of collision_cases as one group: constructed full-hash
    and lo-only twins of a declaration of an earlier chunk (the lazy-hi record
    first matched from a later chunk among them), in both kernel classes."""
    for case in cc.stream_cases():
        name, data, offs, lens, _, kw = case
        exp, _, _ = cc.oracle_case(oracle, case)
        model = cc.model_case(case)
        assert [m[0] for m in model] == exp, name
        got, st = ctx.encode_groups(data, offs, lens, [0, len(lens)], with_stats=True,
                                    max_group_len=(1 << 19) if large else None)
        assert got == exp, name
        assert [tuple(int(v) for v in r[:3]) for r in st] == [m[1] for m in model], name


def test_class_edges(ctx, oracle, capfd):
    edges = gc.class_edge_groups()
    for name, chunks in edges.items():
        d, o, n = gc.lay_out(chunks, np.random.default_rng(5))
        exp = gc.expect_groups(oracle, d, o, n, [0, len(chunks)])
        got, st = ctx.encode_groups(d, o, n, [0, len(chunks)], with_stats=True)
        check_encode(got, st, exp)
    # 512 KiB + 2048: refused as a whole; its neighbours in the launch are encoded
    small = edges['128k_8x16k']
    over = edges['512k_8x64k'] + [small[0][:2048]]
    chunks = small + over + small
    d, o, n = gc.lay_out(chunks, np.random.default_rng(6))
    gf = [0, len(small), len(small) + len(over), len(chunks)]
    exp = gc.expect_groups(oracle, d, o, n, [0, len(small)])
    from wanproxy_amd.xcgpu import Context, XCGError
    c = Context(0, cache_segments=1 << 10)
    got = c.encode_groups(d, o, n, gf, max_group_len=1 << 19, check=False)
    assert got[:len(small)] == exp and got[-len(small):] == exp
    assert got[len(small):-len(small)] == [b''] * len(over)
    assert status_word(c, capfd) == 8        # bit 3 and nothing else
    c.close()
    with pytest.raises(XCGError, match=r'\(-22\)'):
        ctx.encode_groups(d, o, n, gf, max_group_len=(1 << 19) + 1)


def test_chunk_bases_every_residue(ctx, oracle):
    """The second and third chunk of a 3-chunk group at every base mod 16: the
    ring is primed again and the register path taken at each chunk's start."""
    rng = np.random.default_rng(99)
    blocks = [rng.integers(0, 256, SEG, dtype=np.uint8).tobytes() for _ in range(4)]
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()     # noqa: E731
    c0 = blocks[0] + rb(SEG) + blocks[1]
    chunks, sizes, gaps = [], [], []
    for r1 in range(16):
        r2 = (5 * r1 + 3) % 16
        c1 = rb(100 + r1) + blocks[1] + rb(SEG) + blocks[2]
        c2 = blocks[2] + rb(1900 + r1) + blocks[0] + blocks[3]
        pos = sum(len(c) for c in chunks) + sum(gaps)
        g0 = (-pos) % 16
        g1 = (r1 - (pos + g0 + len(c0))) % 16
        g2 = (r2 - (pos + g0 + len(c0) + g1 + len(c1))) % 16
        chunks += [c0, c1, c2]
        gaps += [g0, g1, g2]
        sizes.append(3)
    d, o, n = gc.lay_out(chunks, gaps=gaps)
    assert {int(x) % 16 for x in o[1::3]} == set(range(16)) == {int(x) % 16 for x in o[2::3]}
    gf = gc.group_first_of(sizes)
    exp = gc.expect_groups(oracle, d, o, n, gf)
    assert all(gc.op_counts(exp[3 * k + 1])[1] >= 1 and gc.op_counts(exp[3 * k + 2])[1] >= 2 for k in range(16))
    got, st = ctx.encode_groups(d, o, n, gf, with_stats=True)
    check_encode(got, st, exp)


def test_oob_and_null_cache(oracle, mixed):
    from wanproxy_amd.xcgpu import Context
    data, offs, lens, gf = mixed
    c = Context(0, out_of_band=True, cache_segments=1 << 10)
    assert c.encode_groups(data, offs, lens, gf) == gc.expect_groups(oracle, data, offs, lens, gf, oob=True)
    c.status()
    c.close()
    c = Context(0, out_of_band=True, null_cache=True)
    assert c.encode_groups(data, offs, lens, gf) == c.encode_chunks(data, offs, lens)
    c.status()
    c.close()


def test_context_untouched(oracle, mixed, mixed_expect):
    from wanproxy_amd.synth import chunks_of
    from wanproxy_amd.xcgpu import XCG_SEM_STREAM, Context
    data, offs, lens, gf = mixed
    d = golden_data('c2_small')[:256 << 10]
    so, sl = chunks_of(d, 65536)
    c = Context(0, cache_segments=1 << 12)
    first = c.encode_chunks(d, so[:2], sl[:2], semantics=XCG_SEM_STREAM)
    size0, live0 = c.cache_size(), mem_live()
    assert size0 > 0
    assert c.encode_groups(data, offs, lens, gf) == mixed_expect
    res = c.decode_groups([mixed_expect[a:b] for a, b in zip(gf[:-1], gf[1:])])
    assert all(r[0] == 0 for r in res)
    assert c.cache_size() == size0 and mem_live() == live0
    rest = c.encode_chunks(d, so[2:], sl[2:], semantics=XCG_SEM_STREAM)
    assert first + rest == oracle.encode_batch(d, so, sl, mode=1)
    c.status()
    c.close()
    # bounded contexts: the independent calls' rule
    from wanproxy_amd.xcgpu import XCGError
    tiny = Context(0, memory_cache_limit=2 * 2048)
    with pytest.raises(XCGError, match=r'\(-95\)'):
        tiny.encode_groups(data, offs, lens, gf)
    x = bytes(data[:3000])
    assert tiny.encode_groups(x, [0], [3000], [0, 1], max_group_len=4096) == oracle.encode_batch(x, [0], [3000], mode=1)
    tiny.close()


# ---------------------------------------------------------------- decode

def check_decode(got, exp, name=''):
    assert len(got) == len(exp)
    for k, (g, x) in enumerate(zip(got, exp)):
        assert (g[0], g[2], g[3]) == (x[0], x[2], x[3]), (name, k, g[0], g[2], x[0], x[2])
        assert g[1] == x[1], (name, k)


def test_round_trip(ctx, oracle, mixed, mixed_expect):
    data, offs, lens, gf = mixed
    got = ctx.encode_groups(data, offs, lens, gf)
    res = ctx.decode_groups([got[a:b] for a, b in zip(gf[:-1], gf[1:])])
    for i, (st, out, cons, unk) in enumerate(res):
        assert (st, cons, unk) == (0, len(got[i]), 0), i
        assert out == data[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes(), i
    for name, chunks in gc.class_edge_groups().items():
        d, o, n = gc.lay_out(chunks, np.random.default_rng(5))
        enc = ctx.encode_groups(d, o, n, [0, len(chunks)])
        res = ctx.decode_groups([enc], out_caps=[len(c) for c in chunks])
        assert [r[0] for r in res] == [0] * len(chunks), name
        assert [r[1] for r in res] == chunks and [r[2] for r in res] == [len(e) for e in enc], name


def test_cross_chunk_state(ctx, oracle):
    groups = gc.cross_chunk_groups(oracle)
    names = list(groups)
    exp = [gc.decode_expect(oracle, groups[k]) for k in names]
    assert [r[0] for r in exp[names.index('extract_then_ref')]] == [0, 0]
    assert exp[names.index('wrap_live')][-1][0] == 0 and exp[names.index('wrap_emptied')][-1][0] == -1
    got = ctx.decode_groups([groups[k] for k in names])
    check_decode(got, [x for e in exp for x in e])
    # the same groups in the large class
    got = ctx.decode_groups([groups[k] for k in names], max_group_len=gc.LARGE_DEC)
    check_decode(got, [x for e in exp for x in e])


def test_stop_rule(ctx, oracle):
    stops, neighbour = gc.stop_groups(oracle)
    nexp = gc.decode_expect(oracle, neighbour)
    assert [r[0] for r in nexp] == [0, 0]
    names = list(stops)
    groups, exp = [], []
    for k in names:
        groups += [stops[k], neighbour]
        exp += gc.decode_expect(oracle, stops[k]) + nexp
    got = ctx.decode_groups(groups)
    check_decode(got, exp)
    i = 0
    for k in names:
        st = [g[0] for g in got[i:i + len(stops[k])]]
        if k == 'ref_order_first':
            assert st == [1, 2, 2] and got[i][3] == oracle.hash(seg_of(7))
        else:
            assert st[0] == 0 and st[1] in (-1, 3) and st[2:] == [2, 2], (k, st)
        i += len(stops[k]) + len(neighbour)


def launch_guarded(ctx, groups, caps, max_group_len=None, guard=64, fill=0xA5):
    """One raw launch with `guard` bytes around every slot: per chunk (status,
    stored bytes, consumed, first_unknown, out_len), and whether every guard
    byte survived."""
    import torch
    dev = torch.device('cuda', ctx.device)
    encs = [e for g in groups for e in g]
    n = len(encs)
    lens = np.array([len(e) for e in encs], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]]).astype(np.uint64)
    gf = gc.group_first_of([len(g) for g in groups])
    caps = np.asarray(caps, np.uint64)
    oo = (np.concatenate([[0], np.cumsum(caps + np.uint64(guard))[:-1]]) + guard).astype(np.uint64)
    total = int(oo[-1] + caps[-1]) + guard
    cs = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    mgl = int((cs[gf[1:]] - cs[gf[:-1]]).max()) if max_group_len is None else max_group_len
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)     # noqa: E731
    d_in = torch.from_numpy(np.frombuffer(b''.join(encs) + b'\0', np.uint8).copy()).to(dev)
    d_out = torch.full((total,), fill, dtype=torch.uint8, device=dev)
    d_ol = torch.full((n,), -7, dtype=torch.int64, device=dev)
    d_st = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_cons = torch.full((n,), -7, dtype=torch.int64, device=dev)
    d_unk = torch.full((n,), -7, dtype=torch.int64, device=dev)
    ctx.decode_batch_grouped_device(d_in, t(offs, np.int64), t(lens, np.int32), n, t(gf, np.int32), len(groups), mgl,
                                    d_out, t(oo, np.int64), t(caps, np.int64), d_ol, d_st, d_cons, d_unk)
    torch.cuda.synchronize(dev)
    out = d_out.cpu().numpy()
    keep = np.ones(total, bool)
    res = []
    ol, st, cons, unk = (x.cpu().numpy() for x in (d_ol, d_st, d_cons, d_unk))
    for i in range(n):
        keep[int(oo[i]):int(oo[i] + caps[i])] = False
        stored = min(int(ol[i]), int(caps[i])) if st[i] != 4 else 0
        res.append((int(st[i]), out[int(oo[i]):int(oo[i]) + stored].tobytes(), int(cons[i]),
                    int(np.uint64(unk[i].view(np.uint64))), int(ol[i])))
    return res, bool((out[keep] == fill).all())


def test_room(ctx, oracle):
    grp, blocked = gc.room_groups(oracle)
    U = seg_of(62)
    exp = gc.decode_expect(oracle, grp)
    assert [x[0] for x in exp] == [0, 0, 0]
    need = [len(x[1]) for x in exp]
    bexp = gc.decode_expect(oracle, blocked)
    assert [x[0] for x in bexp] == [0, 1, 2]
    caps = [need[0], need[1] - 1, need[2], 2048, 1, 2048]
    got, guards_ok = launch_guarded(ctx, [grp, blocked], caps)
    assert guards_ok
    assert [g[0] for g in got] == [0, 4, 0, 0, 4, 2]
    assert got[1][4] == need[1] and got[1][2] == len(grp[1])        # the size needed; consumed as if decoded
    assert got[0][1] == exp[0][1] and got[2][1] == exp[2][1]        # later chunks of the group still decode
    assert (got[4][4], got[4][2], got[4][3]) == (2, 2, oracle.hash(U))
    assert (got[5][4], got[5][2], got[5][3]) == (0, 0, 0)
    ctx.status()
    res = ctx.decode_groups([grp, blocked], out_caps=caps)           # the retry yields the true statuses
    check_decode(res, exp + bexp)


def test_capacity(ctx, oracle, capfd):
    from wanproxy_amd.xcgpu import Context, XCGError
    grp, plain = gc.capacity_group(oracle)
    exp = gc.decode_expect(oracle, grp)
    small = gc.cross_chunk_groups(oracle)['name_reuse']
    sexp = gc.decode_expect(oracle, small)
    res = ctx.decode_groups([small, grp, small], out_caps=[len(x[1]) for x in sexp + exp + sexp])
    check_decode(res, sexp + exp + sexp)
    assert sum(len(r[1]) for r in res[3:-3]) == plain
    # 512 EXTRACTs, which is also 1,008 bytes past the largest max_group_len: refused as a whole by its length
    # (the one refusal such a group can meet, see over_capacity_group), its neighbours decoded
    over = gc.over_capacity_group()
    c = Context(0, cache_segments=1 << 10)
    res = c.decode_groups([small, over, small], out_caps=[4096 * 3] * 3 + [1] * 8 + [4096 * 3] * 3,
                          max_group_len=gc.LARGE_DEC, check=False)
    check_decode(res[:3] + res[-3:], sexp + sexp)
    assert [(r[0], r[1], r[2]) for r in res[3:-3]] == [(-1, b'', 0)] * 8
    assert status_word(c, capfd) == 8        # bit 3 and nothing else
    c.close()
    with pytest.raises(XCGError, match=r'\(-22\)'):
        ctx.decode_groups([small], max_group_len=gc.LARGE_DEC + 1)
    c = Context(0, cache_segments=1 << 10)
    got, guards_ok = launch_guarded(c, [small, small, small], [4096 * 3] * 9)
    check_decode([g[:4] for g in got], sexp * 3)
    import torch
    dev = torch.device('cuda', 0)
    encs = small * 3
    lens = np.array([len(e) for e in encs], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    d_in = torch.from_numpy(np.frombuffer(b''.join(encs), np.uint8).copy()).to(dev)
    d_out = torch.zeros(9 * 3 * 4096, dtype=torch.uint8, device=dev)
    d_oo = torch.arange(9, dtype=torch.int64, device=dev) * (3 * 4096)
    d_cap = torch.full((9,), 3 * 4096, dtype=torch.int64, device=dev)
    d_ol, d_cons = (torch.full((9,), -7, dtype=torch.int64, device=dev) for _ in range(2))
    d_st = torch.full((9,), -7, dtype=torch.int32, device=dev)
    d_gf = torch.tensor([0, 3, 12, 9], dtype=torch.int32, device=dev)     # group 1 passes n, group 2 descends
    c.decode_batch_grouped_device(d_in, torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev), 9, d_gf, 3,
                                  gc.SMALL_DEC, d_out, d_oo, d_cap, d_ol, d_st, d_cons)
    torch.cuda.synchronize(dev)
    assert status_word(c, capfd) == 8        # bit 3 and nothing else
    st, ol, out = d_st.cpu().numpy(), d_ol.cpu().numpy(), d_out.cpu().numpy()
    assert list(st[:3]) == [0, 0, 0] and list(ol[:3]) == [len(x[1]) for x in sexp]
    assert [out[k * 3 * 4096:k * 3 * 4096 + int(ol[k])].tobytes() for k in range(3)] == [x[1] for x in sexp]
    assert (st[3:] == -7).all() and (ol[3:] == -7).all() and not out[3 * 3 * 4096:].any()   # nothing written for them
    c.close()


def test_length_sums_do_not_wrap(oracle, capfd):
    """A group's lengths are summed by 64 lanes in 32 bits: a group whose true
    total is 2^32 or a little more (64 chunks of 64 MiB; 2^21 chunks of 2049
    bytes) is refused like any other oversized group, its neighbours untouched.
    Nothing of a refused group is read, so its chunks need no bytes behind them."""
    import torch
    from wanproxy_amd.xcgpu import Context
    dev = torch.device('cuda', 0)
    t = lambda a, dt: torch.from_numpy(np.array(a).view(dt)).to(dev)     # noqa: E731
    # encode: [good group of 3] [64 x 2^26] [the good group again]
    good = gc.pool_chunks(7, [6144, 4096, 6144], npool=3)
    d, o, n = gc.lay_out(good, np.random.default_rng(8))
    exp = gc.expect_groups(oracle, d, o, n, [0, 3])
    assert sum(gc.op_counts(e)[1] for e in exp[1:]) >= 1
    offs = np.concatenate([o, np.zeros(64, np.uint64), o])
    lens = np.concatenate([n, np.full(64, 1 << 26, np.uint32), n])
    assert int(lens[3:67].astype(np.uint64).sum()) == 1 << 32
    m = lens.size
    oo = np.concatenate([np.arange(3) * 16384, np.zeros(64), 49152 + np.arange(3) * 16384]).astype(np.uint64)
    d_out = torch.zeros(6 * 16384, dtype=torch.uint8, device=dev)
    d_ol = torch.full((m,), -7, dtype=torch.int64, device=dev)
    c = Context(0, cache_segments=1 << 10)
    c.encode_batch_grouped_device(t(d, np.uint8), t(offs, np.int64), t(lens, np.int32), m,
                                  t(np.array([0, 3, 67, 70], np.uint32), np.int32), 3, 1 << 17, d_out, t(oo, np.int64),
                                  d_ol)
    torch.cuda.synchronize(dev)
    assert status_word(c, capfd) == 8
    ol, out = d_ol.cpu().numpy(), d_out.cpu().numpy()
    assert not ol[3:67].any()
    for k, i in enumerate([0, 1, 2, 67, 68, 69]):
        assert out[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes() == exp[k % 3], i
    c.close()
    # decode: [good] [64 x 2^26] [2^21 x 2049, no chunk that could hold an EXTRACT] [good]
    small = gc.cross_chunk_groups(oracle)['name_reuse']
    sexp = gc.decode_expect(oracle, small)
    nb = 1 << 21
    slen = np.array([len(e) for e in small], np.uint32)
    soff = np.concatenate([[0], np.cumsum(slen)[:-1]]).astype(np.uint64)
    lens = np.concatenate([slen, np.full(64, 1 << 26, np.uint32), np.full(nb, 2049, np.uint32), slen])
    offs = np.concatenate([soff, np.zeros(64 + nb, np.uint64), soff])
    assert int(lens[67:67 + nb].astype(np.uint64).sum()) == (1 << 32) + nb
    m = lens.size
    oo = np.zeros(m, np.uint64)
    oo[:3] = np.arange(3) * 8192
    oo[-3:] = 24576 + np.arange(3) * 8192
    caps = np.zeros(m, np.uint64)
    caps[:3] = caps[-3:] = 8192
    d_out = torch.zeros(6 * 8192, dtype=torch.uint8, device=dev)
    d_ol, d_cons = (torch.full((m,), -7, dtype=torch.int64, device=dev) for _ in range(2))
    d_st = torch.full((m,), -7, dtype=torch.int32, device=dev)
    c = Context(0, cache_segments=1 << 10)
    c.decode_batch_grouped_device(t(np.frombuffer(b''.join(small), np.uint8), np.uint8), t(offs, np.int64),
                                  t(lens, np.int32), m, t(np.array([0, 3, 67, 67 + nb, m], np.uint32), np.int32), 4,
                                  gc.LARGE_DEC, d_out, t(oo, np.int64), t(caps, np.int64), d_ol, d_st, d_cons)
    torch.cuda.synchronize(dev)
    assert status_word(c, capfd) == 8
    st, ol, cons, out = (x.cpu().numpy() for x in (d_st, d_ol, d_cons, d_out))
    assert (st[3:-3] == -1).all() and not ol[3:-3].any() and not cons[3:-3].any()
    for k, i in enumerate([0, 1, 2, m - 3, m - 2, m - 1]):
        x = sexp[k % 3]
        assert (st[i], cons[i]) == (x[0], x[2]) and out[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes() == x[1], i
    c.close()
