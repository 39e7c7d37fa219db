"""The independent encoder's input ring (xcg_encode_wave.h, encode_chunk DM):
the entering bytes of a chunk's contiguous pieces are staged global -> LDS two
pieces ahead, in two 2 KiB buffers per wave, and taken out behind a counted
wait.  What can go wrong is a piece reading a buffer that holds another
piece's bytes (a transition between the register path and the ring, a jump
after a REF, the guarded tail), or before its load has landed -- both change
the output bytes, so every case here compares the device encoder's output
bytes, out_len and stats words with the CPU oracle (mode 0), and decodes the
result back to the input.

The oracle gives no stats words: n_extract and n_ref (words 0, 1) are counted
from the oracle's own output ops; n_collision (word 2) is 0 here, since random
bytes hold no two different segments with one 64-bit hash (constructed
collisions and their non-zero counts: tests/test_gpu_collisions.py); n_pieces
(word 3) is the kernel's own piece count, bounded below by the windows it has
to cover in pieces of 2048 positions (a REF skips 2048 of them)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEG = 2048
# around every transition of the ring: first piece (register path), the first
# ring piece, the refill stopping two pieces before the end, the guarded tail
LENGTHS = [2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145, 8191, 8192, 8193, 10240 + 1, 3 * 2048 + 17, 65536,
           131072]


@pytest.fixture(scope='module')
def ctx():
    from wanproxy_amd.xcgpu import Context
    c = Context(0)
    yield c
    c.close()


def _count_ops(enc: bytes):
    """(n_extract, n_ref) of one in-band encoded chunk: ops are 0xF1 + code
    (0 an escaped 0xF1, 1 EXTRACT + 2048 bytes, 2 REF + 8 bytes)."""
    n_ext = n_ref = 0
    i = enc.find(b'\xf1')
    while i >= 0:
        op = enc[i + 1]
        assert op in (0, 1, 2), op
        n_ext += op == 1
        n_ref += op == 2
        i = enc.find(b'\xf1', i + (2, 2 + SEG, 10)[op])
    return n_ext, n_ref


def _check(ctx, oracle, data, offs, lens, mis=0):
    """Encode chunks data[offs[i]:offs[i]+lens[i]] from a device tensor that
    starts `mis` bytes into its allocation and ends with data's last byte;
    compare with the oracle; return (encoded chunks, stats[n, 4])."""
    import torch
    dev = torch.device('cuda', 0)
    offs = np.ascontiguousarray(offs, np.uint64)
    lens = np.ascontiguousarray(lens, np.uint32)
    n = offs.size
    big = torch.zeros(mis + data.size, dtype=torch.uint8, device=dev)
    big[mis:] = torch.from_numpy(data).to(dev)
    d_in = big[mis:]
    assert d_in.data_ptr() % 16 == mis
    bounds = 2 * lens.astype(np.uint64) + 16
    oo = np.zeros(n, np.uint64)
    oo[1:] = np.cumsum(bounds)[:-1]
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_oo = torch.from_numpy(oo.view(np.int64)).to(dev)
    d_out = torch.zeros(int(bounds.sum()), dtype=torch.uint8, device=dev)
    d_ol = torch.zeros(n, dtype=torch.int64, device=dev)
    d_st = torch.zeros(4 * n, dtype=torch.int32, device=dev)
    ctx.encode_batch_device(d_in, d_off, d_len, n, int(lens.max()), d_out, d_oo, d_ol, d_st)
    torch.cuda.synchronize(dev)
    ctx.status()
    out = d_out.cpu().numpy()
    ol = d_ol.cpu().numpy()
    st = d_st.cpu().numpy().view(np.uint32).reshape(n, 4)
    exp = oracle.encode_batch(data, offs, lens, mode=0)
    assert [int(v) for v in ol] == [len(e) for e in exp]
    got = [out[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes() for i in range(n)]
    bad = [i for i in range(n) if got[i] != exp[i]]
    assert not bad, (mis, bad[:8])
    for i in range(n):
        ne, nr = _count_ops(exp[i])
        windows = max(int(lens[i]) - SEG + 1, 0)
        assert (int(st[i, 0]), int(st[i, 1]), int(st[i, 2])) == (ne, nr, 0), (i, st[i], ne, nr)
        # (a REF skips 2048 windows; a chunk's last window may ride along with the piece before it)
        assert int(st[i, 3]) >= max((windows - nr * SEG + SEG - 1) // SEG - 1, min(windows, 1)), (i, st[i], windows)
        c = oracle.cache_new()
        ok, back, cons, unk = oracle.decode(got[i], c)
        oracle.cache_free(c)
        assert ok and not unk and back == data[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes(), i
    return got, st


def _pack(rng, lens, residue):
    """Random chunks of the given lengths, each at an offset = residue mod 16
    (so never a multiple of 16); the last one ends the array."""
    offs, pos = [], 0
    for k in lens:
        pos += (residue - pos) % 16
        offs.append(pos)
        pos += k
    return rng.integers(0, 256, pos, dtype=np.uint8), np.array(offs, np.uint64), np.array(lens, np.uint32)


@pytest.mark.parametrize('mis', [0, 1, 7, 15])
def test_lengths_around_ring_transitions(ctx, oracle, mis):
    """Every length at which the piece sequence changes, in a tensor `mis`
    bytes off 16-byte alignment with chunk offsets = 9 mod 16 (absolute
    misalignments 9, 10, 0 and 8); the last chunk ends at the tensor's last
    byte."""
    data, offs, lens = _pack(np.random.default_rng(0x51 + mis), LENGTHS, 9)
    assert int(offs[-1]) + int(lens[-1]) == data.size and all(int(o) % 16 for o in offs)
    _check(ctx, oracle, data, offs, lens, mis)


def _jump_chunks(rng):
    """16 KiB chunks with an earlier 2 KiB block planted again, so that a REF
    makes the parse jump and the next piece starts off the ring's sequence."""
    L = 16384
    out = []
    for d in (8192, 8193, 8192 + 31, 8192 + 32, 8192 + 2047, 10000):
        c = rng.integers(0, 256, L, dtype=np.uint8)
        c[d:d + SEG] = c[2048:4096]
        out.append(c)
    c = rng.integers(0, 256, L, dtype=np.uint8)       # two copies back to back
    c[8192:8192 + SEG] = c[2048:4096]
    c[10240:10240 + SEG] = c[4096:6144]
    out.append(c)
    c = rng.integers(0, 256, L, dtype=np.uint8)       # the re-primed ring meets the guarded tail at once
    c[L - 4096:L - 2048] = c[0:2048]
    out.append(c)
    return out


@pytest.mark.parametrize('mis', [0, 7])
def test_ring_reprime_after_jump(ctx, oracle, mis):
    chunks = _jump_chunks(np.random.default_rng(0x4A))
    lens = np.array([c.size for c in chunks], np.uint32)
    offs, parts, pos = [], [], 0
    for c in chunks:
        pad = (9 - pos) % 16
        parts.append(np.zeros(pad, np.uint8))
        offs.append(pos + pad)
        parts.append(c)
        pos += pad + c.size
    got, st = _check(ctx, oracle, np.concatenate(parts), np.array(offs, np.uint64), lens, mis)
    assert (st[:, 1] >= 1).all(), st[:, 1]            # every chunk took the REF path
    assert all(len(g) < 16384 + 16 for g in got)      # (16400 bytes without the duplicate)


def test_mixed_lengths_in_one_launch(ctx, oracle):
    """64 chunks cycling through the lengths: the four waves of a workgroup run
    different piece counts on neighbouring ring buffers."""
    rng = np.random.default_rng(0x3C)
    lens = [LENGTHS[(5 * i + i // 16) % len(LENGTHS)] for i in range(64)]
    data, offs, lens = _pack(rng, lens, 3)
    _check(ctx, oracle, data, offs, lens, 0)


def test_mixed_lengths_128k_with_duplicates(ctx, oracle):
    """64 chunks of about 128 KiB (8 MiB in all), each with one of its own
    2 KiB blocks planted again further on: long ring runs, a jump, a re-prime."""
    rng = np.random.default_rng(0x3D)
    cut = [0, 1, 17, 2047, 2048, 2049, 4095, 6143]
    lens = np.array([131072 - cut[i % 8] for i in range(64)], np.uint32)
    offs = np.arange(64, dtype=np.uint64) * 131072
    data = rng.integers(0, 256, 64 * 131072, dtype=np.uint8)
    for i in range(64):
        o = int(offs[i])
        src = 2048 * int(rng.integers(1, 20))        # (a declared segment: random data declares every 2 KiB)
        dst = 65536 + int(rng.integers(0, 30000))
        data[o + dst:o + dst + SEG] = data[o + src:o + src + SEG]
    data = data[:int(offs[-1]) + int(lens[-1])]
    got, st = _check(ctx, oracle, data, offs, lens, 0)
    assert (st[:, 1] >= 1).all(), st[:, 1]


def _dm_key(block):
    """The direct-mapped probe key of a 2048-byte window: -(X2 + CLO) mod 2^32,
    X2 = sum (2048 - k) x_k (roll_probe_dm, xcg_encode_wave.h)."""
    w = np.arange(2048, 0, -1, dtype=np.uint64)
    x2 = int((w * block.astype(np.uint64)).sum()) & 0xFFFFFFFF
    return (-(x2 + 0x80200400)) & 0xFFFFFFFF


DM_SLOTS = 1024        # the 64 KiB / 128 KiB instance's table: bits 2..11 of the key


def _block_in_slot(rng, slot):
    """A random 2 KiB block whose key lands in direct-mapped slot `slot`: bytes
    2016 and 2047 (weights 32 and 1) absorb the difference."""
    b = rng.integers(0, 256, 2048, dtype=np.uint8)
    b[2016] = 0
    b[2047] = 0
    r = (_dm_key(b) - 4 * slot) % (4 * DM_SLOTS)      # raising X2 by r lowers the key by r
    b[2016] = r >> 5
    b[2047] = r & 31
    assert (_dm_key(b) >> 2) & (DM_SLOTS - 1) == slot
    return b


@pytest.mark.parametrize('ncoll', [2, 9, 30])
def test_slot_collisions_in_the_smaller_table(ctx, oracle, ncoll):
    """The ring's LDS comes out of the key table (1024 slots per wave): chunks
    whose declarations share one slot (1 slot + up to 32 overflow keys: the
    N1 / N8 / N32 compare variants), then repeat those blocks -- aligned,
    shifted and cut -- so the REFs must be found through the overflow keys."""
    rng = np.random.default_rng(0xE1 + ncoll)
    chunks_, lens = [], []
    for c in range(6):
        slot = int(rng.integers(0, DM_SLOTS))
        coll = [_block_in_slot(rng, slot) for _ in range(ncoll)]
        fresh = [rng.integers(0, 256, 2048, dtype=np.uint8) for _ in range(max(0, 36 - ncoll))]
        blocks = coll + fresh
        parts = list(blocks)
        for k in range(22):
            src = blocks[int(rng.integers(0, len(blocks)))] if k % 2 else coll[int(rng.integers(0, ncoll))]
            if k % 3 == 2:
                parts.append(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8))
            parts.append(src)
        b = np.concatenate(parts)[:131072 - int(rng.integers(0, 3000)) * (c % 2)]
        chunks_.append(b)
        lens.append(b.size)
    offs = np.zeros(len(lens), np.uint64)
    offs[1:] = np.cumsum(np.array(lens, np.uint64))[:-1]
    got, st = _check(ctx, oracle, np.concatenate(chunks_), offs, np.array(lens, np.uint32), 0)
    assert int(st[:, 1].sum()) >= 6 * 10              # the repeats really were found
