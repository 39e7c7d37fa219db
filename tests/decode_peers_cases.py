"""Cases for xcg_decode_call_many (test infrastructure, no GPU in here): one
decode() call per peer cache, many peers in one function call.

A case is {'name', 'kinds', 'steps'}: kinds[p] is peer p's cache ('plain',
'bounded', 'pair' or 'null'); a step is
    ('calls', [(peer, stream, outside)])   one function call; `outside`: the
                                           launch does not serve this call (the
                                           kernel declines it or never takes it)
    ('learn', peer, [segments])            a <LEARN> on that peer's cache
run_model() runs a case on the yardstick: every peer has one cache_new() cache
and one decoder_new decoder, and the calls are served one by one.  A call's
expected result is (rc, status, out, consumed, unknown, extract hashes): the
EXTRACT hashes before the stop in op order for a call the launch serves, None
for one it does not.  At the end every peer's 256 window slots
(decode_windows_cases.probe_window) and its cache.
"""
import numpy as np

import decode_windows_cases as W
from collision_cases import family
from decode_windows_cases import LIT, B, R, X, rnd_segs

SEG = 2048
MODE_STREAM = 1
LIMIT = 64 * SEG                         # the bounded and pair peers' memory limit
DISK = (18 + 205) * SEG                  # the pair peer's disk
MIB = 1 << 20


def rnd_bytes(seed, n):
    return np.random.default_rng([0x9EE5, int(seed)]).integers(0, 256, n, dtype=np.uint8).tobytes()


def extracts_before(enc, stop):
    """The segments of the whole EXTRACT ops in enc[:stop], up to an opcode nobody knows."""
    segs = []
    try:
        for kind, a, b in W.walk(enc[:stop]):
            if kind == 'x':
                segs.append(enc[a + 2:b])
    except KeyError:
        pass
    return segs


class ModelPeer:
    """One peer on the yardstick: a cache and a decoder of its own."""

    def __init__(self, oracle, kind):
        self.o, self.kind = oracle, kind
        if kind == 'bounded':
            self.cache = oracle.cache_new(LIMIT)
        elif kind == 'pair':
            self.cache = oracle.cache_new_pair(LIMIT, DISK)
        else:                            # (a null cache's calls here hold no REF: any cache decodes them alike)
            self.cache = oracle.cache_new()
        self.dec = oracle.decoder_new(self.cache)

    def call(self, enc, outside):
        if not enc:
            return (0, 0, b'', 0, [], None)
        cap = len(enc) + SEG * (enc.count(b'\xf1') + 1)
        ok, out, cons, unk = self.o.decode(enc, self.cache, out_cap=cap, decoder=self.dec)
        st = W.status_of(ok, cons, unk, len(enc))
        ext = None if outside else [self.o.hash(seg) for seg in extracts_before(enc, cons if st != -1 else len(enc))]
        return (0, st, out, cons, sorted(unk), ext)

    def learn(self, segs):
        for seg in segs:                 # (through a decoder of its own: the peer's window does not move)
            assert self.o.decode(X(seg), self.cache)[0]

    def probe(self):
        def decode1(chunk):
            ok, out, c, unk = self.o.decode(chunk, self.cache, decoder=self.dec)
            return W.status_of(ok, c, unk, len(chunk)), out, c
        return W.probe_window(decode1)

    def export(self):
        """{hash: bytes} of a memory cache (None: a pair's or a null cache's is not compared)."""
        if self.kind in ('pair', 'null'):
            return None
        L = self.o.lib
        n = int(L.xco_cache_size(self.cache))
        keys, segs = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1) * SEG, np.uint8)
        import ctypes as C
        m = int(L.xco_cache_export(self.cache, keys.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   segs.ctypes.data_as(C.POINTER(C.c_uint8)), n))
        assert m == n
        return {int(keys[k]): segs[k * SEG:(k + 1) * SEG].tobytes() for k in range(n)}

    def free(self):
        self.o.decoder_free(self.dec)
        self.o.cache_free(self.cache)


def run_model(oracle, case):
    """(results, final): one entry per step -- the calls' expected results, None
    for a learn -- and per peer (256 window slots, cache)."""
    peers = [ModelPeer(oracle, k) for k in case['kinds']]
    results = []
    try:
        for step in case['steps']:
            if step[0] == 'calls':
                results.append([peers[p].call(enc, outside) for p, enc, outside in step[1]])
            else:
                peers[step[1]].learn(step[2])
                results.append(None)
        final = [(pe.probe(), pe.export()) for pe in peers]
    finally:
        for pe in peers:
            pe.free()
    return results, final


# ---- case 1: lengths

LENGTHS = [[75999, 76000, 76001, 300000, 17, 16],
           [300000, 75999, 76000, 76001, 15, 1],
           [76001, 300000, 0, 16, 75999, 76000]]
SHORT = b'a short run of literal bytes'


def case_lengths(oracle):
    """6 peers, 3 rounds of encoder-made streams cut to the call lengths that
    matter: 0, 1 (a lone F1), 15 / 16 / 17 (the byte tail of the staging loop),
    SD_LDS_IN - 1 / SD_LDS_IN / SD_LDS_IN + 1 and 300 KB (staged in LDS or
    not).  A stream holds literals, escaped F1, EXTRACTs and REFs that resolve
    in the call, in the cache (the round before) and -- peer 1, round 1 -- in
    neither: its last REF names a segment only the encoder has seen."""
    enc_caches = [oracle.cache_new() for _ in range(6)]
    missing = rnd_segs(77, 1)[0]
    oracle.encode_batch(missing, [0], [SEG], mode=MODE_STREAM, cache=enc_caches[1])   # (never sent)
    prev = [b''] * 6
    steps = []
    for r in range(3):
        calls = []
        for p in range(6):
            L = LENGTHS[r][p]
            if L < 100:
                enc = b'\xf1' if L == 1 else SHORT[:L]
            else:
                fresh = rnd_bytes(100 * r + p, L - 9000)
                data = fresh[:30000] + b'lit\xf1\xf1erals' + fresh[4096:4096 + 3 * SEG] + prev[p][:4 * SEG] + fresh[30000:]
                if (r, p) == (1, 1):
                    data += missing
                enc = oracle.encode_batch(data, [0], [len(data)], mode=MODE_STREAM, cache=enc_caches[p])[0]
                assert len(enc) <= L, (r, p, len(enc))
                enc += b'p' * (L - len(enc))
                prev[p] = fresh
            assert len(enc) == L
            calls.append((p, enc, False))
        steps.append(('calls', calls))
    for c in enc_caches:
        oracle.cache_free(c)
    return {'name': 'lengths', 'kinds': ['plain'] * 6, 'steps': steps, 'missing': oracle.hash(missing)}


# ---- case 2: a blocked peer

def case_blocked(oracle):
    """Peer 2 of 5 blocks on an unknown REF in the middle of its call; behind
    the stop: an EXTRACT, a REF to it, and REFs to two unknown hashes.  Then
    the <LEARN> and the rest of that call beside new calls of the others."""
    s = rnd_segs(21, 12)
    m1, m2 = s[10], s[11]
    head = LIT + X(s[0]) + R(oracle.hash(s[0])) + b'mid'
    rest = R(oracle.hash(m1)) + X(s[1]) + R(oracle.hash(s[1])) + R(oracle.hash(m2)) + R(oracle.hash(m1)) + LIT
    first = [(p, LIT + X(s[2 + p]) + R(oracle.hash(s[2 + p])) + bytes([65 + p]) * (p + 1), False) for p in range(5)]
    first[2] = (2, head + rest, False)
    second = [(p, R(oracle.hash(s[2 + p])) + X(s[7]) + LIT, False) for p in range(5)]
    second[2] = (2, rest, False)
    steps = [('calls', first), ('learn', 2, [m1, m2]), ('calls', second)]
    return {'name': 'blocked', 'kinds': ['plain'] * 5, 'steps': steps, 'head': len(head),
            'unknown': sorted({oracle.hash(m1), oracle.hash(m2)})}


# ---- case 3: calls the launch does not serve, beside plain ones

def case_outside(oracle):
    s = rnd_segs(31, 100)
    fa, fb = family(0x51)[:2]
    assert oracle.hash(fa) == oracle.hash(fb) and fa != fb
    hs = np.unique(np.random.default_rng(0x2049).integers(1 << 40, 1 << 62, 2200, dtype=np.uint64))[:2049]
    assert hs.size == 2049
    big = X(s[3]) + X(s[4]) + R(oracle.hash(s[3]))
    big += b'q' * (MIB + 1 - len(big))
    # the bounded peer: 31 + 31 + 10 EXTRACTs over three calls on a limit of 64, so the first ones are evicted
    fill = [b''.join(X(s[10 + k]) for k in range(a, b)) for a, b in ((0, 31), (31, 62), (62, 72))]
    calls = [
        (0, LIT + X(s[0]) + R(oracle.hash(s[0])), False),
        (1, X(s[1]) + B(0) + LIT, True),                                          # a BACKREF op
        (2, X(fa) + R(oracle.hash(fa)) + X(fb) + R(oracle.hash(fb)), True),       # name reuse
        (3, LIT + X(s[2]) + b''.join(R(int(h)) for h in hs), True),               # 2049 unknown hashes
        (4, big, True),                                                           # 1 MiB + 1
        (5, LIT + X(s[5]) + b'\xf1\x07' + LIT, False),                            # a bad opcode: -1
        (6, X(s[6]) + LIT + X(s[7])[:700], False),                                # a cut EXTRACT: 3
        (7, fill[2] + R(oracle.hash(s[10])) + R(oracle.hash(s[81])), True),       # bounded: s[10] was evicted
        (8, X(s[8]) + LIT + R(oracle.hash(s[8])) + X(s[9]), True),                # pair
        (9, LIT + X(s[90]) + B(0) + X(s[91]) + B(1), True),                       # null cache
        (10, X(s[92]) + R(oracle.hash(s[92])) + b'end', False),
    ]
    kinds = ['plain'] * 7 + ['bounded', 'pair', 'null', 'plain']
    steps = [('calls', [(7, fill[0], True)]), ('calls', [(7, fill[1], True)]), ('calls', calls)]
    return {'name': 'outside', 'kinds': kinds, 'steps': steps,
            'outside': sum(c[2] for st in steps for c in st[1]), 'calls': sum(len(st[1]) for st in steps)}


# ---- case 6: more calls than compute units

def case_wide(oracle):
    n = 260
    s = rnd_segs(61, n)
    calls = [(p, LIT + X(s[p]) + bytes([97 + p % 20]) * (900 + p % 17) + R(oracle.hash(s[p])) + b'\xf1\x00' * (p % 5),
              False)
             for p in range(n)]
    return {'name': 'wide', 'kinds': ['plain'] * n, 'steps': [('calls', calls)]}


BUILDERS = [case_lengths, case_blocked, case_outside, case_wide]


def all_cases(oracle):
    return [f(oracle) for f in BUILDERS]
