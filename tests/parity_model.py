"""Reference for the parity tests: GF(2^8) over 0x11D with log/exp
tables in numpy (exact integer arithmetic), and the member sets both
test files build."""

import itertools

import numpy as np

BLOCK = 512
SENTINEL = 0xE7
_seq = itertools.count()

EXP = np.zeros(510, np.uint8)
LOG = np.zeros(256, np.int64)
_x = 1
for _i in range(255):
    EXP[_i] = EXP[_i + 255] = _x
    LOG[_x] = _i
    _x = (_x << 1) ^ (0x11D if _x & 0x80 else 0)


def gf_mul(c, a):
    """Scalar c times the uint8 array a."""
    out = EXP[LOG[a] + LOG[c]]
    out[a == 0] = 0
    return out if c else np.zeros_like(a)


def parity(members):
    """(P, Q) bytes of a list of equally long bytes objects."""
    arrays = [np.frombuffer(m, np.uint8) for m in members]
    p = np.bitwise_xor.reduce(arrays)
    q = np.bitwise_xor.reduce([gf_mul(EXP[i], a) for i, a in enumerate(arrays)])
    return p.tobytes(), q.tobytes()


def model_bitmap(n_granules, mismatching):
    """Little-endian bitmap bytes: granule g is byte g//8, bit g%8."""
    out = bytearray((n_granules + 7) // 8)
    for g in mismatching:
        out[g // 8] |= 1 << (g % 8)
    return bytes(out)


class ParitySet:
    """k data bdevs with seeded random content plus P and Q bdevs filled
    with SENTINEL; member i's range starts (i + 1) blocks in, and every
    bdev has room after its range. `create(name, block, blocks)` makes
    one bdev; `kinds` overrides it per member index (k = P, k + 1 = Q)."""

    def __init__(self, create, k, length, kinds=None, seed=7):
        tag = next(_seq)
        rng = np.random.default_rng(seed)
        self.k, self.length = k, length
        self.offsets = [(i + 1) * BLOCK for i in range(k + 2)]
        blocks = length // BLOCK + k + 4
        self.bdevs = [(kinds or {}).get(i, create)(f"par-{tag}-{i}", BLOCK, blocks)
                      for i in range(k + 2)]
        self.data = [rng.integers(0, 256, length, np.uint8).tobytes()
                     for _ in range(k)]
        for bdev in self.bdevs:
            bdev.fill(0, SENTINEL, bdev.size_bytes)
        for bdev, off, payload in zip(self.bdevs, self.offsets, self.data):
            bdev.write(off, payload)
        self.p, self.q = parity(self.data)

    def kwargs(self, p=True, q=True):
        return dict(data=self.bdevs[:self.k],
                    p=self.bdevs[self.k] if p else None,
                    q=self.bdevs[self.k + 1] if q else None,
                    data_offsets=self.offsets[:self.k],
                    p_offset=self.offsets[self.k],
                    q_offset=self.offsets[self.k + 1], length=self.length)

    def store_parity(self):
        self.bdevs[self.k].write(self.offsets[self.k], self.p)
        self.bdevs[self.k + 1].write(self.offsets[self.k + 1], self.q)

    def expected(self, i):
        """What member i's whole bdev holds when its range is intact."""
        payload = (self.data + [self.p, self.q])[i]
        size = self.bdevs[i].size_bytes
        head = bytes([SENTINEL]) * self.offsets[i]
        return head + payload + bytes([SENTINEL]) * (size - len(head) - len(payload))

    def content(self, i):
        return self.bdevs[i].read(0, self.bdevs[i].size_bytes)
