"""A plain AES-256-XTS (IEEE 1619) in pure Python: the yardstick of
test_crypt.py and test_crypt_gpu.py. It shares nothing with the native
implementations: the S-box comes from the field inverse, rounds work on
bytes, and the tweak is doubled as a Python int."""

import functools


def _mul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a = (a << 1) ^ (0x11B if a & 0x80 else 0)
        b >>= 1
    return r


def _sbox_entry(x):
    inv = next((c for c in range(256) if _mul(x, c) == 1), 0)
    rot = lambda v, n: ((v << n) | (v >> (8 - n))) & 0xFF  # noqa: E731
    return inv ^ rot(inv, 1) ^ rot(inv, 2) ^ rot(inv, 3) ^ rot(inv, 4) ^ 0x63


SBOX = bytes(_sbox_entry(x) for x in range(256))
MUL2 = bytes(_mul(x, 2) for x in range(256))
MUL3 = bytes(_mul(x, 3) for x in range(256))
# State byte 4 * c + r is row r of column c.
SHIFT_ROWS = [4 * ((c + r) % 4) + r for c in range(4) for r in range(4)]
DOWN = [[4 * c + (r + k) % 4 for c in range(4) for r in range(4)]
        for k in range(4)]  # row r + k of the same column


def _xor(a, b):
    return (int.from_bytes(a, "little") ^
            int.from_bytes(b, "little")).to_bytes(len(a), "little")


@functools.lru_cache(maxsize=8)
def expand(key):
    """The 15 round keys of a 32-byte key."""
    w = [key[4 * i:4 * i + 4] for i in range(8)]
    rcon = 1
    for i in range(8, 60):
        t = w[i - 1]
        if i % 8 == 0:
            t = _xor((t[1:] + t[:1]).translate(SBOX), bytes([rcon, 0, 0, 0]))
            rcon = _mul(rcon, 2)
        elif i % 8 == 4:
            t = t.translate(SBOX)
        w.append(_xor(w[i - 8], t))
    return [b"".join(w[4 * r:4 * r + 4]) for r in range(15)]


def encrypt_block(round_keys, block):
    s = _xor(block, round_keys[0])
    for r in range(1, 15):
        s = s.translate(SBOX)
        s = bytes(s[i] for i in SHIFT_ROWS)
        if r != 14:  # MixColumns: 2 * row r + 3 * row r+1 + row r+2 + row r+3
            m2, m3 = s.translate(MUL2), s.translate(MUL3)
            s = _xor(_xor(m2, bytes(m3[i] for i in DOWN[1])),
                     _xor(bytes(s[i] for i in DOWN[2]),
                          bytes(s[i] for i in DOWN[3])))
        s = _xor(s, round_keys[r])
    return s


def xts_encrypt(key, unit, data):
    """One data unit (a multiple of 16 bytes) under the 64-byte key."""
    k1, k2 = expand(key[:32]), expand(key[32:])
    t = int.from_bytes(
        encrypt_block(k2, unit.to_bytes(8, "little") + bytes(8)), "little")
    out = b""
    for at in range(0, len(data), 16):
        mask = t.to_bytes(16, "little")
        out += _xor(encrypt_block(k1, _xor(data[at:at + 16], mask)), mask)
        t <<= 1
        if t >> 128:
            t = (t ^ 0x87) & ((1 << 128) - 1)
    return out


def xts_encrypt_units(key, granule, data, first_unit=0):
    return b"".join(xts_encrypt(key, first_unit + i,
                                data[i * granule:(i + 1) * granule])
                    for i in range(len(data) // granule))


def kcv(key):
    return int.from_bytes(xts_encrypt(key, 2 ** 64 - 1, bytes(16))[:4], "little")
