"""numpy restatement of the epoch order of `dsnt_epoch_indices` (construction in csrc/augment.hip's header comment):
Philox4x32-10 in uint64 arithmetic on 32-bit words, an 8-round balanced Feistel network over 2^k >= n, cycle-walking
back into [0, n).  Shared by tests/test_loader_cpu.py and tests/test_loader_gpu.py."""
import numpy as np

U = np.uint64
M32 = U(0xFFFFFFFF)
ROUNDS = 8
DOMAIN = 0x4F524400


def philox4x32_10(c0, c1, c2, c3, seed):
    """Word 0..3 of Philox4x32-10 with counter (c0, c1, c2, c3) and key (seed lo, seed hi); arrays of 32-bit values."""
    c = [np.asarray(x, dtype=U) & M32 for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = U(seed & 0xFFFFFFFF), U((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = U(0xD2511F53) * c[0], U(0xCD9E8D57) * c[2]          # < 2^64: exact
        hi0, lo0, hi1, lo1 = p0 >> U(32), p0 & M32, p1 >> U(32), p1 & M32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + U(0x9E3779B9)) & M32, (k1 + U(0xBB67AE85)) & M32
    return c


def half_bits(n):
    k = 2
    while (1 << k) < n:
        k += 2
    return k // 2


def order(n, seed, epoch, positions=None, shuffle=True):
    """order(p) for each position (default: all of [0, n)), as int64."""
    p = np.arange(n, dtype=U) if positions is None else np.asarray(positions, dtype=U)
    if not shuffle or n == 1:
        return p.astype(np.int64)
    h = half_bits(n)
    mask = U((1 << h) - 1)

    def feistel(x):
        left, right = x >> U(h), x & mask
        for i in range(ROUNDS):
            f = philox4x32_10(right, epoch & 0xFFFFFFFF, (epoch >> 32) & 0xFFFFFFFF, DOMAIN + i, seed)[0]
            left, right = right, left ^ (f & mask)
        return (left << U(h)) | right

    y = feistel(p)
    out = y >= U(n)
    while out.any():
        y[out] = feistel(y[out])
        out = y >= U(n)
    return y.astype(np.int64)
