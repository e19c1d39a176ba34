"""A pure-Python restatement of the noise of include/mgagate.h: Philox4x32-10 (Salmon et al., SC'11; Random123's constants) and the
keying that turns (seed, step, stream_id, element) into the gate's two uniforms.  No import of the package: the library and the kernels are
checked AGAINST this file (tests/test_gate_abi.py on the CPU, tests/test_gpu_gate.py on the device)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl increments of the key
MASK = 0xFFFFFFFF

# Random123's known answers (kat_vectors, philox4x32 10 rounds): (counter, key, output)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32(ctr, key, rounds=10):
    """ctr: 4 words, key: 2 words -> 4 words"""
    c0, c1, c2, c3 = (int(c) & MASK for c in ctr)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(rounds):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def words(seed, step, stream_id, i):
    """The Philox output of element i of a level: key = the seed's halves, counter = (i, stream_id, the step's halves)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    return philox4x32((i, int(stream_id) & MASK, step & MASK, step >> 32), (seed & MASK, seed >> 32))


def uniforms(seed, step, stream_id, i):
    """-> (k1, k2): the uniforms are k * 2^-24, the top 24 bits of words 0 and 1"""
    w = words(seed, step, stream_id, i)
    return w[0] >> 8, w[1] >> 8


def uniform_arrays(seed, step, stream_id, n):
    """u1, u2 of elements 0..n-1 as float32 arrays (vectorised over the elements: the same arithmetic in uint64)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    m = np.uint64(MASK)
    c0 = np.arange(n, dtype=np.uint64)
    c1 = np.full(n, int(stream_id) & MASK, dtype=np.uint64)
    c2 = np.full(n, step & MASK, dtype=np.uint64)
    c3 = np.full(n, step >> 32, dtype=np.uint64)
    k0, k1 = seed & MASK, seed >> 32
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                  # < 2^64: no wrap
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    scale = np.float32(2.0 ** -24)
    return (c0 >> np.uint64(8)).astype(np.float32) * scale, (c1 >> np.uint64(8)).astype(np.float32) * scale
