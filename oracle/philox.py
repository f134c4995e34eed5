"""Philox4x32-10 (Salmon et al. 2011) in numpy: the generator of the DE-MCz chains and of the error-model draws.
TEST INFRASTRUCTURE ONLY.  tests/test_demcz_host.py holds it to the known answers of Random123."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key):
    """counter: four words (numbers or arrays), key: two -> the four output words, uint64 arrays holding 32-bit values"""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in counter])
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def u53(w0, w1):
    return (((w0 >> np.uint64(5)) << np.uint64(26)) + (w1 >> np.uint64(6))).astype(np.float64) * 2.0 ** -53
