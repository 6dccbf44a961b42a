"""Host-side references for the MXW4A8 tests (not a test module): the exact float64 block-scaled product of e4m3 A bytes and packed
e2m1 B codes, the e4m3 bytes on which every sum is exact, the e2m1 -> e4m3 re-encoding table, and the operand builders of the edge tests
(tests/test_gpu_mx_edges.py; tests/test_mxw4a8_host.py asserts on the host what those tests rely on)."""
import numpy as np

import mxfp4_ref
import mxfp8_ref

# e2m1 code -> the e4m3 byte of the same value (every e2m1 value is exact in e4m3):
#   0 0.5 1 1.5 2 3 4 6 -> 0x00 0x30 0x38 0x3C 0x40 0x44 0x48 0x4C, and with the sign bit 0x80 their negatives
E4M3_OF_E2M1 = np.array([0x00, 0x30, 0x38, 0x3C, 0x40, 0x44, 0x48, 0x4C, 0x80, 0xB0, 0xB8, 0xBC, 0xC0, 0xC4, 0xC8, 0xCC], np.uint8)

# the e4m3 bytes whose value is a multiple of 1/8 with magnitude at most 16: against any e2m1 code every product is a multiple of 1/16
# up to 96, so with unit scales and K <= 4096 every partial sum in any order is an fp32 value (below 2^19, four fraction bits)
EXACT_A_BYTES = np.array([b for b in range(256) if (b & 0x7F) != 0x7F and abs(mxfp8_ref.DEC_ZERO[b]) <= 16.0 and
                          mxfp8_ref.DEC_ZERO[b] * 8.0 == np.floor(mxfp8_ref.DEC_ZERO[b] * 8.0)], np.uint8)


def rand_exact_a(rng, rows, K):
    return EXACT_A_BYTES[rng.integers(0, len(EXACT_A_BYTES), size=(rows, K))]


def w_as_e4m3(B):
    """packed e2m1 (N, K/2) -> the (N, K) e4m3 bytes of the same values"""
    return E4M3_OF_E2M1[mxfp4_ref.unpack(B)]


# ---- the operand builders of the edge tests: A (rows, K) e4m3 bytes, B (rows, K / 2) e2m1 pairs, the even k in the low nibble ----------------
INT_A_BYTES = np.array([0x00, 0x38, 0x40, 0x44, 0x48, 0xB8, 0xC0, 0xC4, 0xC8], np.uint8)           # e4m3: 0, +-1, +-2, +-3, +-4
INT_B_CODES = np.array([0x0, 0x2, 0x4, 0x5, 0x6, 0x7, 0xA, 0xC, 0xD, 0xE, 0xF], np.uint8)          # e2m1: 0, +-1, +-2, +-3, +-4, +-6


def pack_e2m1(codes):
    """(rows, K) e2m1 codes -> (rows, K / 2) bytes"""
    return ((codes[:, 1::2] << 4) | codes[:, 0::2]).astype(np.uint8)


def rand_a(rng, rows, K):
    b = rng.integers(0, 256, size=(rows, K), dtype=np.uint8)
    b[(b & 0x7F) == 0x7F] ^= 1          # no NaN bytes unless a test asks for them
    return b


def rand_b(rng, rows, K):
    return rng.integers(0, 256, size=(rows, K // 2), dtype=np.uint8)


def one_hot_a(M, K, ks):
    """1.0 (0x38) at A[m, ks[m]], zero elsewhere"""
    A = np.zeros((M, K), np.uint8)
    A[np.arange(M), ks] = 0x38
    return A


def small_ints_a(rng, rows, K):
    return INT_A_BYTES[rng.integers(0, len(INT_A_BYTES), (rows, K))]


def small_ints_b(rng, rows, K):
    return pack_e2m1(INT_B_CODES[rng.integers(0, len(INT_B_CODES), (rows, K))])


def mm_ref(A, B, sa, sb, nan_zero=True):
    """-> (exact C (M, N) float64, bound sum_k |a 2^sa| |b 2^sb|); A (M, K) e4m3 bytes, B (N, K/2) packed e2m1.  nan_zero: A's bytes
    0x7F / 0xFF count as zero (FP8MI_NAN_ZERO); otherwise they are NaN.  B has no NaN encoding."""
    a = mxfp8_ref.scaled_operand(A, sa, nan_zero)
    b = mxfp4_ref.scaled_operand(B, sb)
    with np.errstate(invalid="ignore", over="ignore"):
        return a @ b.T, np.abs(a) @ np.abs(b).T
