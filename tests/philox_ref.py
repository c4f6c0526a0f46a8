"""An independent reference of the noise the SDE kernels draw (helper module of tests/test_noise_reference.py; numpy only).

philox4x32_10 is written from the published definition of the generator (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as
easy as 1, 2, 3", SC'11, and the Random123 library's known-answer vectors), not from the kernel source:

    one round, counter (c0, c1, c2, c3), key (k0, k1):      (hi0, lo0) = M0 * c0,   (hi1, lo1) = M1 * c2     (32 x 32 -> 64 bit)
                                                            (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)
    between rounds the key is bumped:                       k0 += W0, k1 += W1                                 (mod 2^32)
    M0 = 0xD2511F53, M1 = 0xCD9E8D57, W0 = 0x9E3779B9 (golden ratio), W1 = 0xBB67AE85 (sqrt 3 - 1); ten rounds, nine bumps.

complex_normal_ref is the project's layout on top of it (include/storm_hip.h, storm_complex_randn): key = seed, counter words
(idx low, idx high, offset low, offset high), Box-Muller on the first two output words.  The two uniforms and the angle are single
IEEE fp32 operations of exactly representable inputs and are reproduced bit for bit in np.float32; the radius sqrt(-ln u1) and
cos / sin of the angle are evaluated in float64, so what is left between a kernel and this reference is the rounding of the
kernel's logf, sqrtf, sincosf and one multiply."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
ROUNDS = 10
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
TWO_PI_F32 = np.float32(6.2831855)                    # fl32(2 pi) = 0x40C90FDB


def _u64(v):
    """ints (python ints up to 2^64 - 1, sequences or arrays of them) as a uint64 array"""
    if isinstance(v, np.ndarray) and v.dtype == np.uint64:
        return v
    if isinstance(v, np.ndarray) and v.dtype.kind == "i":
        return v.astype(np.int64).view(np.uint64)      # (the kernels read an int64 key table as unsigned: the same 64 bits)
    if np.ndim(v) == 0:
        return np.array(int(v) % 2 ** 64, dtype=np.uint64)
    obj = np.array(v, dtype=object)                      # (python ints stay python ints: numpy would make floats of a list that mixes 0 and 2^64 - 1)
    return np.array([int(x) % 2 ** 64 for x in obj.ravel()], dtype=np.uint64).reshape(obj.shape)


def philox4x32_10(key64, ctr_lo64, ctr_hi64):
    """Philox4x32-10 of key (k0, k1) = (low, high word of key64) and counter (c0, c1, c2, c3) = (low, high word of ctr_lo64, low,
    high word of ctr_hi64); the arguments broadcast.  Returns the four output words as uint32 arrays."""
    key64, lo, hi = np.broadcast_arrays(_u64(key64), _u64(ctr_lo64), _u64(ctr_hi64))
    k0, k1 = key64 & _MASK, key64 >> _S32              # every 32-bit word lives in a uint64: products fit, sums are masked
    c0, c1, c2, c3 = lo & _MASK, lo >> _S32, hi & _MASK, hi >> _S32
    m0, m1, w0, w1 = np.uint64(M0), np.uint64(M1), np.uint64(W0), np.uint64(W1)
    for rnd in range(ROUNDS):
        if rnd:
            k0, k1 = (k0 + w0) & _MASK, (k1 + w1) & _MASK
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def uniform_f32(word):
    """u = (float(word >> 8) + 0.5f) * 2^-24 in fp32.  word >> 8 < 2^24 is exact; from 2^23 on the fp32 spacing is 1, so + 0.5f is a tie
    that rounds to even: u lies in (0, 1] and reaches 1.0 for word >> 8 = 0xFFFFFF.  The scaling is exact."""
    v = (np.asarray(word, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)
    return (v + np.float32(0.5)) * np.float32(2.0 ** -24)


def complex_normal_ref(seed, idx, offset):
    """(re, im) in float64 of the standard complex normal draw of (key seed, element idx, offset): re, im ~ N(0, 1/2)"""
    c0, c1, _, _ = philox4x32_10(seed, idx, offset)
    u1, u2 = uniform_f32(c0), uniform_f32(c1)
    theta = (TWO_PI_F32 * u2).astype(np.float32)        # one fp32 multiply, as the kernel's
    assert u1.dtype == np.float32 and theta.dtype == np.float32
    r = np.sqrt(-np.log(u1.astype(np.float64)))
    th = theta.astype(np.float64)
    return r * np.cos(th), r * np.sin(th)


def draw_one_seed(seed, B, n, offset):
    """complex128 [B, n]: the one-seed form, element i of row b is the draw of counter b * n + i"""
    idx = np.arange(B * n, dtype=np.uint64).reshape(B, n)
    re, im = complex_normal_ref(seed, idx, offset)
    return re + 1j * im


def draw_row_keys(row_seeds, n, offset):
    """complex128 [B, n]: a key per row, element i of row b is the draw of (key row_seeds[b], counter i)"""
    keys = _u64(row_seeds).reshape(-1, 1)
    re, im = complex_normal_ref(keys, np.arange(n, dtype=np.uint64)[None, :], offset)
    return re + 1j * im


def draw(B, n, offset, seed=0, row_seeds=None):
    """the draw of a call on a batch of B rows of n elements in either key mode (the keywords of storm_amd.ops)"""
    return draw_one_seed(seed, B, n, offset) if row_seeds is None else draw_row_keys(row_seeds, n, offset)


def ulp32(v):
    """the spacing of fp32 at |v| (float64 array): 2^(e - 23) for 2^e <= |v| < 2^(e + 1), the subnormal spacing 2^-149 below 2^-126"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return np.exp2(e - 23)


def ulp_dev(got, ref):
    """per component: |got - ref| in fp32 ulps of the reference component; got complex64 / float32, ref complex128 / float64"""
    got, ref = np.asarray(got), np.asarray(ref)
    if np.iscomplexobj(ref):
        return np.maximum(ulp_dev(got.real, ref.real), ulp_dev(got.imag, ref.imag))
    return np.abs(got.astype(np.float64) - ref) / ulp32(ref)
