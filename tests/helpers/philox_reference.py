"""
The reference of the metacal noise planes (csrc/metacal_noise.hpp), written
from the definition and independent of the library: Philox4x32-10 on Python
integers, the uniforms and Box-Muller in numpy.longdouble.

    philox4x32_10(counter, key)            four words, Python ints
    philox4x32_10_u64(counters, keys)      the same, vectorised on numpy.uint64
    pair_uniform_ints(seed, id, j)         the integers k1, k2 of u = k 2^-53
    normal_pair(seed, id, j)               (z0, z1) in longdouble
    noise_planes(ierr, ids, seed, rot_k)   (n, nrow, ncol) longdouble

The cosine and sine of 2 pi u2 are taken by quadrant: 4 u2 = q + f with the
integer q nearest to it (halves upwards), formed exactly on the integers, and
cos / sin of (pi / 2) f in longdouble -- the same function, without the loss
next to its zeros that rounding 2 pi u2 first would bring.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

LD = np.longdouble
# pi / 2 to the longdouble's last place (arctan(1) = pi / 4 is evaluated in longdouble)
HALF_PI = LD(2) * np.arctan(LD(1))

# Random123's known-answer vectors for philox4x32 with 10 rounds
# (counter, key, output)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox4x32_10_u64(counters, keys):
    """the second, independently written form: arrays (n, 4) and (n, 2)"""
    c = np.array(counters, dtype=np.uint64).reshape(-1, 4) & np.uint64(MASK)
    k = np.array(keys, dtype=np.uint64).reshape(-1, 2) & np.uint64(MASK)
    m32 = np.uint64(MASK)
    sh = np.uint64(32)
    x0, x1, x2, x3 = (c[:, i].copy() for i in range(4))
    ka, kb = k[:, 0].copy(), k[:, 1].copy()
    for r in range(10):
        if r > 0:
            ka = (ka + np.uint64(W0)) & m32
            kb = (kb + np.uint64(W1)) & m32
        prod_a = np.uint64(M0) * x0        # < 2^64: no wrap
        prod_b = np.uint64(M1) * x2
        y0 = (prod_b >> sh) ^ x1 ^ ka
        y1 = prod_b & m32
        y2 = (prod_a >> sh) ^ x3 ^ kb
        y3 = prod_a & m32
        x0, x1, x2, x3 = y0, y1, y2, y3
    return np.stack([x0, x1, x2, x3], axis=1).astype(np.uint32)


def pair_words(seed, obj_id, j):
    seed, obj_id = int(seed) & (2 ** 64 - 1), int(obj_id) & (2 ** 64 - 1)
    return philox4x32_10((obj_id & MASK, obj_id >> 32, int(j), 0), (seed & MASK, seed >> 32))


def pair_uniform_ints(seed, obj_id, j):
    """k1, k2 in [1, 2^53]: u = k 2^-53"""
    w0, w1, w2, w3 = pair_words(seed, obj_id, j)
    return ((w0 >> 5) << 26) + (w1 >> 6) + 1, ((w2 >> 5) << 26) + (w3 >> 6) + 1


def _cossin_2pi(k):
    """cos, sin of 2 pi k 2^-53 in longdouble"""
    q = (k + (1 << 50)) >> 51                  # round(4 u), halves upwards
    f = LD(k - (q << 51)) / LD(2 ** 51)        # exact: |.| <= 2^50
    c, s = np.cos(HALF_PI * f), np.sin(HALF_PI * f)
    return [(c, s), (-s, c), (-c, -s), (s, -c)][q & 3]


def normal_pair(seed, obj_id, j):
    k1, k2 = pair_uniform_ints(seed, obj_id, j)
    u1 = LD(k1) / LD(2 ** 53)                  # exact
    r = np.sqrt(LD(-2) * np.log(u1))
    c, s = _cossin_2pi(k2)
    return r * c, r * s


def unit_normals(seed, obj_id, npix):
    """the npix unit normals of one object, un-rotated row-major, longdouble"""
    z = np.zeros(npix + 1, dtype=LD)
    for j in range((npix + 1) // 2):
        z[2 * j], z[2 * j + 1] = normal_pair(seed, obj_id, j)
    return z[:npix]


def noise_planes(ierr, ids, seed, rot_k=0):
    ierr = np.asarray(ierr, dtype=np.float64)
    n, nrow, ncol = ierr.shape
    out = np.zeros((n, nrow, ncol), dtype=LD)
    for i in range(n):
        z = unit_normals(seed, i if ids is None else ids[i], nrow * ncol).reshape(nrow, ncol)
        pos = ierr[i] > 0
        out[i][pos] = z[pos] / ierr[i][pos].astype(LD)
        if rot_k:
            out[i] = np.rot90(out[i], rot_k)
    return out
