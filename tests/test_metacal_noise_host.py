"""
The metacal noise planes through their host twin (ngmix_metacal_noise_host,
csrc/metacal_noise.hpp: the code the kernel runs, with the host libm) against
tests/helpers/philox_reference.py.  No kernel is launched here.

Tolerance of the normals, from the formats: log within 1 ulp (2^-52), the
square root halves that and adds 2^-53, the angle (pi/2) f carries 2^-53 of its
product and 2^-53 of the constant (|a| <= pi/4, so neither sin nor cos
amplifies it), sincos 2^-52, the product r c and the division by ierr 2^-53
each: 8 x 2^-53 relative in all.
"""
import numpy as np
import pytest

from ngmix_amd import _lib
from helpers import philox_reference as pr

REL_TOL = 8 * 2.0 ** -53
SEED = 2 ** 40 + 7                      # above 2^32: a truncated key shows
IDS = np.array([0, 1, 2 ** 32, 2 ** 40 + 3], dtype=np.int64)
SHAPES = [(7, 9), (16, 16), (12, 17)]


def host(ierr, ids, seed, rot_k=0):
    ierr = np.ascontiguousarray(ierr, dtype=np.float64)
    n, nrow, ncol = ierr.shape
    out = np.full(ierr.shape, np.nan)
    ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int64)
    st = _lib.lib().ngmix_metacal_noise_host(
        _lib.ptr(ierr), None if ids is None else _lib.ptr(ids), seed, n, nrow, ncol, rot_k,
        _lib.ptr(out))
    assert st == _lib.OK, _lib.last_error()
    return out


def make_ierr(shape, seed=5):
    rng = np.random.RandomState(seed)
    ierr = rng.uniform(0.5, 2.0, size=(IDS.size,) + shape)
    ierr[rng.uniform(size=ierr.shape) < 0.1] = 0.0
    ierr[0, 0, 0] = 0.0
    ierr[1, -1, -1] = -1.0               # not > 0: a zero too
    return ierr


def test_reference_reproduces_the_known_answer_vectors():
    for counter, key, want in pr.KNOWN_ANSWERS:
        assert pr.philox4x32_10(counter, key) == want
        assert tuple(int(w) for w in pr.philox4x32_10_u64([counter], [key])[0]) == want


def test_the_two_forms_of_the_reference_agree():
    rng = np.random.RandomState(1)
    c = rng.randint(0, 2 ** 32, size=(50, 4), dtype=np.uint64)
    k = rng.randint(0, 2 ** 32, size=(50, 2), dtype=np.uint64)
    vec = pr.philox4x32_10_u64(c, k)
    for i in range(50):
        assert tuple(int(w) for w in vec[i]) == pr.philox4x32_10(c[i], k[i])


def test_philox_words_equal_the_reference():
    rows = [(c, k) for c, k, _ in pr.KNOWN_ANSWERS]
    for obj_id in IDS:
        for j in (0, 1, 31, 127):
            obj_id = int(obj_id)
            rows.append(((obj_id & pr.MASK, obj_id >> 32, j, 0), (SEED & pr.MASK, SEED >> 32)))
    c = np.array([r[0] for r in rows], dtype=np.uint32)
    k = np.array([r[1] for r in rows], dtype=np.uint32)
    out = np.zeros((len(rows), 4), dtype=np.uint32)
    st = _lib.lib().ngmix_philox4x32_10_host(_lib.ptr(c), _lib.ptr(k), len(rows), _lib.ptr(out))
    assert st == _lib.OK
    for i, (cc, kk) in enumerate(rows):
        assert tuple(int(w) for w in out[i]) == pr.philox4x32_10(cc, kk)
    assert tuple(int(w) for w in out[0]) == pr.KNOWN_ANSWERS[0][2]


@pytest.mark.parametrize("shape", SHAPES)
def test_normals_against_the_longdouble_reference(shape):
    ierr = make_ierr(shape)
    got = host(ierr, IDS, SEED)
    ref = pr.noise_planes(ierr, IDS, SEED)
    zero = ~(ierr > 0)
    assert zero.any() and np.all(ref[zero] == 0)
    assert np.all(got[zero] == 0.0) and not np.signbit(got[zero]).any()
    gap = np.abs(got[~zero] - ref[~zero]) / np.abs(ref[~zero])
    print("shape %s: largest relative gap %.3g (allowed %.3g)" % (shape, gap.max(), REL_TOL))
    assert gap.max() <= REL_TOL
    # a truncated id or seed would repeat another stream
    for a in range(IDS.size):
        for b in range(a):
            assert not np.array_equal(got[a][~zero[a] & ~zero[b]] * ierr[a][~zero[a] & ~zero[b]],
                                      got[b][~zero[a] & ~zero[b]] * ierr[b][~zero[a] & ~zero[b]])
    assert not np.array_equal(got, host(ierr, IDS, SEED & 0xffffffff))


def test_null_ids_are_the_indices():
    ierr = make_ierr((7, 9))
    assert np.array_equal(host(ierr, None, SEED), host(ierr, np.arange(IDS.size), SEED))


def test_rotated_form_is_rot90_to_the_bit():
    ierr = make_ierr((16, 16))
    plain, turned = host(ierr, IDS, SEED), host(ierr, IDS, SEED, rot_k=1)
    for i in range(IDS.size):
        assert np.array_equal(turned[i], np.rot90(plain[i], 1))
        assert np.array_equal(np.signbit(turned[i]), np.signbit(np.rot90(plain[i], 1)))
    ref = pr.noise_planes(ierr, IDS, SEED, rot_k=1)
    assert np.abs(turned - ref).max() <= REL_TOL * np.abs(ref).max()


@pytest.mark.parametrize("shape", SHAPES)
def test_a_stamp_does_not_depend_on_its_batch(shape):
    ierr = make_ierr(shape)
    whole = host(ierr, IDS, SEED)
    for i in range(IDS.size):
        assert np.array_equal(host(ierr[i:i + 1], IDS[i:i + 1], SEED)[0], whole[i])
    perm = np.array([2, 0, 3, 1])
    assert np.array_equal(host(ierr[perm], IDS[perm], SEED), whole[perm])


def test_refusals():
    L = _lib.lib()
    ierr = np.ones((2, 4, 4))
    out = np.zeros_like(ierr)
    ids = np.arange(2, dtype=np.int64)

    def call(ierr_p, n, nrow, ncol, rot_k, out_p):
        return L.ngmix_metacal_noise_host(ierr_p, _lib.ptr(ids), 1, n, nrow, ncol, rot_k, out_p)
    pi, po = _lib.ptr(ierr), _lib.ptr(out)
    assert call(pi, -1, 4, 4, 0, po) == _lib.ERR_BAD_ARG
    assert call(pi, 2, 0, 4, 0, po) == _lib.ERR_BAD_ARG
    assert call(pi, 2, 4, 0, 0, po) == _lib.ERR_BAD_ARG
    assert call(pi, 2, -4, 4, 0, po) == _lib.ERR_BAD_ARG
    assert call(pi, 2, 4, 4, 2, po) == _lib.ERR_BAD_ARG
    assert call(pi, 2, 4, 4, -1, po) == _lib.ERR_BAD_ARG
    assert call(pi, 1, 2, 8, 1, po) == _lib.ERR_BAD_ARG
    assert "square" in _lib.last_error()
    assert call(None, 2, 4, 4, 0, po) == _lib.ERR_BAD_ARG
    assert call(pi, 2, 4, 4, 0, None) == _lib.ERR_BAD_ARG
    assert np.all(out == 0)
    # nothing to do: no pointer is read
    assert call(None, 0, 4, 4, 0, None) == _lib.OK
    assert call(pi, 2, 4, 4, 1, po) == _lib.OK
    # the device entry refuses the same calls before it launches anything
    for args in ((pi, -1, 4, 4, 0, po), (pi, 2, 0, 4, 0, po), (pi, 2, 4, 4, 2, po),
                 (pi, 1, 2, 8, 1, po), (None, 2, 4, 4, 0, po), (pi, 2, 4, 4, 0, None)):
        assert L.ngmix_metacal_noise_batch(args[0], None, 1, *args[1:], None) == _lib.ERR_BAD_ARG
    assert L.ngmix_metacal_noise_batch(None, None, 1, 0, 4, 4, 0, None, None) == _lib.OK


# ---- moments: 70 stamps of 16 x 16 with unit ierr, n = 17920 draws; every
# bound is five standard deviations of the statistic for independent unit normals

MOMENT_SEEDS = [11, 2 ** 40 + 7]


def _moments(z):
    """z (70, 16, 16): mean, variance - 1, lag-1 correlation along rows, the
    correlation of the cosine and sine members, and their 5 sigma bounds"""
    n = z.size
    flat = z.reshape(z.shape[0], -1)
    lag = np.corrcoef(z[:, :, :-1].ravel(), z[:, :, 1:].ravel())[0, 1]
    pair = np.corrcoef(flat[:, 0::2].ravel(), flat[:, 1::2].ravel())[0, 1]
    # (the two correlations rest on fewer than n products: 5 / sqrt(n) is the
    # tighter bound for them)
    return [("mean", abs(z.mean()), 5 / np.sqrt(n)),
            ("variance", abs(z.var() - 1), 5 * np.sqrt(2.0 / n)),
            ("lag-1", abs(lag), 5 / np.sqrt(n)),
            ("cos-sin", abs(pair), 5 / np.sqrt(n))]


@pytest.mark.parametrize("seed", MOMENT_SEEDS)
def test_moments(seed):
    ierr = np.ones((70, 16, 16))
    got = host(ierr, None, seed)
    # (the reference's own draws meet the same conditions for these seeds)
    ref = np.stack([pr.unit_normals(seed, i, 256).astype(np.float64).reshape(16, 16)
                    for i in range(70)])
    for what, z in (("reference", ref), ("host twin", got)):
        for name, value, bound in _moments(z):
            print("%s seed %d %s: %.4g (bound %.4g)" % (what, seed, name, value, bound))
            assert value <= bound, (what, name)
