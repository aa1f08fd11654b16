"""
A dense reference of the covariance sums of the sheared pre-psf moments when
the noise power comes from a noise image (DESIGN.md 3.28;
PrePSFMom(use_noise_image=True).measure_arrays_sheared(noise_images=),
ngmix_prepsf_shear_*power_sums_*): the definition evaluated directly, explicit
phase matrices, no recurrence, in np.longdouble.  It shares no code with
csrc/prepsf_shear.hpp; the kept modes, the sheared frequencies, the dense
transform and the psf's floor are those of helpers/prepsf_shear_reference.py
and helpers/prepsf_shear_noise_reference.py, imported, not restated.

For one stamp of side dim, its psf stamp P, its UN-tapered noise image N and
every kept mode k of weight w(k) (1 or 2) and kernels K_a = fkp, fkc, fkr, fkf,
with eff = D / dim, k' the sheared frequency of k, q = (-k_c, k_r) and q' its
sheared frequency:

    cov_ab = D^-4 eff^2 sum_k w K_a K_b [ |N^(k')|^2 / |P^(k')|^2
                                          + (fixnoise) |N^(q'_c, -q'_r)|^2 / |P^(q')|^2 ]

The moment sums are not restated here: they are those of the forms without
the noise image, to the bit (the tests compare them with those entries).

THE BOUND, in the form of helpers/kfit_cases.py: C_ROUND(n) 2^-52 sum |terms|
per covariance sum, n = max(dim, pdim).  A term of the sum is itself a triple
sum -- |N^|^2 = sum_pp' N_p N_p' cos(k'.(x_p - x_p')) and the same for the psf --
and its rounding error is not relative to the term (|N^| has zeros) but to the
sum of the absolute values of what it is made of, A_N = sum |N| and A_P =
sum |P|.  The |term| of a mode is therefore its majorant

    w |K_a K_b| eff^2 A_N^2 A_P / |P^|^3        (>= the term: A_P >= |P^|)

to which both the error of |N^|^2 (<= 2 A_N dN) and that of 1 / |P^|^2 (<= 2
dP / |P^|^3) are relative.  Counted on csrc/prepsf_shear.hpp and dtft.hpp, in
units of 2^-52 (a rounding is half a unit), for one transform relative to A:
  the frequency: mode_freq (3 roundings), the two 2 x 2 maps and the closing sum
    (10 roundings on the sheared part, which is <= 0.4 of k at |g| = 0.3): k' is
    <= 4 units of pi off; the phase of a pixel up to n from the centre on both
    axes moves by 4 pi 2 n                                                25 n
  the seeds' arguments q (rs - r0): half a unit of <= pi n, two axes       3 n
  sincos of the seeds (2 ulp each) and their product                          6
  the recurrence: <= 15 + 15 complex products of 2 units                   4 n
  its steps exp(-i q): 2 ulp of sincos, carried <= 15 + 15 times           4 n
  the sum of n^2 terms, half a unit each                               n^2 / 2
which is c_T(n) = n^2 / 2 + 36 n + 6 (with 16 for the 15 + 15 <= 2 n of the
seeded recurrence: SEED = 16 bounds it for every n).  A term takes 2 c_T from
|N^|^2 and 2 c_T from |P^|^2, 4 units from its own products and quotient, and
8 from the sum over the block (<= ceil(modes / 64) + 10 additions):

    C_ROUND(n) = 4 c_T(n) + 12 = 2 n^2 + 144 n + 36        (2852 at n = 16)

Measured (tests/test_prepsf_shear_power_host.py prints the figures): the host
twins are 0.14 units off at most (dim 9 / 7, ksigma), at g = 0 they and the
unsheared measurement's stages differ by 0.086 units at most (DESIGN.md 3.28
has the kernel's figures) -- the majorant is far above a typical term, by
A_N^2 / |N^|^2 ~ 0.6 n^2 and A_P / |P^| up to 10^2, so the bound is loose for
rounding; a wrong frequency, a tapered plane or a missing eff^2 moves a sum by
10^-3 to 1 of itself, 10^5 and more times the bound
(test_the_noise_image_is_seen).
"""
import numpy as np

from . import prepsf_shear_noise_reference as pn
from . import prepsf_shear_reference as ps
from .prepsf_shear_noise_reference import (  # noqa: F401  (what the tests take from here)
    AP_RADS, DERIV, KINDS, STEP, TYPES, case, gaussian_stamp, host_fexp, measure_of, noise_planes,
    plan_of, turned, type_shears)

LD = np.longdouble
EPS = 2.0 ** -52
# (dim, pdim, number of stamps): an odd stamp with a smaller psf, one where both
# are the same and no multiple of the recurrence's seed distance, one at it
SHAPES = ((9, 7, 3), (12, 12, 3), (16, 9, 3))


def c_round(dim, pdim):
    n = max(dim, pdim)
    return 2.0 * n * n + 144.0 * n + 36.0


def power_planes(dim, pdim, n, seed=23):
    """the noise images of case(dim, pdim, n): seeded normals smoothed along the
    rows (correlated, not the fixnoise field of noise_planes)"""
    rng = np.random.RandomState(seed + 100 * dim + pdim + n)
    z = rng.normal(scale=0.25, size=(n, dim, dim + 2))
    return np.ascontiguousarray(z[:, :, :-2] + 0.7 * z[:, :, 1:-1] + 0.3 * z[:, :, 2:])


def frequencies(deriv, g, rows, cols, D, dtype=LD):
    """(k', q') of the kept modes, each (2, M): the sheared frequency of k and
    that of the turned q = (-k_c, k_r)"""
    f = (np.fft.fftfreq(D) * (2.0 * np.pi)).astype(dtype)
    k = np.stack([f[rows], f[cols]])
    q = np.stack([-k[1], k[0]])
    return pn._sheared(k, deriv, g, dtype), pn._sheared(q, deriv, g, dtype)


def plane_power(plane, qr, qc, dtype=LD):
    """|N^(qr, qc)|^2 of the plane as it is (no taper), dense"""
    t = pn._dtft(np.asarray(plane, dtype=dtype), np.zeros(2, dtype=dtype), qr, qc)
    return t.real ** 2 + t.imag ** 2


def cov_sums(power_k, power_q, psf, psf_cen, ks, qs, wgt, fk, D, dim, a_n, dtype=LD):
    """the ten covariance sums from the noise power at the modes: power_k at k',
    power_q at (q'_c, -q'_r) or None without fixnoise; a_n = sum |N| of the
    plane the powers came from (for the majorants).  Returns (sums (10,), flag,
    absum (10,): the sum of the terms' majorants)"""
    pi = dtype(np.pi)
    psf = np.asarray(psf, dtype=dtype)
    psf_cen = np.asarray(psf_cen, dtype=dtype)
    band = [ks] if power_q is None else [ks, qs]
    out_of_band = any(bool(np.any(~(np.abs(b) < pi))) for b in band)
    wg, fk = wgt.astype(dtype), fk.astype(dtype)
    eff2 = (dtype(D) / dtype(dim)) ** 2
    df4 = (dtype(1) / dtype(D)) ** 4
    a_p = np.abs(psf).sum()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        parts = []
        for power, fr in ((power_k, ks), (power_q, qs)):
            if power is None:
                continue
            tp = pn._floored(pn._dtft(psf, psf_cen, fr[0], fr[1]), psf, dtype)
            amp2 = tp.real ** 2 + tp.imag ** 2
            parts.append((wg * eff2 * power / amp2,
                          wg * eff2 * dtype(a_n) ** 2 * a_p / amp2 ** dtype(1.5)))
        sums, absum = [], []
        for a in range(4):
            for b in range(a, 4):
                sums.append(sum((fk[a] * fk[b] * c).sum() for c, _ in parts) * df4)
                absum.append(sum((np.abs(fk[a] * fk[b]) * m).sum() for _, m in parts) * df4)
    sums, absum = np.array(sums, dtype=dtype), np.array(absum, dtype=dtype)
    if out_of_band or not np.all(np.isfinite(sums.astype(np.float64))):
        return np.full(10, np.nan, dtype=dtype), 1, absum
    return sums, 0, absum


def power_sums(power_plane, psf, psf_cen, deriv, g, rows, cols, wgt, fk, D, fixnoise,
               dtype=LD):
    """the definition for one stamp's noise image and one shear"""
    dim = power_plane.shape[0]
    ks, qs = frequencies(deriv, g, rows, cols, D, dtype)
    pk = plane_power(power_plane, ks[0], ks[1], dtype)
    pq = plane_power(power_plane, qs[1], -qs[0], dtype) if fixnoise else None
    return cov_sums(pk, pq, psf, psf_cen, ks, qs, wgt, fk, D, dim,
                    np.abs(np.asarray(power_plane, dtype=dtype)).sum(), dtype)


_CACHE = {}


def reference(dim, pdim, n, kind, ap_rad, fixnoise):
    """
    The reference covariance sums of case(dim, pdim, n) with power_planes(dim,
    pdim, n) under measure_of(kind, dim, ap_rad), computed once per process and
    not changed afterwards: 'types' (n, 5, 10) with flags and absum, 'galshear'
    (n, 1, 10) likewise (the per-stamp shears).  (The taper does not enter the
    covariance: ap_rad only names the measurement.)
    """
    key = (dim, pdim, n, kind, ap_rad, bool(fixnoise))
    if key in _CACHE:
        return _CACHE[key]
    c, planes = case(dim, pdim, n), power_planes(dim, pdim, n)
    _, D, rows, cols, wgt, fk = plan_of(measure_of(kind, dim, ap_rad), dim, pdim)
    out = {}
    for name, shears in (("types", None), ("galshear", c["shears"])):
        nt = 5 if shears is None else 1
        sums = np.full((n, nt, 10), np.nan, dtype=LD)
        absum = np.full((n, nt, 10), np.nan, dtype=LD)
        flags = np.zeros((n, nt), dtype=np.int32)
        for i in range(n):
            for t in range(nt):
                g = type_shears()[t] if shears is None else shears[i]
                sums[i, t], flags[i, t], absum[i, t] = power_sums(
                    planes[i], c["psfs"][i], c["pcen"][i], DERIV, g, rows, cols, wgt, fk, D,
                    fixnoise)
        for a in (sums, absum, flags):
            a.setflags(write=False)
        out[name] = dict(sums=sums, absum=absum, flags=flags)
    _CACHE[key] = out
    return out


def worst_ratio(got, ref):
    """max |got - ref| / (2^-52 sum |terms|) over a reference dict's unflagged
    covariance sums; got: (..., 10)"""
    ok = ref["flags"] == 0
    err = np.abs(np.asarray(got, dtype=LD)[ok] - ref["sums"][ok])
    return float((err / (LD(EPS) * ref["absum"][ok])).max())


def call_host(L, ptr, c, power, nturned, g, rows, cols, kwgt, kfk, D, ap_rad, deriv=DERIV,
              host=True, base=False, **over):
    """ngmix_prepsf_shear_power_sums_host, or with TURNED fixnoise planes nturned
    ngmix_prepsf_shear_fixnoise_power_sums_host (host=False: the _batch entries
    with a null stream, for the refusals; base=True: the entries without the
    noise image, on the same arrays) (ps.call_entry)."""
    return ps.call_entry(L, ptr, c, g, rows, cols, kwgt, kfk, D, ap_rad, deriv, host,
                         fixnoise=nturned is not None or "noise_turned" in over,
                         nturned=nturned, with_power=not base, power=power, **over)


# ---------------------------------------------------------------------------
# stationary correlated noise: white noise on an (n + 2)^2 grid convolved
# ('valid') with a fixed 3 x 3 kernel that has no mirror symmetry, so that the
# power at (q_c, -q_r) differs from that at (q_r, q_c) and at (q_c, q_r)

STAT_DIM, STAT_N = 16, 256
STAT_KERNEL = np.array([[0.0, 0.5, 1.0],
                        [0.3, 2.0, 0.5],
                        [1.0, 0.2, 0.0]])
STAT_SIGMA = 0.5


def correlated_noise(rng, n, dim, kernel=STAT_KERNEL, sigma=STAT_SIGMA):
    z = rng.normal(scale=sigma, size=(n, dim + 2, dim + 2))
    out = np.zeros((n, dim, dim))
    for a in range(3):
        for b in range(3):
            out += kernel[a, b] * z[:, a:a + dim, b:b + dim]
    return out


def autocorrelation(kernel=STAT_KERNEL, sigma=STAT_SIGMA):
    """{(dr, dc): xi(dr, dc)} of the process: <N[r, c] N[r + dr, c + dc]>"""
    xi = {}
    for dr in range(-2, 3):
        for dc in range(-2, 3):
            s = 0.0
            for a in range(3):
                for b in range(3):
                    if 0 <= a - dr < 3 and 0 <= b - dc < 3:
                        s += kernel[a, b] * kernel[a - dr, b - dc]
            xi[dr, dc] = sigma ** 2 * s
    return xi


def expected_power(qr, qc, dim, xi, dtype=LD):
    """E |N^(q)|^2 = sum_D xi(D) (n - |D_r|) (n - |D_c|) cos(q . D)"""
    out = np.zeros(qr.shape, dtype=dtype)
    for (dr, dc), v in xi.items():
        out = out + dtype(v) * (dim - abs(dr)) * (dim - abs(dc)) * np.cos(qr * dr + qc * dc)
    return out
