"""
A dense reference of the sheared pre-psf moments WITH the fixnoise term
(PrePSFMom.measure_arrays_sheared(noise=),
ngmix_prepsf_shear_fixnoise_sums_*): the restatement of
helpers/prepsf_shear_reference.py with the term of the noise plane added, in
np.longdouble, or in float64 with dtype=np.float64.  A literal np.rot90 of the
plane, explicit phase matrices, no recurrence.

Besides the image term of that file, for the un-turned noise plane N of a
stamp of side n, centre (r0, c0), and every kept mode k = (k_r, k_c):

  1. q = (-k_c, k_r);
  2. q' = q + J^T (A - 1) J^-T q;
  3. N'^(q') = sum edge[i] edge[j] N'[i, j] exp(-i (q'_r (i - r0) + q'_c (j - c0))),
     N' = rot90(N); P^(q') about the psf's own centre, with the floor;
  4. F^(k) = N'^(q') / P^(q') exp(-i (q_r (r0 + c0 - (n - 1)) + q_c (c0 - r0)));
  5. the four sums gain D^-2 sum_k w fk Re F^(k); the covariance sums are
     D^-4 sum_k fk_a fk_b w pnoise (1 / |P^(k')|^2 + 1 / |P^(q')|^2);
  6. a kept mode with |q'| or |k'| at or beyond pi in a component, or a sum
     that is not finite: all fourteen NaN, flag 1.

Measured with this file (tests/test_prepsf_shear_noise_host.py prints the
figures): F64_VS_LONGDOUBLE below.
"""
import numpy as np

from ngmix_amd import prepsfmom
from . import prepsf_shear_reference as ps
from .prepsf_shear_reference import (  # noqa: F401  (what the tests take from here)
    AP_RADS, DERIV, KINDS, STEP, TYPES, _dtft, call_host as call_host_plain, case, gap,
    gaussian_stamp, host_fexp, plan_of, type_shears)

# the largest deviation of the float64 restatement from the longdouble one over
# SHAPES x ap_rad (1.5, 0) x kind (pgauss, ksigma), five types at step 0.01 and
# the per-stamp shears, relative to each sum's scale (the largest |term| of that
# sum, image and noise terms together).  Measured: 1.127e-13, at dim 11 / pdim
# 17 under pgauss in a covariance sum: all its terms are positive, the sum is
# about a thousand times its largest term, and half a unit in the last place
# of the float64 result is that many times 1.1e-16 (3.2e-14 at most on the
# other three shapes).  test_float64_against_longdouble prints every figure
# and asserts that it stays at or below this.  The host twin and the kernel are
# allowed four times this (TWIN_TOL) for their summation order and the phase
# recurrence; measured: host twin 1.127e-13, at the same place (6.3e-14 at most
# on the other shapes; DESIGN.md 3.22 has the kernel's figure).
F64_VS_LONGDOUBLE = 1.15e-13
TWIN_TOL = 4 * F64_VS_LONGDOUBLE

# (dim, pdim, number of stamps): those of the image term, and a psf stamp
# larger than the plane
SHAPES = ((16, 16, 70), (17, 11, 3), (11, 17, 2), (32, 32, 1))


def measure_of(kind, dim, ap_rad, fwhm=None):
    """the measurement of a case: prepsf_shear_reference's weight of 0.4 of the
    stamp's width, whose modes end near 5 / sigma and stay inside the band
    under |g| = 0.3 -- for both k' and q', a factor of 1.36 at most -- down to a
    stamp of 14 pixels (5 / (0.4 x 14 / 2.355) x 1.36 = 2.86 < pi); a smaller
    stamp (dim 11: 3.64) takes the weight of a 14 pixel one, so that its |g| =
    0.3 stamp is measured and not flagged"""
    return ps.measure_of(kind, dim, ap_rad, fwhm=ps.fwhm_of(max(dim, 14)) if fwhm is None else fwhm)


def noise_planes(dim, pdim, n, seed=11):
    """the UN-turned noise planes of case(dim, pdim, n): seeded normals over
    the square root of the weight, +0.0 where the weight is not positive"""
    w = case(dim, pdim, n)["weights"]
    rng = np.random.RandomState(seed + 100 * dim + pdim + n)
    z = rng.normal(size=w.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(w > 0, z / np.sqrt(np.where(w > 0, w, 1.0)), 0.0)


def turned(noise):
    """(N, n, n) planes as the entries take them"""
    return np.ascontiguousarray(np.rot90(noise, 1, axes=(1, 2)))


def _floored(tp, psf, dtype):
    min_amp = dtype(1e-5) * np.abs(psf.sum())
    amp = np.abs(tp)
    low = amp <= min_amp
    tp = np.where(low & (amp != 0), tp / np.where(amp == 0, 1, amp) * min_amp, tp)
    return np.where(low & (amp == 0), min_amp + 0j, tp)


def _sheared(k, deriv, g, dtype):
    jm = np.array([[deriv[0], deriv[1]], [deriv[2], deriv[3]]], dtype=dtype)
    det = jm[0, 0] * jm[1, 1] - jm[0, 1] * jm[1, 0]
    jit = (np.array([[jm[1, 1], -jm[0, 1]], [-jm[1, 0], jm[0, 0]]], dtype=dtype) / det).T
    g1, g2 = dtype(g[0]), dtype(g[1])
    root = np.sqrt(dtype(1) - g1 * g1 - g2 * g2)
    d = np.array([[(dtype(1) - g1) / root - dtype(1), g2 / root],
                  [g2 / root, (dtype(1) + g1) / root - dtype(1)]], dtype=dtype)
    return k + jm.T @ (d @ (jit @ k))


def fixnoise_sums(image, weight, noise, cen, deriv, psf, psf_cen, g, rows, cols, wgt, fk, D,
                  ap_rad, dtype=np.longdouble):
    """steps 1-6 for one stamp, its UN-turned noise plane and one shear;
    returns (sums (14,), flag, scale (14,): the largest |term| of every sum over
    the image and the noise terms together, image part (4,): the image term of
    the four moment sums alone)"""
    dim = image.shape[0]
    pi = dtype(np.pi)
    image, psf = np.asarray(image, dtype=dtype), np.asarray(psf, dtype=dtype)
    noise = np.asarray(noise, dtype=dtype)
    if ap_rad > 0:
        edge = prepsfmom._apodization_edge(dim, ap_rad).astype(dtype)
        image = image * np.outer(edge, edge)
        noise = noise * np.outer(edge, edge)
    nturned = np.rot90(noise, 1)
    cen, psf_cen = np.asarray(cen, dtype=dtype), np.asarray(psf_cen, dtype=dtype)
    f = (np.fft.fftfreq(D) * (2.0 * np.pi)).astype(dtype)
    k = np.stack([f[rows], f[cols]])
    q = np.stack([-k[1], k[0]])
    ks, qs = _sheared(k, deriv, g, dtype), _sheared(q, deriv, g, dtype)
    out_of_band = bool(np.any(~((np.abs(ks) < pi) & (np.abs(qs) < pi))))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ti = _dtft(image, cen, ks[0], ks[1])
        tp = _floored(_dtft(psf, psf_cen, ks[0], ks[1]), psf, dtype)
        tn = _dtft(nturned, cen, qs[0], qs[1])
        tq = _floored(_dtft(psf, psf_cen, qs[0], qs[1]), psf, dtype)
        back = np.exp(-1j * (q[0] * (cen[0] + cen[1] - dtype(dim - 1)) + q[1] * (cen[1] - cen[0])))
        ri, rn = ti / tp, tn / tq * back
        w = np.asarray(weight, dtype=dtype)
        pnoise = np.sum(1 / w[w > 0]) * (dtype(D) / dtype(dim)) ** 2
        wg, fk = wgt.astype(dtype), fk.astype(dtype)
        cp = wg * pnoise / (tp.real ** 2 + tp.imag ** 2)
        cq = wg * pnoise / (tq.real ** 2 + tq.imag ** 2)
        terms = [(ri.real * wg * fk[a], rn.real * wg * fk[a]) for a in range(4)]
        for a in range(4):
            for b in range(a, 4):
                terms.append((fk[a] * fk[b] * cp, fk[a] * fk[b] * cq))
        df2 = (dtype(1) / dtype(D)) ** 2
        norm = np.array([df2] * 4 + [df2 * df2] * 10, dtype=dtype)
        sums = np.array([s.sum() + t.sum() for s, t in terms], dtype=dtype) * norm
        scale = np.array([max(np.abs(s).max(), np.abs(t).max()) for s, t in terms],
                         dtype=dtype) * norm
        image_part = np.array([s.sum() for s, _ in terms[:4]], dtype=dtype) * norm[:4]
    if out_of_band or not np.all(np.isfinite(sums.astype(np.float64))):
        return np.full(14, np.nan, dtype=dtype), 1, scale, image_part
    return sums, 0, scale, image_part


_CACHE = {}


def reference(dim, pdim, n, kind, ap_rad, dtype=np.longdouble, rows_of=None):
    """
    The reference sums of case(dim, pdim, n) with noise_planes(dim, pdim, n)
    under measure_of(kind, dim, ap_rad), computed once per process and not
    changed afterwards: 'types' (n, 5, 14) with its flags and scales,
    'galshear' (n, 1, 14) likewise (the per-stamp shears).  rows_of: only these
    stamps (the others NaN).
    """
    key = (dim, pdim, n, kind, ap_rad, np.dtype(dtype).name, rows_of)
    if key in _CACHE:
        return _CACHE[key]
    c, noise = case(dim, pdim, n), noise_planes(dim, pdim, n)
    _, D, rows, cols, wgt, fk = plan_of(measure_of(kind, dim, ap_rad), dim, pdim)
    out = {}
    for name, shears in (("types", None), ("galshear", c["shears"])):
        nt = 5 if shears is None else 1
        sums = np.full((n, nt, 14), np.nan, dtype=dtype)
        scale = np.full((n, nt, 14), np.nan, dtype=dtype)
        flags = np.zeros((n, nt), dtype=np.int32)
        for i in (range(n) if rows_of is None else rows_of):
            for t in range(nt):
                g = type_shears()[t] if shears is None else shears[i]
                sums[i, t], flags[i, t], scale[i, t], _ = fixnoise_sums(
                    c["images"][i], c["weights"][i], noise[i], c["cen"][i], DERIV, c["psfs"][i],
                    c["pcen"][i], g, rows, cols, wgt, fk, D, ap_rad, dtype)
        for a in (sums, scale, flags):
            a.setflags(write=False)
        out[name] = dict(sums=sums, scale=scale, flags=flags)
    _CACHE[key] = out
    return out


def call_host(L, ptr, c, nturned, g, rows, cols, kwgt, kfk, D, ap_rad, deriv=DERIV, host=True,
              **over):
    """ngmix_prepsf_shear_fixnoise_sums_host (host=False: _batch with a null
    stream, for the refusals) on a case's arrays and its TURNED noise planes
    nturned (ps.call_entry)."""
    return ps.call_entry(L, ptr, c, g, rows, cols, kwgt, kfk, D, ap_rad, deriv, host,
                         fixnoise=True, nturned=nturned, **over)


# ---------------------------------------------------------------------------
# the turning identity: under a conformal jacobian, a psf stamp symmetric under
# rot90 and the centre at the stamp's own, the noise term of a plane N at shear
# g is the image term of N, taken as the image, at shear -g

def conformal_deriv(s=0.27, theta=0.4):
    """s (cos, sin, sin, -cos): J J^T = s^2, with a flip (det < 0)"""
    return (s * np.cos(theta), s * np.sin(theta), s * np.sin(theta), -s * np.cos(theta))


def turning_case(dim, pdim, n, seed=5):
    """n stamps whose image IS the noise plane N, a round gaussian psf about the
    centre of its stamp (symmetric under rot90 to the bit: built from its
    upper-left quadrant's distances), both centres at the stamps' own"""
    deriv = conformal_deriv()
    rng = np.random.RandomState(seed + dim)
    planes = rng.normal(scale=0.25, size=(n, dim, dim))
    d2 = (np.arange(pdim) - (pdim - 1) / 2.0) ** 2
    psf = np.exp(-0.5 * (d2[:, None] + d2[None, :]) / (0.08 * pdim) ** 2)
    assert np.array_equal(psf, np.rot90(psf))
    c = dict(images=planes, psfs=np.tile(psf / psf.sum(), (n, 1, 1)),
             weights=np.full((n, dim, dim), 16.0), cen=np.full((n, 2), (dim - 1) / 2.0),
             pcen=np.full((n, 2), (pdim - 1) / 2.0))
    return c, planes, deriv
