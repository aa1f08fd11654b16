"""
Dense longdouble reference of the metacal shear from Fourier-space fits
(DESIGN.md 3.26), written from the definition:

  weighted_sums    the sums of kfit_reference.stamp_sums with omega u in place
                   of the Parseval weight omega, and the count of components
                   with omega u > 0
  kspectra         D^ = I^(q') / P^(q') T^(q) about the jacobian centre, P^n =
                   T^(q) / sum P, the keep mask and rho^2 = |T^|^2 / |P^(q')|^2
                   on the rfft2 half plane, for the round gaussian target and
                   for the dilated psf
  mode_weights     the common mask of an object's types and the noise weight
  closure_case     noise-free sampled gaussians whose metacal fits have a
                   closed form: g = g0 (+) shear
"""
import functools

import numpy as np

from helpers import kfit_cases as KC
from helpers import kfit_reference as K
from helpers import metacal_reference as M

LD = np.longdouble
# The rounding bound of a weighted sum, in kfit_cases.py's unit 2^-52 sum
# |terms|: its count of 96 (93 counted) and one more rounding per term, half a
# unit, for the product omega u
C_ROUND_W = KC.C_ROUND + 1.0
RHO2_FLOOR = 1.0e-24


# ---- weighted sums -----------------------------------------------------------------

def random_weights(shape, seed, zero_fraction=0.3):
    """u (R, C//2+1) drawn from {0, uniform in (0, 1]}"""
    rng = np.random.RandomState(seed)
    R, C = shape
    u = 1.0 - rng.uniform(size=(R, C // 2 + 1))             # (0, 1]
    u[rng.uniform(size=u.shape) < zero_fraction] = 0.0
    return u


def weighted_sums(st, u, p=None):
    """kfit_cases.reference(st) with the weight omega u: the reference walks
    the modes whose multiplicity is positive, so the multiplicity carries u"""
    md = dict(st["md"])
    md["mult"] = md["mult"] * np.asarray(u, dtype=LD)
    return KC.reference(dict(st, md=md), p)


def components(st, u):
    """the residual components with omega u > 0: a stored mode off the Nyquist
    row and column stands for one (column 0) or two of them"""
    w = (LD(st["wbar"]) / (st["md"]["R"] * st["md"]["C"])) * st["md"]["mult"] * np.asarray(u, LD)
    return int(np.sum(st["md"]["mult"][w > 0]))


# ---- spectra -----------------------------------------------------------------------

def _sinc(x):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(x == 0, x.dtype.type(1), np.sin(x) / x)


def _pixel_ft(qr, qc):
    two = qr.dtype.type(2)
    return _sinc(qr / two) * _sinc(qc / two)


def kspectra(image, psf, jac, psf_cen, g, sigma_t=None, dil=None, shear_psf=False, dtype=LD):
    """
    dhat, phat (R, C//2+1) complex, keep (bool) and rho2 of one stamp and one
    shear.  sigma_t: the round gaussian target of width sigma_t (1 + 2|g|)
    carrying the psf's flux; else dil: the psf stamp's own transform,
    deconvolved from the pixel, dilated by dil and reconvolved, the psf
    sheared instead of the image with shear_psf.  A mode is kept where the
    frequencies the image and the psf are read at lie strictly inside the band;
    a dropped mode and the Nyquist row and column are zeros.
    """
    image = np.asarray(image, dtype=dtype)
    psf = np.asarray(psf, dtype=dtype)
    nr, nc = image.shape
    ch = nc // 2 + 1
    jac = np.asarray(jac, dtype=dtype)
    cen, pcen = jac[0:2], np.asarray(psf_cen, dtype=dtype)
    jm = M._jmat(jac, dtype)
    jit = M._inv2(jm).T
    g1, g2 = dtype(g[0]), dtype(g[1])
    root = np.sqrt(dtype(1) - g1 * g1 - g2 * g2)
    d = np.array([[(dtype(1) - g1) / root - dtype(1), g2 / root],
                  [g2 / root, (dtype(1) + g1) / root - dtype(1)]], dtype=dtype)
    qa, qb = np.meshgrid(M.grid_freqs(nr, dtype), M.grid_freqs(nc, dtype)[:ch], indexing="ij")
    if nc % 2 == 0:
        qb = np.abs(qb)                 # (the Nyquist column is dropped below either way)
    q = np.stack([qa.ravel(), qb.ravel()])
    kw = jit @ q
    qs = q + jm.T @ (d @ kw)
    pi = M._pi(dtype)
    inside = lambda f: (np.abs(f[0]) < pi) & (np.abs(f[1]) < pi)
    if sigma_t is not None:
        qim = qs
        keep = inside(qim)
        gabs = np.sqrt(g1 * g1 + g2 * g2)
        sig = dtype(sigma_t) * (dtype(1) + dtype(2) * gabs)
        tt = psf.sum() * np.exp(-(sig * sig) * (kw[0] ** 2 + kw[1] ** 2) / dtype(2)) + 0j
    else:
        qim = q if shear_psf else qs
        qt = dtype(dil) * (qs if shear_psf else q)
        keep = inside(qim) & inside(qt)
        with np.errstate(divide="ignore", invalid="ignore"):
            tt = M._transform(psf, pcen, qt[0], qt[1]) / _pixel_ft(qt[0], qt[1]) \
                * _pixel_ft(q[0], q[1])
    nyq = np.zeros(q.shape[1], dtype=bool)
    a = np.repeat(np.arange(nr), ch)
    b = np.tile(np.arange(ch), nr)
    if nr % 2 == 0:
        nyq |= 2 * a == nr
    if nc % 2 == 0:
        nyq |= 2 * b == nc
    keep = keep & ~nyq
    ti = M._transform(image, cen, qim[0], qim[1])
    tp = M._transform(psf, pcen, qim[0], qim[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        dhat = np.where(keep, ti / tp * tt, 0)
        phat = np.where(keep, tt / psf.sum(), 0)
        rho2 = np.where(keep, np.abs(tt) ** 2 / np.abs(tp) ** 2, 0)
    shape = (nr, ch)
    return dhat.reshape(shape), phat.reshape(shape), keep.reshape(shape), rho2.reshape(shape)


def mode_weights(keep, rho2, weight):
    """u (T, R, C//2+1) of ONE object from its types' keep and rho2 planes"""
    mask = np.all(keep, axis=0)
    if weight == "flat":
        return np.broadcast_to(mask, keep.shape).astype(np.float64)
    rmax = np.where(mask, rho2, 0).max(axis=(1, 2), keepdims=True)
    mask = mask & np.all(rho2 >= LD(RHO2_FLOOR) * rmax, axis=0)
    rmin = np.where(mask, rho2, np.inf).min(axis=(1, 2), keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(mask, rmin / rho2, 0).astype(np.float64)


@functools.lru_cache(maxsize=None)
def spectra_reference(shape, psf_shape, n, step=0.01, dtype_name="longdouble"):
    """kspectra of metacal_reference.device_case(shape, psf_shape, n) for the
    five types (the case's target widths) and for its per-stamp shears, built
    once and left unchanged: {name: (dhat, phat, keep, rho2)}, each (n, R, CH)"""
    dtype = np.dtype(dtype_name).type
    case = M.device_case(shape, psf_shape, n)
    out = {}
    for name in M.TYPES + ("galshear",):
        planes = []
        for i in range(n):
            g = case["shears"][i] if name == "galshear" else M.shear_of_type(name, step)
            planes.append(kspectra(case["images"][i], case["psfs"][i], case["jacs"][i],
                                   case["pjacs"][i][0:2], g, sigma_t=case["sigma"][i],
                                   dtype=dtype))
        out[name] = tuple(np.stack([p[k] for p in planes]) for k in range(4))
        for v in out[name]:
            v.setflags(write=False)
    return out


# ---- closure -----------------------------------------------------------------------

CLOSURE_SHAPE = (24, 24)
CLOSURE_SCALE = 0.263
CLOSURE_G0 = ((0.0, 0.0), (0.0, 0.0), (0.2, -0.1), (-0.15, 0.25))    # |g0| <= 0.3
CLOSURE_FLUX = (80.0, 120.0, 100.0, 150.0)


def _g_to_cov(g, T):
    g1, g2 = g
    gsq = g1 * g1 + g2 * g2
    e1, e2 = 2 * g1 / (1 + gsq), 2 * g2 / (1 + gsq)
    # (v, u) order: irr = <v v> = T/2 (1 - e1), icc = <u u> = T/2 (1 + e1)
    return np.array([[T / 2 * (1 - e1), T / 2 * e2], [T / 2 * e2, T / 2 * (1 + e1)]])


@functools.lru_cache(maxsize=None)
def closure_case():
    """
    Four noise-free point-sampled gaussians on 24 x 24 with a round gaussian
    psf, the convolved size sigma_total = 2 pixels (DESIGN.md 3.24's window
    between aliasing and wrapped tails): two round objects and two of |g0| up
    to 0.3 (their covariance at the same T).  The metacal image of type s is
    the object sheared by s through the target psf, and the k-space 'gauss'
    fit with that target recovers g = g0 (+) s.
    """
    n = len(CLOSURE_G0)
    nr, nc = CLOSURE_SHAPE
    s = CLOSURE_SCALE
    sig_psf = 1.2 * s
    T_obj = 2 * ((2.0 * s) ** 2 - sig_psf ** 2)
    images, psfs = np.zeros((n, nr, nc)), np.zeros((n, nr, nc))
    jacs, pjacs = np.zeros((n, 8)), np.zeros((n, 8))
    for i in range(n):
        jacs[i] = M.jac_record((nr - 1) / 2 + 0.1 * i, (nc - 1) / 2 - 0.07 * i, s, 0.0, 0.0, s)
        pjacs[i] = M.jac_record((nr - 1) / 2, (nc - 1) / 2, s, 0.0, 0.0, s)
        pcov = np.eye(2) * sig_psf ** 2
        images[i] = M.gaussian_stamp((nr, nc), jacs[i], _g_to_cov(CLOSURE_G0[i], T_obj) + pcov,
                                     CLOSURE_FLUX[i])
        psfs[i] = M.gaussian_stamp((nr, nc), pjacs[i], pcov, 1.0)
    out = dict(images=images, psfs=psfs, jacs=jacs, pjacs=pjacs,
               weights=np.full((n, nr, nc), 1.0e4), sigma=np.full(n, 1.1 * sig_psf),
               g0=np.array(CLOSURE_G0))
    for v in out.values():
        v.setflags(write=False)
    return out


def closure_expected(step=0.01):
    """{type: g0 (+) shear (n, 2)} by ngmix_amd.shape's addition, and the
    finite difference of that closed form R (n, 2, 2)"""
    from ngmix_amd.shape import Shape
    g0 = closure_case()["g0"]
    exp = {}
    for name in M.TYPES:
        s1, s2 = M.shear_of_type(name, step)
        rows = []
        for a, b in g0:
            sh = Shape(a, b).get_sheared(s1, s2)
            rows.append((sh.g1, sh.g2))
        exp[name] = np.array(rows)
    R = np.empty((g0.shape[0], 2, 2))
    for j in (0, 1):
        R[:, :, j] = (exp["%dp" % (j + 1)] - exp["%dm" % (j + 1)]) / (2 * step)
    return exp, R


# What the closure can hold on the host-composed path, reasoned before it was
# measured: the sampled gaussians are not band-limited and not periodic.  At
# sigma_total = 2 pixels the transform at the band edge is exp(-(2 pi)^2 / 2) =
# 3e-9 of its peak and the profile at the stamp's edge, 6 sigma out, exp(-18) =
# 2e-8; along the major axis of |g0| = 0.3 both are some ten times larger.  So
# 1e-6 in g; R is a difference of two such errors over 2 step = 0.02, fifty
# times as much, held to the 1e-4 that exact shear composition allows.
HOST_CLOSURE_G = 1.0e-6
HOST_CLOSURE_R = 1.0e-4
# Measured on that path (tests/test_kfit_metacal_host.py prints them): worst
# |g - g0 (+) s| 5.6e-9 (flat), 1.1e-8 (noise); worst |R - R0| 3.7e-8 (flat),
# 6.2e-9 (noise).  The device is held to ten times the worst of each.
DEVICE_CLOSURE_G = 10 * 1.1e-8
DEVICE_CLOSURE_R = 10 * 3.7e-8
