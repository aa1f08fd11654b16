"""
A dense reference of the metacalibration operation of ngmix_amd.metacal
("metacalibration images"): the object deconvolved from its psf,
sheared and reconvolved with a round gaussian, as sums over explicit phase
matrices -- no FFT, no recurrence -- in float64 or np.longdouble.

For one stamp I (R x C) with jacobian centre (r0, c0) and derivative matrix
J = [[dvdrow, dvdcol], [dudrow, dudcol]], its psf stamp P (Rp x Cp, own centre,
same J), a shear (g1, g2) and a target width sigma_T:

  1. output modes q = 2 pi (fftfreq(R)[a], fftfreq(C)[b]), every (a, b)
  2. source frequency q' = J^T A J^-T q, A = [[1-g1, g2], [g2, 1+g1]] / sqrt(1-g^2)
     in (v, u) order (written q + J^T (A - 1) J^-T q: exactly q at g = 0)
  3. the transforms about the centres,
     I^(q') = sum I[r, c] exp(-i (q'_r (r - r0) + q'_c (c - c0))), P^ likewise
  4. a mode is kept only if |q'_r| < pi and |q'_c| < pi, strictly
  5. T^(q) = sum(P) exp(-(sigma_T (1 + 2|g|))^2 |J^-T q|^2 / 2)
  6. O^ = I^ / P^ T^ on kept modes, 0 elsewhere; the image is the real part of
     the inverse DFT of O^ exp(-i (q_r r0 + q_c c0))
  7. the target psf image is that gaussian point-sampled on the psf stamp's
     grid about ((Rp-1)/2, (Cp-1)/2)
  8. noshear is g = 0

Measured with this file (tests/test_metacal_reference_host.py prints them):

  * against the analytic sheared and reconvolved gaussian (the eight cases of
    test_reference_reproduces_analytic_gaussians), float64: at most 8.2e-9 of
    the peak (bound of the test: 5e-8);
  * float64 against longdouble over analytic_cases() and the stamps of
    DEVICE_SHAPES, all five types and the per-stamp shears: 1.08e-13 of each
    stamp's peak at most (F64_VS_LONGDOUBLE below).
"""
import numpy as np

TYPES = ("noshear", "1p", "1m", "2p", "2m")

# the largest deviation of the float64 reference from the longdouble one,
# relative to each output stamp's peak, over analytic_cases() and
# DEVICE_SHAPES (images, fixnoise images and target psf images).  Measured:
# 1.08e-13 (test_float64_against_longdouble prints the figure and asserts that
# it stays at or below this); the device tests allow four times this for the
# order of their sums.
F64_VS_LONGDOUBLE = 1.1e-13


def shear_of_type(name, step):
    return {"noshear": (0.0, 0.0), "1p": (step, 0.0), "1m": (-step, 0.0),
            "2p": (0.0, step), "2m": (0.0, -step)}[name]


def _pi(dtype):
    return dtype(4) * np.arctan(dtype(1))


def grid_freqs(n, dtype):
    """2 pi fftfreq(n) in dtype; the Nyquist entry of an even n is exactly -pi"""
    k = np.arange(n)
    k = np.where(k < (n + 1) // 2, k, k - n)
    return (dtype(2) * _pi(dtype)) * (k.astype(dtype) / dtype(n))


def _jmat(jac, dtype):
    """J of a jacobian record (row0, col0, dvdrow, dvdcol, dudrow, dudcol, ...)"""
    jac = np.asarray(jac, dtype=dtype)
    return np.array([[jac[2], jac[3]], [jac[4], jac[5]]], dtype=dtype)


def _inv2(m):
    det = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    return np.array([[m[1, 1], -m[0, 1]], [-m[1, 0], m[0, 0]]], dtype=m.dtype) / det


def _transform(img, cen, qr, qc):
    """sum img[r, c] exp(-i (qr (r - r0) + qc (c - c0))) at every listed mode:
    one phase matrix per axis, (modes, rows) and (modes, columns)"""
    dtype = qr.dtype
    rows = np.arange(img.shape[0]).astype(dtype) - cen[0]
    cols = np.arange(img.shape[1]).astype(dtype) - cen[1]
    er = np.exp(-1j * np.outer(qr, rows))
    ec = np.exp(-1j * np.outer(qc, cols))
    return np.einsum("mr,rc,mc->m", er, img, ec)


def spectrum(image, psf, jac, psf_cen, g, sigma_t, dtype=np.float64):
    """steps 1-6 up to O^(q) exp(-i q . centre) on the full R x C plane of modes;
    returns (spectrum (R, C) complex, kept (R, C) bool)"""
    image = np.asarray(image, dtype=dtype)
    psf = np.asarray(psf, dtype=dtype)
    nr, nc = image.shape
    jac = np.asarray(jac, dtype=dtype)
    cen = jac[0:2]
    pcen = np.asarray(psf_cen, dtype=dtype)
    jm = _jmat(jac, dtype)
    jit = _inv2(jm).T
    g1, g2 = dtype(g[0]), dtype(g[1])
    root = np.sqrt(dtype(1) - g1 * g1 - g2 * g2)
    # A - 1: exactly zero at g = 0
    d = np.array([[(dtype(1) - g1) / root - dtype(1), g2 / root],
                  [g2 / root, (dtype(1) + g1) / root - dtype(1)]], dtype=dtype)
    qa, qb = np.meshgrid(grid_freqs(nr, dtype), grid_freqs(nc, dtype), indexing="ij")
    q = np.stack([qa.ravel(), qb.ravel()])                  # (2, modes)
    kw = jit @ q                                            # world frequencies (v, u)
    qs = q + jm.T @ (d @ kw)
    pi = _pi(dtype)
    kept = (np.abs(qs[0]) < pi) & (np.abs(qs[1]) < pi)
    ti = _transform(image, cen, qs[0], qs[1])
    tp = _transform(psf, pcen, qs[0], qs[1])
    gabs = np.sqrt(g1 * g1 + g2 * g2)
    sig = dtype(sigma_t) * (dtype(1) + dtype(2) * gabs)
    tt = psf.sum() * np.exp(-(sig * sig) * (kw[0] ** 2 + kw[1] ** 2) / dtype(2))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(kept, ti / tp * tt, 0)
    out = out * np.exp(-1j * (q[0] * cen[0] + q[1] * cen[1]))
    return out.reshape(nr, nc), kept.reshape(nr, nc)


def metacal_image(image, psf, jac, psf_cen, g, sigma_t, dtype=np.float64):
    """steps 1-6: the sheared, reconvolved image (R, C) and its flag (1 when a
    kept mode is not finite: the image is NaN then)"""
    spec, kept = spectrum(image, psf, jac, psf_cen, g, sigma_t, dtype)
    nr, nc = spec.shape
    if not np.all(np.isfinite(spec[kept])):
        return np.full((nr, nc), np.nan, dtype=dtype), 1
    er = np.exp(1j * np.outer(np.arange(nr).astype(dtype), grid_freqs(nr, dtype)))
    ec = np.exp(1j * np.outer(np.arange(nc).astype(dtype), grid_freqs(nc, dtype)))
    out = np.einsum("ra,ab,cb->rc", er, spec, ec).real / dtype(nr * nc)
    return out, 0


def target_psf_image(shape, jac, flux, g, sigma_t, dtype=np.float64):
    """step 7: flux |det J| / (2 pi s^2) exp(-(v^2 + u^2) / (2 s^2)), s = sigma_T
    (1 + 2|g|), at the pixels of a stamp of `shape` about its exact centre"""
    jm = _jmat(jac, dtype)
    g1, g2 = dtype(g[0]), dtype(g[1])
    sig = dtype(sigma_t) * (dtype(1) + dtype(2) * np.sqrt(g1 * g1 + g2 * g2))
    r = np.arange(shape[0]).astype(dtype) - dtype(shape[0] - 1) / dtype(2)
    c = np.arange(shape[1]).astype(dtype) - dtype(shape[1] - 1) / dtype(2)
    rr, cc = np.meshgrid(r, c, indexing="ij")
    v = jm[0, 0] * rr + jm[0, 1] * cc
    u = jm[1, 0] * rr + jm[1, 1] * cc
    det = np.abs(jm[0, 0] * jm[1, 1] - jm[0, 1] * jm[1, 0])
    norm = dtype(flux) * det / (dtype(2) * _pi(dtype) * sig * sig)
    return norm * np.exp(-(v * v + u * u) / (dtype(2) * sig * sig))


def fixnoise_weight(weight):
    """1 / (1/w + 1/w) where w > 0, 0 elsewhere"""
    weight = np.asarray(weight)
    out = np.zeros_like(weight)
    pos = weight > 0
    out[pos] = 1.0 / (1.0 / weight[pos] + 1.0 / weight[pos])
    return out


def metacal_fixnoise_image(image, noise, psf, jac, psf_cen, g, sigma_t, dtype=np.float64):
    """the image plus its noise stamp turned by rot90(k=1), put through the
    same operation and turned back by k=3 (square stamps)"""
    if image.shape[0] != image.shape[1]:
        raise ValueError("fixnoise needs square stamps")
    out, flag = metacal_image(image, psf, jac, psf_cen, g, sigma_t, dtype)
    nout, nflag = metacal_image(np.rot90(np.asarray(noise), k=1), psf, jac, psf_cen, g,
                                sigma_t, dtype)
    return out + np.rot90(nout, k=3), flag | nflag


def fitgauss_sigma(irr, irc, icc):
    """the target width of psf='fitgauss' from the adaptive-moments gaussian of
    the psf: T dilated by the largest eigenvalue of its covariance, at most 1.1"""
    T = irr + icc
    eig = 0.5 * T + np.sqrt((0.5 * (icc - irr)) ** 2 + irc ** 2)
    dilation = np.minimum(1.0 + 2.0 * (np.sqrt(eig / (T / 2.0)) - 1.0), 1.1)
    return np.sqrt(T * dilation / 2.0)


# ---------------------------------------------------------------------------
# inputs

def gaussian_stamp(shape, jac, cov, flux, dtype=np.float64):
    """a point-sampled gaussian of world covariance cov ((v, u) order)"""
    jac = np.asarray(jac, dtype=dtype)
    jm = _jmat(jac, dtype)
    cov = np.asarray(cov, dtype=dtype)
    rr, cc = np.meshgrid(np.arange(shape[0]).astype(dtype) - jac[0],
                         np.arange(shape[1]).astype(dtype) - jac[1], indexing="ij")
    v = jm[0, 0] * rr + jm[0, 1] * cc
    u = jm[1, 0] * rr + jm[1, 1] * cc
    det = cov[0, 0] * cov[1, 1] - cov[0, 1] * cov[1, 0]
    chi2 = (cov[1, 1] * v * v - dtype(2) * cov[0, 1] * v * u + cov[0, 0] * u * u) / det
    area = np.abs(jm[0, 0] * jm[1, 1] - jm[0, 1] * jm[1, 0])
    return dtype(flux) * area / (dtype(2) * _pi(dtype) * np.sqrt(det)) * np.exp(-chi2 / dtype(2))


def periodic_gaussian_psf(shape, jac, sigma, flux):
    """a psf stamp whose transform AT THE GRID'S OWN FREQUENCIES is the round
    gaussian's, flux exp(-sigma^2 |J^-T q|^2 / 2), about the jacobian's centre
    (the gaussian wrapped around the stamp): with it as the psf and sigma as
    the target, the unsheared operation is the identity on every kept mode"""
    jac = np.asarray(jac, dtype=np.float64)
    jit = _inv2(_jmat(jac, np.float64)).T
    qa, qb = np.meshgrid(grid_freqs(shape[0], np.float64), grid_freqs(shape[1], np.float64),
                         indexing="ij")
    kv = jit[0, 0] * qa + jit[0, 1] * qb
    ku = jit[1, 0] * qa + jit[1, 1] * qb
    f = flux * np.exp(-0.5 * sigma ** 2 * (kv ** 2 + ku ** 2)) * \
        np.exp(-1j * (qa * jac[0] + qb * jac[1]))
    return np.fft.ifft2(f).real


def drop_nyquist(image):
    """the image without the Nyquist row and column of its transform"""
    f = np.fft.fft2(image)
    if image.shape[0] % 2 == 0:
        f[image.shape[0] // 2, :] = 0
    if image.shape[1] % 2 == 0:
        f[:, image.shape[1] // 2] = 0
    return np.fft.ifft2(f).real


def jac_record(row0, col0, dvdrow, dvdcol, dudrow, dudcol):
    det = dvdrow * dudcol - dvdcol * dudrow
    return np.array([row0, col0, dvdrow, dvdcol, dudrow, dudcol, det, np.sqrt(abs(det))])


ANALYTIC_OBJ_COV = np.array([[0.20, 0.03], [0.03, 0.12]])
ANALYTIC_PSF_SIGMA = 0.35
ANALYTIC_TARGET_SIGMA = 0.40
ANALYTIC_FLUX = 100.0
ANALYTIC_SHEARS = ((0.0, 0.0), (0.01, 0.0), (0.0, -0.01), (0.05, 0.03))
ANALYTIC_JACOBIANS = ((0.263, 0.0, 0.0, 0.263), (0.02, 0.27, -0.25, 0.05))


def shear_matrix(g, dtype=np.float64):
    g1, g2 = dtype(g[0]), dtype(g[1])
    return np.array([[dtype(1) - g1, g2], [g2, dtype(1) + g1]], dtype=dtype) / \
        np.sqrt(dtype(1) - g1 * g1 - g2 * g2)


def analytic_cases():
    """the stamps of the analytic check: (image, psf, jac record, psf centre)
    per jacobian, 32 x 32"""
    out = []
    eye = np.eye(2)
    for deriv in ANALYTIC_JACOBIANS:
        jac = jac_record(15.3, 16.2, *deriv)
        pjac = jac_record(15.5, 15.5, *deriv)
        image = gaussian_stamp((32, 32), jac, ANALYTIC_OBJ_COV + ANALYTIC_PSF_SIGMA ** 2 * eye,
                               ANALYTIC_FLUX)
        psf = gaussian_stamp((32, 32), pjac, ANALYTIC_PSF_SIGMA ** 2 * eye, 1.0)
        out.append((image, psf, jac, pjac[0:2]))
    return out


def analytic_expected(jac, g):
    """the object sheared and convolved with the dilated target gaussian"""
    a = shear_matrix(g)
    sig = ANALYTIC_TARGET_SIGMA * (1.0 + 2.0 * np.hypot(g[0], g[1]))
    return gaussian_stamp((32, 32), jac, a @ ANALYTIC_OBJ_COV @ a.T + sig ** 2 * np.eye(2),
                          ANALYTIC_FLUX)


_DERIVS = (
    (0.263, 0.0, 0.0, 0.263),          # diagonal
    (0.02, 0.27, -0.25, 0.05),         # rotated, sheared
    (-0.26, 0.01, 0.02, 0.27),         # flipped
    (0.19, -0.18, 0.18, 0.2),          # rotated by about 45 degrees
)

# (shape, psf shape, number of stamps) of the device tests
DEVICE_SHAPES = (((16, 16), (16, 16), 70), ((12, 17), (11, 11), 3), ((32, 32), (32, 32), 1),
                 ((32, 32), (25, 25), 3))


def device_case(shape, psf_shape, n, seed=11):
    """
    n stamps of one shape for the device tests, each with its own jacobian
    (the four of _DERIVS in turn, scaled by a few per cent), off-pixel
    centres, a gaussian object of its own covariance seen through a slightly
    elliptical gaussian psf, a little noise on the image, a noise plane, a
    target width 8 to 15 per cent above the psf's and a per-stamp shear of up
    to |g| = 0.3.  Pixel scales follow the stamp: small stamps have coarse
    pixels so that object and psf stay inside.
    """
    rng = np.random.RandomState(seed + 1000 * shape[0] + shape[1] + n)
    nr, nc = shape
    zoom = 32.0 / min(nr, nc)
    images = np.zeros((n, nr, nc))
    psfs = np.zeros((n,) + tuple(psf_shape))
    noise = np.zeros((n, nr, nc))
    jacs = np.zeros((n, 8))
    pjacs = np.zeros((n, 8))
    sigma = np.zeros(n)
    shears = np.zeros((n, 2))
    for i in range(n):
        deriv = np.array(_DERIVS[i % len(_DERIVS)]) * zoom * rng.uniform(0.95, 1.05)
        jacs[i] = jac_record((nr - 1) / 2 + rng.uniform(-0.9, 0.9),
                             (nc - 1) / 2 + rng.uniform(-0.9, 0.9), *deriv)
        pjacs[i] = jac_record((psf_shape[0] - 1) / 2 + rng.uniform(-0.5, 0.5),
                              (psf_shape[1] - 1) / 2 + rng.uniform(-0.5, 0.5), *deriv)
        # (a psf of at most a fifth of its stamp's half width: its transform
        # has no zero inside the band)
        s_pix = min(1.33, (min(psf_shape) - 1) / 10.0)
        s = zoom * 0.263 * s_pix * rng.uniform(0.95, 1.1)
        e = rng.uniform(-0.03, 0.03, size=2) * s * s
        pcov = np.array([[s * s + e[0], e[1]], [e[1], s * s - e[0]]])
        a = zoom ** 2 * rng.uniform(0.08, 0.2, size=2)
        b = zoom ** 2 * rng.uniform(-0.03, 0.03)
        ocov = np.array([[a[0], b], [b, a[1]]])
        flux = rng.uniform(50.0, 200.0)
        images[i] = gaussian_stamp(shape, jacs[i], ocov + pcov, flux)
        images[i] += rng.normal(scale=1e-3 * images[i].max(), size=shape)
        psfs[i] = gaussian_stamp(psf_shape, pjacs[i], pcov, rng.uniform(0.9, 1.1))
        noise[i] = rng.normal(scale=1e-3 * images[i].max(), size=shape)
        sigma[i] = s * rng.uniform(1.08, 1.15)
        gabs, ang = rng.uniform(0.0, 0.3), rng.uniform(0, 2 * np.pi)
        shears[i] = gabs * np.cos(ang), gabs * np.sin(ang)
    if n > 1:
        shears[1] = 0.3 * np.cos(0.7), 0.3 * np.sin(0.7)
    weights = np.full((n, nr, nc), 1.0e4)
    return dict(images=images, psfs=psfs, noise=noise, weights=weights, jacs=jacs,
                pjacs=pjacs, sigma=sigma, shears=shears)


_REFERENCE_CACHE = {}


def device_reference(shape, psf_shape, n, step=0.01, dtype=np.longdouble):
    """the reference outputs of device_case(...), computed once per process and
    not changed afterwards: per type the images (n, R, C), the target psf
    images, the images with fixnoise (square stamps), and for the per-stamp
    shears 'galshear'"""
    key = (tuple(shape), tuple(psf_shape), n, step, np.dtype(dtype).name)
    if key in _REFERENCE_CACHE:
        return _REFERENCE_CACHE[key]
    case = device_case(shape, psf_shape, n)
    square = shape[0] == shape[1]
    out = {}
    for name in TYPES + ("galshear",):
        ims, pims, fims = [], [], []
        for i in range(n):
            g = case["shears"][i] if name == "galshear" else shear_of_type(name, step)
            args = (case["psfs"][i], case["jacs"][i], case["pjacs"][i][0:2], g, case["sigma"][i])
            ims.append(metacal_image(case["images"][i], *args, dtype=dtype)[0])
            pims.append(target_psf_image(psf_shape, case["jacs"][i], case["psfs"][i].sum(), g,
                                         case["sigma"][i], dtype=dtype))
            if square and name != "galshear":
                fims.append(metacal_fixnoise_image(case["images"][i], case["noise"][i], *args,
                                                   dtype=dtype)[0])
        out[name] = dict(images=np.stack(ims), psf_images=np.stack(pims),
                         fixnoise_images=np.stack(fims) if fims else None)
        for v in out[name].values():
            if v is not None:
                v.setflags(write=False)
    _REFERENCE_CACHE[key] = out
    return out


def cabi_refusals(L, bad_arg):
    """ngmix_metacal_spectrum_batch refuses bad calls before anything runs (no
    pointer below is ever read but g_host): returns the list of failed checks"""
    import ctypes
    g = np.array([[0.01, 0.0], [0.0, 0.3]])
    gp = ctypes.c_void_p(g.ctypes.data)
    p = ctypes.c_void_p(4096)       # stands for a device pointer; never read

    def call(**kw):
        a = dict(images=p, noise=None, psf=p, jac=p, psf_cen=p, psf_flux=p, sigma=p, g=p,
                 g_host=gp, per_stamp_g=0, n=2, ntypes=2, nrow=16, ncol=16, prow=11, pcol=11,
                 spec=p, flags=p)
        a.update(kw)
        return L.ngmix_metacal_spectrum_batch(
            a["images"], a["noise"], a["psf"], a["jac"], a["psf_cen"], a["psf_flux"], a["sigma"],
            a["g"], a["g_host"], a["per_stamp_g"], a["n"], a["ntypes"], a["nrow"], a["ncol"],
            a["prow"], a["pcol"], a["spec"], a["flags"], None)
    failed = []
    for name in ("images", "psf", "jac", "psf_cen", "psf_flux", "sigma", "g", "g_host", "spec",
                 "flags"):
        if call(**{name: None}) != bad_arg:
            failed.append("null " + name)
    for name in ("ntypes", "nrow", "ncol", "prow", "pcol"):
        for v in (0, -3):
            if call(**{name: v}) != bad_arg:
                failed.append("%s = %d" % (name, v))
    for gbad in ([[0.01, 0.0], [1.0, 0.0]], [[0.8, 0.7], [0.0, 0.0]], [[np.nan, 0.0], [0.0, 0.0]]):
        gb = np.array(gbad)
        if call(g_host=ctypes.c_void_p(gb.ctypes.data)) != bad_arg:
            failed.append("g = %s" % (gbad,))
    if call(nrow=200, ncol=200) != bad_arg:
        failed.append("a stamp beyond the LDS")
    # no stamps: nothing to do, whatever else is passed
    for n in (0, -1):
        if call(n=n, images=None, spec=None) != 0:
            failed.append("n = %d is not a no-op" % n)
    return failed
