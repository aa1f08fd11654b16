"""
A dense reference of metacalibration with the psf's own dilated, sheared image
as the reconvolution target (ngmix_amd.metacal, psf='dilate-exact'; DESIGN.md
3.23), written from the definition: explicit phase matrices, no FFT, no
recurrence, in float64 or np.longdouble.  The inputs, the jacobian helpers and
the inverse transform's conventions are those of metacal_reference.py.

Every (stamp, type) has a shear g, a dilation d >= 1 and a kind, 'image' or
'psf'.  With q the grid frequencies, S(g) q = q + J^T (A - 1) J^-T q and
Pi(q) = sinc(q_r / 2) sinc(q_c / 2) the transform of the pixel:

  kind    image frequency q'    target frequency q_t
  image   S(g) q                d q
  psf     q                     d S(g) q

  1. a mode is kept only if |q'_r|, |q'_c|, |q_t,r|, |q_t,c| are all < pi
  2. T^(q) = P^(q_t) / Pi(q_t) Pi(q), P^ the psf stamp's transform about the
     psf's own centre
  3. O^(q) = I^(q') / P^(q') T^(q) on kept modes, 0 elsewhere; the image is the
     real part of the inverse DFT of O^(q) exp(-i q . centre)
  4. the target psf image is the real part of the inverse DFT, on the psf
     stamp's own grid q_p, of T^(q_p) exp(-i q_p . psf centre), kept where
     q_t(q_p) is inside the band
  5. fixnoise: the noise stamp turned by rot90(k=1), the same operation, turned
     back by k=3 and added

Measured with this file (tests/test_metacal_dilate_reference_host.py prints
them):

  * against the closed form for point-sampled gaussians (both kinds, four
    jacobians, five shears, modes with max(|q_r|, |q_c|) <= 2), float64: at
    most 5.02e-13 of the largest |O^| (CLOSED_FORM_MEASURED below; the aliasing
    of the sigma = 2 px psf at |q| = 2, the bound is eight times it);
  * float64 against longdouble over the device cases, all nine types and the
    per-stamp shears of both kinds, images, fixnoise images and target psf
    images: F64_VS_LONGDOUBLE below, of each stamp's peak.
"""
import numpy as np

from . import metacal_reference as M
from .metacal_reference import (  # noqa: F401  (what the tests take from here)
    device_case, drop_nyquist, fixnoise_weight, gaussian_stamp, grid_freqs, jac_record)

IMAGE, PSF = "image", "psf"
TYPES = M.TYPES + ("1p_psf", "1m_psf", "2p_psf", "2m_psf")

# the largest deviation of the float64 form from the longdouble one, relative
# to each output stamp's peak, over DEVICE_SHAPES (images, fixnoise images and
# target psf images of the nine types, 'galshear' and 'psfshear').
# test_float64_against_longdouble prints the figure and asserts that it stays
# at or below this; the device tests allow four times this for the order of
# their sums.
F64_VS_LONGDOUBLE = 6.2e-13     # measured: 6.08e-13

# the closed-form check's figure, float64, relative to the largest |O^|
CLOSED_FORM_MEASURED = 5.1e-13   # measured: 5.02e-13, at (0.2, -0.1), where d = 1.45

# (shape, psf shape, number of stamps) of the device tests
DEVICE_SHAPES = (((16, 16), (16, 16), 70), ((12, 17), (11, 11), 3), ((32, 32), (25, 25), 1),
                 ((32, 32), (25, 25), 3))


def type_spec(name, step):
    """(shear, dilation, kind) of a type of get_all: every type, noshear
    included, has the dilation 1 + 2 step"""
    kind = PSF if name.endswith("_psf") else IMAGE
    base = name[:-4] if kind == PSF else name
    return M.shear_of_type(base, step), 1.0 + 2.0 * step, kind


def shear_spec(g, kind):
    """(shear, dilation, kind) of get_obs_galshear / get_obs_psfshear: d = 1 + 2|g|"""
    return (g[0], g[1]), 1.0 + 2.0 * float(np.hypot(g[0], g[1])), kind


def _sinc(x):
    safe = np.where(x == 0, 1, x)
    return np.where(x == 0, 1, np.sin(safe) / safe)


def pixel_ft(q):
    """Pi(q) of q (2, modes): the transform of the unit-square pixel"""
    two = q.dtype.type(2)
    return _sinc(q[0] / two) * _sinc(q[1] / two)


def frequencies(shape, jac, g, dil, kind, dtype=np.float64):
    """the grid's q, the image frequency q' and the target frequency q_t, each
    (2, modes) in row-major order of the shape's modes"""
    jac = np.asarray(jac, dtype=dtype)
    jm = M._jmat(jac, dtype)
    jit = M._inv2(jm).T
    g1, g2 = dtype(g[0]), dtype(g[1])
    root = np.sqrt(dtype(1) - g1 * g1 - g2 * g2)
    a_minus_1 = np.array([[(dtype(1) - g1) / root - dtype(1), g2 / root],
                          [g2 / root, (dtype(1) + g1) / root - dtype(1)]], dtype=dtype)
    qa, qb = np.meshgrid(grid_freqs(shape[0], dtype), grid_freqs(shape[1], dtype), indexing="ij")
    q = np.stack([qa.ravel(), qb.ravel()])
    qs = q + jm.T @ (a_minus_1 @ (jit @ q))
    if kind == IMAGE:
        return q, qs, dtype(dil) * q
    if kind == PSF:
        return q, q, dtype(dil) * qs
    raise ValueError("kind is 'image' or 'psf'")


def _inside(q):
    pi = M._pi(q.dtype.type)
    return (np.abs(q[0]) < pi) & (np.abs(q[1]) < pi)


_PHASES = {}


def _phases(q, n):
    """the phase matrices exp(-i q_r r) and exp(-i q_c c), (modes, n), r, c =
    0 .. n-1, of a frequency list.  Many (stamp, type) pairs share a list (d q is
    the same for every stamp of a shape): the last few are kept"""
    key = (q.tobytes(), q.dtype.str, n)
    if key not in _PHASES:
        if len(_PHASES) >= 6:
            _PHASES.clear()
        x = np.arange(n).astype(q.dtype)
        _PHASES[key] = (np.exp(-1j * np.outer(q[0], x)), np.exp(-1j * np.outer(q[1], x)))
    return _PHASES[key]


def _transform(img, cen, q):
    """sum img[r, c] exp(-i (q_r (r - r0) + q_c (c - c0))) at every listed mode,
    as exp(i q . centre) sum img[r, c] exp(-i q_r r) exp(-i q_c c)"""
    er, ec = _phases(q, max(img.shape))
    nr, nc = img.shape
    return ((er[:, :nr] @ img) * ec[:, :nc]).sum(axis=1) * np.exp(1j * (q[0] * cen[0] + q[1] * cen[1]))


def _target(psf, pcen, q, qt):
    """T^(q) = P^(q_t) / Pi(q_t) Pi(q) (meaningful where q_t is inside the band)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return _transform(psf, pcen, qt) / pixel_ft(qt) * pixel_ft(q)


def spectra(planes, psf, jac, psf_cen, g, dil, kind, dtype=np.float64):
    """O^(q) exp(-i q . centre) of every plane of `planes` (k, R, C) -- an image
    and its turned noise stamp go through the same operation -- on the full R x
    C plane of modes; returns (spectra (k, R, C) complex, kept (R, C) bool)"""
    planes = np.asarray(planes, dtype=dtype)
    psf = np.asarray(psf, dtype=dtype)
    jac = np.asarray(jac, dtype=dtype)
    shape = planes.shape[1:]
    cen, pcen = jac[0:2], np.asarray(psf_cen, dtype=dtype)
    q, qi, qt = frequencies(shape, jac, g, dil, kind, dtype)
    kept = _inside(qi) & _inside(qt)
    with np.errstate(divide="ignore", invalid="ignore"):
        factor = _target(psf, pcen, q, qt) / _transform(psf, pcen, qi)
        out = np.stack([np.where(kept, _transform(p, cen, qi) * factor, 0) for p in planes])
    out = out * np.exp(-1j * (q[0] * cen[0] + q[1] * cen[1]))
    return out.reshape(planes.shape), kept.reshape(shape)


def spectrum(image, psf, jac, psf_cen, g, dil, kind, dtype=np.float64):
    """spectra() of one image: (spectrum (R, C) complex, kept (R, C) bool)"""
    out, kept = spectra(np.asarray(image)[None], psf, jac, psf_cen, g, dil, kind, dtype)
    return out[0], kept


def psf_spectrum(psf, jac, psf_cen, g, dil, kind, dtype=np.float64):
    """T^(q_p) exp(-i q_p . psf centre) on the psf stamp's own grid; returns
    (spectrum (Rp, Cp) complex, kept (Rp, Cp) bool): kept where q_t is inside"""
    psf = np.asarray(psf, dtype=dtype)
    pcen = np.asarray(psf_cen, dtype=dtype)
    q, _, qt = frequencies(psf.shape, jac, g, dil, kind, dtype)
    kept = _inside(qt)
    out = np.where(kept, _target(psf, pcen, q, qt), 0)
    out = out * np.exp(-1j * (q[0] * pcen[0] + q[1] * pcen[1]))
    return out.reshape(psf.shape), kept.reshape(psf.shape)


def _real_inverse(spec, kept, dtype):
    """(the real part of the inverse DFT, flag): NaN and 1 when a kept mode is
    not finite"""
    nr, nc = spec.shape
    if not np.all(np.isfinite(spec[kept])):
        return np.full((nr, nc), np.nan, dtype=dtype), 1
    er = np.exp(1j * np.outer(np.arange(nr).astype(dtype), grid_freqs(nr, dtype)))
    ec = np.exp(1j * np.outer(np.arange(nc).astype(dtype), grid_freqs(nc, dtype)))
    return ((er @ spec) @ ec.T).real / dtype(nr * nc), 0


def metacal_image(image, psf, jac, psf_cen, g, dil, kind, dtype=np.float64):
    """the metacal image (R, C) and its flag"""
    return _real_inverse(*spectrum(image, psf, jac, psf_cen, g, dil, kind, dtype), dtype)


def target_psf_image(psf, jac, psf_cen, g, dil, kind, dtype=np.float64):
    """the target psf image (Rp, Cp) about the psf stamp's own centre, and its flag"""
    return _real_inverse(*psf_spectrum(psf, jac, psf_cen, g, dil, kind, dtype), dtype)


def metacal_fixnoise_image(image, noise, psf, jac, psf_cen, g, dil, kind, dtype=np.float64):
    """the image plus its noise stamp turned by rot90(k=1), put through the same
    operation and turned back by k=3 (square stamps), and the flag"""
    out, nout, flag = _image_and_noise(image, noise, psf, jac, psf_cen, g, dil, kind, dtype)
    return out + np.rot90(nout, k=3), flag


def _image_and_noise(image, noise, psf, jac, psf_cen, g, dil, kind, dtype):
    if image.shape[0] != image.shape[1]:
        raise ValueError("fixnoise needs square stamps")
    spec, kept = spectra(np.stack([image, np.rot90(np.asarray(noise), k=1)]), psf, jac, psf_cen, g,
                         dil, kind, dtype)
    (out, flag), (nout, nflag) = _real_inverse(spec[0], kept, dtype), \
        _real_inverse(spec[1], kept, dtype)
    return out, nout, flag | nflag


# ---------------------------------------------------------------------------
# the closed form for gaussians

CLOSED_FORM_SHAPE = (64, 64)
CLOSED_FORM_PSF_SIGMA_PIX = 2.0
CLOSED_FORM_OBJ_PIXCOV = np.array([[7.0, 0.8], [0.8, 5.5]])     # the object, in pixels^2
CLOSED_FORM_SHEARS = ((0.01, 0.0), (-0.01, 0.0), (0.0, 0.01), (0.0, -0.01), (0.2, -0.1))
CLOSED_FORM_QMAX = 2.0


def closed_form_case(deriv):
    """(image, psf, jac record, psf centre, object covariance, psf covariance)
    for one set of jacobian derivatives: point-sampled gaussians on 64 x 64, the
    psf round in pixels with sigma = 2 px, off-pixel centres; world covariances"""
    jac = jac_record(31.3, 32.2, *deriv)
    pjac = jac_record(31.6, 31.1, *deriv)
    jm = M._jmat(jac, np.float64)
    pcov = CLOSED_FORM_PSF_SIGMA_PIX ** 2 * (jm @ jm.T)
    ocov = jm @ CLOSED_FORM_OBJ_PIXCOV @ jm.T
    image = gaussian_stamp(CLOSED_FORM_SHAPE, jac, ocov + pcov, 100.0)
    psf = gaussian_stamp(CLOSED_FORM_SHAPE, pjac, pcov, 1.3)
    return image, psf, jac, pjac[0:2], ocov, pcov


def closed_form_spectrum(jac, ocov, pcov, g, dil, kind):
    """G^_obj+psf(k') / G^_psf(k') G^_psf(k_t) Pi(q) / Pi(q_t) exp(-i q . centre)
    with k = J^-T q, for fluxes 100 and 1.3, on the full plane of modes"""
    jac = np.asarray(jac, dtype=np.float64)
    jit = M._inv2(M._jmat(jac, np.float64)).T
    q, qi, qt = frequencies(CLOSED_FORM_SHAPE, jac, g, dil, kind)
    ki, kt = jit @ qi, jit @ qt

    def gauss(k, cov):
        return np.exp(-0.5 * np.einsum("im,ij,jm->m", k, cov, k))
    out = 100.0 * gauss(ki, ocov + pcov) / (1.3 * gauss(ki, pcov)) * (1.3 * gauss(kt, pcov)) \
        * pixel_ft(q) / pixel_ft(qt)
    out = out * np.exp(-1j * (q[0] * jac[0] + q[1] * jac[1]))
    low = np.maximum(np.abs(q[0]), np.abs(q[1])) <= CLOSED_FORM_QMAX
    return out.reshape(CLOSED_FORM_SHAPE), low.reshape(CLOSED_FORM_SHAPE)


# ---------------------------------------------------------------------------
# the device cases

_REFERENCE_CACHE = {}


def device_reference(shape, psf_shape, n, step=0.01, dtype=np.longdouble):
    """the reference outputs of device_case(shape, psf_shape, n), computed once
    per process and not changed afterwards: per type of TYPES, and for the
    per-stamp shears 'galshear' and 'psfshear', the images (n, R, C), the
    target psf images (n, Rp, Cp) and, for the types on square stamps, the
    images with fixnoise"""
    key = (tuple(shape), tuple(psf_shape), n, step, np.dtype(dtype).name)
    if key in _REFERENCE_CACHE:
        return _REFERENCE_CACHE[key]
    case = device_case(shape, psf_shape, n)
    square = shape[0] == shape[1]
    out = {}
    for name in TYPES + ("galshear", "psfshear"):
        ims, pims, fims = [], [], []
        for i in range(n):
            if name == "galshear":
                spec = shear_spec(case["shears"][i], IMAGE)
            elif name == "psfshear":
                spec = shear_spec(case["shears"][i], PSF)
            else:
                spec = type_spec(name, step)
            args = (case["psfs"][i], case["jacs"][i], case["pjacs"][i][0:2]) + spec
            pims.append(target_psf_image(*args, dtype=dtype)[0])
            if square and name in TYPES:
                im, nim, _ = _image_and_noise(case["images"][i], case["noise"][i], *args,
                                              dtype=dtype)
                ims.append(im)
                fims.append(im + np.rot90(nim, k=3))
            else:
                ims.append(metacal_image(case["images"][i], *args, dtype=dtype)[0])
        out[name] = dict(images=np.stack(ims), psf_images=np.stack(pims),
                         fixnoise_images=np.stack(fims) if fims else None)
        for v in out[name].values():
            if v is not None:
                v.setflags(write=False)
    _REFERENCE_CACHE[key] = out
    return out


def cabi_refusals(L, bad_arg, psf_only):
    """ngmix_metacal_dilate_spectrum_batch (psf_only: ngmix_metacal_dilate_psf_
    spectrum_batch) refuses bad calls before anything runs (no pointer below is
    ever read but g_host, dil_host and kind_host): the list of failed checks"""
    import ctypes
    keep = []

    def host(a, dtype):
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        return ctypes.c_void_p(a.ctypes.data)
    p = ctypes.c_void_p(4096)       # stands for a device pointer; never read
    good = dict(images=p, noise=None, psf=p, jac=p, psf_cen=p, g=p, dil=p, kind=p,
                g_host=host([[0.01, 0.0], [0.0, 0.3]], np.float64),
                dil_host=host([1.02, 1.6], np.float64), kind_host=host([0, 1], np.int32),
                per_stamp_g=0, n=2, ntypes=2, nrow=16, ncol=16, prow=11, pcol=11, spec=p, flags=p)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        if psf_only:
            return L.ngmix_metacal_dilate_psf_spectrum_batch(
                a["psf"], a["jac"], a["psf_cen"], a["g"], a["dil"], a["kind"], a["g_host"],
                a["dil_host"], a["kind_host"], a["per_stamp_g"], a["n"], a["ntypes"], a["prow"],
                a["pcol"], a["spec"], a["flags"], None)
        return L.ngmix_metacal_dilate_spectrum_batch(
            a["images"], a["noise"], a["psf"], a["jac"], a["psf_cen"], a["g"], a["dil"], a["kind"],
            a["g_host"], a["dil_host"], a["kind_host"], a["per_stamp_g"], a["n"], a["ntypes"],
            a["nrow"], a["ncol"], a["prow"], a["pcol"], a["spec"], a["flags"], None)
    failed = []
    pointers = ["psf", "jac", "psf_cen", "g", "dil", "kind", "g_host", "dil_host", "kind_host",
                "spec", "flags"] + ([] if psf_only else ["images"])
    for name in pointers:
        if call(**{name: None}) != bad_arg:
            failed.append("null " + name)
    for name in ["ntypes", "prow", "pcol"] + ([] if psf_only else ["nrow", "ncol"]):
        for v in (0, -3):
            if call(**{name: v}) != bad_arg:
                failed.append("%s = %d" % (name, v))
    for gbad in ([[0.01, 0.0], [1.0, 0.0]], [[0.8, 0.7], [0.0, 0.0]], [[np.nan, 0.0], [0.0, 0.0]]):
        if call(g_host=host(gbad, np.float64)) != bad_arg:
            failed.append("g = %s" % (gbad,))
    for dbad in ([1.02, 0.999], [np.nan, 1.0], [1.0, np.inf], [-2.0, 1.0]):
        if call(dil_host=host(dbad, np.float64)) != bad_arg:
            failed.append("dil = %s" % (dbad,))
    for kbad in ([0, 2], [-1, 0]):
        if call(kind_host=host(kbad, np.int32)) != bad_arg:
            failed.append("kind = %s" % (kbad,))
    if call(n=2 ** 30, ntypes=2) != bad_arg:
        failed.append("too many (stamp, type) pairs")
    big = dict(prow=200, pcol=200) if psf_only else dict(nrow=200, ncol=200)
    if call(**big) != bad_arg:
        failed.append("a stamp beyond the LDS")
    # a dilation of exactly 1 and both kinds are served arguments: with no
    # stamps nothing is done, whatever else is passed
    for n in (0, -1):
        if call(n=n, psf=None, spec=None) != 0:
            failed.append("n = %d is not a no-op" % n)
    return failed
