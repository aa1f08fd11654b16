"""
A dense reference of the sheared pre-psf moments (DESIGN.md 3.21;
PrePSFMom.measure_arrays_sheared, csrc/prepsf_shear.hip): direct sums over
explicit phase matrices -- no recurrence, no FFT -- in np.longdouble, or in
float64 with dtype=np.float64.

For one stamp I (dim x dim, centre (r0, c0)), its psf stamp P (pdim x pdim, own
centre), the derivative matrix J = [[dvdrow, dvdcol], [dudrow, dudcol]] both
share, a shear (g1, g2) and the kernels of prepsfmom._kernels on the padded
size D = int(max(dim, pdim) pad_factor):

  1. kept modes and their weights (1 or 2) from prepsfmom._mode_plan, at
     k = 2 pi fftfreq(D)[a, b] (numpy's own float64 values, widened);
  2. k' = k + J^T (A - 1) J^-T k, A = [[1-g1, g2], [g2, 1+g1]] / sqrt(1-g^2) in
     (v, u) order: exactly k at g = 0;
  3. I^(k') = sum edge[r] edge[c] I[r, c] exp(-i (k'_r (r - r0) + k'_c (c - c0))),
     edge = prepsfmom._apodization_edge(dim, ap_rad), ones for ap_rad = 0;
     P^(k') the same sum over the psf stamp about its own centre, no taper;
  4. |P^| <= 1e-5 |sum P| is held at that amplitude (at the amplitude itself,
     real, where P^ = 0);
  5. M = D^-2 sum_k w fk Re(I^ / P^) for fk = fkp, fkc, fkr, fkf; the covariance
     D^-4 sum_k fk_a fk_b w pnoise / |P^|^2, pnoise = sum(1 / weight, weight > 0)
     (D / dim)^2;
  6. any kept mode with |k'_r| >= pi or |k'_c| >= pi, or a sum that is not
     finite: all fourteen NaN, flag 1.

unsheared_sums() is the same with step 2 left out: k on the grid, what
measure_arrays sums (there the padding offsets are put back through the centre
phases; here the transforms are about the centres from the start).

Measured with this file (tests/test_prepsf_shear_host.py prints the figures):
F64_VS_LONGDOUBLE and PHYSICS_BOUND below.
"""
import numpy as np

from ngmix_amd import prepsfmom

# the largest deviation of the float64 restatement from the longdouble one over
# cases() x ap_rad (1.5, 0) x kind (pgauss, ksigma), five types at step 0.01 and
# the per-stamp shears, relative to each sum's scale (the largest |term| of that
# sum).  Measured: 2.03e-14 (test_float64_against_longdouble prints the figure
# and asserts that it stays at or below this).  The host twin and the kernel
# are allowed four times this (TWIN_TOL) for their summation order and the
# phase recurrence; measured: host twin 2.55e-14 (DESIGN.md 3.21 has the
# kernel's figure).
F64_VS_LONGDOUBLE = 2.1e-14
TWIN_TOL = 4 * F64_VS_LONGDOUBLE

TYPES = ("noshear", "1p", "1m", "2p", "2m")
STEP = 0.01
DERIV = (-0.26, 0.02, 0.03, 0.27)       # not diagonal, flipped (det < 0)
# (dim, pdim, number of stamps)
SHAPES = ((16, 16, 70), (17, 11, 3), (32, 32, 1))
KINDS = ("pgauss", "ksigma")
AP_RADS = (1.5, 0.0)


def host_fexp(x):
    """the fast exponential exp5_smooth of ngmix_amd.fastexp_nb in numpy, for
    building the gaussian kernels where no device is present (the package
    evaluates it with its device function; the kernels are INPUTS of the
    reference and of the code under test alike)"""
    x = np.asarray(x, dtype=np.float64)
    ival = (x - 0.5).astype(np.int64)              # truncation toward zero
    f = x - ival
    poly = 1.0000011318561302 + f * (0.999993601071577 + f * (0.49992478810274166 + f * (
        0.16674612720799442 + f * (0.042330947141114836 + f * 0.008197933236258961))))
    return np.exp(ival.astype(np.float64)) * poly


def type_shears(step=STEP):
    return np.array([(0.0, 0.0), (step, 0.0), (-step, 0.0), (0.0, step), (0.0, -step)])


def fwhm_of(dim, deriv=DERIV):
    """a weight kernel that fits the stamp and whose modes stay inside the
    band under |g| = 0.3 (they end near 5 / sigma for pgauss: 2 rad per pixel
    at most, times 1.36): a fwhm of 0.4 of the stamp's width"""
    scale = np.sqrt(abs(deriv[0] * deriv[3] - deriv[1] * deriv[2]))
    return 0.4 * dim * scale


def measure_of(kind, dim, ap_rad, fwhm=None):
    return prepsfmom.PrePSFMom(fwhm_of(dim) if fwhm is None else fwhm, kind, ap_rad=ap_rad)


def plan_of(measure, dim, pdim, deriv=DERIV):
    """(kernels, D, signed rows, signed cols, wgt, fk (4, M)) of a measurement"""
    D = int(max(dim, pdim) * measure.pad_factor)
    kernels = prepsfmom._kernels(measure.kind, D, float(measure.fwhm), deriv,
                                 float(measure.fwhm_smooth))
    plan = prepsfmom._mode_plan(kernels, None)
    fk = np.stack([kernels[k][plan["keep"]] for k in ("fkp", "fkc", "fkr", "fkf")])
    return kernels, D, plan["rows"], plan["cols"], plan["wgt"], fk


def _dtft(img, cen, qr, qc):
    dtype = qr.dtype
    er = np.exp(-1j * np.outer(qr, np.arange(img.shape[0]).astype(dtype) - cen[0]))
    ec = np.exp(-1j * np.outer(qc, np.arange(img.shape[1]).astype(dtype) - cen[1]))
    return np.einsum("mr,rc,mc->m", er, img, ec)


def _sums_at(image, weight, cen, psf, psf_cen, qr, qc, wgt, fk, D, ap_rad, dtype):
    """steps 3-6 at the frequencies (qr, qc); returns (sums (14,), flag, scale
    (14,): the largest |term| of every sum)"""
    dim = image.shape[0]
    # the band's edge is the grid's own Nyquist frequency, 2 pi fftfreq(D)[D/2] =
    # -(float64 pi), in every dtype
    pi = dtype(np.pi)
    image = np.asarray(image, dtype=dtype)
    psf = np.asarray(psf, dtype=dtype)
    if ap_rad > 0:
        edge = prepsfmom._apodization_edge(dim, ap_rad).astype(dtype)
        image = image * np.outer(edge, edge)
    out_of_band = bool(np.any(~((np.abs(qr) < pi) & (np.abs(qc) < pi))))
    ti = _dtft(image, np.asarray(cen, dtype=dtype), qr, qc)
    tp = _dtft(psf, np.asarray(psf_cen, dtype=dtype), qr, qc)
    min_amp = dtype(1e-5) * np.abs(psf.sum())
    amp = np.abs(tp)
    with np.errstate(divide="ignore", invalid="ignore"):
        low = amp <= min_amp
        tp = np.where(low & (amp != 0), tp / np.where(amp == 0, 1, amp) * min_amp, tp)
        tp = np.where(low & (amp == 0), min_amp + 0j, tp)
        ratio = ti / tp
        w = np.asarray(weight, dtype=dtype)
        pnoise = np.sum(1 / w[w > 0]) * (dtype(D) / dtype(dim)) ** 2
        cw = wgt.astype(dtype) * pnoise / (tp.real ** 2 + tp.imag ** 2)
        fk = fk.astype(dtype)
        terms = [ratio.real * wgt.astype(dtype) * fk[a] for a in range(4)]
        for a in range(4):
            for b in range(a, 4):
                terms.append(fk[a] * fk[b] * cw)
        df2 = (dtype(1) / dtype(D)) ** 2
        norm = np.array([df2] * 4 + [df2 * df2] * 10, dtype=dtype)
        sums = np.array([t.sum() for t in terms], dtype=dtype) * norm
        scale = np.array([np.abs(t).max() for t in terms], dtype=dtype) * norm
    if out_of_band or not np.all(np.isfinite(sums.astype(np.float64))):
        return np.full(14, np.nan, dtype=dtype), 1, scale
    return sums, 0, scale


def sheared_sums(image, weight, cen, deriv, psf, psf_cen, g, rows, cols, wgt, fk, D, ap_rad,
                 dtype=np.longdouble):
    """steps 1-6 for one stamp and one shear"""
    f = (np.fft.fftfreq(D) * (2.0 * np.pi)).astype(dtype)
    k = np.stack([f[rows], f[cols]])
    jm = np.array([[deriv[0], deriv[1]], [deriv[2], deriv[3]]], dtype=dtype)
    det = jm[0, 0] * jm[1, 1] - jm[0, 1] * jm[1, 0]
    jit = (np.array([[jm[1, 1], -jm[0, 1]], [-jm[1, 0], jm[0, 0]]], dtype=dtype) / det).T
    g1, g2 = dtype(g[0]), dtype(g[1])
    root = np.sqrt(dtype(1) - g1 * g1 - g2 * g2)
    d = np.array([[(dtype(1) - g1) / root - dtype(1), g2 / root],
                  [g2 / root, (dtype(1) + g1) / root - dtype(1)]], dtype=dtype)
    ks = k + jm.T @ (d @ (jit @ k))
    return _sums_at(image, weight, cen, psf, psf_cen, ks[0], ks[1], wgt, fk, D, ap_rad, dtype)


def unsheared_sums(image, weight, cen, deriv, psf, psf_cen, rows, cols, wgt, fk, D, ap_rad,
                   dtype=np.longdouble):
    """the reference's own unsheared sums: k on the grid, no shear map at all"""
    f = (np.fft.fftfreq(D) * (2.0 * np.pi)).astype(dtype)
    return _sums_at(image, weight, cen, psf, psf_cen, f[rows], f[cols], wgt, fk, D, ap_rad, dtype)


# ---------------------------------------------------------------------------
# inputs

def gaussian_stamp(dim, cen, deriv, cov, flux, dtype=np.float64):
    """a point-sampled gaussian of world covariance cov ((v, u) order)"""
    rr, cc = np.meshgrid(np.arange(dim).astype(dtype) - dtype(cen[0]),
                         np.arange(dim).astype(dtype) - dtype(cen[1]), indexing="ij")
    v = dtype(deriv[0]) * rr + dtype(deriv[1]) * cc
    u = dtype(deriv[2]) * rr + dtype(deriv[3]) * cc
    cov = np.asarray(cov, dtype=dtype)
    det = cov[0, 0] * cov[1, 1] - cov[0, 1] * cov[1, 0]
    chi2 = (cov[1, 1] * v * v - 2 * cov[0, 1] * v * u + cov[0, 0] * u * u) / det
    area = abs(dtype(deriv[0]) * dtype(deriv[3]) - dtype(deriv[1]) * dtype(deriv[2]))
    pi = dtype(4) * np.arctan(dtype(1))
    return dtype(flux) * area / (2 * pi * np.sqrt(det)) * np.exp(-chi2 / 2)


def case(dim, pdim, n, seed=7):
    """
    n stamps of one shape: gaussian objects of their own covariance seen through
    a slightly elliptical gaussian psf, a little noise, centres off the pixel
    grid and different for image and psf, the jacobian derivatives DERIV, a
    weight map of 16 with a few zeros (its square root is exact), and a
    per-stamp shear of up to |g| = 0.3 (stamp 1, where there is one: 0.3).
    """
    rng = np.random.RandomState(seed + 100 * dim + pdim + n)
    scale = np.sqrt(abs(DERIV[0] * DERIV[3] - DERIV[1] * DERIV[2]))
    images, psfs = np.zeros((n, dim, dim)), np.zeros((n, pdim, pdim))
    cen, pcen, shears = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2))
    for i in range(n):
        cen[i] = (dim - 1) / 2 + rng.uniform(-0.9, 0.9, size=2)
        pcen[i] = (pdim - 1) / 2 + rng.uniform(-0.5, 0.5, size=2)
        s = scale * min(1.3, (pdim - 1) / 10.0) * rng.uniform(0.95, 1.1)
        e = rng.uniform(-0.03, 0.03, size=2) * s * s
        pcov = np.array([[s * s + e[0], e[1]], [e[1], s * s - e[0]]])
        a = (scale * dim / 16.0) ** 2 * rng.uniform(1.0, 2.5, size=2)
        b = (scale * dim / 16.0) ** 2 * rng.uniform(-0.4, 0.4)
        images[i] = gaussian_stamp(dim, cen[i], DERIV, np.array([[a[0], b], [b, a[1]]]) + pcov,
                                   rng.uniform(50.0, 200.0))
        images[i] += rng.normal(scale=1e-3 * images[i].max(), size=(dim, dim))
        psfs[i] = gaussian_stamp(pdim, pcen[i], DERIV, pcov, rng.uniform(0.9, 1.1))
        gabs, ang = rng.uniform(0.0, 0.3), rng.uniform(0, 2 * np.pi)
        shears[i] = gabs * np.cos(ang), gabs * np.sin(ang)
    if n > 1:
        shears[1] = 0.3 * np.cos(0.7), 0.3 * np.sin(0.7)
    weights = np.full((n, dim, dim), 16.0)
    weights[:, 0, 0] = 0.0
    weights[:, dim // 2, 1] = -1.0
    return dict(images=images, psfs=psfs, weights=weights, cen=cen, pcen=pcen, shears=shears)


_CACHE = {}


def reference(dim, pdim, n, kind, ap_rad, dtype=np.longdouble, rows_of=None):
    """
    The reference sums of case(dim, pdim, n) under measure_of(kind, dim,
    ap_rad), computed once per process and not changed afterwards: 'types'
    (n, 5, 14) with its flags and scales, 'galshear' (n, 1, 14) likewise (the
    per-stamp shears).  rows_of: only these stamps (the others NaN) -- for the
    70-stamp case, where every stamp is the same code path.
    """
    key = (dim, pdim, n, kind, ap_rad, np.dtype(dtype).name, rows_of)
    if key in _CACHE:
        return _CACHE[key]
    c = case(dim, pdim, n)
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
                sums[i, t], flags[i, t], scale[i, t] = sheared_sums(
                    c["images"][i], c["weights"][i], c["cen"][i], DERIV, c["psfs"][i],
                    c["pcen"][i], g, rows, cols, wgt, fk, D, ap_rad, dtype)
        for a in (sums, scale, flags):
            a.setflags(write=False)
        out[name] = dict(sums=sums, scale=scale, flags=flags)
    _CACHE[key] = out
    return out


# ---------------------------------------------------------------------------
# physics: a round gaussian through a gaussian psf under the pgauss weight

PHYS_DIM = 32
PHYS_FWHM = 1.2                         # of the weight, in the jacobian's units
PHYS_OBJ_SIGMA, PHYS_PSF_SIGMA, PHYS_FLUX = 0.5, 0.4, 100.0
PHYS_CEN, PHYS_PCEN = (15.3, 16.2), (15.6, 15.4)
# |R(reference) - R(analytic)| over the four entries of the e response at step
# 0.01, measured on the longdouble reference at PHYS_DIM: PHYS_MEASURED (the
# stamp's truncation, the kernel's cut at chi2 = 25 and its fast exponential;
# not rounding).  The test allows twice that.
PHYS_MEASURED = 2.18e-6
PHYSICS_BOUND = 2 * PHYS_MEASURED


def physics_case():
    eye = np.eye(2)
    image = gaussian_stamp(PHYS_DIM, PHYS_CEN, DERIV,
                           (PHYS_OBJ_SIGMA ** 2 + PHYS_PSF_SIGMA ** 2) * eye, PHYS_FLUX)
    psf = gaussian_stamp(PHYS_DIM, PHYS_PCEN, DERIV, PHYS_PSF_SIGMA ** 2 * eye, 1.0)
    return image, np.ones_like(image), psf


def analytic_pgauss_e(g):
    """(e1, e2) = (M+, Mx) / Mr of the round gaussian sheared by g under the
    weight exp(-x^2 / (2 sw^2)): the weighted second moments of a gaussian of
    covariance S are proportional to (S^-1 + 1 / sw^2)^-1; + is u^2 - v^2 and x
    is 2 u v in the (v, u) order of the covariance"""
    g1, g2 = g
    a = np.array([[1 - g1, g2], [g2, 1 + g1]]) / np.sqrt(1 - g1 * g1 - g2 * g2)
    cov = a @ (PHYS_OBJ_SIGMA ** 2 * np.eye(2)) @ a.T
    sw = PHYS_FWHM / (2 * np.sqrt(2 * np.log(2)))
    c = np.linalg.inv(np.linalg.inv(cov) + np.eye(2) / sw ** 2)
    return np.array([c[1, 1] - c[0, 0], 2 * c[0, 1]]) / (c[0, 0] + c[1, 1])


def response(e_of_type, step=STEP):
    """R[i, j] = (e_i(jp) - e_i(jm)) / (2 step) from e (5, 2) in TYPES' order"""
    e = np.asarray(e_of_type, dtype=np.float64)
    return np.stack([(e[1] - e[2]) / (2 * step), (e[3] - e[4]) / (2 * step)], axis=1)


def gap(got, ref):
    """the largest |got - ref| / scale over the unflagged entries of a reference
    dict's sums"""
    ok = ref["flags"] == 0
    got = np.asarray(got)[ok].astype(np.longdouble)
    return float(np.max(np.abs(got - ref["sums"][ok].astype(np.longdouble)) /
                        ref["scale"][ok].astype(np.longdouble)))


def call_entry(L, ptr, c, g, rows, cols, kwgt, kfk, D, ap_rad, deriv=DERIV, host=True,
               fixnoise=False, nturned=None, with_power=False, power=None, **over):
    """One of the eight ngmix_prepsf_shear_*sums_{host,batch} entries on a case's
    arrays (host=False: _batch with a null stream, for the refusals).  fixnoise:
    the entries that take the TURNED noise planes nturned; with_power: those
    that take the noise images `power`.  Returns (status, sums (n, T, 14), flags
    (n, T)).  `over` replaces arguments by name (refusals)."""
    n, dim = c["images"].shape[0], c["images"].shape[1]
    pdim = c["psfs"].shape[1]
    g = np.ascontiguousarray(g, dtype=np.float64)
    nt = g.shape[-2]
    half = (D + 1) // 2
    a = dict(
        images=np.ascontiguousarray(c["images"]), weights=np.ascontiguousarray(c["weights"]),
        psf=np.ascontiguousarray(c["psfs"]),
        noise_turned=None if nturned is None else np.ascontiguousarray(nturned),
        noise_power=None if power is None else np.ascontiguousarray(power),
        cen=np.ascontiguousarray(c["cen"]), psf_cen=np.ascontiguousarray(c["pcen"]),
        edge=prepsfmom._apodization_edge(dim, ap_rad) if ap_rad > 0 else None,
        g=g, g_host=g, per_stamp_g=1 if g.ndim == 3 else 0,
        mrow=np.where(rows < half, rows, rows - D).astype(np.int32),
        mcol=np.where(cols < half, cols, cols - D).astype(np.int32),
        wgt=np.ascontiguousarray(kwgt, dtype=np.float64),
        fk=np.ascontiguousarray(kfk, dtype=np.float64), n=n, ntypes=nt, nmodes=int(rows.size),
        dim=dim, pdim=pdim, fft_dim=D, deriv=deriv,
        sums=np.full((n, nt, 14), -7.0), flags=np.full((n, nt), -7, dtype=np.int32))
    a.update(over)

    def p(x):
        return None if x is None else ptr(x)
    names = ["images", "weights", "psf"] + (["noise_turned"] if fixnoise else []) + \
        (["noise_power"] if with_power else []) + ["cen", "psf_cen", "edge", "g", "g_host"]
    args = [p(a[k]) for k in names]
    args += [a["per_stamp_g"]] + [p(a[k]) for k in ("mrow", "mcol", "wgt", "fk")]
    args += [a["n"], a["ntypes"], a["nmodes"], a["dim"], a["pdim"], a["fft_dim"]]
    args += [float(d) for d in a["deriv"]] + [p(a["sums"]), p(a["flags"])]
    entry = "ngmix_prepsf_shear_%s%ssums_%s" % ("fixnoise_" if fixnoise else "",
                                                "power_" if with_power else "",
                                                "host" if host else "batch")
    st = getattr(L, entry)(*(args + ([] if host else [None])))
    return st, a["sums"], a["flags"]


def call_host(L, ptr, c, g, rows, cols, kwgt, kfk, D, ap_rad, deriv=DERIV, host=True, **over):
    """ngmix_prepsf_shear_sums_host on a case's arrays (call_entry)."""
    return call_entry(L, ptr, c, g, rows, cols, kwgt, kfk, D, ap_rad, deriv, host, **over)
