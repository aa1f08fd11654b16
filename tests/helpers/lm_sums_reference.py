"""
Dense reference of the LM normal-equation sums (CPU only; TEST INFRASTRUCTURE).

What ngmix_lm_eval_batch leaves per stamp -- J^T J (upper triangle), J^T f,
f.f over the stamp's nloc local parameters (the shared shape parameters
followed by the flux of the stamp's band), and the two get_loglike statistics
-- and what ngmix_lm_advance_batch folds per object, made the slow way:

  * the mixture by oracle.gmix_fill + oracle.gmix_convolve_fill, the pixels by
    oracle.make_pixels(ignore_zero_weight=True), the residuals by
    oracle.fill_fdiff (the C restatement of the reference's loops, pinned to
    the reference's goldens by tests/test_oracle_golden.py);
  * the analytic J (gauss / exp / dev) by oracle.deriv_images with dcov from
    the chain rule of calc_jacobian (results.py:955-1010) written out below,
    times ierr, the flux column the model image over the flux;
  * the forward-difference J (every model the kernel takes) column by column,
    (fdiff(x with x_j := x_j + h_j) - fdiff(x)) / h_j with fdjac2's step
    h_j = sqrt(eps) |x_j| (sqrt(eps) at x_j == 0); each fdiff is the oracle's
    float64 vector, the subtraction, the division and all that follows are in
    np.longdouble;
  * every sum in np.longdouble, in the layout of NGMIX_LM_NSUMS, with the
    Cauchy-Schwarz scale of every entry next to it.

The case table at the end is data: the host test checks the reference and the
table's own conditions on the CPU, the GPU test walks the same cases.
"""
import numpy as np

from oracle import oracle as ora

LD = np.longdouble
SQRT_EPS = 2.0 ** -26          # fdjac2: sqrt of the double machine epsilon
MAX_CHI2 = 25.0
SCALE = 0.263

NG0 = {"gauss": 1, "turb": 3, "exp": 6, "dev": 10, "bdf": 16, "bd": 16}
NLOC = {"gauss": 6, "turb": 6, "exp": 6, "dev": 6, "bdf": 7, "bd": 8}
ANALYTIC_MODELS = ("gauss", "exp", "dev")


def model_name(model):
    """'coellip3' -> ('coellip', 3); 'exp' -> ('exp', None)"""
    if model.startswith("coellip"):
        return "coellip", int(model[7:])
    return model, None


def nloc_of(model):
    name, ng = model_name(model)
    return 4 + 2 * ng if name == "coellip" else NLOC[name]


def ngauss_of(model):
    name, ng = model_name(model)
    return ng if name == "coellip" else NG0[name]


def nsums(nloc):
    """NGMIX_LM_NSUMS"""
    return nloc * (nloc + 1) // 2 + nloc + 1


def tri_index(nloc):
    """(a, b), a <= b, in the order of the packed upper triangle"""
    return [(a, b) for a in range(nloc) for b in range(a, nloc)]


def jac_record(row0, col0, dvdrow, dvdcol, dudrow, dudcol):
    """the reference's 8-double jacobian record"""
    det = dvdrow * dudcol - dvdcol * dudrow
    return np.array([row0, col0, dvdrow, dvdcol, dudrow, dudcol, det, np.sqrt(abs(det))])


def _ora_jac(rec):
    j = np.zeros(1, dtype=ora.JACOBIAN_DTYPE)
    j[0] = tuple(np.asarray(rec, dtype="f8").reshape(8))
    return j


def local_pars(model, pars, band):
    """the stamp's local parameters out of the object's: shape parameters, then
    the flux of `band` (coellip has one band and all its parameters local)"""
    pars = np.asarray(pars, dtype="f8")
    name, _ = model_name(model)
    if name == "coellip":
        return pars.copy()
    ns = nloc_of(model) - 1
    return np.concatenate([pars[:ns], pars[ns + band:ns + band + 1]])


def make_mixture(model, lpars, psf):
    """(status, gm0, gmc): the object's mixture at its local parameters and the
    one composed with the stamp's psf (psf: (npsf, 6) 'full' rows or None)"""
    name, _ = model_name(model)
    gm0 = np.zeros(ngauss_of(model), dtype=ora.GAUSS2D_DTYPE)
    st = ora.gmix_fill(gm0, np.asarray(lpars, dtype="f8"), name)
    if st != ora.OK:
        return st, None, None
    if psf is None:
        return ora.OK, gm0, gm0.copy()
    psf = np.asarray(psf, dtype="f8").reshape(-1, 6)
    gp = np.zeros(psf.shape[0], dtype=ora.GAUSS2D_DTYPE)
    assert ora.gmix_fill(gp, psf.ravel(), "full") == ora.OK
    gmc = np.zeros(gm0.size * gp.size, dtype=ora.GAUSS2D_DTYPE)
    st = ora.gmix_convolve_fill(gmc, gm0, gp)
    return st, gm0, gmc


def stamp_pixels(image, weight, jac):
    return ora.make_pixels(np.asarray(image, dtype="f8"), np.asarray(weight, dtype="f8"),
                           _ora_jac(jac), ignore_zero_weight=True)


def fdiff_at(model, lpars, psf, pixels):
    """the oracle's float64 residual vector, or None where the model is out of
    range (the reference's LOWVAL vector)"""
    st, _, gmc = make_mixture(model, lpars, psf)
    if st != ora.OK:
        return None
    fd = np.zeros(pixels.size)
    if ora.fill_fdiff(gmc, pixels, fd, 0) != ora.OK:
        return None
    return fd


def model_image(gmc, pixels):
    """the model at the kept pixels, as get_loglike evaluates it"""
    coords = np.zeros(pixels.size, dtype=ora.COORD_DTYPE)
    for n in ("u", "v", "area"):
        coords[n] = pixels[n]
    im = np.zeros(pixels.size)
    g = gmc.copy()
    assert ora.render(g, coords, im, fast_exp=1) == ora.OK
    return im


def deriv_data(gm0, gmc, g1, g2, T):
    """gpars (ngauss, 6) = [p, v, u, irr, irc, icc] of the composed gaussians
    and dcov (ngauss, 3, 3) = d(irr, irc, icc)/d(g1 | g2 | T).

    Only the object's part of a composed covariance moves with the model:
    Sigma_k = (T_k / 2) [[1 - e1, e2], [e2, 1 + e1]] with e = 2 g / (1 + |g|^2),
    so d Sigma_k / d g_i = (T_k / 2) [[-d e1, d e2], [d e2, d e1]] / d g_i and
    d Sigma_k / dT = Sigma_k / T (T_k is linear in T)."""
    npsf = gmc.size // gm0.size
    gpars = np.column_stack([gmc[n] for n in ("p", "row", "col", "irr", "irc", "icc")])
    cov0 = np.repeat(np.column_stack([gm0[n] for n in ("irr", "irc", "icc")]), npsf, axis=0)
    half_tk = 0.5 * (cov0[:, 0] + cov0[:, 2])
    s = 1.0 + g1 * g1 + g2 * g2
    # d e_a / d g_b = 2 delta_ab / s - 4 g_a g_b / s^2
    de = np.array([[2.0 / s - 4.0 * g1 * g1 / s ** 2, -4.0 * g1 * g2 / s ** 2],
                   [-4.0 * g1 * g2 / s ** 2, 2.0 / s - 4.0 * g2 * g2 / s ** 2]])
    dcov = np.zeros((gmc.size, 3, 3))
    for b in range(2):
        de1, de2 = de[0, b], de[1, b]
        dcov[:, b, 0] = -half_tk * de1
        dcov[:, b, 1] = half_tk * de2
        dcov[:, b, 2] = half_tk * de1
    dcov[:, 2, :] = cov0 / T
    return gpars, dcov


def analytic_jacobian(model, lpars, psf, pixels):
    """(J (npix, 6) float64, fdiff, model image) for gauss / exp / dev"""
    assert model in ANALYTIC_MODELS
    st, gm0, gmc = make_mixture(model, lpars, psf)
    assert st == ora.OK
    g1, g2, T, flux = lpars[2:6]
    gpars, dcov = deriv_data(gm0, gmc, g1, g2, T)
    out = np.zeros((6, pixels.size))
    ora.deriv_images(gpars, dcov, pixels["v"], pixels["u"], pixels["area"], out)
    J = np.zeros((pixels.size, 6))
    for k in range(5):
        J[:, k] = out[1 + k] * pixels["ierr"]
    J[:, 5] = out[0] * (pixels["ierr"] / flux)
    fd = np.zeros(pixels.size)
    assert ora.fill_fdiff(gmc, pixels, fd, 0) == ora.OK
    return J, fd, out[0].copy()


def fd_steps(lpars):
    """fdjac2's (h, x + h): h_j = sqrt(eps) |x_j|, sqrt(eps) at x_j == 0"""
    x = np.asarray(lpars, dtype="f8")
    h = SQRT_EPS * np.abs(x)
    h[h == 0.0] = SQRT_EPS
    return h, x + h


def forward_jacobian(model, lpars, psf, pixels):
    """(J (npix, nloc) longdouble, fdiff float64), or (None, None) when the
    model is out of range at the point or one step from it"""
    x = np.asarray(lpars, dtype="f8")
    f0 = fdiff_at(model, x, psf, pixels)
    if f0 is None:
        return None, None
    h, xs = fd_steps(x)
    J = np.zeros((pixels.size, x.size), dtype=LD)
    for j in range(x.size):
        p = x.copy()
        p[j] = xs[j]
        fj = fdiff_at(model, p, psf, pixels)
        if fj is None:
            return None, None
        J[:, j] = (fj.astype(LD) - f0.astype(LD)) / LD(h[j])
    return J, f0


def central_jacobian(model, lpars, psf, pixels, rel=1e-5):
    """longdouble central differences of the oracle's model, and an estimate of
    the second derivative (from the same three points), per column"""
    x = np.asarray(lpars, dtype="f8")
    f0 = fdiff_at(model, x, psf, pixels).astype(LD)
    J = np.zeros((pixels.size, x.size), dtype=LD)
    D2 = np.zeros((pixels.size, x.size), dtype=LD)
    for j in range(x.size):
        d = rel * max(abs(x[j]), 0.1)
        p, m = x.copy(), x.copy()
        p[j] += d
        m[j] -= d
        dd = (LD(p[j]) - LD(m[j]))
        fp = fdiff_at(model, p, psf, pixels).astype(LD)
        fm = fdiff_at(model, m, psf, pixels).astype(LD)
        J[:, j] = (fp - fm) / dd
        D2[:, j] = (fp - 2 * f0 + fm) / (dd / 2) ** 2
    return J, D2


def fd_floor(ref):
    """the reference's own rounding floor, column by column, relative to the
    column's norm: each of the two float64 residual vectors behind a column is
    rounded at eps (|model ierr| + |fdiff|) or so, and the column divides
    that by h_j:  eps (|m ierr|_2 + |f|_2) / (h_j |J_j|_2); 0 for a zero column"""
    px = ref["pixels"]
    f = np.asarray(ref["fdiff"], dtype="f8")
    m = f / np.where(px["ierr"] > 0, px["ierr"], 1.0) + px["val"]
    top = np.finfo("f8").eps * (np.linalg.norm(m * px["ierr"]) + np.linalg.norm(f))
    col = np.sqrt(np.asarray((np.asarray(ref["J"], dtype=LD) ** 2).sum(axis=0), dtype="f8"))
    out = np.zeros(col.size)
    nz = col > 0
    out[nz] = top / (ref["h"][nz] * col[nz])
    return out


def sums_of(J, f):
    """longdouble [J^T J upper triangle | J^T f | f.f] and the Cauchy-Schwarz
    scale of every entry: sqrt(A_ii A_jj) | sqrt(A_ii ff) | ff"""
    J = np.asarray(J, dtype=LD)
    f = np.asarray(f, dtype=LD)
    n = J.shape[1]
    A = J.T @ J
    g = J.T @ f
    ff = f @ f
    tri = tri_index(n)
    d = np.sqrt(np.diag(A))
    sums = np.array([A[a, b] for a, b in tri] + list(g) + [ff], dtype=LD)
    scale = np.array([d[a] * d[b] for a, b in tri] + list(d * np.sqrt(ff)) + [ff], dtype=LD)
    return sums, scale


def stamp_reference(model, lpars, stamp, fd):
    """the reference of one stamp at its local parameters.

    Returns a dict: status (0 or oracle.ERR_G_RANGE), sums / scale (longdouble,
    NGMIX_LM_NSUMS(nloc)), stats = (s2n_numer, s2n_denom) and stats_scale (the
    scale of s2n_numer), J, fdiff, pixels, h, xstep.  Out of range: sums 0 with
    ff = +inf and statistics 0, as the kernels leave them."""
    nloc = nloc_of(model)
    pixels = stamp_pixels(stamp["image"], stamp["weight"], stamp["jac"])
    h, xs = fd_steps(lpars)
    out = {"pixels": pixels, "h": h, "xstep": xs, "nloc": nloc}
    if fd:
        J, f = forward_jacobian(model, lpars, stamp["psf"], pixels)
    else:
        st, _, _ = make_mixture(model, lpars, stamp["psf"])
        if st != ora.OK:
            J = f = None
        else:
            J, f, _ = analytic_jacobian(model, lpars, stamp["psf"], pixels)
    if J is None:
        s = np.zeros(nsums(nloc), dtype=LD)
        s[-1] = np.inf
        out.update(status=ora.ERR_G_RANGE, sums=s, scale=np.zeros_like(s), J=None, fdiff=None,
                   stats=np.zeros(2, dtype=LD), stats_scale=LD(0))
        return out
    sums, scale = sums_of(J, f)
    _, _, gmc = make_mixture(model, lpars, stamp["psf"])
    m = model_image(gmc, pixels).astype(LD)
    ierr = pixels["ierr"].astype(LD)
    val = pixels["val"].astype(LD)
    ivar = ierr * ierr
    numer = (val * m * ivar).sum()
    denom = (m * m * ivar).sum()
    out.update(status=ora.OK, sums=sums, scale=scale, J=J, fdiff=f,
               stats=np.array([numer, denom], dtype=LD),
               stats_scale=np.sqrt(((m * ierr) ** 2).sum() * ((val * ierr) ** 2).sum()))
    return out


def fold(blocks, bands, nloc, nband):
    """scatter-add per-stamp sums (longdouble) into an object's global system of
    n = nloc - 1 + nband parameters: the shape parameters are shared, the flux
    of band b sits at nloc - 1 + b.  Returns (A (n, n), g (n,), ff)."""
    n = nloc - 1 + nband
    ntri = nloc * (nloc + 1) // 2
    A = np.zeros((n, n), dtype=LD)
    g = np.zeros(n, dtype=LD)
    ff = LD(0)
    for s, band in zip(blocks, bands):
        gi = [a if a < nloc - 1 else nloc - 1 + band for a in range(nloc)]
        for k, (a, b) in enumerate(tri_index(nloc)):
            A[gi[a], gi[b]] += s[k]
            if a != b:
                A[gi[b], gi[a]] += s[k]
        for a in range(nloc):
            g[gi[a]] += s[ntri + a]
        ff += s[ntri + nloc]
    return A, g, ff


def stacked_global_jacobian(Js, fs, bands, nloc, nband):
    """the object's global J built directly: the stamps' rows stacked, every
    stamp's flux column put at its band"""
    n = nloc - 1 + nband
    rows = sum(J.shape[0] for J in Js)
    G = np.zeros((rows, n), dtype=LD)
    F = np.zeros(rows, dtype=LD)
    r = 0
    for J, f, band in zip(Js, fs, bands):
        k = J.shape[0]
        G[r:r + k, :nloc - 1] = J[:, :nloc - 1]
        G[r:r + k, nloc - 1 + band] = J[:, nloc - 1]
        F[r:r + k] = f
        r += k
    return G, F


# ---------------------------------------------------------------- skipping
def pair_census(model, lpars, stamp, tiles=True):
    """over the (8 x 8 tile, composed gaussian) pairs of a stamp: how many have
    no pixel with chi2 < 25 ("skipped"), how many there are, and the smallest
    |chi2 - 25| over the KEPT pixels and gaussians -- all in longdouble.
    Out of range: (0, 0, inf)."""
    st, _, gmc = make_mixture(model, lpars, stamp["psf"])
    if st != ora.OK or ora.gmix_set_norms(gmc) != ora.OK:
        return 0, 0, np.inf
    nrow, ncol = stamp["image"].shape
    j = np.asarray(stamp["jac"], dtype="f8")
    rr, cc = np.mgrid[0:nrow, 0:ncol]
    rd, cd = rr.astype(LD) - LD(j[0]), cc.astype(LD) - LD(j[1])
    v = LD(j[2]) * rd + LD(j[3]) * cd
    u = LD(j[4]) * rd + LD(j[5]) * cd
    kept = np.asarray(stamp["weight"]) > 0.0
    skipped = total = 0
    margin = np.inf
    for g in gmc:
        dv, du = v - LD(g["row"]), u - LD(g["col"])
        chi2 = LD(g["dcc"]) * dv * dv + LD(g["drr"]) * du * du - 2 * LD(g["drc"]) * dv * du
        if kept.any():
            margin = min(margin, float(np.abs(chi2[kept] - MAX_CHI2).min()))
        inside = chi2 < MAX_CHI2
        if not tiles:
            continue
        for r0 in range(0, nrow, 8):
            for c0 in range(0, ncol, 8):
                total += 1
                skipped += int(not inside[r0:r0 + 8, c0:c0 + 8].any())
    return skipped, total, margin


# ------------------------------------------------------------ the case table
ANALYTIC_SHAPES = [(5, 5), (8, 8), (9, 7), (16, 16), (17, 19), (25, 25), (33, 31), (48, 48),
                   (8, 65), (65, 8)]
FD_SHAPES = [(5, 5), (9, 7), (25, 25), (33, 31), (17, 64)]
FD_MODELS = ["gauss", "turb", "exp", "dev", "bdf", "bd",
             "coellip1", "coellip2", "coellip3", "coellip4", "coellip5"]
JACOBIANS = ["diag", "rot30", "flip", "aniso"]
ORIGINS = [(0.0, 0.0), (0.5, -0.5), (3.3, -2.7)]
WEIGHTS = ["uniform", "random", "tile", "edges"]
TRIALS = ["sheared", "small", "wide", "outside", "far"]
PSFS = [None, 1, 3]


def make_jacobian(kind, shape, origin):
    nrow, ncol = shape
    row0 = (nrow - 1) / 2.0 + origin[0]
    col0 = (ncol - 1) / 2.0 + origin[1]
    s = SCALE
    if kind == "diag":
        m = (s, 0.0, 0.0, s)
    elif kind == "rot30":
        c, sn = np.cos(np.pi / 6), np.sin(np.pi / 6)
        m = (s * c, -s * sn, s * sn, s * c)
    elif kind == "flip":                      # det < 0
        m = (s, 0.02 * s, 0.0, -s)
    elif kind == "aniso":                     # 2 : 1
        m = (1.4 * s, 0.1 * s, -0.05 * s, 0.7 * s)
    else:
        raise ValueError(kind)
    return jac_record(row0, col0, *m)


def make_psf(kind, rng):
    """'full' rows (npsf, 6), flux 1; three and more gaussians have components
    off the psf centre; None: no psf"""
    if kind is None:
        return None
    frac = np.array([0.55, 0.25, 0.12, 0.08])[:kind]
    frac = frac / frac.sum()
    rows = np.zeros((kind, 6))
    for i in range(kind):
        sig2 = 0.135 * (1.0 + 0.9 * i)
        rows[i] = [frac[i], 0.0, 0.0, sig2 * (1.0 + 0.05 * i), 0.01 * sig2 * (-1) ** i, sig2]
        if kind >= 2 and i > 0:
            rows[i, 1:3] = rng.uniform(-0.04, 0.04, size=2)
    return rows


def make_weight(kind, shape, noise, rng):
    """(weight map, the kind applied): a stamp that IS one tile gets 'edges'
    where the table asks for 'tile', and is labelled so"""
    nrow, ncol = shape
    w = np.full(shape, 1.0 / noise ** 2)
    if kind == "tile" and nrow <= 8 and ncol <= 8:
        kind = "edges"            # the stamp IS one tile: keep some pixels
    if kind == "random":
        w[rng.uniform(size=shape) < 0.1] = 0.0
    elif kind == "tile":
        r0 = 8 * min(1, (nrow - 1) // 8)
        c0 = 8 * min(1, (ncol - 1) // 8)
        w[r0:r0 + 8, c0:c0 + 8] = 0.0
    elif kind == "edges":
        w[0, :] = 0.0
        w[:, -1] = 0.0
    return w, kind


def pixel_to_vu(jac, row, col):
    rd, cd = row - jac[0], col - jac[1]
    return jac[2] * rd + jac[3] * cd, jac[4] * rd + jac[5] * cd


def _away(rng, lo, hi, size=2):
    """magnitudes in [lo, hi] with random signs"""
    return rng.uniform(lo, hi, size=size) * rng.choice([-1.0, 1.0], size=size)


def shape_pars(model, rng):
    """the parameters between T and the flux(es)"""
    if model == "bdf":
        return [rng.uniform(0.3, 0.7)]
    if model == "bd":
        # (log10 of Td / Te well away from 0: its column is faint and its
        # forward step is sqrt(eps) |x|)
        return [_away(rng, 1.0, 1.5, 1)[0], rng.uniform(0.3, 0.7)]
    return []


def truth_pars(model, rng, nband=1):
    name, ng = model_name(model)
    cen = list(rng.uniform(-0.3, 0.3, size=2) * SCALE)
    g = list(rng.normal(scale=0.1, size=2))
    if name == "coellip":
        # (components of comparable weight: the column of a faint one is a
        # small difference of the whole model's rounding)
        Ts = [0.25, 0.4, 0.65, 1.0, 1.6][:ng]
        Fs = [25.0, 22.0, 20.0, 18.0, 15.0][:ng]
        return np.array(cen + g + Ts + Fs)
    T = rng.uniform(0.3, 0.8)
    return np.array(cen + g + [T] + shape_pars(name, rng) +
                    list(rng.uniform(80.0, 200.0, size=nband)))


def trial_pars(model, truth, kind, stamp_shape, jac, rng, fd=False):
    """a trial point away from the optimum (`truth` made the image).  fd: for a
    forward-difference case, whose step is h_j = sqrt(eps) |x_j| -- no centre
    or shear NEAR 0 (exactly 0 is a case of its own): fdjac2's column then
    divides the rounding of the residuals by a step of 1e-11 and less, and
    the reference is no better than that itself (fd_floor below)"""
    name, ng = model_name(model)
    p = np.array(truth, dtype="f8")
    nrow, ncol = stamp_shape or (0, 0)
    if fd:
        p[0:2] = _away(rng, 0.4, 0.7) * SCALE
        p[2:4] = _away(rng, 0.15, 0.3)
    else:
        p[0:2] += rng.uniform(-0.6, 0.6, size=2) * SCALE
        p[2:4] = rng.uniform(-0.25, 0.25, size=2)
    nT = ng if name == "coellip" else 1
    p[4:4 + nT] *= rng.uniform(0.7, 1.4, size=nT)
    f0 = 4 + ng if name == "coellip" else nloc_of(model) - 1   # the first flux
    p[f0:] *= rng.uniform(0.6, 1.5, size=p.size - f0)
    if kind == "sheared":                     # |g| up to 0.8
        gt = rng.uniform(0.6, 0.8)
        # (fd: both components well away from 0, see above)
        th = (np.pi / 4 + np.pi / 2 * rng.randint(4) + rng.uniform(-0.3, 0.3)) if fd else \
            rng.uniform(0, 2 * np.pi)
        p[2:4] = gt * np.cos(th), gt * np.sin(th)
    elif kind == "small":                     # sigma 0.3 pixel
        p[4:4 + nT] = 2.0 * (0.3 * SCALE) ** 2 * np.linspace(1.0, 2.0, nT)
    elif kind == "wide":                      # sigma 1.5 x the stamp's long side
        p[4:4 + nT] = 2.0 * (1.5 * max(nrow, ncol) * SCALE) ** 2 * np.linspace(1.0, 2.0, nT)
    elif kind == "outside":                   # 3 pixels past a corner of the stamp
        p[0:2] = pixel_to_vu(jac, nrow + 2.3, -3.4)
        p[4:4 + nT] *= 4.0
    elif kind == "far":                       # every pair skipped
        p[0:2] = pixel_to_vu(jac, nrow + 3000.0, ncol + 2000.0)
    elif kind is not None:
        raise ValueError(kind)
    return p


def make_image(model, lpars, psf, shape, jac, noise, rng):
    """truth + noise through the oracle's render"""
    st, _, gmc = make_mixture(model, lpars, psf)
    assert st == ora.OK
    im = np.zeros(shape[0] * shape[1])
    ora.render(gmc, ora.make_coords(shape, _ora_jac(jac)), im, fast_exp=1)
    return im.reshape(shape) + noise * rng.normal(size=shape)


def _stamp(model, truth, band, obj, shape, jk, origin, wk, psf_kind, rng, noise=0.01):
    jac = make_jacobian(jk, shape, origin)
    psf = make_psf(psf_kind, rng)
    image = make_image(model, local_pars(model, truth, band), psf, shape, jac, noise, rng)
    weight, wk = make_weight(wk, shape, noise, rng)
    return {"image": image, "weight": weight, "jac": jac,
            "psf": psf, "band": band, "obj": obj, "shape": shape, "jacobian": jk,
            "weights": wk, "origin": origin}


def _case(name, model, fd, stamps, pars, nband, marks, npsf, seed):
    return {"name": name, "model": model, "fd": fd, "stamps": stamps,
            "pars": np.asarray(pars, dtype="f8"), "nband": nband, "marks": marks,
            "npsf": npsf, "seed": seed}


def analytic_case(model, psf_kind, seed):
    """the ten shapes in one ragged batch, one object per stamp; jacobians,
    origins, weight maps and trial points go round at different strides"""
    rng = np.random.RandomState(seed)
    shift = (ANALYTIC_MODELS.index(model) + 2 * PSFS.index(psf_kind)) % 5
    stamps, pars, marks = [], [], []
    for i, shape in enumerate(ANALYTIC_SHAPES):
        truth = truth_pars(model, rng)
        s = _stamp(model, truth, 0, i, shape, JACOBIANS[i % 4], ORIGINS[(i + i // 3) % 3],
                   WEIGHTS[(i + i // 4 + shift) % 4], psf_kind, rng)
        kind = TRIALS[(i + shift) % 5]
        pars.append(trial_pars(model, truth, kind, shape, s["jac"], rng))
        s["trial"] = kind
        # (a small object skips pairs only on a stamp of several tiles a side)
        marks.append({"small": "some" if max(shape) >= 33 else None, "far": "all",
                      "wide": "none" if model == "gauss" else None}.get(kind))
        stamps.append(s)
    return _case("analytic-%s-psf%s" % (model, psf_kind or 0), model, 0, stamps, pars, 1, marks,
                 psf_kind or 0, seed)


def dev_psf4_case(seed=4100):
    """dev (x) 4 psf gaussians: 40 composed gaussians, the path above 32"""
    rng = np.random.RandomState(seed)
    stamps, pars, marks = [], [], []
    for i, shape in enumerate([(17, 19), (25, 25), (33, 31), (9, 7)]):
        truth = truth_pars("dev", rng)
        s = _stamp("dev", truth, 0, i, shape, JACOBIANS[i], ORIGINS[i % 3], WEIGHTS[(i + 1) % 4],
                   4, rng)
        kind = ["sheared", "small", None, "outside"][i]
        pars.append(trial_pars("dev", truth, kind, shape, s["jac"], rng))
        marks.append("some" if kind == "small" else None)
        stamps.append(s)
    return _case("analytic-dev-psf4", "dev", 0, stamps, pars, 1, marks, 4, seed)


def multiband_case(model, fd, nobj, nband, nepoch, psf_kind, seed, shapes=None):
    """nobj objects x nband bands x nepoch epochs: the stamps of an object are
    contiguous, every object at its own trial point, every band its own flux"""
    rng = np.random.RandomState(seed)
    shapes = shapes or [(17, 19), (25, 25), (9, 7), (16, 16)]
    stamps, pars, k = [], [], 0
    for o in range(nobj):
        truth = truth_pars(model, rng, nband)
        truth[nloc_of(model) - 1:] *= np.linspace(1.0, 2.5, nband)
        for b in range(nband):
            for e in range(nepoch):
                stamps.append(_stamp(model, truth, b, o, shapes[k % len(shapes)],
                                     JACOBIANS[k % 4], ORIGINS[k % 3], WEIGHTS[k % 4], psf_kind,
                                     rng))
                k += 1
        pars.append(trial_pars(model, truth, "sheared" if o == 1 else None, None,
                               stamps[-1]["jac"], rng, fd=bool(fd)))
    return _case("%s-%s-%dx%dx%d-%d" % ("fd" if fd else "analytic", model, nobj, nband, nepoch,
                                        seed),
                 model, fd, stamps, pars, nband, [None] * len(stamps), psf_kind or 0, seed)


def big_gauss_case(seed=264):
    """two 264 x 264 'gauss' stamps: 1089 tiles, more than the records kept in LDS"""
    rng = np.random.RandomState(seed)
    stamps, pars = [], []
    for i in range(2):
        truth = truth_pars("gauss", rng)
        truth[4] = 20.0 + 15.0 * i
        truth[5] = 5000.0
        stamps.append(_stamp("gauss", truth, 0, i, (264, 264), JACOBIANS[i], ORIGINS[i + 1],
                             WEIGHTS[i + 1], 1, rng, noise=0.001))
        pars.append(trial_pars("gauss", truth, None, (264, 264), stamps[-1]["jac"], rng))
    return _case("analytic-gauss-264", "gauss", 0, stamps, pars, 1, [None, None], 1, seed)


def g_range_case(seed=31):
    """five objects, one stamp each; `bad` is the object to push to g >= 1"""
    rng = np.random.RandomState(seed)
    stamps, pars = [], []
    for i, shape in enumerate([(17, 19), (9, 7), (25, 25), (16, 16), (33, 31)]):
        truth = truth_pars("exp", rng)
        stamps.append(_stamp("exp", truth, 0, i, shape, JACOBIANS[i % 4], ORIGINS[i % 3],
                             WEIGHTS[i % 4], 1, rng))
        pars.append(trial_pars("exp", truth, None, shape, stamps[-1]["jac"], rng))
    c = _case("analytic-exp-grange", "exp", 0, stamps, pars, 1, [None] * 5, 1, seed)
    c["bad"] = 2
    c["bad_g"] = (0.8, 0.7)
    return c


def fd_case(model, seed):
    """the five shapes, then three special points: a flux exactly 0, a shape
    parameter exactly 0, a strongly sheared one; the psf goes round over the
    models (none, one gaussian, two and three with components off centre)"""
    rng = np.random.RandomState(seed)
    psf_kind = [None, 1, 2, 3][FD_MODELS.index(model) % 4]
    name, ng = model_name(model)
    nloc = nloc_of(model)
    shapes = FD_SHAPES + [(9, 7), (25, 25), (17, 64)]
    stamps, pars = [], []
    for i, shape in enumerate(shapes):
        truth = truth_pars(model, rng)
        if i == 5:
            # (the image under the flux-0 point is faint: its flux column is
            # ulp(val ierr) / sqrt(eps) away from exact, whoever computes it)
            truth[4 + (ng or 0) if name == "coellip" else nloc - 1:] *= 0.05
        s = _stamp(model, truth, 0, i, shape, JACOBIANS[(i + 1) % 4], ORIGINS[i % 3],
                   WEIGHTS[i % 4], psf_kind, rng)
        p = trial_pars(model, truth, "sheared" if i == 7 else None, shape, s["jac"], rng,
                       fd=True)
        if i == 5:
            p[nloc - 1] = 0.0                  # flux exactly 0 (coellip: the last one)
        if i == 6:
            p[2] = 0.0                         # g1 exactly 0: h = sqrt(eps)
            p[0] = 0.0
        s["special"] = {5: "flux0", 6: "shape0"}.get(i)
        stamps.append(s)
        pars.append(p)
    return _case("fd-%s" % model, model, 1, stamps, pars, 1, [None] * len(stamps),
                 psf_kind or 0, seed)


def analytic_cases():
    out = []
    for m, model in enumerate(ANALYTIC_MODELS):
        for k, psf_kind in enumerate(PSFS):
            out.append((model, psf_kind, 1000 + 10 * m + k))
    return out


def fd_cases():
    return [(model, 2000 + i) for i, model in enumerate(FD_MODELS)]


def fold_cases():
    """(model, fd, nband, nepoch, seed): the fits of the fold-and-step test"""
    return [("exp", 0, 2, 2, 3001), ("bdf", 1, 3, 2, 3002)]


_CACHE = {}


def cached(key, make):
    """cases and references are made once per process and left unchanged"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def get_case(kind, *args):
    makers = {"analytic": analytic_case, "dev4": dev_psf4_case, "multi": multiband_case,
              "big": big_gauss_case, "grange": g_range_case, "fd": fd_case}
    return cached(("case", kind) + args, lambda: makers[kind](*args))


def case_reference(case):
    """stamp_reference of every stamp of a case (cached by the case's name)"""
    def make():
        return [stamp_reference(case["model"],
                                local_pars(case["model"], case["pars"][s["obj"]], s["band"]),
                                s, case["fd"]) for s in case["stamps"]]
    return cached(("ref", case["name"]), make)
