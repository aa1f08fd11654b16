"""
Dense longdouble reference of the Fourier-space profile fits,
written from the definition and not from the kernel:

  modes           the rfft2 half plane of an R x C stamp, its world frequencies
                  and Parseval multiplicities
  dense_transform sum_pixels I exp(-i q.(x - cen)), pixel by pixel
  model           M^ and its analytic jacobian from the EXPANDED quadratic form
                  of s and logarithmic derivatives (the kernel differentiates
                  the factored form and carries real multiples of G)
  stamp_sums      J^T J | J^T f | f.f, the two statistics, and sum |terms| of
                  every entry for the rounding bound
  c_nu            the Spergel half-light radius by root-finding
"""
import functools

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
GAUSS, EXP, SPERGEL = 0, 1, 2
MODEL_ID = {"gauss": GAUSS, "exp": EXP, "spergel": SPERGEL}
NLOC = {GAUSS: 6, EXP: 6, SPERGEL: 7}
PI = LD("3.14159265358979323846264338327950288")
HLR_GAUSS = np.sqrt(2 * np.log(LD(2)))
HLR_EXP = LD("1.6783469900166605")
NU_MIN, NU_MAX = -0.85, 4.0
R50_MIN = 1.0e-4
ERR_G_RANGE, ERR_NOT_FINITE = 3, 8


def nsums(nloc):
    return nloc * (nloc + 1) // 2 + nloc + 1


# ---- the Spergel half-light radius ------------------------------------------------

def _enclosed_minus_half(c, nu):
    from scipy import special
    return 0.5 - 2.0 * (0.5 * c) ** (nu + 1.0) * special.kv(nu + 1.0, c) / special.gamma(nu + 1.0)


@functools.lru_cache(maxsize=None)
def c_nu(nu):
    """c solving 2 (c/2)^(nu+1) K_(nu+1)(c) / Gamma(nu+1) = 1/2, by bracketing"""
    from scipy import optimize
    return optimize.brentq(_enclosed_minus_half, 1.0e-8, 20.0, args=(float(nu),),
                           xtol=1e-300, rtol=4 * np.finfo(float).eps, maxiter=500)


def dc_dnu_central(nu, h):
    """central difference of the root; the ends of the range use a one-sided
    second-order stencil"""
    if nu - h < NU_MIN:
        return (-3 * c_nu(nu) + 4 * c_nu(nu + h) - c_nu(nu + 2 * h)) / (2 * h)
    if nu + h > NU_MAX:
        return (3 * c_nu(nu) - 4 * c_nu(nu - h) + c_nu(nu - 2 * h)) / (2 * h)
    return (c_nu(nu + h) - c_nu(nu - h)) / (2 * h)


# ---- geometry -------------------------------------------------------------------

JACOBIANS = {
    # (dvdrow, dvdcol, dudrow, dudcol)
    "diag": (0.8, 0.0, 0.0, 0.8),
    "rotflip": (0.31, 0.74, 0.69, -0.36),       # det < 0
    "aniso": (1.1, 0.12, -0.07, 0.62),
}


def modes(R, C, deriv):
    """a, b, q_r, q_c, k_v, k_u, mult of the stored modes, each (R, C//2+1)"""
    dvdrow, dvdcol, dudrow, dudcol = (LD(x) for x in deriv)
    CH = C // 2 + 1
    a = np.arange(R)[:, None] * np.ones(CH, dtype=int)[None, :]
    b = np.ones(R, dtype=int)[:, None] * np.arange(CH)[None, :]
    fa = np.where(2 * a < R, a, a - R).astype(LD)
    qr = 2 * PI * fa / R
    qc = 2 * PI * b.astype(LD) / C
    det = dvdrow * dudcol - dvdcol * dudrow
    # (k_v, k_u) = J^-T q,  J = [[dvdrow, dvdcol], [dudrow, dudcol]]
    kv = (dudcol * qr - dudrow * qc) / det
    ku = (-dvdcol * qr + dvdrow * qc) / det
    mult = np.where(b == 0, 1.0, 2.0)
    if R % 2 == 0:
        mult = np.where(2 * a == R, 0.0, mult)
    if C % 2 == 0:
        mult = np.where(2 * b == C, 0.0, mult)
    return {"a": a, "b": b, "qr": qr, "qc": qc, "kv": kv, "ku": ku, "mult": mult.astype(LD),
            "det": det, "R": R, "C": C}


def dense_transform(img, cen, md):
    """sum I[r, c] exp(-i (q_r (r - r0) + q_c (c - c0))) at the modes md, the
    stamp placed anywhere on the grid the modes belong to (zero padding)"""
    img = np.asarray(img, dtype=LD)
    out = np.zeros(md["qr"].shape, dtype=CLD)
    rr = np.arange(img.shape[0]).astype(LD) - LD(cen[0])
    cc = np.arange(img.shape[1]).astype(LD) - LD(cen[1])
    for i in range(img.shape[0]):
        er = np.exp(-1j * (md["qr"] * rr[i]).astype(CLD))
        row = np.zeros(md["qr"].shape, dtype=CLD)
        for j in range(img.shape[1]):
            row += img[i, j] * np.exp(-1j * (md["qc"] * cc[j]).astype(CLD))
        out += er * row
    return out


# ---- the model ------------------------------------------------------------------

def out_of_range(model, p):
    p = np.asarray(p, dtype=float)
    bad = not (p[2] ** 2 + p[3] ** 2 < 1.0) or not (p[4] >= R50_MIN)
    if model == SPERGEL:
        bad = bad or not (NU_MIN <= p[5] <= NU_MAX)
    return bad


def model(model_id, p, md, phat=None, c=None, dc=None, jac=True):
    """M^ (modes) and, with jac, the nloc complex jacobian columns.  p: the
    local parameters [cen1, cen2, g1, g2, r50, (nu,) F].  c, dc: c_nu and its
    derivative when the caller fixes them (the sums tests hand over the
    library's own table values, held to the root-finder elsewhere); else the
    root-finder and its central difference."""
    p = [LD(x) for x in p]
    cen1, cen2, g1, g2, r50 = p[:5]
    F = p[-1]
    nu = p[5] if model_id == SPERGEL else LD(0.5)
    if model_id == GAUSS:
        cc, dcc = HLR_GAUSS, LD(0)
    elif model_id == EXP:
        cc, dcc = HLR_EXP, LD(0)
    else:
        cc = LD(c_nu(float(nu))) if c is None else LD(c)
        dcc = LD(dc_dnu_central(float(nu), 1e-4)) if dc is None else LD(dc)
    kv, ku = md["kv"], md["ku"]
    r0 = r50 / cc
    D = 1 - g1 * g1 - g2 * g2
    # the quadratic form of the sheared frequency, expanded
    N = ku * ku * ((1 + g1) ** 2 + g2 * g2) + kv * kv * ((1 - g1) ** 2 + g2 * g2) \
        + 4 * g2 * ku * kv
    s = r0 * r0 * N / D
    if model_id == GAUSS:
        phi = np.exp(-s / 2)
        dlnphi = -LD(0.5) * np.ones_like(s)
    elif model_id == EXP:
        phi = (1 + s) ** LD(-1.5)
        dlnphi = -LD(1.5) / (1 + s)
    else:
        phi = np.exp(-(1 + nu) * np.log1p(s))
        dlnphi = -(1 + nu) / (1 + s)
    theta = kv * cen1 + ku * cen2
    P = np.ones(s.shape, dtype=CLD) if phat is None else np.asarray(phat, dtype=CLD)
    unit = phi * np.exp(-1j * theta.astype(CLD)) * P     # M^ / F
    M = F * unit
    out = {"M": M, "s": s, "theta": theta}
    if not jac:
        return out
    dN1 = 2 * (1 + g1) * ku * ku - 2 * (1 - g1) * kv * kv
    dN2 = 2 * g2 * (ku * ku + kv * kv) + 4 * ku * kv
    ds1 = r0 * r0 * (dN1 / D + 2 * g1 * N / (D * D))
    ds2 = r0 * r0 * (dN2 / D + 2 * g2 * N / (D * D))
    cols = [(-1j * kv.astype(CLD)) * M, (-1j * ku.astype(CLD)) * M,
            (dlnphi * ds1) * M, (dlnphi * ds2) * M, (dlnphi * 2 * s / r50) * M]
    if model_id == SPERGEL:
        cols.append((-np.log1p(s) + dlnphi * s * (-2 * dcc / cc)) * M)
    cols.append(unit)
    out["cols"] = cols
    return out


def stamp_sums(model_id, p, md, dhat, phat, wbar, c=None, dc=None):
    """the stamp's sums [J^T J triangle | J^T f | f.f], stats (sum w Re(M D*),
    sum w |M|^2), and for each of them the sum of the absolute values of the
    terms it is made of -- products taken BEFORE the subtraction M^ - D^, which
    is where the kernel's roundings are"""
    nloc = NLOC[model_id]
    ns = nsums(nloc)
    if out_of_range(model_id, p):
        z = np.zeros(ns, dtype=LD)
        z[-1] = np.inf
        return {"sums": z, "abs": np.zeros(ns, dtype=LD), "stats": np.zeros(2, dtype=LD),
                "stats_abs": np.zeros(2, dtype=LD), "status": ERR_G_RANGE}
    m = model(model_id, p, md, phat, c, dc)
    keep = md["mult"] > 0
    w = (LD(wbar) / (md["R"] * md["C"])) * md["mult"][keep]
    M = m["M"][keep]
    Dh = np.asarray(dhat, dtype=CLD)[keep]
    cols = [col[keep] for col in m["cols"]]
    f = M - Dh
    sums, absum = [], []
    for i in range(nloc):
        for j in range(i, nloc):
            rr, ii = cols[i].real * cols[j].real, cols[i].imag * cols[j].imag
            sums.append(np.sum(w * (rr + ii)))
            absum.append(np.sum(w * (np.abs(rr) + np.abs(ii))))
    for i in range(nloc):
        sums.append(np.sum(w * (cols[i].real * f.real + cols[i].imag * f.imag)))
        absum.append(np.sum(w * (np.abs(cols[i].real) * (np.abs(M.real) + np.abs(Dh.real))
                                 + np.abs(cols[i].imag) * (np.abs(M.imag) + np.abs(Dh.imag)))))
    sums.append(np.sum(w * (f.real ** 2 + f.imag ** 2)))
    absum.append(np.sum(w * ((np.abs(M.real) + np.abs(Dh.real)) ** 2
                             + (np.abs(M.imag) + np.abs(Dh.imag)) ** 2)))
    mm = np.sum(w * np.abs(M) ** 2)
    md_ = np.sum(w * (M.real * Dh.real + M.imag * Dh.imag))
    amd = np.sum(w * np.abs(M) * (np.abs(M) + np.abs(Dh))) + mm
    return {"sums": np.array(sums, dtype=LD), "abs": np.array(absum, dtype=LD),
            "stats": np.array([md_, mm], dtype=LD), "stats_abs": np.array([amd, mm], dtype=LD),
            "status": 0, "M": m["M"]}


def model_image(model_id, p, md, phat=None):
    """the real-space image of the band-limited, periodic model by the inverse of
    dense_transform about the jacobian centre `md['cen']`"""
    R, C = md["R"], md["C"]
    M = model(model_id, p, md, phat, jac=False)["M"]
    r0, c0 = md["cen"]
    shift = np.exp(-1j * (md["qr"] * LD(r0) + md["qc"] * LD(c0)).astype(CLD))
    return np.fft.irfft2((M * shift).astype(complex), s=(R, C))


# ---- what the tests hand to the entry points ----------------------------------------

def interleaved(z):
    """complex (..., R, CH) -> float64 (..., R, CH, 2)"""
    z = np.asarray(z)
    return np.ascontiguousarray(np.stack([z.real.astype(np.float64), z.imag.astype(np.float64)],
                                         axis=-1))


def from_interleaved(x):
    x = np.asarray(x)
    return x[..., 0].astype(LD) + 1j * x[..., 1].astype(LD)


def gauss_image(shape, cen, deriv, pars):
    """a sampled elliptical gaussian as ngmix renders one -- the density times
    the pixel area, so that the pixels sum to the flux: pars = (v0, u0, g1, g2,
    T, flux), ngmix's T = irr + icc with e = 2 g / (1 + g^2)"""
    v0, u0, g1, g2, T, flux = (LD(x) for x in pars)
    dvdrow, dvdcol, dudrow, dudcol = (LD(x) for x in deriv)
    r = np.arange(shape[0]).astype(LD)[:, None] - LD(cen[0])
    c = np.arange(shape[1]).astype(LD)[None, :] - LD(cen[1])
    v = dvdrow * r + dvdcol * c - v0
    u = dudrow * r + dudcol * c - u0
    gsq = g1 * g1 + g2 * g2
    e1, e2 = 2 * g1 / (1 + gsq), 2 * g2 / (1 + gsq)
    irr, irc, icc = T / 2 * (1 - e1), T / 2 * e2, T / 2 * (1 + e1)
    det = irr * icc - irc * irc
    chi2 = (icc * v * v - 2 * irc * v * u + irr * u * u) / det
    area = abs(dvdrow * dudcol - dvdcol * dudrow)
    return flux * area * np.exp(-chi2 / 2) / (2 * PI * np.sqrt(det))
