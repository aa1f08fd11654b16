"""
Dense longdouble reference of the Fourier-space gaussian-mixture models 'dev10'
and 'bdf' (DESIGN.md 3.27), written from the pixel-space definition and not
from the kernel:

  components   the mixture GMixModel(pars, 'dev' | 'bdf') builds -- amplitude
               and COVARIANCE MATRIX (irr, irc, icc) of every gaussian -- from
               the tables below, restated here as data (held to the library's
               own by tests/test_kfit_mix_host.py through ngmix_fill_model)
  unit_model   M^ / F = sum a_i exp(-k^T C_i k / 2) exp(-i k.cen) P^n; nothing
               of the kernel's s, t or 1 + g^2 appears
  model        M^ and the jacobian columns by central differences of unit_model
  stamp_sums   J^T J | J^T f | f.f, the statistics and sum |terms|, as
               kfit_reference.stamp_sums forms them
  flux_sums    the three sums of the fixed template

The central differences: the eighth-order stencil
  f'(x) = sum_{m=1..4} c_m (f(x + m h) - f(x - m h)) / h,
  c = 4/5, -1/5, 4/105, -1/280,
whose truncation error is h^8 f^(9) / 630.  Every parameter enters a mode as
exp(-x(par)) or as a phase, so f^(9) / f' <= L^8 with L the logarithmic rate
below, and each MODE takes its own step h = H / L(mode): the relative
truncation is then H^8 / 630 = 4e-25 at H = 2^-7 and the rounding of the
differences 2^-64 / H = 7e-18 of |M^|, both far below the 2^-52 the sums are
held to.  L: |k_v| or |k_u| for the centre; for g1, g2, T and fracdev the
largest exponent x_max = max_i k^T C_i k / 2 of the mode times the parameter's
own rate (4 / (1 - |g|) for g, 1 / T for T, 3 for fracdev, tau's being
|sum_dev p f - sum_exp p f| tau < 1), and at least that rate.
"""
import numpy as np

from helpers import kfit_reference as K

LD = K.LD
CLD = K.CLD
DEV10, BDF = 8, 9
MODEL_ID = {"dev10": DEV10, "bdf": BDF}
NLOC = {DEV10: 6, BDF: 7}
ERR_G_RANGE = K.ERR_G_RANGE
H = LD(2.0) ** -7
STENCIL = (LD(4) / 5, -LD(1) / 5, LD(4) / 105, -LD(1) / 280)

# ngmix's mixture tables (gmix_nb.py): amplitudes p and T fractions f of the
# six gaussians of 'exp' and the ten of 'dev'
EXP_P = [LD(x) for x in (
    "0.00061601229677880041", "0.0079461395724623237", "0.053280454055540001",
    "0.21797364640726541", "0.45496740582554868", "0.26521634184240478")]
EXP_F = [LD(x) for x in (
    "0.002467115141477932", "0.018147435573256168", "0.07944063151366336",
    "0.27137669897479122", "0.79782256866993773", "2.1623306025075739")]
DEV_P = [LD(x) for x in (
    "6.5288960012625658e-05", "0.00044199216814302695", "0.0020859587871659754",
    "0.0075913681418996841", "0.02260266219257237", "0.056532254390212859",
    "0.11939049233042602", "0.20969545753234975", "0.29254151133139222",
    "0.28905301416582552")]
DEV_F = [LD(x) for x in (
    "2.9934935706271918e-07", "3.4651596338231207e-06", "2.4807910570562753e-05",
    "1.4307404300535354e-04", "7.2753169298239500e-04", "3.4582464394427260e-03",
    "1.6086645440719100e-02", "7.7006776775654429e-02", "4.1012562102501476e-01",
    "2.9812509778548648e00")]
# (the doubles the library holds, exactly: the strings above are their digits)
EXP_P, EXP_F, DEV_P, DEV_F = ([LD(float(v)) for v in t] for t in (EXP_P, EXP_F, DEV_P, DEV_F))


def tau_denominator(fd):
    """1 / tau of 'bdf': get_cm_Tfactor's sum at TdByTe = 1"""
    return (1 - fd) * sum(p * f for p, f in zip(EXP_P, EXP_F)) \
        + fd * sum(p * f for p, f in zip(DEV_P, DEV_F))


def components(model_id, g1, g2, T, fd=None, only=None):
    """[(a_i, irr_i, irc_i, icc_i)] of the pixel-space mixture: gaussian i has
    trace T_i = T f_i (tau) and ngmix's covariance at shear g, e = 2 g / (1 +
    g^2): irr = T_i (1 - e1) / 2, irc = T_i e2 / 2, icc = T_i (1 + e1) / 2, row
    = v, col = u.  only='exp': the six exp components of 'bdf' alone"""
    gsq = g1 * g1 + g2 * g2
    e1, e2 = 2 * g1 / (1 + gsq), 2 * g2 / (1 + gsq)
    if model_id == DEV10:
        parts = [(p, T * f) for p, f in zip(DEV_P, DEV_F)]
    else:
        tau = 1 / tau_denominator(fd)
        parts = [((1 - fd) * p, T * f * tau) for p, f in zip(EXP_P, EXP_F)]
        if only != "exp":
            parts += [(fd * p, T * f * tau) for p, f in zip(DEV_P, DEV_F)]
    return [(a, Ti / 2 * (1 - e1), Ti / 2 * e2, Ti / 2 * (1 + e1)) for a, Ti in parts]


def _ld(p):
    return [v if isinstance(v, np.ndarray) else LD(v) for v in p]


def exponents(model_id, p, md):
    """k^T C_i k / 2 of every component at the modes, (ncomp, R, CH)"""
    p = _ld(p)
    comps = components(model_id, p[2], p[3], p[4], p[5] if model_id == BDF else None)
    kv, ku = md["kv"], md["ku"]
    return np.array([(irr * kv * kv + 2 * irc * kv * ku + icc * ku * ku) / 2
                     for _, irr, irc, icc in comps])


def unit_model(model_id, p, md, phat=None, only=None):
    """M^ / F at the local parameters p without the flux, [cen1, cen2, g1, g2,
    T(, fracdev)], each a number or an array over the modes"""
    p = _ld(p)
    kv, ku = md["kv"], md["ku"]
    phi = np.zeros(kv.shape, dtype=LD)
    for a, irr, irc, icc in components(model_id, p[2], p[3], p[4],
                                       p[5] if model_id == BDF else None, only):
        phi = phi + a * np.exp(-(irr * kv * kv + 2 * irc * kv * ku + icc * ku * ku) / 2)
    theta = kv * p[0] + ku * p[1]
    P = np.ones(kv.shape, dtype=CLD) if phat is None else np.asarray(phat, dtype=CLD)
    return phi * np.exp(-1j * theta.astype(CLD)) * P


def out_of_range(model_id, p):
    p = np.asarray(p, dtype=float)
    bad = not np.all(np.isfinite(p)) or not (p[2] ** 2 + p[3] ** 2 < 1.0) or not (p[4] > 0.0)
    if not bad and model_id == BDF:
        bad = tau_denominator(LD(p[5])) == 0
    return bad


def _rates(model_id, p, md):
    """the logarithmic rate L of every differenced parameter at every mode"""
    one = np.ones(md["kv"].shape, dtype=LD)
    xmax = np.maximum(exponents(model_id, p, md).max(axis=0), 1)
    g = LD(np.hypot(float(p[2]), float(p[3])))
    rg = xmax * 4 / (1 - g)
    rates = [np.maximum(np.abs(md["kv"]), one), np.maximum(np.abs(md["ku"]), one), rg, rg,
             xmax / LD(p[4])]
    if model_id == BDF:
        rates.append(3 * xmax)
    return rates


def model(model_id, p, md, phat=None, jac=True):
    """M^ (modes) and, with jac, the nloc complex jacobian columns"""
    p = [LD(v) for v in p]
    F = p[-1]
    unit = unit_model(model_id, p[:-1], md, phat)
    out = {"M": F * unit}
    if not jac:
        return out
    cols = []
    for k, rate in enumerate(_rates(model_id, p, md)):
        # (a power of two: the steps m h are exact)
        h = H / 2 ** np.ceil(np.log2(rate.astype(float))).astype(LD)
        d = np.zeros(unit.shape, dtype=CLD)
        for m, c in enumerate(STENCIL, start=1):
            hi, lo = list(p[:-1]), list(p[:-1])
            hi[k], lo[k] = p[k] + m * h, p[k] - m * h
            d = d + c * (unit_model(model_id, hi, md, phat) - unit_model(model_id, lo, md, phat))
        cols.append(F * d / h)
    cols.append(unit)
    out["cols"] = cols
    return out


def stamp_sums(model_id, p, md, dhat, phat, wbar, mode_weight=None):
    """the stamp's sums [J^T J triangle | J^T f | f.f], stats (sum w Re(M D*),
    sum w |M|^2), the sum of the absolute values of the terms of each --
    products taken BEFORE the subtraction M^ - D^ --, and with mode_weight
    (R, CH) the components that enter dof"""
    nloc = NLOC[model_id]
    ns = K.nsums(nloc)
    mult = md["mult"] if mode_weight is None else md["mult"] * np.asarray(mode_weight, dtype=LD)
    ncomp = int(md["mult"][mult > 0].sum())
    if out_of_range(model_id, p):
        z = np.zeros(ns, dtype=LD)
        z[-1] = np.inf
        return {"sums": z, "abs": np.zeros(ns, dtype=LD), "stats": np.zeros(2, dtype=LD),
                "stats_abs": np.zeros(2, dtype=LD), "status": ERR_G_RANGE, "ncomp": ncomp}
    m = model(model_id, p, md, phat)
    keep = mult > 0
    w = (LD(wbar) / (md["R"] * md["C"])) * mult[keep]
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
            "status": 0, "M": m["M"], "ncomp": ncomp}


def flux_sums(model_id, pars, md, dhat, phat, wbar, mode_weight=None):
    """A = sum w Re(T^* D^), B = sum w |T^|^2, E = sum w |D^|^2 of the unit-flux
    template at pars [cen1, cen2, g1, g2, T(, fracdev)], and sum |terms|"""
    T = unit_model(model_id, pars, md, phat)
    mult = md["mult"] if mode_weight is None else md["mult"] * np.asarray(mode_weight, dtype=LD)
    keep = mult > 0
    w = (LD(wbar) / (md["R"] * md["C"])) * mult[keep]
    T = T[keep]
    D = np.asarray(dhat, dtype=CLD)[keep]
    rr, ii = T.real * D.real, T.imag * D.imag
    A = np.sum(w * (rr + ii))
    aA = np.sum(w * (np.abs(rr) + np.abs(ii)))
    B = np.sum(w * np.abs(T) ** 2)
    E = np.sum(w * np.abs(D) ** 2)
    return np.array([A, B, E], dtype=LD), np.array([aA, B, E], dtype=LD)


def model_image(model_id, p, md, phat=None):
    """the real-space image of the band-limited, periodic model by the inverse
    of dense_transform about the jacobian centre md['cen']"""
    R, C = md["R"], md["C"]
    M = model(model_id, p, md, phat, jac=False)["M"]
    r0, c0 = md["cen"]
    shift = np.exp(-1j * (md["qr"] * LD(r0) + md["qc"] * LD(c0)).astype(CLD))
    return np.fft.irfft2((M * shift).astype(complex), s=(R, C))
