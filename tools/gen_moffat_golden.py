#!/usr/bin/env python
"""
Writes the two fixtures of the Moffat Fourier-space fits with
mpmath at 40 digits:

  tests/golden/moffat_phi.npz   nu, x, Phi, D_x = x dPhi/dx, D_nu = dPhi/dnu on
      the grid nu x x below, and three values on either side of moffat_phi.hpp's
      one switch point in x > 0 (MOFFAT_X_TINY = 1e-10)
  tests/golden/kfit_moffat.npz  the evaluation cases of tests/test_kfit_moffat_host.py
      -- their inputs (made by tests/helpers/kfit_cases.make_stamp) and their
      expected sums in the ngmix_lm_eval_batch layout, the two statistics and
      sum |terms| of each, all summed in mpmath from the definition (the
      expanded quadratic form of s, logarithmic derivatives)

    python tools/gen_moffat_golden.py [--phi-only]

The tests read the fixtures and never mpmath.
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")

mp.mp.dps = 40

NUS = [0.1, 0.3, 0.5, 0.999, 1, 1.001, 1.5, 2, 2.5, 3.7, 5]
XS = [0, 1e-8, 1e-3, 0.1, 0.5, 1, 2, 5, 20, 100, 700, 800]
X_TINY = 1e-10
XS_SWITCH = [0.5 * X_TINY, 0.9 * X_TINY, X_TINY * (1 - 2.0 ** -52), X_TINY,
             1.1 * X_TINY, 2 * X_TINY]

MOFFAT, MOFFAT_FWHM = 3, 4
SHAPES = [((8, 8), None), ((8, 8), (8, 8)), ((9, 12), None), ((9, 12), (7, 7)),
          ((16, 16), None), ((16, 16), (7, 7))]
BETAS = [1.3, 2.5, 4.5]


def phi3(nu, x):
    """Phi, D_x, D_nu of the Moffat transform at (nu, x), mpf"""
    nu, x = mp.mpf(nu), mp.mpf(x)
    if x == 0:
        return mp.mpf(1), mp.mpf(0), mp.mpf(0)
    pref = mp.mpf(2) ** (1 - nu) / mp.gamma(nu)
    k = mp.besselk(nu, x)
    phi = pref * x ** nu * k
    dx = -pref * x ** (nu + 1) * mp.besselk(nu - 1, x)
    dk = mp.diff(lambda n: mp.besselk(n, x), nu)
    dnu = phi * (mp.log(x / 2) - mp.digamma(nu)) + pref * x ** nu * dk
    return phi, dx, dnu


def write_phi():
    rows = []
    for nu in NUS:
        for x in XS + XS_SWITCH:
            rows.append((float(nu), float(x)) + tuple(float(v) for v in phi3(float(nu), float(x))))
    a = np.array(rows)
    np.savez(os.path.join(GOLDEN, "moffat_phi.npz"), nu=a[:, 0], x=a[:, 1], phi=a[:, 2],
             dx=a[:, 3], dnu=a[:, 4])
    print("moffat_phi.npz: %d points" % len(a))


def size_factor(model, beta):
    """c = size / r_d and d ln c / d beta"""
    b = beta - 1 if model == MOFFAT else beta
    em = mp.mpf(2) ** (1 / b) - 1
    c = (1 if model == MOFFAT else 2) * mp.sqrt(em)
    return c, -mp.log(2) * (1 + em) / (2 * b * b * em)


def expected(model, p, deriv, R, C, dhat, phat, wbar):
    """sums, sum |terms|, stats, sum |terms| of the stats: K.stamp_sums in mpmath"""
    cen1, cen2, g1, g2, size, beta, F = (mp.mpf(float(v)) for v in p)
    dvdrow, dvdcol, dudrow, dudcol = (mp.mpf(float(v)) for v in deriv)
    det = dvdrow * dudcol - dvdcol * dudrow
    c, dlnc = size_factor(model, beta)
    rd = size / c
    D = 1 - g1 * g1 - g2 * g2
    CH = C // 2 + 1
    cols, Ms, Ds, ws = [], [], [], []
    for a in range(R):
        for b in range(CH):
            if (R % 2 == 0 and 2 * a == R) or (C % 2 == 0 and 2 * b == C):
                continue
            qr = 2 * mp.pi * (a if 2 * a < R else a - R) / R
            qc = 2 * mp.pi * b / C
            kv = (dudcol * qr - dudrow * qc) / det
            ku = (-dvdcol * qr + dvdrow * qc) / det
            N = ku * ku * ((1 + g1) ** 2 + g2 * g2) + kv * kv * ((1 - g1) ** 2 + g2 * g2) \
                + 4 * g2 * ku * kv
            s = rd * rd * N / D
            phi, dx, dnu = phi3(beta - 1, mp.sqrt(s))
            if N == 0:
                dl1 = dl2 = mp.mpf(0)
            else:
                dl1 = (2 * (1 + g1) * ku * ku - 2 * (1 - g1) * kv * kv) / N + 2 * g1 / D
                dl2 = (2 * g2 * (ku * ku + kv * kv) + 4 * ku * kv) / N + 2 * g2 / D
            P = mp.mpc(1) if phat is None else mp.mpc(float(phat[a, b, 0]), float(phat[a, b, 1]))
            G = mp.expj(-(kv * cen1 + ku * cen2)) * P
            M = F * phi * G
            half = dx / 2                               # s dPhi/ds
            cols.append([-1j * kv * M, -1j * ku * M, F * half * dl1 * G, F * half * dl2 * G,
                         F * half * (2 / size) * G, F * (dnu - half * 2 * dlnc) * G, phi * G])
            Ms.append(M)
            Ds.append(mp.mpc(float(dhat[a, b, 0]), float(dhat[a, b, 1])))
            ws.append(mp.mpf(float(wbar)) / (R * C) * (1 if b == 0 else 2))
    n = 7
    sums, absum = [], []
    for i in range(n):
        for j in range(i, n):
            rr = [w * (q[i].real * q[j].real) for w, q in zip(ws, cols)]
            ii = [w * (q[i].imag * q[j].imag) for w, q in zip(ws, cols)]
            sums.append(mp.fsum(rr) + mp.fsum(ii))
            absum.append(mp.fsum(abs(v) for v in rr) + mp.fsum(abs(v) for v in ii))
    for i in range(n):
        sums.append(mp.fsum(w * (q[i].real * (M.real - d.real) + q[i].imag * (M.imag - d.imag))
                            for w, q, M, d in zip(ws, cols, Ms, Ds)))
        absum.append(mp.fsum(w * (abs(q[i].real) * (abs(M.real) + abs(d.real))
                                  + abs(q[i].imag) * (abs(M.imag) + abs(d.imag)))
                             for w, q, M, d in zip(ws, cols, Ms, Ds)))
    sums.append(mp.fsum(w * ((M.real - d.real) ** 2 + (M.imag - d.imag) ** 2)
                        for w, M, d in zip(ws, Ms, Ds)))
    absum.append(mp.fsum(w * ((abs(M.real) + abs(d.real)) ** 2 + (abs(M.imag) + abs(d.imag)) ** 2)
                         for w, M, d in zip(ws, Ms, Ds)))
    mm = mp.fsum(w * abs(M) ** 2 for w, M in zip(ws, Ms))
    md = mp.fsum(w * (M.real * d.real + M.imag * d.imag) for w, M, d in zip(ws, Ms, Ds))
    amd = mp.fsum(w * abs(M) * (abs(M) + abs(d)) for w, M, d in zip(ws, Ms, Ds)) + mm
    f = lambda v: np.array([float(t) for t in v])
    return f(sums), f(absum), f([md, mm]), f([amd, mm])


def write_kfit():
    from helpers import kfit_cases as KC
    from helpers import kfit_reference as K
    stamps = []
    seed = 3000
    for shape, psf_shape in SHAPES:
        for jname in K.JACOBIANS:
            for beta in BETAS:
                for model in (MOFFAT, MOFFAT_FWHM):
                    seed += 1
                    gmag = 0.6 if (jname == "aniso" and beta == 2.5) else None
                    st = KC.make_stamp(shape, jname, ("spergel", beta), psf_shape, seed, gmag=gmag)
                    st["model"] = model
                    stamps.append(st)
    # one object of 2 bands x 2 epochs: shared shape parameters, a flux per band
    mb = [KC.make_stamp((16, 16), ("diag", "aniso")[e], ("spergel", 2.5), (7, 7),
                        3900 + 2 * band + e, band=band) for band in range(2) for e in range(2)]
    pars = np.concatenate([mb[0]["p"][:6], [55.0, 31.0]])
    for st in mb:
        st["model"] = MOFFAT
        st["p"] = np.concatenate([pars[:6], [pars[6 + st["band"]]]])
        st["obj"] = 1
    stamps += mb
    out = {"n": np.array(len(stamps))}
    meta = np.zeros((len(stamps), 8))            # R, C, model, with psf, band, multiband, wbar, -
    for i, st in enumerate(stamps):
        R, C = st["shape"]
        meta[i] = R, C, st["model"], st["phat"] is not None, st["band"], st["obj"], st["wbar"], 0
        out["dhat%d" % i] = st["dhat"]
        if st["phat"] is not None:
            out["phat%d" % i] = st["phat"]
        out["jac%d" % i] = st["jac"].view(np.float64)
        out["p%d" % i] = st["p"]
        s, a, t, ta = expected(st["model"], st["p"], st["deriv"], R, C, st["dhat"], st["phat"],
                               st["wbar"])
        out["sums%d" % i], out["abs%d" % i], out["stats%d" % i], out["stats_abs%d" % i] = s, a, t, ta
        print("kfit_moffat.npz: stamp %d / %d" % (i + 1, len(stamps)), flush=True)
    out["meta"] = meta
    np.savez_compressed(os.path.join(GOLDEN, "kfit_moffat.npz"), **out)


if __name__ == "__main__":
    write_phi()
    if "--phi-only" not in sys.argv:
        write_kfit()
