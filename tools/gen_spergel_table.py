#!/usr/bin/env python3
"""
Writes the constant table of ngmix_amd/csrc/spergel_hlr.hpp: the half-light
radius of the Spergel profile in units of its scale radius, c_nu, as a
Chebyshev series of ln c_nu in x = ln(1 + nu) mapped onto [-1, 1], for nu in
[-0.85, 4].

c_nu solves  2 (c/2)^(nu+1) K_(nu+1)(c) / Gamma(nu+1) = 1/2  (the enclosed
flux of the profile at r = c r0 is a half); it is found here with
scipy.special.kv and a bracketing root-finder.  The variable ln(1 + nu) moves
the singularity of ln c_nu at nu = -1 to infinity, which shortens the series.
The series is cut at the shortest length whose error against the root-finder
on a dense grid is below TOL; the achieved error is printed.

    python tools/gen_spergel_table.py            # prints the table's text
    python tools/gen_spergel_table.py --check    # compares it with the header
"""
import argparse
import os
import re

import numpy as np
from numpy.polynomial import chebyshev as C
from scipy import optimize, special

NU_MIN, NU_MAX = -0.85, 4.0
TOL = 1.0e-12
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                      "ngmix_amd", "csrc", "spergel_hlr.hpp")


def enclosed_flux_minus_half(c, nu):
    # 1 - 2 (c/2)^(nu+1) K_(nu+1)(c) / Gamma(nu+1) is the enclosed flux
    return 0.5 - 2.0 * (0.5 * c) ** (nu + 1.0) * special.kv(nu + 1.0, c) / special.gamma(nu + 1.0)


def c_nu(nu):
    """the root, to the root-finder's limit (a few ulp)"""
    return optimize.brentq(enclosed_flux_minus_half, 1.0e-8, 20.0, args=(nu,),
                           xtol=1.0e-300, rtol=4.0 * np.finfo(float).eps, maxiter=500)


XLO, XHI = np.log1p(NU_MIN), np.log1p(NU_MAX)


def to_unit(nu):
    return (2.0 * np.log1p(nu) - (XHI + XLO)) / (XHI - XLO)


def make_series(nmax=96):
    k = np.arange(nmax)
    t = np.cos(np.pi * (k + 0.5) / nmax)                  # Chebyshev nodes
    nu = np.expm1(0.5 * (t * (XHI - XLO) + XHI + XLO))
    y = np.log([c_nu(v) for v in nu])
    return C.chebfit(t, y, nmax - 1)


def series_error(coef, nus, truth):
    got = np.exp(C.chebval(to_unit(nus), coef))
    return np.max(np.abs(got / truth - 1.0))


def shortest(full, nus, truth):
    for n in range(4, full.size + 1):
        err = series_error(full[:n], nus, truth)
        if err < TOL:
            return full[:n], err
    raise SystemExit("no series of %d terms reaches %g" % (full.size, TOL))


def table_text(coef):
    rows = ["    %s," % repr(float(c)) for c in coef]
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    nus = np.concatenate([np.linspace(NU_MIN, NU_MAX, 2001),
                          NU_MIN + (NU_MAX - NU_MIN) * np.random.RandomState(5).rand(500)])
    truth = np.array([c_nu(v) for v in nus])
    coef, err = shortest(make_series(), nus, truth)
    print("// %d terms; max relative error against the root-finder on %d points: %.2e"
          % (coef.size, nus.size, err))
    if args.check:
        text = open(HEADER).read()
        body = re.search(r"SPERGEL_LNC_COEF\[\w*\]\s*=\s*\{(.*?)\};", text, flags=re.S).group(1)
        have = np.array([float(v) for v in re.findall(r"[-+0-9.eE]+", body)])
        ok = have.size == coef.size and np.max(np.abs(have - coef)) < 1e-15
        print("header table %s" % ("matches" if ok else "DIFFERS"))
        raise SystemExit(0 if ok else 1)
    print(table_text(coef))


if __name__ == "__main__":
    main()
