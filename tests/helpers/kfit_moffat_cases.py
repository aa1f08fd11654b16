"""
The cases the host and GPU tests of the Moffat Fourier-space fits and of the
template fluxes share: the stamps of tests/golden/kfit_moffat.npz
with their expected sums (mpmath, tools/gen_moffat_golden.py), the glue that
calls the entry points on them, and a dense longdouble restatement of the three
flux sums.  Loaded once per process and left unchanged.
"""
import functools
import os

import numpy as np

from ngmix_amd import _lib

from helpers import kfit_cases as KC
from helpers import kfit_reference as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "golden")
MOFFAT, MOFFAT_FWHM, POINT = 3, 4, -1
NLOC = 7
NSUMS = K.nsums(NLOC)
EPS = 2.0 ** -52
# Gates, from the measurements recorded in DESIGN.md 3.25 (host twin, x86-64):
#   moffat_phi against the fixture: 8 x the measured maximum, rounded up to one
#   digit (measured 1.7e-14, 4.4e-16, 2.6e-14; caps 1e-12, 1e-12, 1e-8)
PHI_GATES = (2e-13, 4e-15, 3e-13)
#   the evaluation's sums in units of 2^-52 sum |terms|: the next round figure
#   above 4 x the measured worst.  Entries without the beta column: measured
#   14.5 (statistics 9.2).  Entries with it: measured 942 -- D_nu
#   is held to an ABSOLUTE error (a few 1e-15), and where Phi is close to 1 it
#   is small against the two terms it is the sum of
C_ROUND = 60.0
C_ROUND_BETA = 4000.0
BETA_ENTRIES = np.array([5 in (i, j) for i in range(NLOC) for j in range(i, NLOC)]
                        + [i == 5 for i in range(NLOC)] + [False])
#   the flux sums against the dense restatement: the issue's 64
C_FLUX = 64.0


@functools.lru_cache(maxsize=None)
def phi_fixture():
    g = np.load(os.path.join(GOLDEN, "moffat_phi.npz"))
    return {k: np.ascontiguousarray(g[k]) for k in ("nu", "x", "phi", "dx", "dnu")}


@functools.lru_cache(maxsize=None)
def stamps():
    """every stamp of the fixture: the dict of kfit_cases.make_stamp (without the
    image) plus 'ref', the expected sums, statistics and their sum |terms|"""
    g = np.load(os.path.join(GOLDEN, "kfit_moffat.npz"))
    out = []
    for i in range(int(g["n"])):
        R, C, model, has_psf, band, obj, wbar, _ = g["meta"][i]
        jac = np.ascontiguousarray(g["jac%d" % i]).view(_lib.JACOBIAN_DTYPE)
        deriv = tuple(float(jac[k][0]) for k in ("dvdrow", "dvdcol", "dudrow", "dudcol"))
        md = K.modes(int(R), int(C), deriv)
        md["cen"] = (float(jac["row0"][0]), float(jac["col0"][0]))
        out.append({
            "shape": (int(R), int(C)), "model": int(model), "band": int(band), "obj": int(obj),
            "wbar": float(wbar), "jac": jac, "deriv": deriv, "md": md,
            "dhat": np.ascontiguousarray(g["dhat%d" % i]),
            "phat": np.ascontiguousarray(g["phat%d" % i]) if has_psf else None,
            "p": np.array(g["p%d" % i]),
            "ref": {"sums": g["sums%d" % i].astype(K.LD), "abs": g["abs%d" % i].astype(K.LD),
                    "stats": g["stats%d" % i].astype(K.LD),
                    "stats_abs": g["stats_abs%d" % i].astype(K.LD)},
        })
    return out


def groups():
    """{(model, shape, with psf): [stamps]} of the single-stamp cases"""
    out = {}
    for st in stamps():
        if st["obj"] == 0:
            out.setdefault((st["model"], st["shape"], st["phat"] is not None), []).append(st)
    return out


def multiband():
    sts = [st for st in stamps() if st["obj"] == 1]
    pars = np.concatenate([sts[0]["p"][:6], [0.0, 0.0]])
    for st in sts:
        pars[6 + st["band"]] = st["p"][6]
    return sts, pars


def eval_host(sts, states, model=None, stamp_obj=None, stamp_band=None, sums=None):
    """ngmix_kfit_eval_host on stamps of one shape: sums, status, stats"""
    dhat, phat, wbar, jac = KC.pack_stamps(sts)
    R, C = sts[0]["shape"]
    n = len(sts)
    if sums is None:
        sums = np.full((n, NSUMS), np.nan)
    status = np.full(n, -7, dtype=np.int32)
    stats = np.full((n, 2), np.nan)
    so = None if stamp_obj is None else np.ascontiguousarray(stamp_obj, dtype=np.int32)
    sb = None if stamp_band is None else np.ascontiguousarray(stamp_band, dtype=np.int32)
    rc = _lib.lib().ngmix_kfit_eval_host(
        _lib.ptr(dhat), None if phat is None else _lib.ptr(phat), _lib.ptr(wbar), _lib.ptr(jac),
        R, C, n, sts[0]["model"] if model is None else model, _lib.ptr(states),
        None if so is None else _lib.ptr(so), None if sb is None else _lib.ptr(sb),
        _lib.ptr(sums), _lib.ptr(status), _lib.ptr(stats))
    assert rc == 0, _lib.last_error()
    return sums, status, stats


def flux_host(sts, model, pars):
    """ngmix_kfit_flux_host on stamps of one shape: out (n, 3), status"""
    dhat, phat, wbar, jac = KC.pack_stamps(sts)
    R, C = sts[0]["shape"]
    n = len(sts)
    pars = np.ascontiguousarray(pars, dtype=np.float64)
    out = np.full((n, 3), np.nan)
    status = np.full(n, -7, dtype=np.int32)
    rc = _lib.lib().ngmix_kfit_flux_host(
        _lib.ptr(dhat), None if phat is None else _lib.ptr(phat), _lib.ptr(wbar), _lib.ptr(jac),
        R, C, n, model, _lib.ptr(pars), _lib.ptr(out), _lib.ptr(status))
    assert rc == 0, _lib.last_error()
    return out, status


def library_moffat_phi(nu, x):
    nu = np.ascontiguousarray(np.broadcast_to(nu, np.shape(x)), dtype=np.float64).ravel()
    xx = np.ascontiguousarray(x, dtype=np.float64).ravel()
    out = np.zeros((xx.size, 3))
    assert _lib.lib().ngmix_moffat_phi_host(_lib.ptr(nu), _lib.ptr(xx), xx.size,
                                            _lib.ptr(out)) == 0
    return out.reshape(np.shape(x) + (3,))


def moffat_size_factor(model, beta):
    b = beta - 1.0 if model == MOFFAT else beta
    return (1.0 if model == MOFFAT else 2.0) * np.sqrt(np.expm1(np.log(K.LD(2)) / K.LD(b)))


def template(st, model, pars):
    """the unit-flux template T^ = Phi exp(-i k.cen) P^n at the stored modes, in
    longdouble from the definition; the Moffat Phi is the library's own, held
    to its fixture elsewhere"""
    md = st["md"]
    phat = None if st["phat"] is None else K.from_interleaved(st["phat"])
    if model == POINT:
        theta = md["kv"] * K.LD(pars[0]) + md["ku"] * K.LD(pars[1])
        P = np.ones(theta.shape, dtype=K.CLD) if phat is None else phat
        return np.exp(-1j * theta.astype(K.CLD)) * P
    if model in (K.GAUSS, K.EXP, K.SPERGEL):
        # (the Spergel c_nu is the library's table value, as in kfit_cases.reference)
        c = KC.library_hlr(pars[5])[0] if model == K.SPERGEL else None
        return K.model(model, list(pars) + [1.0], md, phat, c=c, dc=0.0, jac=False)["M"]
    cen1, cen2, g1, g2, size, beta = (K.LD(v) for v in pars)
    rd = size / moffat_size_factor(model, float(beta))
    kv, ku = md["kv"], md["ku"]
    N = ku * ku * ((1 + g1) ** 2 + g2 * g2) + kv * kv * ((1 - g1) ** 2 + g2 * g2) \
        + 4 * g2 * ku * kv
    s = rd * rd * N / (1 - g1 * g1 - g2 * g2)
    phi = library_moffat_phi(float(beta) - 1.0, np.sqrt(s).astype(np.float64))[..., 0].astype(K.LD)
    P = np.ones(s.shape, dtype=K.CLD) if phat is None else phat
    return phi * np.exp(-1j * (kv * cen1 + ku * cen2).astype(K.CLD)) * P


def flux_sums(st, model, pars):
    """A = sum w Re(T^* D^), B = sum w |T^|^2, E = sum w |D^|^2 and sum |terms|"""
    md = st["md"]
    T = template(st, model, pars)
    keep = md["mult"] > 0
    w = (K.LD(st["wbar"]) / (md["R"] * md["C"])) * md["mult"][keep]
    T = T[keep]
    D = K.from_interleaved(st["dhat"])[keep]
    rr, ii = T.real * D.real, T.imag * D.imag
    A = np.sum(w * (rr + ii))
    aA = np.sum(w * (np.abs(rr) + np.abs(ii)))
    B = np.sum(w * np.abs(T) ** 2)
    E = np.sum(w * np.abs(D) ** 2)
    return np.array([A, B, E], dtype=K.LD), np.array([aA, B, E], dtype=K.LD)


def worst_ratios(got, ref):
    """the worst error of a stamp's sums in units of 2^-52 sum |terms|: over the
    entries without the beta column, over those with it, over the statistics"""
    sums, stats = got
    plain = KC.worst_ratio(sums[~BETA_ENTRIES], ref["sums"][~BETA_ENTRIES],
                           ref["abs"][~BETA_ENTRIES])
    beta = KC.worst_ratio(sums[BETA_ENTRIES], ref["sums"][BETA_ENTRIES], ref["abs"][BETA_ENTRIES])
    return plain, beta, KC.worst_ratio(stats, ref["stats"], ref["stats_abs"])
