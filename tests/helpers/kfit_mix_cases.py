"""
The cases the host and GPU tests of the Fourier-space 'dev10' and 'bdf' fits
share: stamps with their dense transforms, trial points, mode
weights, the dense reference of each (tests/helpers/kfit_mix_reference.py) and
the glue that calls the host entry points.  Built once per process and left
unchanged.
"""
import functools

import numpy as np

from ngmix_amd import _lib

from helpers import kfit_cases as KC
from helpers import kfit_mix_reference as MR
from helpers import kfit_reference as K

SHAPES = [(8, 8), (9, 12), (15, 15)]
FRACDEVS = [0.0, 0.3, 1.0, -0.1, 1.2]
# The gate of the sums: kfit_cases' C_ROUND = 96 units of 2^-52 sum |terms|.  Its
# count holds for the mixtures with one change: Phi is a sum of 10 or 16 terms
# a_i exp(h_i s) of ONE sign for fracdev in [0, 1] (each 4 roundings, like the
# single libm call it replaces, against the sum of their absolute values) and
# the conditioning of an exponential in s is its own exponent, which falls on
# terms exp(-x) down, as the gaussian's does there.  Outside [0, 1] the
# amplitudes change sign and sum |a_i e_i| exceeds |Phi|, by at most
# (1 + 2 * 0.2) at the fracdev of these cases: inside the count's slack.
# Measured on the host twin (x86-64) against the longdouble reference: worst
# 14.8 units (sums), 2.9 (statistics), 3.4 (flux sums, gate kfit_moffat_cases'
# C_FLUX = 64), with and without mode weights; no wider constant is needed.
C_ROUND = KC.C_ROUND
C_FLUX = 64.0


def _mode_weights(shape, rng):
    """a plane of u >= 0: a tenth of the modes masked, the rest in [0.2, 3]"""
    R, C = shape
    u = rng.uniform(0.2, 3.0, size=(R, C // 2 + 1))
    u[rng.uniform(size=u.shape) < 0.1] = 0.0
    return u


def make_stamp(model, shape, jname, psf, seed, fracdev=None, gmag=None, band=0):
    """kfit_cases.make_stamp's image and transforms with a trial point of
    `model`: the size is T = 2 sigma^2 of a sigma between 1 and 1.8 pixels"""
    st = KC.make_stamp(shape, jname, ("gauss", None), shape if psf else None, seed, gmag=gmag,
                       band=band)
    rng = np.random.RandomState(seed + 7000)
    scale = np.sqrt(abs(np.linalg.det(np.reshape(st["deriv"], (2, 2)))))
    p = list(st["p"][:4]) + [2.0 * (scale * rng.uniform(1.0, 1.8)) ** 2]
    if model == MR.BDF:
        p.append(fracdev)
    p.append(st["p"][-1])
    st["model"], st["p"], st["u"] = model, np.array(p), _mode_weights(shape, rng)
    return st


@functools.lru_cache(maxsize=None)
def sums_cases():
    """{(model id, shape, with psf): [stamps]}: every shape x jacobian, with a
    psf plane of the stamp's own shape and without one; 'bdf' at every fracdev
    of FRACDEVS; |g| drawn up to 0.6, and 0.6 exactly under 'aniso' with a psf"""
    groups = {}
    seed = 4100
    for shape in SHAPES:
        for jname in K.JACOBIANS:
            for psf in (False, True):
                gmag = 0.6 if (jname == "aniso" and psf) else None
                for model, fds in ((MR.DEV10, [None]), (MR.BDF, FRACDEVS)):
                    for fd in fds:
                        seed += 1
                        st = make_stamp(model, shape, jname, psf, seed, fd, gmag)
                        groups.setdefault((model, shape, psf), []).append(st)
    return groups


def phat_of(st):
    return None if st["phat"] is None else K.from_interleaved(st["phat"])


@functools.lru_cache(maxsize=None)
def references(weighted):
    """{key: [stamp_sums of each stamp of sums_cases()[key]]}, with or without
    the stamps' mode weights"""
    return {key: [MR.stamp_sums(st["model"], st["p"], st["md"], K.from_interleaved(st["dhat"]),
                                phat_of(st), st["wbar"], st["u"] if weighted else None)
                  for st in sts] for key, sts in sums_cases().items()}


@functools.lru_cache(maxsize=None)
def flux_references(weighted):
    nl = MR.NLOC
    return {key: [MR.flux_sums(st["model"], st["p"][:nl[st["model"]] - 1], st["md"],
                               K.from_interleaved(st["dhat"]), phat_of(st), st["wbar"],
                               st["u"] if weighted else None)
                  for st in sts] for key, sts in sums_cases().items()}


@functools.lru_cache(maxsize=None)
def multiband_case():
    """one 'bdf' object of 2 bands x 2 epochs (15 x 15, with psf): the stamps
    and the object's 8 parameters"""
    stamps = []
    for band in range(2):
        for epoch in range(2):
            stamps.append(make_stamp(MR.BDF, (15, 15), ("diag", "aniso")[epoch], True,
                                     4900 + 2 * band + epoch, 0.4, band=band))
    pars = np.concatenate([stamps[0]["p"][:6], [55.0, 31.0]])
    for s in stamps:
        s["p"] = np.concatenate([pars[:6], [pars[6 + s["band"]]]])
    return stamps, pars


def _opt(a, dtype=None):
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, _lib.ptr(a)


def eval_host(stamps, states, weighted=False, stamp_obj=None, stamp_band=None, sums=None):
    """ngmix_kfit_eval_host, or weighted ngmix_kfit_eval_w_host with the stamps'
    own planes, on stamps of one shape and model: sums, status, stats, ncomp"""
    L = _lib.lib()
    dhat, phat, wbar, jac = KC.pack_stamps(stamps)
    R, C = stamps[0]["shape"]
    n = len(stamps)
    if sums is None:
        sums = np.full((n, K.nsums(MR.NLOC[stamps[0]["model"]])), np.nan)
    status = np.full(n, -7, dtype=np.int32)
    stats = np.full((n, 2), np.nan)
    ncomp = np.full(n, -7, dtype=np.int32)
    _so, so = _opt(stamp_obj, np.int32)
    _sb, sb = _opt(stamp_band, np.int32)
    head = (_lib.ptr(dhat), None if phat is None else _lib.ptr(phat))
    mid = (_lib.ptr(wbar), _lib.ptr(jac), R, C, n, stamps[0]["model"], _lib.ptr(states), so, sb,
           _lib.ptr(sums), _lib.ptr(status), _lib.ptr(stats))
    if weighted:
        u = np.ascontiguousarray(np.stack([s["u"] for s in stamps]))
        rc = L.ngmix_kfit_eval_w_host(*head, _lib.ptr(u), *mid, _lib.ptr(ncomp))
    else:
        rc = L.ngmix_kfit_eval_host(*head, *mid)
    assert rc == 0, _lib.last_error()
    return sums, status, stats, ncomp


def flux_host(stamps, pars, weighted=False):
    """ngmix_kfit_flux_host or _w_host on stamps of one shape and model: out
    (n, 3), status"""
    L = _lib.lib()
    dhat, phat, wbar, jac = KC.pack_stamps(stamps)
    R, C = stamps[0]["shape"]
    n = len(stamps)
    pars = np.ascontiguousarray(pars, dtype=np.float64)
    out = np.full((n, 3), np.nan)
    status = np.full(n, -7, dtype=np.int32)
    head = (_lib.ptr(dhat), None if phat is None else _lib.ptr(phat))
    mid = (_lib.ptr(wbar), _lib.ptr(jac), R, C, n, stamps[0]["model"], _lib.ptr(pars),
           _lib.ptr(out), _lib.ptr(status))
    if weighted:
        u = np.ascontiguousarray(np.stack([s["u"] for s in stamps]))
        rc = L.ngmix_kfit_flux_w_host(*head, _lib.ptr(u), *mid, None)
    else:
        rc = L.ngmix_kfit_flux_host(*head, *mid)
    assert rc == 0, _lib.last_error()
    return out, status


def trial_points(stamps):
    return np.stack([s["p"] for s in stamps])


def worst_of_group(got_sums, got_stats, refs):
    """the worst error of a group's sums and of its statistics, in units of
    2^-52 sum |terms|"""
    ws = max(KC.worst_ratio(got_sums[i], r["sums"], r["abs"]) for i, r in enumerate(refs))
    wt = max(KC.worst_ratio(got_stats[i], r["stats"], r["stats_abs"]) for i, r in enumerate(refs))
    return ws, wt
