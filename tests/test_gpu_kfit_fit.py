"""
KSpaceBatchFitter / KSpaceFitter (ngmix_amd/kfit.py) on the device: noise-free
fits reach the truth, priors and bounds, the parameter counts the step forms
serve, go against go_many, and the independent cross-check against the
real-space LMBatchFitter("gauss").
"""
import ctypes

import numpy as np
import pytest

import ngmix_amd
from ngmix_amd import _lib, prior_batch as PB
from ngmix_amd.kfit import KSpaceBatchFitter, KSpaceFitter, KStampBatch, kmodel_images

from helpers import kfit_cases as KC
from helpers import kfit_reference as K

pytestmark = pytest.mark.gpu

TIGHT = {"ftol": 1e-10, "xtol": 1e-10, "maxfev": 400}
SHAPE = (16, 16)


def _torch():
    import torch
    return torch


def _kbatch(stamps):
    """a KStampBatch straight from transforms made by the helper"""
    torch = _torch()
    dhat, phat, wbar, jac = KC.pack_stamps(stamps)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    R, C = stamps[0]["shape"]
    return KStampBatch(dev(dhat), None if phat is None else dev(phat), dev(wbar),
                       dev(jac.view(np.float64).reshape(-1, 8)), R, C)


def _truths(name, nobj, nband, seed):
    rng = np.random.RandomState(seed)
    cols = [rng.uniform(-0.3, 0.3, nobj), rng.uniform(-0.3, 0.3, nobj),
            rng.uniform(-0.3, 0.3, nobj), rng.uniform(-0.3, 0.3, nobj),
            rng.uniform(1.3, 2.2, nobj)]
    if name == "spergel":
        cols.append(rng.uniform(-0.4, 2.5, nobj))
    cols += [rng.uniform(30.0, 90.0, nobj) for _ in range(nband)]
    return np.stack(cols, axis=1)


def _noise_free(name, truth, nband, psf=True):
    """one stamp per (object, band), its transform the helper's model at the truth"""
    mid = K.MODEL_ID[name]
    nloc = K.NLOC[mid]
    base = [KC.make_stamp(SHAPE, jn, (name, 0.5), SHAPE if psf else None, 60 + b)
            for b, jn in zip(range(nband), ["diag", "aniso", "rotflip", "diag", "aniso"])]
    stamps, sobj, sband = [], [], []
    for i, t in enumerate(truth):
        for b in range(nband):
            s = dict(base[b])
            p = np.concatenate([t[:nloc - 1], [t[nloc - 1 + b]]])
            phat = None if s["phat"] is None else K.from_interleaved(s["phat"])
            s["dhat"] = K.interleaved(K.model(mid, p, s["md"], phat, jac=False)["M"])
            stamps.append(s)
            sobj.append(i)
            sband.append(b)
    return stamps, sobj, sband


def _guess(truth, seed):
    rng = np.random.RandomState(seed)
    g = truth * (1.0 + 0.04 * rng.uniform(-1, 1, truth.shape))
    g[:, :4] = truth[:, :4] + 0.03 * rng.uniform(-1, 1, (truth.shape[0], 4))
    return g


@pytest.mark.parametrize("name,nband", [("gauss", 1), ("exp", 1), ("spergel", 1),
                                        ("spergel", 3), ("exp", 5)])
def test_noise_free_fits_reach_the_truth(name, nband):
    """64 objects (16 for the many-band cases), zero residual at the truth:
    the last accepted step bounds the error -- 1e-7 relative, ier in 1..4.
    npars = 6, 7, 9 (the team step, by the census) and 10."""
    nobj = 64 if nband == 1 else 16
    truth = _truths(name, nobj, nband, 11)
    stamps, sobj, sband = _noise_free(name, truth, nband)
    kb = _kbatch(stamps)
    _lib.launch_census(reset=True)
    fitter = KSpaceBatchFitter(name, fit_pars=TIGHT)
    res = fitter.go(kb, _guess(truth, 12), stamp_obj=sobj, stamp_band=sband)
    census = _lib.launch_census()
    n = truth.shape[1]
    assert res["pars"].shape == (nobj, n) and res["pars_cov"].shape == (nobj, n, n)
    assert np.all(res["flags"] == 0), res["flags"]
    assert np.all((res["ier"] >= 1) & (res["ier"] <= 4)), res["ier"]
    err = np.abs(res["pars"] - truth) / np.abs(truth)
    print("kfit fit %s x %d bands: worst relative error %.2e, nfev <= %d, rounds %d"
          % (name, nband, err.max(), res["nfev"].max(), fitter.rounds_launched))
    assert err.max() <= 1e-7
    assert any(k.startswith("kfit_eval_kernel<%s>" % name) for k in census), census
    team = sum(v for k, v in census.items() if k.startswith("lm_advance_team_kernel"))
    assert (team > 0) == (n >= 9), census
    assert np.all(res["dof"] == nband * 15 * 15 - n)
    assert np.array_equal(res["r50"], res["pars"][:, 4])
    assert np.array_equal(res["flux"], res["pars"][:, n - nband:])
    if name == "spergel":
        assert np.array_equal(res["nu"], res["pars"][:, 5])
    # the model image of the fit is the data's, through kmodel_images
    nloc = K.NLOC[K.MODEL_ID[name]]
    loc = np.concatenate([res["pars"][sobj, :nloc - 1],
                          res["pars"][sobj, nloc - 1 + np.array(sband)][:, None]], axis=1)
    img = kmodel_images(kb, loc, name).cpu().numpy()
    want = K.model_image(K.MODEL_ID[name], loc[0], stamps[0]["md"],
                         K.from_interleaved(stamps[0]["phat"]))
    assert np.abs(img[0] - want).max() <= 1e-9 * np.abs(want).max()


def _priors(nband=1):
    cen = PB.GaussianCen(0.0, 0.0, 0.5, 0.5)
    g = PB.GPriorBA(0.3)
    r50 = PB.TwoSidedErf(0.2, 0.05, 6.0, 0.3, bounds=(0.05, 8.0))
    nu = PB.TwoSidedErf(-0.7, 0.05, 3.5, 0.1, bounds=(-0.84, 3.9))
    F = [PB.TwoSidedErf(1.0, 0.5, 500.0, 20.0, bounds=(0.01, 1000.0)) for _ in range(nband)]
    return cen, g, r50, nu, F


@pytest.mark.parametrize("name", ["exp", "spergel"])
def test_priors_rows_and_bounds(name):
    """the device record's rows (ngmix_simple_sep_prior_eval: the code the prior
    kernel runs) equal the torch path's fill_fdiff_batch to 4e-15, the project's
    figure for prior rows; fits under the prior stay inside its bounds"""
    torch = _torch()
    cen, g, r50, nu, F = _priors()
    if name == "exp":
        prior = PB.PriorSimpleSepBatch(cen, g, r50, F)
    else:
        prior = PB.PriorSpergelSepBatch(cen, g, r50, nu, F)
    desc = prior.descriptor()
    assert desc is not None and int(desc["nmid"][0]) == (1 if name == "spergel" else 0)
    truth = _truths(name, 32, 1, 21)
    rows_t, bad = prior.fill_fdiff_batch(torch.from_numpy(truth).cuda())
    rows_t = rows_t.cpu().numpy()
    assert not bool(bad.any())
    nrows = rows_t.shape[1]
    assert nrows == truth.shape[1] - 1
    for i, p in enumerate(truth):
        rows = np.zeros(16)
        lnp = ctypes.c_double()
        k = _lib.lib().ngmix_simple_sep_prior_eval(_lib.ptr(desc), _lib.ptr(p), _lib.ptr(rows),
                                                   ctypes.byref(lnp))
        assert k == nrows
        assert np.abs(rows[:k] - rows_t[i]).max() <= 4e-15 * max(1.0, np.abs(rows_t[i]).max())
    stamps, sobj, sband = _noise_free(name, truth, 1)
    fitter = KSpaceBatchFitter(name, prior=prior)       # (the default tolerances)
    res = fitter.go(_kbatch(stamps), _guess(truth, 22), stamp_obj=sobj, stamp_band=sband)
    assert np.all(res["flags"] == 0), (res["flags"], res["ier"])
    # the bounds ran leastsqbound's transform, and the prior kernel its rows
    assert np.all(fitter.states()["bounded"] == 1)
    lo, hi = PB.bounds_arrays(prior.bounds, truth.shape[1])
    assert np.all(res["pars"] >= lo) and np.all(res["pars"] <= hi)
    assert np.all(np.isfinite(res["lnprob"])) and np.all(res["s2n"] > 0)
    # a prior of the wrong layout is refused
    with pytest.raises(ValueError):
        KSpaceBatchFitter("gauss" if name == "spergel" else "spergel", prior=prior).go(
            _kbatch(stamps), _guess(truth, 22))


def test_go_is_go_many_of_one_and_dev_is_refused():
    rng = np.random.RandomState(31)
    deriv = K.JACOBIANS["diag"]
    objs, guesses = [], []
    for i in range(3):
        mb = ngmix_amd.MultiBandObsList()
        for band in range(2):
            ol = ngmix_amd.ObsList()
            cen = (7.5 + 0.2 * i, 7.4)
            jac = ngmix_amd.Jacobian(row=cen[0], col=cen[1], dvdrow=deriv[0], dvdcol=deriv[1],
                                     dudrow=deriv[2], dudcol=deriv[3])
            pim = np.asarray(K.gauss_image(SHAPE, cen, deriv, (0, 0, 0, 0, 2 * 0.9 ** 2, 1.0)),
                             dtype=float)
            im = np.asarray(K.gauss_image(SHAPE, cen, deriv,
                                          (0.1, -0.1, 0.1, 0.05, 2 * 1.7 ** 2, 60.0 + 20 * band)),
                            dtype=float) + 0.01 * rng.standard_normal(SHAPE)
            ol.append(ngmix_amd.Observation(im, weight=np.full(SHAPE, 1e4), jacobian=jac,
                                            psf=ngmix_amd.Observation(pim, jacobian=jac)))
            mb.append(ol)
        objs.append(mb)
        guesses.append([0.0, 0.0, 0.0, 0.0, 1.5, 0.7, 50.0, 70.0])
    fitter = KSpaceFitter("spergel", fit_pars=TIGHT)
    many = fitter.go_many(objs, guesses)
    assert len(many) == 3
    for i in (0, 2):
        one = fitter.go(objs[i], guesses[i])
        assert sorted(one) == sorted(many[i])
        for k in one:
            assert np.array_equal(one[k], many[i][k], equal_nan=True) if k != "model" \
                else one[k] == many[i][k], k
    for k in ("pars", "pars_err", "pars_cov", "flags", "nfev", "njev", "ier", "dof", "chi2per",
              "lnprob", "s2n", "g", "g_cov", "r50", "flux", "nu"):
        assert k in many[0], k
    with pytest.raises(ValueError):
        KSpaceFitter("dev")
    with pytest.raises(ValueError):
        KSpaceBatchFitter("dev")


# gated at 10 x the largest difference measured on one MI355X:
# parameters relative to max(|value|, 1): 1.866e-06; covariances relative to
# sqrt(C_ii C_jj): 4.370e-02.  The parameters differ by the noise of the 47
# Nyquist components the k-space fit leaves out, not by aliasing alone; the
# covariances by run_leastsq's factor |f|^2 / dof, which the two fits take from
# 570 and from 523 residual components of the same noise.
CROSS_TOL = {"pars": 1.9e-5, "cov": 0.44}


def test_cross_check_against_the_real_space_gaussian_fit():
    """32 noisy 24 x 24 gaussians, uniform weight, sigma_total >= 2 pixels, a
    1-gaussian psf: KSpaceBatchFitter('gauss') with the psf STAMP against
    LMBatchFitter('gauss') with the psf MIXTURE.  cen, g, F and
    T = 2 sigma^2 (1 + g^2) / (1 - g^2) agree, and pars_cov after the same
    change of variable; the difference is aliasing, stamp truncation and the
    dropped Nyquist modes."""
    from ngmix_amd.batch import GMixBatch, StampBatch
    from ngmix_amd import LMBatchFitter
    rng = np.random.RandomState(77)
    n, shape = 32, (24, 24)
    deriv = (0.0, 0.9, 0.9, 0.0)          # rows along u, columns along v: det < 0
    cens = np.stack([11.5 + rng.uniform(-0.4, 0.4, n), 11.5 + rng.uniform(-0.4, 0.4, n)], axis=1)
    Tpsf = 2 * (1.3 * 0.9) ** 2
    truth = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n),
                      rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n),
                      2 * (1.6 * 0.9) ** 2 * rng.uniform(0.9, 1.2, n),
                      rng.uniform(80.0, 120.0, n)], axis=1)
    sigma_noise = 0.01
    imgs, psfs, jacs = [], [], []
    for i in range(n):
        t = truth[i]
        gsq = t[2] ** 2 + t[3] ** 2
        e1o, e2o = 2 * t[2] / (1 + gsq), 2 * t[3] / (1 + gsq)
        T = t[4] + Tpsf
        e1, e2 = e1o * t[4] / T, e2o * t[4] / T
        e = np.hypot(e1, e2)
        f = np.tanh(0.5 * np.arctanh(e)) / e
        imgs.append(np.asarray(K.gauss_image(shape, cens[i], deriv,
                                             (t[0], t[1], f * e1, f * e2, T, t[5])), dtype=float)
                    + sigma_noise * rng.standard_normal(shape))
        psfs.append(np.asarray(K.gauss_image(shape, cens[i], deriv, (0, 0, 0, 0, Tpsf, 1.0)),
                               dtype=float))
        jacs.append(KC.jac_record(cens[i], deriv))
    imgs, psfs = np.stack(imgs), np.stack(psfs)
    jac = np.concatenate(jacs).view(np.float64).reshape(-1, 8)
    wts = np.full(imgs.shape, 1.0 / sigma_noise ** 2)
    fp = {"ftol": 1e-12, "xtol": 1e-12, "maxfev": 400}
    guess = truth * (1 + 0.02 * rng.uniform(-1, 1, truth.shape))
    # real space: T, psf mixture
    sb = StampBatch.from_images(imgs, wts, jac)
    psf_pars = np.tile([0.0, 0.0, 0.0, 0.0, Tpsf, 1.0], (n, 1))
    real = LMBatchFitter("gauss", fit_pars=fp).go(sb, guess,
                                                  psf=GMixBatch.from_pars(psf_pars, "gauss")[0])
    # k space: r50, psf stamp
    kb = KStampBatch.from_images(imgs, wts, jac, psf_images=psfs, psf_jacobians=jac)
    gk = guess.copy()
    gsq = guess[:, 2] ** 2 + guess[:, 3] ** 2
    gk[:, 4] = np.sqrt(guess[:, 4] * (1 - gsq) / (2 * (1 + gsq))) * float(K.HLR_GAUSS)
    kres = KSpaceBatchFitter("gauss", fit_pars=fp).go(kb, gk)
    assert np.all(real["flags"] == 0) and np.all(kres["flags"] == 0)
    # the change of variable (g1, g2, r50) -> T and its jacobian
    p = kres["pars"]
    gsq = p[:, 2] ** 2 + p[:, 3] ** 2
    h = float(K.HLR_GAUSS)
    Tk = 2 * (p[:, 4] / h) ** 2 * (1 + gsq) / (1 - gsq)
    conv = p.copy()
    conv[:, 4] = Tk
    A = np.tile(np.eye(6), (n, 1, 1))
    dT_dg = 2 * (p[:, 4] / h) ** 2 * 4 / (1 - gsq) ** 2
    A[:, 4, 2], A[:, 4, 3] = dT_dg * p[:, 2], dT_dg * p[:, 3]
    A[:, 4, 4] = 2 * Tk / p[:, 4]
    cov = np.einsum("nij,njk,nlk->nil", A, kres["pars_cov"], A)
    dp = np.abs(conv - real["pars"]) / np.maximum(np.abs(real["pars"]), 1.0)
    rc = real["pars_cov"]
    sc = np.sqrt(np.einsum("nii->ni", rc)[:, :, None] * np.einsum("nii->ni", rc)[:, None, :])
    dc = np.abs(cov - rc) / sc
    print("kfit cross-check: worst parameter difference %.3e, worst covariance difference %.3e"
          % (dp.max(), dc.max()))
    # the fits see the noise: the parameters moved from the truth by far more
    assert np.abs(real["pars"] - truth).max() > 1e-4
    assert dp.max() <= CROSS_TOL["pars"] and dc.max() <= CROSS_TOL["cov"]
