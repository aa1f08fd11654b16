"""
The team form of the lmder step (csrc/lm_core_team.hpp: 16 lanes per fit, the
fit's arrays in LDS -- what fits of 11-14 parameters run) against the generic
one-thread form (csrc/lm_core.hpp, itself pinned to scipy's MINPACK on the CPU
by tests/test_lm_core.py and to the reference's fits by test_gpu_lm_batch.py):
the STATE RECORDS of the two forms are compared after every lock-step round,
byte for byte over their live part -- analytic and forward-difference modes,
multi-band objects, co-elliptical psf fits with their long lmpar iterations,
bounds and prior rows, out-of-range starts, poor guesses (rejected steps), and
one, two or four fits per wave.

Reference semantics: ngmix/fitting/leastsqbound.py:289-552 (scipy's lmder /
lmdif), results.py:439-570.
"""
import numpy as np
import pytest
import torch

import ngmix_amd as ngmix
from ngmix_amd import _lib
from ngmix_amd.batch import StampBatch, GMixBatch
from ngmix_amd.lm_batch import LMBatchFitter

from test_gpu_lm_batch import _make_objects

pytestmark = pytest.mark.gpu

VECTORS = ("x", "xt", "diag", "qtf", "step", "xi", "xti", "lo", "hi", "xstep", "hstep", "ipvt")
SCALARS = ("fnorm", "xnorm", "delta", "par", "gnorm", "pnorm", "ftol", "xtol", "gtol",
           "factor", "n", "iter", "nfev", "njev", "info", "phase", "maxfev", "mode",
           "bounded", "fonly")


def _live(rec):
    """the live part of the state records as bytes-comparable arrays"""
    n = int(rec["n"][0])
    assert np.all(rec["n"] == n)
    out = {k: rec[k].copy() for k in SCALARS}
    for k in VECTORS:
        out[k] = rec[k][:, :n].copy()
    nmax = _lib.LM_NPMAX
    out["R"] = rec["R"].reshape(-1, nmax, nmax)[:, :n, :n].copy()
    return out


def _rounds(fitter, go, hint):
    """run go() through the host-driven loop with the step's kernel selected
    by the hint; returns (result, [live state after each round])"""
    snaps = []

    def hook(job, r):
        torch.cuda.synchronize()
        rec = job.d_states.cpu().numpy().view(_lib.LM_STATE_DTYPE).reshape(-1)
        snaps.append(_live(rec))
    fitter.host_loop = True
    fitter.advance_hint = hint
    fitter.round_hook = hook
    res = go(fitter)
    return res, snaps


def _assert_same_rounds(a, b):
    assert len(a) == len(b) and len(a) > 1
    for r, (sa, sb) in enumerate(zip(a, b)):
        for k in sa:
            # bytes, not values: NaNs and signed zeros included
            assert sa[k].tobytes() == sb[k].tobytes(), "round %d, field %s" % (r, k)


def _census_has(seen, frag):
    return any(frag in k for k in seen)


def _multiband(nobj, nband, model, rng):
    ns = nobj * nband
    pars, guess, images, weights, jac, sb, psf = _make_objects(ns, model, rng)
    sobj = np.repeat(np.arange(nobj), nband).astype(np.int32)
    sband = np.tile(np.arange(nband), nobj).astype(np.int32)
    shape = guess[::nband, :5]
    g2 = np.concatenate([shape, guess[:, 5].reshape(nobj, nband)], axis=1)
    return sb, psf, g2, sobj, sband


@pytest.mark.parametrize("nband, lazy, teams", [(4, True, 4), (5, False, 4), (6, True, 4),
                                                (7, False, 2), (9, True, 1)])
def test_team_step_equals_generic_step_multiband_lmder(nband, lazy, teams, monkeypatch):
    """'exp' over 4 / 5 / 6 / 7 / 9 bands: 9 / 10 / 11 / 12 / 14 parameters (the
    kernel's builds for 10, 12 and 14), lmder (lazy and eager jacobians)"""
    monkeypatch.setenv("NGMIX_LM_TEAMS", str(teams))
    rng = np.random.RandomState(100 + nband)
    nobj = 37
    sb, psf, guess, sobj, sband = _multiband(nobj, nband, "exp", rng)
    guess[::4, 4:] *= 1.6                      # poor guesses: rejected steps, lmpar iterations
    guess[::6, 2:4] = 0.4, -0.3

    def go(f):
        f.lazy_jacobian = lazy
        return f.go(sb, guess, psf=psf, stamp_obj=sobj, stamp_band=sband)
    _lib.launch_census(reset=True)
    rt, st = _rounds(LMBatchFitter("exp"), go, True)
    seen = _lib.launch_census(reset=True)
    assert _census_has(seen, "lm_advance_team_kernel<%d," % teams), seen
    assert not _census_has(seen, "lm_advance_kernel<")
    rg, sg = _rounds(LMBatchFitter("exp"), go, False)
    seen = _lib.launch_census(reset=True)
    assert _census_has(seen, "lm_advance_kernel<14, false>") and not _census_has(seen, "team")
    _assert_same_rounds(st, sg)
    for k in ("flags", "nfev", "njev", "ier", "pars", "pars_cov", "lnprob"):
        np.testing.assert_array_equal(rt[k], rg[k], err_msg=k)
    assert np.mean(rt["flags"] == 0) > 0.7
    # and the host-free rounds (what go() runs by default) give the same fit
    plain = LMBatchFitter("exp")
    plain.lazy_jacobian = lazy
    rp = plain.go(sb, guess, psf=psf, stamp_obj=sobj, stamp_band=sband)
    for k in ("flags", "nfev", "ier", "pars", "pars_cov"):
        np.testing.assert_array_equal(rp[k], rt[k], err_msg=k)


@pytest.mark.parametrize("ngauss", [4, 5])
def test_team_step_equals_generic_step_coellip(ngauss, monkeypatch):
    """co-elliptical psf fits with 4 / 5 gaussians (12 / 14 parameters, lmdif):
    nearly degenerate valleys -- many lmpar iterations with qrsolv, steps
    against a singular factor"""
    rng = np.random.RandomState(7 + ngauss)
    dim, scale, n = 25, 0.263, 29
    jac = ngmix.DiagonalJacobian(row=12.0, col=12.0, scale=scale)
    gm = ngmix.GMixModel([0.0, 0.0, 0.02, -0.01, 0.3, 1.0], "turb")
    im0 = gm.make_image((dim, dim), jacobian=jac)
    images = im0[None] + 2.0e-4 * rng.normal(size=(n, dim, dim))
    weights = np.full((n, dim, dim), 1.0 / 2.0e-4 ** 2)
    sb = StampBatch.from_images(images, weights, jac)
    T = 0.3 * np.array([0.3, 0.7, 1.5, 3.0, 6.0])[:ngauss]
    F = np.array([0.25, 0.35, 0.25, 0.1, 0.05])[:ngauss]
    g0 = np.concatenate([[0.0, 0.0, 0.02, -0.01], T, F / F.sum()])
    guess = g0[None] * rng.uniform(0.9, 1.1, size=(n, g0.size))
    guess[:, :2] = rng.uniform(-0.01, 0.01, size=(n, 2))
    guess[3, 4:4 + ngauss] = guess[3, 4]       # identical components: a singular jacobian
    pars = {"maxfev": 120, "ftol": 1e-5, "xtol": 1e-5}

    def go(f):
        return f.go(sb, guess)
    rt, st = _rounds(LMBatchFitter("coellip", ngauss=ngauss, fit_pars=pars), go, True)
    rg, sg = _rounds(LMBatchFitter("coellip", ngauss=ngauss, fit_pars=pars), go, False)
    _assert_same_rounds(st, sg)
    assert len(st) > 10
    for k in ("flags", "nfev", "ier", "pars"):
        np.testing.assert_array_equal(rt[k], rg[k], err_msg=k)


def test_team_step_equals_generic_step_bdf_bands(monkeypatch):
    """'bdf' over 5 bands: 11 parameters, lmdif with the MFMA normal equations"""
    rng = np.random.RandomState(55)
    nobj, nband = 21, 5
    ns = nobj * nband
    pars, guess, images, weights, jac, sb, psf = _make_objects(ns, "exp", rng)
    sobj = np.repeat(np.arange(nobj), nband).astype(np.int32)
    sband = np.tile(np.arange(nband), nobj).astype(np.int32)
    g2 = np.concatenate([guess[::nband, :5], np.full((nobj, 1), 0.2),
                         guess[:, 5].reshape(nobj, nband)], axis=1)
    fp = {"maxfev": 150, "ftol": 1e-5, "xtol": 1e-5}

    def go(f):
        return f.go(sb, g2, psf=psf, stamp_obj=sobj, stamp_band=sband)
    rt, st = _rounds(LMBatchFitter("bdf", fit_pars=fp), go, True)
    rg, sg = _rounds(LMBatchFitter("bdf", fit_pars=fp), go, False)
    _assert_same_rounds(st, sg)
    for k in ("flags", "nfev", "ier", "pars", "pars_cov"):
        np.testing.assert_array_equal(rt[k], rg[k], err_msg=k)


@pytest.mark.parametrize("fd", [False, True])
def test_team_step_with_bounds_prior_rows_and_bad_starts(fd, monkeypatch):
    """the paths only small fits reach (the separable prior holds three bands):
    NGMIX_LM_TEAM_MIN = 6 sends 6- to 8-parameter fits through the team form --
    bounds (leastsqbound's transforms, the scaled analytic jacobian), prior
    rows folded into the normal equations, a start out of range (g >= 1: the
    fit ends at once, info 4), masked stamps"""
    from ngmix_amd import prior_batch as pb
    monkeypatch.setenv("NGMIX_LM_TEAM_MIN", "6")
    rng = np.random.RandomState(91 + int(fd))
    nobj, nband = 26, 2
    sb, psf, guess, sobj, sband = _multiband(nobj, nband, "exp", rng)
    guess[5, 2:4] = 0.9, 0.8                   # |g| >= 1 at the start
    guess[::7, 4] *= 2.5
    prior = pb.PriorSimpleSepBatch(
        pb.GaussianCen(0.0, 0.0, 0.3, 0.3), pb.GPriorBA(0.3),
        pb.Normal(0.6, 0.5, bounds=[0.05, 4.0]),
        [pb.Normal(120.0, 200.0, bounds=[1.0, None]), pb.TwoSidedErf(-1.0e3, 1.0, 1.0e5, 10.0)])

    def go(f):
        return f.go(sb, guess, psf=psf, stamp_obj=sobj, stamp_band=sband)

    def make():
        return LMBatchFitter("exp", prior=prior, analytic_jacobian=not fd)
    _lib.launch_census(reset=True)
    rt, st = _rounds(make(), go, True)
    seen = _lib.launch_census(reset=True)
    assert _census_has(seen, "lm_advance_team_kernel<4,"), seen
    rg, sg = _rounds(make(), go, False)
    _assert_same_rounds(st, sg)
    assert np.all(st[-1]["bounded"] == 1)
    for k in ("flags", "nfev", "ier", "pars", "pars_cov", "lnprob"):
        np.testing.assert_array_equal(rt[k], rg[k], err_msg=k)
    assert rt["flags"][5] != 0
    # the register form (the default for these sizes) is the same fit too
    monkeypatch.delenv("NGMIX_LM_TEAM_MIN")
    rr = make().go(sb, guess, psf=psf, stamp_obj=sobj, stamp_band=sband)
    for k in ("flags", "nfev", "ier", "pars"):
        np.testing.assert_array_equal(rr[k], rt[k], err_msg=k)


@pytest.mark.parametrize("teams", [4, 2])
def test_team_step_under_load_is_the_generic_fit_and_order_independent(teams, monkeypatch):
    """thousands of fits in flight (several waves per SIMD, four fits per wave
    each at its own point of lmder's control flow: guesses from good to bad,
    some starts out of range): the complete fits of the team form are the
    generic form's to the bit, run after run, and a fit's result does not depend
    on which wave or team slot it sits in (a permuted batch gives the permuted
    results) -- the checks a cross-lane hazard in the LDS protocol would fail"""
    monkeypatch.setenv("NGMIX_LM_TEAMS", str(teams))
    rng = np.random.RandomState(404 + teams)
    nobj, nband = 3001, 6                       # (not a multiple of the fits per wave)
    sb, psf, guess, sobj, sband = _multiband(nobj, nband, "exp", rng)
    bad = rng.uniform(size=nobj)
    guess[bad < 0.3, 4:] *= rng.uniform(0.4, 2.5, size=(int((bad < 0.3).sum()), guess.shape[1] - 4))
    guess[bad < 0.1, 2:4] = rng.uniform(-0.6, 0.6, size=(int((bad < 0.1).sum()), 2))
    guess[7, 2:4] = 0.95, 0.9                   # |g| >= 1
    kw = dict(psf=psf, stamp_obj=sobj, stamp_band=sband)
    keys = ("flags", "nfev", "njev", "ier", "pars", "pars_cov", "lnprob")
    team = LMBatchFitter("exp")
    _lib.launch_census(reset=True)
    a = team.go(sb, guess, **kw)
    seen = _lib.launch_census(reset=True)
    assert _census_has(seen, "lm_advance_team_kernel<%d, 12>" % teams), seen
    generic = LMBatchFitter("exp")
    generic.advance_hint = False
    b = generic.go(sb, guess, **kw)
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert team.rounds == generic.rounds and team.rounds > 8
    assert 0.5 < np.mean(a["flags"] == 0) < 1.0 and a["flags"][7] != 0
    # run-to-run
    c = team.go(sb, guess, **kw)
    for k in keys:
        np.testing.assert_array_equal(a[k], c[k], err_msg=k)
    # the objects in another order (their stamps moved along)
    perm = rng.permutation(nobj)
    sidx = (perm[:, None] * nband + np.arange(nband)[None, :]).reshape(-1)
    d = team.go(sb.select(sidx), guess[perm], psf=psf.select(sidx), stamp_obj=sobj,
                stamp_band=sband)
    for k in keys:
        np.testing.assert_array_equal(d[k], a[k][perm], err_msg=k)


def test_team_step_coellip_under_load(monkeypatch):
    """the same for two thousand 5-gaussian co-elliptical psf fits (14
    parameters; lmpar's iterations with the wavefront form of qrsolv's sweeps
    on most steps), and the launch census: no one-thread lm_advance kernel"""
    rng = np.random.RandomState(77)
    dim, scale, n, ngauss = 25, 0.263, 2003, 5
    jac = ngmix.DiagonalJacobian(row=12.0, col=12.0, scale=scale)
    gm = ngmix.GMixModel([0.0, 0.0, 0.02, -0.01, 0.3, 1.0], "turb")
    im0 = gm.make_image((dim, dim), jacobian=jac)
    images = im0[None] + 2.0e-4 * rng.normal(size=(n, dim, dim))
    sb = StampBatch.from_images(images, np.full((n, dim, dim), 1.0 / 2.0e-4 ** 2), jac)
    T = 0.3 * np.array([0.3, 0.7, 1.5, 3.0, 6.0])
    F = np.array([0.25, 0.35, 0.25, 0.1, 0.05])
    g0 = np.concatenate([[0.0, 0.0, 0.02, -0.01], T, F / F.sum()])
    guess = g0[None] * rng.uniform(0.9, 1.1, size=(n, g0.size))
    guess[:, :2] = rng.uniform(-0.01, 0.01, size=(n, 2))
    pars = {"maxfev": 100, "ftol": 1e-5, "xtol": 1e-5}
    team = LMBatchFitter("coellip", ngauss=ngauss, fit_pars=pars)
    _lib.launch_census(reset=True)
    a = team.go(sb, guess)
    seen = _lib.launch_census(reset=True)
    assert _census_has(seen, "lm_advance_team_kernel<4, 14>"), seen
    assert not _census_has(seen, "lm_advance_kernel<"), seen
    generic = LMBatchFitter("coellip", ngauss=ngauss, fit_pars=pars)
    generic.advance_hint = False
    b = generic.go(sb, guess)
    for k in ("flags", "nfev", "ier", "pars", "pars_cov"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    perm = rng.permutation(n)
    d = team.go(sb.select(perm), guess[perm])
    for k in ("flags", "nfev", "ier", "pars"):
        np.testing.assert_array_equal(d[k], a[k][perm], err_msg=k)


def test_team_step_wrong_hint_ends_the_fit(monkeypatch):
    """a parameter-count hint below a fit's n (the team kernel is built for the
    hinted count rounded up to 8 / 10 / 12 / 14): the fit is ended as MINPACK
    ends a call with improper input (info 0), not left un-advanced"""
    monkeypatch.setenv("NGMIX_LM_TEAM_MIN", "6")
    rng = np.random.RandomState(3)
    nobj, nband = 8, 7
    sb, psf, guess, sobj, sband = _multiband(nobj, nband, "exp", rng)
    f = LMBatchFitter("exp")
    f._nloc_npars = lambda npars: f.nloc + 256 * 10     # says 10, the fits have 12
    f.host_loop = True
    res = f.go(sb, guess, psf=psf, stamp_obj=sobj, stamp_band=sband)
    assert np.all(res["flags"] != 0) and f.rounds <= 2


def test_no_parameter_count_hint_runs_the_team_form_for_any_count():
    """ngmix_lm_advance_batch told nothing about the fits' parameter count
    (nloc alone): the team form built for 14 parameters serves them -- six- and
    twelve-parameter fits alike, the same fits as with the hint to the bit --
    and the one-thread code runs only when asked for
    (NGMIX_LM_NPARS_GENERIC, fitter.advance_hint = False)"""
    rng = np.random.RandomState(33)
    for nband in (1, 7):
        nobj = 40
        sb, psf, guess, sobj, sband = _multiband(nobj, nband, "exp", rng)
        kw = dict(psf=psf, stamp_obj=sobj, stamp_band=sband)
        ref = LMBatchFitter("exp").go(sb, guess, **kw)
        bare = LMBatchFitter("exp")
        bare._nloc_npars = lambda npars, f=bare: f.nloc
        _lib.launch_census(reset=True)
        got = bare.go(sb, guess, **kw)
        seen = _lib.launch_census(reset=True)
        assert _census_has(seen, "lm_advance_team_kernel<4, 14>"), seen
        assert not _census_has(seen, "lm_advance_kernel<"), seen
        for k in ("flags", "nfev", "njev", "ier", "pars", "pars_cov", "lnprob"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
        generic = LMBatchFitter("exp")
        generic.advance_hint = False
        _lib.launch_census(reset=True)
        gen = generic.go(sb, guess, **kw)
        seen = _lib.launch_census(reset=True)
        assert _census_has(seen, "lm_advance_kernel<14, false>") and not _census_has(seen, "team")
        for k in ("flags", "nfev", "pars", "pars_cov"):
            np.testing.assert_array_equal(gen[k], ref[k], err_msg=k)


@pytest.mark.parametrize("order", ["sorted", "interleaved", "ragged"])
def test_team_fold_with_epochs_and_any_band_order(order, monkeypatch):
    """objects with several epochs per band, the stamps of an object in band
    order, interleaved ([0, 1, 2, 0, 1, 2, ...]) or ragged (another number of
    epochs per band and per object): the team form's fold of the stamps' sums
    keeps an entry in a register while the band stays and writes / reads it
    when the band changes -- the state records after every round are the
    generic form's, byte for byte (NGMIX_LM_TEAM_MIN = 6: with three bands the
    fits have eight parameters)"""
    monkeypatch.setenv("NGMIX_LM_TEAM_MIN", "6")
    rng = np.random.RandomState({"sorted": 1, "interleaved": 2, "ragged": 3}[order])
    nobj, nband = 23, 3
    if order == "ragged":
        nep = rng.randint(1, 4, size=(nobj, nband))
    else:
        nep = np.full((nobj, nband), 3)
    sobj, sband = [], []
    for o in range(nobj):
        bands = np.concatenate([np.full(nep[o, b], b) for b in range(nband)])
        if order != "sorted":
            bands = rng.permutation(bands) if order == "ragged" else \
                np.tile(np.arange(nband), 3)
        sobj += [o] * bands.size
        sband += list(bands)
    sobj = np.array(sobj, dtype=np.int32)
    sband = np.array(sband, dtype=np.int32)
    ns = sobj.size
    pars, guess, images, weights, jac, sb, psf = _make_objects(ns, "exp", rng)
    # one shape per object, one flux per band
    first = np.searchsorted(sobj, np.arange(nobj))
    g2 = np.concatenate([guess[first, :5], np.stack(
        [guess[first + 0, 5], guess[first + 0, 5] * 1.1, guess[first + 0, 5] * 0.9], axis=1)],
        axis=1)

    def go(f):
        return f.go(sb, g2, psf=psf, stamp_obj=sobj, stamp_band=sband)
    _lib.launch_census(reset=True)
    rt, st = _rounds(LMBatchFitter("exp"), go, True)
    assert _census_has(_lib.launch_census(reset=True), "lm_advance_team_kernel<4, 8>")
    rg, sg = _rounds(LMBatchFitter("exp"), go, False)
    _assert_same_rounds(st, sg)
    for k in ("flags", "nfev", "ier", "pars", "pars_cov", "lnprob"):
        np.testing.assert_array_equal(rt[k], rg[k], err_msg=k)
    # and the register form (the default for eight parameters)
    monkeypatch.delenv("NGMIX_LM_TEAM_MIN")
    rr = LMBatchFitter("exp").go(sb, g2, psf=psf, stamp_obj=sobj, stamp_band=sband)
    for k in ("flags", "nfev", "ier", "pars"):
        np.testing.assert_array_equal(rr[k], rt[k], err_msg=k)


@pytest.mark.parametrize("nband", [1, 2, 3, 4, 5, 6, 7])
def test_reference_multiband_fits_for_every_parameter_count(golden, nband):
    """tests/golden/lm_mb.npz (oracle/gen_golden_mb.py): the REFERENCE's Fitter
    (MINPACK lmder on MultiBandObsLists) on objects of 1-7 bands -- 6 to 12
    parameters -- with one or two epochs per band, a gaussian or three-gaussian
    psf, DEFAULT_LM_PARS and tolerances of 1e-10, against the lock-step driver:
    the same nfev / ier / flags, pars / covariance / statistics to the
    tolerances the other reference fits are held to.  Four bands and up run the
    team form of the step (9+ parameters), which this pins to the reference
    directly and not through the generic form"""
    g = golden("lm_mb")
    per = int(g["per"])
    groups = {}
    for k in range(per):
        tag = "b%d_o%d_" % (nband, k)
        groups.setdefault((g[tag + "psf_pars"].size, float(g[tag + "tol"])), []).append(tag)
    for (_, tol), tags in sorted(groups.items()):
        obs, psfs, sobj, sband = [], [], [], []
        for o, tag in enumerate(tags):
            jac = g[tag + "jac"]
            rec = ngmix.GMix(pars=g[tag + "psf_pars"]).get_data().copy()
            for s, b in enumerate(g[tag + "band"]):
                r = jac[s]
                j = ngmix.Jacobian(row=float(r["row0"]), col=float(r["col0"]),
                                   dvdrow=float(r["dvdrow"]), dvdcol=float(r["dvdcol"]),
                                   dudrow=float(r["dudrow"]), dudcol=float(r["dudcol"]))
                im = g[tag + "images"][s]
                obs.append(ngmix.Observation(
                    im, weight=np.full(im.shape, 1.0 / g[tag + "sigma"][s] ** 2), jacobian=j))
                psfs.append(rec)
                sobj.append(o)
                sband.append(int(b))
        sb = StampBatch.from_observations(obs)
        psf = GMixBatch.from_numpy(np.stack(psfs))
        fit_pars = None if tol == 1.0e-5 else {"ftol": tol, "xtol": tol, "maxfev": 4000}
        _lib.launch_census(reset=True)
        res = LMBatchFitter("exp", fit_pars=fit_pars).go(
            sb, np.stack([g[t + "guess"] for t in tags]), psf=psf,
            stamp_obj=np.array(sobj, dtype=np.int32), stamp_band=np.array(sband, dtype=np.int32))
        seen = _lib.launch_census(reset=True)
        assert _census_has(seen, "lm_advance_team_kernel") == (5 + nband >= 9), seen
        for o, tag in enumerate(tags):
            assert res["flags"][o] == int(g[tag + "flags"]) == 0
            assert res["nfev"][o] == int(g[tag + "nfev"]), (tag, res["nfev"][o])
            assert res["ier"][o] == int(g[tag + "ier"])
            np.testing.assert_allclose(res["pars"][o], g[tag + "pars"], rtol=1e-6, atol=1e-8)
            refcov = g[tag + "pars_cov"]
            sig = np.sqrt(np.diag(refcov))
            lim = 1e-4 * np.abs(refcov) + 1e-7 * np.outer(sig, sig)
            assert np.all(np.abs(res["pars_cov"][o] - refcov) <= lim), tag
            np.testing.assert_allclose(res["pars_err"][o], g[tag + "pars_err"], rtol=1e-4)
            for k in ("lnprob", "chi2per", "s2n"):
                np.testing.assert_allclose(res[k][o], float(g[tag + k]), rtol=1e-5)
            assert res["dof"][o] == int(g[tag + "dof"]) and res["npix"][o] == int(g[tag + "npix"])


@pytest.mark.parametrize("hint", [True, False], ids=["team", "generic"])
def test_a_band_the_fit_has_no_flux_for_ends_that_fit_alone(hint):
    """a stamp_band beyond the fit's fluxes (nloc - 1 + band >= n: a caller of
    ngmix_lm_advance_batch's mistake, LMBatchFitter validates its maps) would put
    the stamp's sums outside the fit's arrays -- in the team form, inside a
    NEIGHBOURING fit's LDS block.  The step ends that fit as it ends one with a
    wrong parameter-count hint (info 0) and every other fit of the wave is what
    it is without the corruption, to the bit"""
    rng = np.random.RandomState(13)
    nobj, nband = 8, 7
    sb, psf, guess, sobj, sband = _multiband(nobj, nband, "exp", rng)

    def run(corrupt):
        f = LMBatchFitter("exp")
        f.host_loop = True
        f.advance_hint = hint

        def hook(job, r):
            if corrupt and r == 0:
                first = int(np.nonzero(sobj == 3)[0][0])
                job.d_sband[first] = 9        # 5 + 9 = 14 >= n = 12
        f.round_hook = hook
        return f.go(sb, guess, psf=psf, stamp_obj=sobj, stamp_band=sband)
    clean, bad = run(False), run(True)
    assert np.all(clean["flags"] == 0)
    assert bad["flags"][3] == ngmix.flags.LM_FUNC_NOTFINITE and bad["ier"][3] == 0
    others = np.arange(nobj) != 3
    for k in ("flags", "nfev", "ier", "pars", "pars_err"):
        np.testing.assert_array_equal(bad[k][others], clean[k][others], err_msg=k)


def test_coellip3_small_batch_equals_a_batch_of_65():
    """co-elliptical fits with 3 gaussians (10 parameters: the team step and the
    double-double covariance of ngmix_lm_precise_cov_batch) on 17 x 19 stamps:
    five objects (three fits that end with flags == 0, two that run out of
    evaluations) out of the small batch's single allocation against the same
    five among 65 objects in separate buffers -- every key to the bit"""
    from ngmix_amd.lm_batch import SMALL_BATCH
    rng = np.random.RandomState(17)
    nrow, ncol, n, few, ngauss = 17, 19, SMALL_BATCH + 1, 5, 3
    jac = ngmix.Jacobian(row=8.0, col=9.0, dvdrow=0.263, dvdcol=0.0, dudrow=0.0, dudcol=0.263)
    gm = ngmix.GMixModel([0.0, 0.0, 0.02, -0.01, 0.3, 1.0], "turb")
    im0 = gm.make_image((nrow, ncol), jacobian=jac)
    images = im0[None] + 2.0e-4 * rng.normal(size=(n, nrow, ncol))
    weights = np.full((n, nrow, ncol), 1.0 / 2.0e-4 ** 2)
    T = 0.3 * np.array([0.3, 0.7, 1.5])
    F = np.array([0.3, 0.45, 0.25])
    g0 = np.concatenate([[0.0, 0.0, 0.02, -0.01], T, F / F.sum()])
    guess = g0[None] * rng.uniform(0.9, 1.1, size=(n, g0.size))
    guess[:, :2] = rng.uniform(-0.01, 0.01, size=(n, 2))
    pars = {"maxfev": 120, "ftol": 1e-5, "xtol": 1e-5}

    def fit(idx):
        f = LMBatchFitter("coellip", ngauss=ngauss, fit_pars=pars)
        f.keep_job = True
        res = f.go(StampBatch.from_images(images[idx], weights[idx], jac), guess[idx])
        assert f.last_job.d_jacpt is not None and f.last_job.d_psums is not None
        assert (f.last_job.arena is not None) == (len(idx) <= SMALL_BATCH)
        return res
    _lib.launch_census(reset=True)
    large = fit(np.arange(n))
    assert _census_has(_lib.launch_census(reset=True), "lm_advance_team_kernel<")
    ended, not_ended = np.flatnonzero(large["flags"] == 0), np.flatnonzero(large["flags"] != 0)
    assert ended.size >= 3 and not_ended.size >= 2
    idx = np.sort(np.concatenate([ended[:3], not_ended[:2]]))
    assert idx.size == few
    small = fit(idx)
    assert set(small.keys()) == set(large.keys())
    for k in small.keys():
        if k != "model":
            assert np.array_equal(np.asarray(small[k]), np.asarray(large[k])[idx],
                                  equal_nan=True), k
