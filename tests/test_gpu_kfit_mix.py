"""
The Fourier-space 'dev10' and 'bdf' models on the device:
kfit_eval_kernel and kfit_flux_kernel against the dense longdouble reference at
the host tests' gate, what only a launch can show (the census, repeatability, a
stamp independent of its batch), and the Python layer -- noise-free fits, a
PriorBDFSep, the metacal route and the template flux.
"""
import ctypes

import numpy as np
import pytest

from ngmix_amd import _lib, joint_prior, priors, prior_batch as PB
from ngmix_amd.kfit import (KSpaceBatchFitter, KSpaceFluxBatch, KStampBatch, kmodel_images)

from helpers import kfit_cases as KC
from helpers import kfit_mix_cases as MC
from helpers import kfit_mix_reference as MR
from helpers import kfit_reference as K

pytestmark = pytest.mark.gpu

KEYS = sorted(MC.sums_cases())
NAME = {MR.DEV10: "dev10", MR.BDF: "bdf"}
TIGHT = {"ftol": 1e-10, "xtol": 1e-10, "maxfev": 400}
SHAPE = (15, 15)


def _torch():
    import torch
    return torch


def _dev(a, dtype=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.dtype.names is not None:
        a = a.view(np.uint8)
    return _torch().from_numpy(a).cuda()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def eval_device(stamps, states, weighted=False, stamp_obj=None, stamp_band=None):
    """ngmix_kfit_eval_batch, or weighted ngmix_kfit_eval_w_batch with the
    stamps' own planes: sums, status, stats, ncomp"""
    torch = _torch()
    dhat, phat, wbar, jac = KC.pack_stamps(stamps)
    R, C = stamps[0]["shape"]
    n = len(stamps)
    d = [_dev(dhat), _dev(phat), _dev(wbar), _dev(jac), _dev(states)]
    so, sb = _dev(stamp_obj, np.int32), _dev(stamp_band, np.int32)
    sums = torch.full((n, K.nsums(MR.NLOC[stamps[0]["model"]])), np.nan, dtype=torch.float64,
                      device="cuda")
    status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    stats = torch.full((n, 2), np.nan, dtype=torch.float64, device="cuda")
    ncomp = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    mid = (_ptr(d[2]), _ptr(d[3]), R, C, n, stamps[0]["model"], _ptr(d[4]), _ptr(so), _ptr(sb),
           _ptr(sums), _ptr(status), _ptr(stats))
    if weighted:
        u = _dev(np.stack([s["u"] for s in stamps]))
        rc = _lib.lib().ngmix_kfit_eval_w_batch(_ptr(d[0]), _ptr(d[1]), _ptr(u), *mid,
                                                _ptr(ncomp), None)
    else:
        rc = _lib.lib().ngmix_kfit_eval_batch(_ptr(d[0]), _ptr(d[1]), *mid, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return sums.cpu().numpy(), status.cpu().numpy(), stats.cpu().numpy(), ncomp.cpu().numpy()


def flux_device(stamps, pars, weighted=False):
    torch = _torch()
    dhat, phat, wbar, jac = KC.pack_stamps(stamps)
    R, C = stamps[0]["shape"]
    n = len(stamps)
    d = [_dev(dhat), _dev(phat), _dev(wbar), _dev(jac), _dev(pars, np.float64)]
    out = torch.full((n, 3), np.nan, dtype=torch.float64, device="cuda")
    status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    mid = (_ptr(d[2]), _ptr(d[3]), R, C, n, stamps[0]["model"], _ptr(d[4]), _ptr(out),
           _ptr(status))
    if weighted:
        u = _dev(np.stack([s["u"] for s in stamps]))
        rc = _lib.lib().ngmix_kfit_flux_w_batch(_ptr(d[0]), _ptr(d[1]), _ptr(u), *mid, None, None)
    else:
        rc = _lib.lib().ngmix_kfit_flux_batch(_ptr(d[0]), _ptr(d[1]), *mid, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "modew"])
@pytest.mark.parametrize("key", KEYS, ids=str)
def test_device_sums_against_the_dense_reference(key, weighted):
    """the host tests' fixtures and gate; one kfit_eval_kernel<dev10 | bdf>
    launch per call (this is the test that the parent commit fails: it has no
    such model ids)"""
    sts = MC.sums_cases()[key]
    refs = MC.references(weighted)[key]
    states = KC.host_states(MC.trial_points(sts))
    _lib.launch_census(reset=True)
    sums, status, stats, ncomp = eval_device(sts, states, weighted)
    census = _lib.launch_census()
    name = "kfit_eval_kernel<%s%s>" % (NAME[key[0]], ", modew" if weighted else "")
    assert census.get(name) == 1 and sum(census.values()) == 1, census
    assert np.all(status == 0)
    ws, wt = MC.worst_of_group(sums, stats, refs)
    print("kfit mix gpu %s %s worst %.2f (stats %.2f) of 2^-52 sum|terms|"
          % (key, "modew" if weighted else "plain", ws, wt))
    assert ws <= MC.C_ROUND and wt <= MC.C_ROUND
    if weighted:
        assert list(ncomp) == [r["ncomp"] for r in refs]


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "modew"])
@pytest.mark.parametrize("key", KEYS, ids=str)
def test_device_flux_sums_against_the_dense_reference(key, weighted):
    sts = MC.sums_cases()[key]
    refs = MC.flux_references(weighted)[key]
    _lib.launch_census(reset=True)
    out, status = flux_device(sts, MC.trial_points(sts)[:, :MR.NLOC[key[0]] - 1], weighted)
    census = _lib.launch_census()
    name = "kfit_flux_kernel<%s%s>" % (NAME[key[0]], ", modew" if weighted else "")
    assert census.get(name) == 1 and sum(census.values()) == 1, census
    assert np.all(status == 0)
    worst = max(KC.worst_ratio(out[i], r[0], r[1]) for i, r in enumerate(refs))
    print("kfit mix flux gpu %s worst %.2f of 2^-52 sum|terms|" % (key, worst))
    assert worst <= MC.C_FLUX


@pytest.mark.parametrize("model", [MR.DEV10, MR.BDF], ids=["dev10", "bdf"])
def test_launches_repeat_and_a_stamp_does_not_see_its_batch(model):
    """37 stamps (ten blocks, the last one a single wave): a second launch is
    equal bit for bit, and so is every stamp launched alone"""
    base = MC.sums_cases()[(model, (9, 12), True)]
    stamps = [base[i % len(base)] for i in range(37)]
    x0 = MC.trial_points(stamps)
    x0[:, 4] *= 1.0 + 0.01 * np.arange(37)       # (every stamp its own point)
    states = KC.host_states(x0)
    a = eval_device(stamps, states)
    b = eval_device(stamps, states)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert np.all(a[1] == 0) and np.all(np.isfinite(a[0]))
    for i in range(37):
        alone = eval_device([stamps[i]], states[i:i + 1])
        assert np.array_equal(alone[0][0], a[0][i]) and np.array_equal(alone[2][0], a[2][i])


def test_two_bands_two_epochs_on_the_device():
    stamps, pars = MC.multiband_case()
    states = KC.host_states(pars[None, :])
    sums, status, stats, _ = eval_device(stamps, states, stamp_obj=[0] * 4,
                                         stamp_band=[s["band"] for s in stamps])
    assert np.all(status == 0)
    refs = [MR.stamp_sums(MR.BDF, s["p"], s["md"], K.from_interleaved(s["dhat"]), MC.phat_of(s),
                          s["wbar"]) for s in stamps]
    ws, wt = MC.worst_of_group(sums, stats, refs)
    assert ws <= MC.C_ROUND and wt <= MC.C_ROUND


def test_out_of_range_points_on_the_device():
    base = MC.sums_cases()[(MR.BDF, (9, 12), True)][1]
    x0 = np.stack([base["p"]] * 5)
    x0[1, 4] = 0.0
    x0[2, 2:4] = 0.8, 0.7
    x0[3, 5] = np.nan
    x0[4, 5] = 7.5                   # fracdev itself is unrestricted
    sums, status, stats, _ = eval_device([base] * 5, KC.host_states(x0))
    assert list(status) == [0] + [_lib.ERR_G_RANGE] * 3 + [0]
    for i in (1, 2, 3):
        assert np.isposinf(sums[i, -1]) and np.all(sums[i, :-1] == 0) and np.all(stats[i] == 0)


# ---- the Python layer ----------------------------------------------------------------

def _kbatch(stamps):
    dhat, phat, wbar, jac = KC.pack_stamps(stamps)
    R, C = stamps[0]["shape"]
    return KStampBatch(_dev(dhat), _dev(phat), _dev(wbar),
                       _dev(jac.view(np.float64).reshape(-1, 8)), R, C)


def _truths(name, nobj, nband, seed):
    """fracdev in [0.2, 0.8], T in [3, 8] of the stamps' units^2, |cen_a| and
    |g_a| in [0.05, 0.3] (away from zero: the gate is relative to the truth)"""
    rng = np.random.RandomState(seed)
    signed = lambda: rng.uniform(0.05, 0.3, nobj) * rng.choice([-1.0, 1.0], nobj)
    cols = [signed(), signed(), signed(), signed(), rng.uniform(3.0, 8.0, nobj)]
    if name == "bdf":
        cols.append(rng.uniform(0.2, 0.8, nobj))
    cols += [rng.uniform(30.0, 90.0, nobj) for _ in range(nband)]
    return np.stack(cols, axis=1)


def _noise_free(name, truth, nband):
    """one stamp per (object, band), its transform the helper's model at the truth"""
    mid = MR.MODEL_ID[name]
    nloc = MR.NLOC[mid]
    base = [KC.make_stamp(SHAPE, jn, ("gauss", None), SHAPE, 60 + b)
            for b, jn in zip(range(nband), ["diag", "aniso", "rotflip"])]
    stamps, sobj, sband = [], [], []
    for i, t in enumerate(truth):
        for b in range(nband):
            s = dict(base[b])
            p = np.concatenate([t[:nloc - 1], [t[nloc - 1 + b]]])
            s["dhat"] = K.interleaved(MR.model(mid, p, s["md"], MC.phat_of(s), jac=False)["M"])
            s["model"] = mid
            stamps.append(s)
            sobj.append(i)
            sband.append(b)
    return stamps, sobj, sband


def _guess(truth, seed):
    rng = np.random.RandomState(seed)
    g = truth * (1.0 + 0.04 * rng.uniform(-1, 1, truth.shape))
    g[:, :4] = truth[:, :4] + 0.03 * rng.uniform(-1, 1, (truth.shape[0], 4))
    return g


@pytest.mark.parametrize("name,nband", [("dev10", 1), ("bdf", 1), ("bdf", 3)])
def test_noise_free_fits_reach_the_truth(name, nband):
    """64 objects (16 with three bands: npars = 9, the team step), zero residual
    at the truth: 1e-7 relative on every parameter, ier in 1..4"""
    nobj = 64 if nband == 1 else 16
    truth = _truths(name, nobj, nband, 11)
    stamps, sobj, sband = _noise_free(name, truth, nband)
    kb = _kbatch(stamps)
    _lib.launch_census(reset=True)
    fitter = KSpaceBatchFitter(name, fit_pars=TIGHT)
    res = fitter.go(kb, _guess(truth, 12), stamp_obj=sobj, stamp_band=sband)
    census = _lib.launch_census()
    n = truth.shape[1]
    assert np.all(res["flags"] == 0), res["flags"]
    assert np.all((res["ier"] >= 1) & (res["ier"] <= 4)), res["ier"]
    err = np.abs(res["pars"] - truth) / np.abs(truth)
    print("kfit fit %s x %d bands: worst relative error per parameter %s, nfev <= %d, rounds %d"
          % (name, nband, np.array2string(err.max(axis=0), precision=2), res["nfev"].max(),
             fitter.rounds_launched))
    assert err.max() <= 1e-7
    assert any(k.startswith("kfit_eval_kernel<%s>" % name) for k in census), census
    team = sum(v for k, v in census.items() if k.startswith("lm_advance_team_kernel"))
    assert (team > 0) == (n >= 9), census
    assert "r50" not in res
    assert np.array_equal(res["T"], res["pars"][:, 4])
    assert np.array_equal(res["T_err"], res["pars_err"][:, 4])
    assert np.array_equal(res["flux"], res["pars"][:, n - nband:])
    if name == "bdf":
        assert np.array_equal(res["fracdev"], res["pars"][:, 5])
        assert np.array_equal(res["fracdev_err"], res["pars_err"][:, 5])
    else:
        assert "fracdev" not in res
    # the model image of the fit is the data's, through kmodel_images
    nloc = MR.NLOC[MR.MODEL_ID[name]]
    loc = np.concatenate([res["pars"][sobj, :nloc - 1],
                          res["pars"][sobj, nloc - 1 + np.array(sband)][:, None]], axis=1)
    img = kmodel_images(kb, loc, name).cpu().numpy()
    want = MR.model_image(MR.MODEL_ID[name], loc[0], stamps[0]["md"], MC.phat_of(stamps[0]))
    assert np.abs(img[0] - want).max() <= 1e-9 * np.abs(want).max()
    with pytest.raises(ValueError):
        KSpaceBatchFitter(name, size_type="r50")


def test_bdf_prior_rows_and_bounds():
    """a joint_prior.PriorBDFSep: the device record's rows equal the torch
    path's fill_fdiff_batch to 4e-15, the project's figure for prior rows; the
    fit stays inside the bounds; a prior without the fracdev term is refused"""
    torch = _torch()
    rs = lambda s: np.random.RandomState(s)
    fd = priors.TruncatedGaussian(0.5, 0.3, 0.0, 1.0, rng=rs(4))
    fd.bounds = (0.0, 1.0)           # (its range, handed to leastsqbound too)
    host = joint_prior.PriorBDFSep(
        priors.CenPrior(0.0, 0.0, 0.5, 0.5, rng=rs(1)), priors.GPriorBA(0.3, rng=rs(2)),
        priors.TwoSidedErf(0.5, 0.1, 30.0, 1.0, rng=rs(3)), fd,
        [priors.TwoSidedErf(1.0, 0.5, 500.0, 20.0, rng=rs(5))])
    fitter = KSpaceBatchFitter("bdf", prior=host)
    prior = fitter.prior
    desc = prior.descriptor()
    assert desc is not None and int(desc["nmid"][0]) == 1
    truth = _truths("bdf", 32, 1, 21)
    rows_t, bad = prior.fill_fdiff_batch(torch.from_numpy(truth).cuda())
    rows_t = rows_t.cpu().numpy()
    assert not bool(bad.any())
    for i, p in enumerate(truth):
        rows = np.zeros(16)
        lnp = ctypes.c_double()
        k = _lib.lib().ngmix_simple_sep_prior_eval(_lib.ptr(desc), _lib.ptr(p), _lib.ptr(rows),
                                                   ctypes.byref(lnp))
        assert k == rows_t.shape[1]
        assert np.abs(rows[:k] - rows_t[i]).max() <= 4e-15 * max(1.0, np.abs(rows_t[i]).max())
    stamps, sobj, sband = _noise_free("bdf", truth, 1)
    kb = _kbatch(stamps)
    res = fitter.go(kb, _guess(truth, 22), stamp_obj=sobj, stamp_band=sband)
    assert np.all(res["flags"] == 0), (res["flags"], res["ier"])
    lo, hi = PB.bounds_arrays(prior.bounds, truth.shape[1])
    assert lo[5] == 0.0 and hi[5] == 1.0 and np.all(fitter.states()["bounded"] == 1)
    assert np.all(res["pars"] >= lo) and np.all(res["pars"] <= hi)
    assert np.all(np.isfinite(res["lnprob"]))
    simple = PB.PriorSimpleSepBatch(PB.GaussianCen(0.0, 0.0, 0.5, 0.5), PB.GPriorBA(0.3),
                                    PB.TwoSidedErf(0.5, 0.1, 30.0, 1.0),
                                    PB.TwoSidedErf(1.0, 0.5, 500.0, 20.0))
    with pytest.raises(ValueError):
        KSpaceBatchFitter("bdf", prior=simple).go(kb, _guess(truth, 22))
    # 'dev10' takes it, the size term a T prior
    KSpaceBatchFitter("dev10", prior=simple)._prior_record(6, 1)


def test_template_flux_of_the_truth():
    """KSpaceFluxBatch('bdf') at the truth's shape on noise-free stamps: the
    truth's flux to 1e-12, the flux route's gate for noise-free stamps"""
    truth = _truths("bdf", 16, 1, 31)
    stamps, _, _ = _noise_free("bdf", truth, 1)
    kb = _kbatch(stamps)
    res = KSpaceFluxBatch(model="bdf", pars=truth[:, :6]).go(kb)
    assert np.all(res["flags"] == 0)
    err = np.abs(res["flux"] - truth[:, 6]) / truth[:, 6]
    print("kfit mix template flux: worst relative error %.2e" % err.max())
    assert err.max() <= 1e-12
    with pytest.raises(ValueError):
        KSpaceFluxBatch(model="dev10", pars=truth[:, :5], size_type="fwhm")


def test_metacal_route_takes_bdf():
    """metacal_kfit_batch(model='bdf') on 8 noise-free 24 x 24 stamps of a
    sheared 'bdf' truth under a round gaussian psf of sigma = 2 pixels: every
    type fitted and unflagged, a finite response whose diagonal lies within the
    band the same call with model='exp' gives, +-0.1.  A sanity check of the
    plumbing, not an accuracy claim: the route's accuracy is DESIGN.md 3.26's
    and is not re-measured here."""
    from ngmix_amd.batch import StampBatch
    from ngmix_amd.metacal import metacal_kfit_batch, shear_response
    n, shape = 8, (24, 24)
    deriv = (1.0, 0.0, 0.0, 1.0)
    rng = np.random.RandomState(41)
    md = K.modes(shape[0], shape[1], deriv)
    ksq = md["kv"] ** 2 + md["ku"] ** 2
    P = np.exp(-K.LD(2.0) ** 2 * ksq / 2).astype(K.CLD)
    imgs, psfs, jacs = [], [], []
    for i in range(n):
        cen = (11.5 + rng.uniform(-0.3, 0.3), 11.5 + rng.uniform(-0.3, 0.3))
        md["cen"] = cen
        p = [0.0, 0.0, 0.02, 0.0, rng.uniform(3.0, 5.0), rng.uniform(0.3, 0.7), 100.0]
        imgs.append(MR.model_image(MR.BDF, p, md, P))
        psfs.append(np.asarray(K.gauss_image(shape, cen, deriv, (0, 0, 0, 0, 8.0, 1.0)),
                               dtype=float))
        jacs.append(KC.jac_record(cen, deriv))
    jac = np.concatenate(jacs).view(np.float64).reshape(-1, 8)
    imgs, psfs = np.stack(imgs), np.stack(psfs)
    sb = StampBatch.from_images(imgs, np.full(imgs.shape, 1.0e4), jac)
    psf_sb = StampBatch.from_images(psfs, None, jac)
    R = {}
    for model in ("bdf", "exp"):
        res = metacal_kfit_batch(sb, psf_sb, model=model, weight="noise")
        assert sorted(res) == ["1m", "1p", "2m", "2p", "noshear"]
        for t, r in res.items():
            assert np.all(r["mcal_flags"] == 0) and np.all(r["flags"] == 0), (model, t)
        if model == "bdf":
            assert "T" in res["noshear"] and "fracdev" in res["noshear"]
        R[model] = shear_response(res)["R"]
        assert np.all(np.isfinite(R[model]))
    for a in range(2):
        lo, hi = R["exp"][:, a, a].min() - 0.1, R["exp"][:, a, a].max() + 0.1
        assert np.all((R["bdf"][:, a, a] >= lo) & (R["bdf"][:, a, a] <= hi)), (R["bdf"], R["exp"])
