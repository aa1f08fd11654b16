"""
The noise-power sandwich covariance on the device (csrc/noisecov.hip,
noise_cov.noise_cov_device) and the public routes that use it:
LMBatchFitter(use_noise_image=True), Fitter(use_noise_image=True).go_many,
runners.run_fitter_many, pipeline.bootstrap_batch / bootstrap_many.

Checked against numpy's FFT (the Gram blocks), against the torch path
calc_noise_cov_batch (the covariances), against the reference's own numbers
(tests/golden), and against the per-object MINPACK route.
"""
import numpy as np
import pytest

import ngmix_amd as ngmix

pytestmark = pytest.mark.gpu

SCALE = 0.263
NSHAPE = {"gauss": 5, "exp": 5, "dev": 5, "turb": 5, "bdf": 6, "bd": 7}


def _torch():
    import torch
    return torch


def _jac(rec):
    v = {k: np.asarray(rec[k]).item() for k in ("row0", "col0", "dvdrow", "dvdcol",
                                                 "dudrow", "dudcol")}
    return ngmix.Jacobian(row=v["row0"], col=v["col0"], dvdrow=v["dvdrow"],
                          dvdcol=v["dvdcol"], dudrow=v["dudrow"], dudcol=v["dudcol"])


def _corr_noise(rng, shape, sigma=0.02, axis=None):
    """stationary correlated noise: neighbours along rows and columns, or along
    one axis only"""
    w = rng.normal(size=shape)
    if axis is None:
        return sigma * (w + np.roll(w, 1, axis=0) + np.roll(w, 1, axis=1))
    return sigma * (w + np.roll(w, 1, axis=axis) + 0.5 * np.roll(w, 2, axis=axis))


def _truth(rng, model, nband):
    shape = [rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05),
             rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.4, 0.9)]
    if model == "bdf":
        shape.append(rng.uniform(0.3, 0.7))
    if model == "bd":
        shape += [rng.uniform(-0.3, 0.3), rng.uniform(0.3, 0.7)]
    return np.array(shape + list(rng.uniform(60.0, 120.0, size=nband)))


def _sim(rng, model="exp", nep=1, nband=1, dims=(32, 32), noise_nan=False):
    """one object: a MultiBandObsList (nband > 1), an ObsList (nep > 1) or an
    Observation, every observation with a noise image and a psf observation
    (image and mixture); returns (obs, truth)"""
    truth = _truth(rng, model, nband)
    nshape = NSHAPE[model]
    pgm = ngmix.GMixModel([0.0, 0.0, 0.01, 0.02, 0.25, 1.0], "gauss")
    mb = ngmix.MultiBandObsList()
    for b in range(nband):
        ol = ngmix.ObsList()
        bpars = np.concatenate([truth[:nshape], truth[nshape + b:nshape + b + 1]])
        for e in range(nep):
            cen = ((dims[0] - 1) / 2.0 + rng.uniform(-0.3, 0.3),
                   (dims[1] - 1) / 2.0 + rng.uniform(-0.3, 0.3))
            jac = ngmix.DiagonalJacobian(row=cen[0], col=cen[1], scale=SCALE)
            im = ngmix.GMixModel(bpars, model).convolve(pgm).make_image(
                dims, jacobian=jac, fast_exp=True)
            noise = _corr_noise(rng, (2,) + tuple(dims))
            if noise_nan:
                noise[1, 3, 4] = np.nan
            pjac = ngmix.DiagonalJacobian(row=7.0, col=7.0, scale=SCALE)
            pim = pgm.make_image((15, 15), jacobian=pjac) + 1.0e-5 * rng.normal(size=(15, 15))
            pobs = ngmix.Observation(pim, weight=np.full(pim.shape, 1.0e10), jacobian=pjac,
                                     gmix=pgm.copy())
            ol.append(ngmix.Observation(im + noise[0],
                                        weight=np.full(im.shape, 1.0 / (3 * 0.02 ** 2)),
                                        jacobian=jac, psf=pobs, noise=noise[1]))
        mb.append(ol)
    if nband > 1:
        return mb, truth
    if nep > 1:
        return mb[0], truth
    return mb[0][0], truth


def _guess(rng, truth):
    g = truth * (1.0 + 0.02 * rng.uniform(-1, 1, size=truth.size))
    g[0:2] = truth[0:2] + 0.01 * rng.uniform(-1, 1, size=2)
    return g


def _flatten(objs):
    """StampBatch, noise (per stamp), psf records, stamp_obj, stamp_band"""
    from ngmix_amd.batch import flatten_observations
    from ngmix_amd.noise_cov import noise_of_observations
    stamps, sobj, sband, nband, psf = flatten_observations(objs)
    return stamps, noise_of_observations(objs), psf, sobj, sband, nband


def _scaled_diff(a, b):
    """max |a - b| / sqrt(|b_aa b_bb|) over the entries of each matrix"""
    d = np.sqrt(np.abs(np.diagonal(b, axis1=-2, axis2=-1)))
    scale = d[..., :, None] * d[..., None, :]
    return float(np.max(np.abs(a - b) / scale))


# ---------------------------------------------------------------------------
# 1. the kernel against numpy's FFT
# ---------------------------------------------------------------------------

def _blocks_np(D, w, n):
    npix = n[0].size
    K = np.fft.fft2(w[:, None] * D, axes=(2, 3))
    P = np.abs(np.fft.fft2(n, axes=(1, 2))) ** 2
    return np.einsum("saxy,sbxy,sxy->sab", K.conj(), K, P).real / float(npix) ** 2


@pytest.mark.parametrize("shape", [(17, 17), (25, 25), (32, 32), (31, 45), (48, 48),
                                   (64, 64), (128, 96)])
@pytest.mark.parametrize("nloc", [6, 8])
def test_blocks_kernel_vs_numpy_fft(shape, nloc):
    from ngmix_amd import _lib
    from ngmix_amd.batch import _dptr
    torch = _torch()
    rng = np.random.RandomState(sum(shape) + nloc)
    nrow, ncol = shape
    m = 5
    D = rng.normal(size=(m, nloc, nrow, ncol)) * rng.uniform(0.1, 10.0, size=(1, nloc, 1, 1))
    ierr = rng.uniform(0.5, 2.0, size=(m, nrow, ncol))
    noise = np.stack([_corr_noise(rng, shape, axis=s % 2) for s in range(m)])
    # the stamps lie in the batch in another order than in the chunk
    order = np.array([3, 0, 4, 1, 2])
    pix_off = np.arange(m, dtype=np.int64) * nrow * ncol
    dev = torch.device("cuda")
    d_ierr = torch.from_numpy(ierr[np.argsort(order)].reshape(-1)).to(dev)
    d_noise = torch.from_numpy(noise[np.argsort(order)].reshape(-1)).to(dev)
    out = torch.full((m, nloc, nloc), np.nan, dtype=torch.float64, device=dev)
    d_D = torch.from_numpy(D.reshape(-1).copy()).to(dev)
    d_idx = torch.from_numpy(order.astype(np.int64)).to(dev)
    d_off = torch.from_numpy(pix_off).to(dev)
    st = _lib.lib().ngmix_noise_cov_blocks_batch(
        _dptr(d_D), _dptr(d_idx), m, _dptr(d_off), _dptr(d_ierr),
        _dptr(d_noise), None, nloc, nrow, ncol, _dptr(out), None)
    _lib.check(st, "ngmix_noise_cov_blocks_batch")
    got = out.cpu().numpy()[order]
    del d_D, d_idx, d_off, d_ierr, d_noise
    ref = _blocks_np(D, ierr * ierr, noise)
    assert _scaled_diff(got, ref) <= 1e-11
    np.testing.assert_array_equal(got, np.transpose(got, (0, 2, 1)))


def test_blocks_kernel_deriv_planes():
    """the flux form: deriv_images' six planes [value, cen1, cen2, g1, g2, T],
    the flux derivative value / flux"""
    from ngmix_amd import _lib
    from ngmix_amd.batch import _dptr
    torch = _torch()
    rng = np.random.RandomState(5)
    nrow, ncol, m = 31, 45, 3
    D6 = rng.normal(size=(m, 6, nrow, ncol))
    flux = rng.uniform(10.0, 100.0, size=m)
    ierr = rng.uniform(0.5, 2.0, size=(m, nrow, ncol))
    noise = np.stack([_corr_noise(rng, (nrow, ncol)) for _ in range(m)])
    dev = torch.device("cuda")
    out = torch.zeros((m, 6, 6), dtype=torch.float64, device=dev)
    # (every input held by a name until the kernel has run)
    d = [torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev)
         for a in (D6, np.arange(m, dtype=np.int64), np.arange(m, dtype=np.int64) * nrow * ncol,
                   ierr, noise, flux)]
    st = _lib.lib().ngmix_noise_cov_blocks_batch(
        _dptr(d[0]), _dptr(d[1]), m, _dptr(d[2]), _dptr(d[3]), _dptr(d[4]), _dptr(d[5]), 6,
        nrow, ncol, _dptr(out), None)
    _lib.check(st, "ngmix_noise_cov_blocks_batch")
    D = np.concatenate([D6[:, 1:6], (D6[:, 0] / flux[:, None, None])[:, None]], axis=1)
    assert _scaled_diff(out.cpu().numpy(), _blocks_np(D, ierr * ierr, noise)) <= 1e-11


# ---------------------------------------------------------------------------
# 2. / 3. against the torch path, and deterministic
# ---------------------------------------------------------------------------

def _catalogue(model, nobj, seed, nband=1, max_ep=4, dims=(32, 32)):
    rng = np.random.RandomState(seed)
    objs, truths = [], []
    for o in range(nobj):
        nep = 1 + o % max_ep
        ob, truth = _sim(rng, model, nep=nep, nband=nband, dims=dims)
        objs.append(ob)
        truths.append(truth)
    return objs, np.array(truths)


def _at_truth_inputs(objs, truths, model, seed):
    """pars near the truth and a positive definite pars_cov0 per object"""
    rng = np.random.RandomState(seed)
    n = truths.shape[1]
    pars = truths * (1.0 + 1.0e-3 * rng.uniform(-1, 1, size=truths.shape))
    a = rng.normal(size=(truths.shape[0], n, n)) * 0.1
    cov0 = np.einsum("oij,okj->oik", a, a) + np.eye(n)[None] * 0.05
    cov0 *= (np.abs(truths)[:, :, None] * np.abs(truths)[:, None, :]) ** 0.5 * 1e-2
    return pars, cov0


@pytest.mark.parametrize("model,nband", [("exp", 1), ("exp", 2), ("turb", 1), ("bdf", 2),
                                         ("bd", 1)])
def test_device_vs_torch_path(model, nband):
    from ngmix_amd.noise_cov import calc_noise_cov_batch, noise_cov_device
    torch = _torch()
    objs, truths = _catalogue(model, 9, 11 + nband, nband=nband)
    stamps, noise, psf, sobj, sband, _ = _flatten(objs)
    pars, cov0 = _at_truth_inputs(objs, truths, model, 3)
    flat_noise = torch.from_numpy(np.concatenate([n.reshape(-1) for n in noise])).to(
        stamps.device)
    from ngmix_amd.noise_cov import _psf_batch
    gpsf = _psf_batch(psf, stamps.n, stamps.device)
    ref = calc_noise_cov_batch(stamps, flat_noise, model, pars, cov0, psf=gpsf,
                               stamp_obj=sobj, stamp_band=sband)
    # host noise arrays, objects spread over chunk boundaries (7 stamps a chunk)
    got = noise_cov_device(stamps, noise, model, pars, cov0, psf=psf, stamp_obj=sobj,
                           stamp_band=sband, chunk_stamps=7).cpu().numpy()
    assert np.all(np.isfinite(ref))
    assert _scaled_diff(got, ref) <= 1e-11
    # device inputs and the flat noise tensor: the same bits
    again = noise_cov_device(stamps, flat_noise, model, torch.from_numpy(pars).cuda(),
                             torch.from_numpy(cov0).cuda(), psf=gpsf, stamp_obj=sobj,
                             stamp_band=sband, chunk_stamps=7).cpu().numpy()
    np.testing.assert_array_equal(again, got)


def test_device_deterministic_across_batches():
    """two runs give the same bits; so does an object alone, and inside a
    larger, reordered batch of other chunks"""
    from ngmix_amd.noise_cov import noise_cov_device
    objs, truths = _catalogue("exp", 12, 21, nband=2, max_ep=3)
    pars, cov0 = _at_truth_inputs(objs, truths, "exp", 4)
    stamps, noise, psf, sobj, sband, _ = _flatten(objs)
    a = noise_cov_device(stamps, noise, "exp", pars, cov0, psf=psf, stamp_obj=sobj,
                         stamp_band=sband).cpu().numpy()
    b = noise_cov_device(stamps, noise, "exp", pars, cov0, psf=psf, stamp_obj=sobj,
                         stamp_band=sband).cpu().numpy()
    np.testing.assert_array_equal(a, b)
    perm = np.random.RandomState(0).permutation(len(objs))
    sub = [objs[i] for i in perm]
    stamps2, noise2, psf2, sobj2, sband2, _ = _flatten(sub)
    c = noise_cov_device(stamps2, noise2, "exp", pars[perm], cov0[perm], psf=psf2,
                         stamp_obj=sobj2, stamp_band=sband2, chunk_stamps=5).cpu().numpy()
    np.testing.assert_array_equal(c, a[perm])
    k = int(perm[3])
    stamps3, noise3, psf3, sobj3, sband3, _ = _flatten([objs[k]])
    d = noise_cov_device(stamps3, noise3, "exp", pars[k:k + 1], cov0[k:k + 1], psf=psf3,
                         stamp_obj=sobj3, stamp_band=sband3).cpu().numpy()
    np.testing.assert_array_equal(d[0], a[k])


# ---------------------------------------------------------------------------
# 4. the reference's own numbers
# ---------------------------------------------------------------------------

def _nc_obslist(g):
    psf = ngmix.Observation(g["psf_image"], jacobian=_jac(g["psf_jac"]),
                            gmix=ngmix.GMix(pars=g["psf_pars"]))
    ol = ngmix.ObsList()
    for e in range(2):
        pre = "nc_e%d_" % e
        ol.append(ngmix.Observation(g[pre + "image"], weight=g[pre + "weight"],
                                    jacobian=_jac(g[pre + "jac"]), psf=psf,
                                    noise=g[pre + "noise"]))
    return ol


def test_go_many_golden_sandwich(golden):
    g = golden("extra")
    res = ngmix.fitting.Fitter(model="exp", use_noise_image=True).go_many(
        [_nc_obslist(g)], g["nc_guess"][None])[0]
    tag = "nc_sandwich"
    assert res["flags"] == int(g[tag + "_flags"]) == 0
    assert res["nfev"] == int(g[tag + "_nfev"])
    np.testing.assert_allclose(res["pars"], g[tag + "_pars"], rtol=1e-7, atol=1e-9)
    refcov = g[tag + "_pars_cov"]
    sig = np.sqrt(np.diag(refcov))
    assert np.all(np.abs(res["pars_cov"] - refcov) <=
                  1e-5 * np.abs(refcov) + 1e-8 * np.outer(sig, sig))
    np.testing.assert_allclose(res["pars_err"], g[tag + "_pars_err"], rtol=1e-5)
    # the derived keys come from the sandwich
    np.testing.assert_array_equal(res["g_cov"], res["pars_cov"][2:4, 2:4])
    assert res["T_err"] == res["pars_err"][4]
    assert res["flux_err"] == res["pars_err"][5]


@pytest.mark.parametrize("model", ["turb", "bdf"])
def test_device_central_differences_vs_reference(golden, model):
    from ngmix_amd.noise_cov import noise_cov_device
    from ngmix_amd.batch import StampBatch
    g, g2 = golden("extra"), golden("api2")
    ol = _nc_obslist(g)
    sb = StampBatch.from_observations(list(ol))
    psf = np.stack([ob.psf.gmix.get_data().copy() for ob in ol])
    pre = "ncfd_%s_" % model
    pars, cov0, ref = g2[pre + "pars"], g2[pre + "pars_cov0"], g2[pre + "pars_cov"]
    cov = noise_cov_device(sb, [ob.noise for ob in ol], model, pars[None], cov0[None],
                           psf=psf, stamp_obj=np.zeros(2, dtype=np.int64)).cpu().numpy()[0]
    sig = np.sqrt(np.diag(ref))
    np.testing.assert_allclose(cov, ref, rtol=1e-6, atol=1e-8 * np.outer(sig, sig).max())


# ---------------------------------------------------------------------------
# 5. many against one
# ---------------------------------------------------------------------------

def _prior():
    from ngmix_amd import priors, joint_prior
    prng = np.random.RandomState(3)
    return joint_prior.PriorSimpleSep(
        priors.CenPrior(0.0, 0.0, SCALE, SCALE, rng=prng), priors.GPriorBA(0.3, rng=prng),
        priors.LogNormal(0.6, 0.4, rng=prng),
        priors.TwoSidedErf(-10.0, 1.0, 1.0e4, 100.0, rng=prng))


def _compare_one(r, one, tsig, rtol):
    """a go_many element against the per-object MINPACK result: pars within
    tsig of the errors, the covariance and the errors cut from it to rtol"""
    assert r["flags"] == one["flags"]
    if r["flags"] != 0:
        assert r["errmsg"] == one["errmsg"]
    assert np.all(np.abs(r["pars"] - one["pars"]) <= tsig * one["pars_err"])
    sig = np.sqrt(np.abs(np.diag(one["pars_cov"])))
    assert np.all(np.abs(r["pars_cov"] - one["pars_cov"]) <=
                  rtol * np.abs(one["pars_cov"]) + rtol * np.outer(sig, sig))
    np.testing.assert_allclose(r["pars_err"], one["pars_err"], rtol=rtol)
    if r["flags"] == 0:
        for k in ("g_cov", "g_err", "T_err", "flux_err"):
            np.testing.assert_allclose(r[k], one[k], rtol=rtol, atol=rtol * 1e-6, err_msg=k)


@pytest.mark.parametrize("case", ["exp", "bdf", "exp2band", "exp_prior"])
def test_go_many_matches_per_object(case):
    model = "bdf" if case == "bdf" else "exp"
    nband = 2 if case == "exp2band" else 1
    prior = _prior() if case == "exp_prior" else None
    rng = np.random.RandomState({"exp": 1, "bdf": 2, "exp2band": 3, "exp_prior": 4}[case])
    objs, guesses = [], []
    nobj = 14 if case == "exp" else 12
    for o in range(nobj):
        ob, truth = _sim(rng, model, nep=1 + o % 2, nband=nband)
        objs.append(ob)
        guesses.append(_guess(rng, truth))
    guesses = np.array(guesses)
    many = ngmix.fitting.Fitter(model=model, prior=prior, use_noise_image=True).go_many(
        objs, guesses)
    plain = ngmix.fitting.Fitter(model=model, prior=prior).go_many(objs, guesses)
    tsig, rtol = (1e-3, 1e-4) if model == "exp" else (2e-2, 2e-2)
    for i, ob in enumerate(objs):
        one = ngmix.fitting.Fitter(model=model, prior=prior, use_noise_image=True,
                                   batched=False).go(obs=ob, guess=guesses[i])
        r = many[i]
        assert one["flags"] == 0 and r["flags"] == 0
        assert sorted(r.keys()) == sorted(plain[i].keys())
        _compare_one(r, one, tsig, rtol)
        # the fit itself is the plain one, bit for bit
        np.testing.assert_array_equal(r["pars"], plain[i]["pars"])
        assert r["nfev"] == plain[i]["nfev"]


def test_sandwich_failure_flags_match_per_object():
    """a solution where a central-difference step leaves the model's domain:
    the covariance flags, 'bad noise covariance matrix' and the default
    errors, as the per-object apply_noise_cov gives them"""
    from ngmix_amd.defaults import CDEF
    from ngmix_amd.fitting import FitModel, ManyResults
    from ngmix_amd.noise_cov import apply_noise_cov, apply_noise_cov_device
    rng = np.random.RandomState(7)
    objs, truths = [], []
    for o in range(3):
        ob, truth = _sim(rng, "turb")
        objs.append(ob)
        truths.append(truth)
    pars = np.array(truths)
    pars[1, 2:4] = [0.99995, 0.0]   # g1 + 1e-4 >= 1: out of range
    n = pars.shape[1]
    cov0 = np.tile(np.eye(n) * 1e-3, (3, 1, 1))
    stamps, noise, psf, sobj, sband, _ = _flatten(objs)
    res = {"flags": np.zeros(3, dtype=np.int64), "pars": pars.copy(),
           "pars_err": np.full((3, n), 0.1), "pars_cov0": cov0,
           "pars_cov": cov0.copy(), "nfev": np.ones(3, dtype=np.int64),
           "ier": np.ones(3, dtype=np.int64)}
    apply_noise_cov_device(res, stamps, noise, "turb", psf=psf, stamp_obj=sobj,
                           stamp_band=sband)
    for i, ob in enumerate(objs):
        one = {"flags": 0, "pars": pars[i].copy(), "pars_cov0": cov0[i].copy(),
               "pars_cov": cov0[i].copy(), "pars_err": np.full(n, 0.1), "errmsg": ""}
        apply_noise_cov(FitModel(obs=ob, model="turb", guess=pars[i]), one)
        assert res["flags"][i] == one["flags"]
        assert bool(res["noise_cov_failed"][i]) == (one["flags"] != 0)
        if one["flags"]:
            assert one["errmsg"] == "bad noise covariance matrix"
            np.testing.assert_array_equal(res["pars_cov"][i], CDEF)
            np.testing.assert_array_equal(res["pars_err"][i], CDEF)
            assert ManyResults(res, "turb", 1)[i]["errmsg"] == one["errmsg"]
        else:
            sig = np.sqrt(np.diag(one["pars_cov"]))
            assert np.all(np.abs(res["pars_cov"][i] - one["pars_cov"]) <=
                          1e-5 * np.outer(sig, sig))
    assert res["flags"][1] != 0 and res["flags"][0] == 0


# ---------------------------------------------------------------------------
# 6. retries and the bootstrap
# ---------------------------------------------------------------------------

def test_run_fitter_many_retries_failed_sandwich():
    """objects whose fit converges but whose sandwich fails (a NaN in the noise
    image) are fitted again; the others are not"""
    from ngmix_amd.runners import run_fitter_many
    rng = np.random.RandomState(8)
    objs, truths = [], []
    bad = {1, 4}
    for o in range(6):
        ob, truth = _sim(rng, "exp", noise_nan=o in bad)
        objs.append(ob)
        truths.append(truth)
    truths = np.array(truths)
    calls = []

    def guesser(obs):
        i = next(k for k, o in enumerate(objs) if o is obs)
        calls.append(i)
        return truths[i] * 1.01

    out = run_fitter_many(objs, ngmix.fitting.Fitter(model="exp", use_noise_image=True),
                          guesser, ntry=2)
    assert sorted(calls) == sorted(list(range(6)) + sorted(bad))
    for i, r in enumerate(out):
        if i in bad:
            assert r["ntry"] == 2 and r["flags"] != 0
            assert r["errmsg"] == "bad noise covariance matrix"
        else:
            assert r["ntry"] == 1 and r["flags"] == 0


def _boot_objects(seed, nobj, nband=1, nan_obj=()):
    rng = np.random.RandomState(seed)
    objs = []
    for o in range(nobj):
        ob, _ = _sim(rng, "exp", nep=1 + o % 2, nband=nband, noise_nan=o in nan_obj)
        objs.append(ob)
    return objs


def test_bootstrap_many_and_batch_noise_image():
    from ngmix_amd.batch import flatten_observations
    from ngmix_amd.noise_cov import calc_noise_cov_batch, noise_of_observations
    from ngmix_amd.pipeline import bootstrap_many, bootstrap_batch
    objs = _boot_objects(9, 10, nan_obj=(3,))
    plain = bootstrap_many(objs, model="exp", ntry=2, rng=np.random.RandomState(1))
    nc = bootstrap_many(objs, model="exp", ntry=2, rng=np.random.RandomState(1),
                        use_noise_image=True)
    stamps, sobj, sband, _, _ = flatten_observations(objs)
    noise = noise_of_observations(objs)
    torch = _torch()
    flat_noise = torch.from_numpy(np.concatenate([n.reshape(-1) for n in noise])).cuda()
    pa, na = plain.arrays, nc.arrays
    for i in range(len(objs)):
        if i == 3:
            # the sandwich fails: flagged, retried
            assert na["flags"][i] != 0 and na["ntry"][i] == 2
            assert nc[i]["errmsg"] == "bad noise covariance matrix"
            continue
        assert na["flags"][i] == pa["flags"][i] == 0
        assert na["nfev"][i] == pa["nfev"][i]
        np.testing.assert_array_equal(na["pars"][i], pa["pars"][i])
    ok = np.nonzero(na["flags"] == 0)[0]
    ref = calc_noise_cov_batch(stamps, flat_noise, "exp", na["pars"], na["pars_cov0"],
                               psf=na["psf_gmix"], stamp_obj=sobj, stamp_band=sband)
    assert _scaled_diff(np.asarray(na["pars_cov"])[ok], ref[ok]) <= 1e-11
    # bootstrap_batch with the flat noise tensor: the same result
    from ngmix_amd.batch import StampBatch
    from ngmix_amd.observation import get_mb_obs
    flat = [e for o in objs for ol in get_mb_obs(o) for e in ol]
    psb = StampBatch.from_observations([e.psf for e in flat])
    bb = bootstrap_batch(stamps, psb, model="exp", ntry=2, rng=np.random.RandomState(1),
                         stamp_obj=sobj, stamp_band=sband, use_noise_image=True,
                         noise=flat_noise)
    np.testing.assert_array_equal(bb["flags"], na["flags"])
    np.testing.assert_array_equal(np.asarray(bb["pars_cov"])[ok], np.asarray(na["pars_cov"])[ok])


def test_lm_batch_fitter_noise_image_go_stream():
    """LMBatchFitter(use_noise_image=True): go and go_stream agree"""
    from ngmix_amd.lm_batch import LMBatchFitter
    rng = np.random.RandomState(10)
    objs, guesses = [], []
    for o in range(8):
        ob, truth = _sim(rng, "exp")
        objs.append(ob)
        guesses.append(_guess(rng, truth))
    guesses = np.array(guesses)
    stamps, noise, psf, sobj, sband, _ = _flatten(objs)
    f = LMBatchFitter("exp", use_noise_image=True)
    a = f.go(stamps, guesses, psf=psf, noise=noise)
    b = list(f.go_stream([(stamps, guesses, {"psf": psf, "noise": noise})] * 2))
    for r in b:
        np.testing.assert_array_equal(np.asarray(r["pars_cov"]), np.asarray(a["pars_cov"]))
    with pytest.raises(ValueError, match="noise image"):
        f.go(stamps, guesses, psf=psf, noise=noise[:-1])
