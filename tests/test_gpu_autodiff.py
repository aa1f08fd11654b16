"""
Batched log-likelihood gradients (csrc/loglike_grad.hip through
ngmix_amd.autodiff), checked against the existing value kernels, against the
LM driver's own derivative images (deriv_images + fill_fdiff), against
central finite differences (torch.autograd.gradcheck) and against the fits of
LMBatchFitter.
"""
import math

import numpy as np
import pytest

import ngmix_amd as ngmix
from ngmix_amd import _lib
from ngmix_amd import prior_batch as pb
from ngmix_amd.batch import GMixBatch, StampBatch
from ngmix_amd.gmix import GMix, GMixModel, GMixCoellip

pytestmark = pytest.mark.gpu

SCALE = 0.263
NSHAPE = {"gauss": 5, "turb": 5, "exp": 5, "dev": 5, "bdf": 6, "bd": 7}
# exp5_smooth's derivative is not exactly fexp (fastexp_nb.py): the analytic
# gradient (the convention of deriv_images, fexp' = fexp) and central
# differences of the value differ by this much, relative to the largest
# gradient entry of the object (its pars and the psf entries of its stamps).
# Measured on MI355X over the gradcheck cases below (step 1e-6): at most
# 4.6e-6; the bound keeps a factor ~4 above it.
FD_RTOL = 2.0e-5


def _torch():
    import torch
    return torch


def _autodiff():
    from ngmix_amd import autodiff
    return autodiff


def _jacrec(row0, col0, shear=0.0):
    dvdrow, dvdcol = SCALE * (1.0 + shear), 0.4 * SCALE * shear
    dudrow, dudcol = -0.3 * SCALE * shear, SCALE * (1.0 - 0.5 * shear)
    det = dvdrow * dudcol - dvdcol * dudrow
    return np.array([row0, col0, dvdrow, dvdcol, dudrow, dudcol, det, math.sqrt(abs(det))])


def _host_gmix(bp, model):
    if model == "coellip":
        return GMixCoellip(bp)
    return GMixModel(bp, model)


def _shape(rng, model, nband, ngauss=None):
    base = [rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1),
            rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)]
    if model == "coellip":
        return np.array(base + list(rng.uniform(0.2, 1.5, ngauss)) +
                        list(rng.uniform(20.0, 60.0, ngauss)))
    base.append(rng.uniform(0.5, 1.5))
    if model == "bdf":
        base.append(rng.uniform(0.2, 0.8))
    if model == "bd":
        base += [rng.uniform(-0.3, 0.3), rng.uniform(0.2, 0.8)]
    return np.array(base + list(rng.uniform(80.0, 200.0, nband)))


def _band_pars(pars, model, o, b):
    if model == "coellip":
        return pars[o]
    ns = NSHAPE[model]
    return np.concatenate([pars[o, :ns], pars[o, ns + b:ns + b + 1]])


def _psf(rng, npsf):
    psf = np.zeros((npsf, 6))
    psf[:, 0] = rng.uniform(0.2, 1.0, npsf)
    psf[:, 1:3] = rng.uniform(-0.03, 0.03, (npsf, 2))
    T = rng.uniform(0.15, 0.5, npsf)
    e1, e2 = rng.uniform(-0.05, 0.05, (2, npsf))
    psf[:, 3], psf[:, 4], psf[:, 5] = 0.5 * T * (1 - e1), 0.5 * T * e2, 0.5 * T * (1 + e1)
    return psf


def _make(rng, model, nobj, nep=1, nband=1, dims=(25, 25), npsf=3, shear=0.0,
          zero_frac=0.0, ngauss=None, ragged=False, noise=0.05, pars=None):
    """objects (pars), their stamps and psfs: stamp order objects, then bands,
    then epochs, as flatten_observations"""
    if pars is None:
        pars = np.array([_shape(rng, model, nband, ngauss) for _ in range(nobj)])
    imgs, wts, jacs, psfs, sobj, sband = [], [], [], [], [], []
    for o in range(nobj):
        for b in range(nband):
            for e in range(nep):
                shp = dims
                if ragged:
                    shp = (int(rng.randint(17, 26)), int(rng.randint(17, 26)))
                rec = _jacrec((shp[0] - 1) / 2.0 + rng.uniform(-0.5, 0.5),
                              (shp[1] - 1) / 2.0 + rng.uniform(-0.5, 0.5), shear)
                jac = ngmix.Jacobian(row=rec[0], col=rec[1], dvdrow=rec[2], dvdcol=rec[3],
                                     dudrow=rec[4], dudcol=rec[5])
                p = _psf(rng, npsf) if npsf else None
                gm = _host_gmix(_band_pars(pars, model, o, b), model)
                if p is not None:
                    gm = gm.convolve(GMix(pars=p.reshape(-1)))
                im = gm.make_image(shp, jacobian=jac, fast_exp=True)
                im = im + rng.normal(scale=noise, size=shp)
                w = np.full(shp, 1.0 / noise ** 2) * rng.uniform(0.5, 1.5, size=shp)
                if zero_frac:
                    w[rng.uniform(size=shp) < zero_frac] = 0.0
                imgs.append(im)
                wts.append(w)
                jacs.append(rec)
                psfs.append(p)
                sobj.append(o)
                sband.append(b)
    sb = StampBatch.from_arrays(imgs, wts, np.array(jacs), [True] * len(imgs))
    psf = np.array(psfs) if npsf else None
    return sb, pars, psf, np.array(sobj), np.array(sband)


def _gm_records(gpars):
    """GMixBatch of (n, G, 6) numpy mixtures"""
    n, G, _ = gpars.shape
    arr = np.zeros((n, G), dtype=_lib.GAUSS2D_DTYPE)
    for k, name in enumerate(("p", "row", "col", "irr", "irc", "icc")):
        arr[name] = gpars[:, :, k]
    arr["det"] = arr["irr"] * arr["icc"] - arr["irc"] * arr["irc"]
    return GMixBatch.from_numpy(arr)


def _stamp_mixtures(pars, model, psf, sobj, sband, ngauss=None):
    out = []
    for s in range(len(sobj)):
        gm = _host_gmix(_band_pars(pars, model, sobj[s], sband[s]), model)
        if psf is not None:
            gm = gm.convolve(GMix(pars=psf[s].reshape(-1)))
        out.append(gm.get_full_pars().reshape(-1, 6))
    return np.array(out)


# ------------------------------------------------------------------ value


@pytest.mark.parametrize("model,npsf", [("exp", 3), ("bd", 5), ("coellip", 1)])
def test_value_matches_loglike_kernels(model, npsf):
    """per stamp: StampBatch.loglike's record (exact kernel) to 1e-12, npix
    exact; per object: loglike_objects.  Ragged shapes, zero-weight pixels,
    sheared jacobians, several epochs."""
    torch = _torch()
    ad = _autodiff()
    rng = np.random.RandomState(1)
    ng = 5 if model == "coellip" else None
    sb, pars, psf, sobj, sband = _make(rng, model, 12, nep=2, npsf=npsf, shear=0.08,
                                       zero_frac=0.1, ragged=True, ngauss=ng)
    mix = _stamp_mixtures(pars, model, psf, sobj, sband)
    gm = _gm_records(mix)
    ref, st = sb.loglike(gm.clone(), exact=True)
    ll, rec, status = ad.stamp_loglike_grad(sb, torch.from_numpy(mix).cuda())
    assert int(status.abs().sum()) == 0 and int(st.abs().sum()) == 0
    ref = ref.cpu().numpy()
    rec = rec.cpu().numpy()
    np.testing.assert_allclose(rec[:, 0], ref[:, 0], rtol=1e-12, atol=0)
    np.testing.assert_allclose(rec[:, 1:3], ref[:, 1:3], rtol=1e-12,
                               atol=1e-12 * np.abs(ref[:, 1:3]).max())
    np.testing.assert_array_equal(rec[:, 3], ref[:, 3])
    assert np.all(rec[:, 3] < np.array([r * c for r, c in zip(sb.nrow, sb.ncol)]))
    # per object, through the public function
    obj_start = np.concatenate([[0], np.cumsum(np.bincount(sobj))])
    per_obj, _, _ = sb.loglike_objects(gm.clone(), obj_start, exact=True)
    got = ad.loglike(sb, torch.from_numpy(pars).cuda(), model,
                     psf=torch.from_numpy(psf).cuda(), stamp_obj=sobj, stamp_band=sband,
                     ngauss=ng)
    np.testing.assert_allclose(got.cpu().numpy(), per_obj[:, 0].cpu().numpy(), rtol=1e-12)


# ------------------------------------------------------- against the LM jacobian


def _lm_gradient(sb, pars, model, psf):
    """-sum fdiff J with J from deriv_images (the LM driver's analytic
    jacobian images) and fdiff from fill_fdiff; one stamp per object, no
    masked pixels"""
    torch = _torch()
    n = pars.shape[0]
    gm0, _ = GMixBatch.from_pars(pars, model)
    gmc, _ = gm0.convolve(_gm_records(psf[:, :, :]))
    ng0, G = gm0.ngauss, gmc.ngauss
    G0 = gm0.data.reshape(n, ng0, 13)
    gpars = gmc.data.reshape(n, G, 13)[:, :, 0:6].contiguous()
    modcov = G0[:, :, 3:6].repeat_interleave(G // ng0, dim=1)
    d = torch.from_numpy(pars).cuda()
    g1, g2, T = d[:, 2], d[:, 3], d[:, 4]
    gsq = g1 * g1 + g2 * g2
    f = 2.0 / (1.0 + gsq)
    dfac = -f / (1.0 + gsq)
    de1 = torch.stack([f + 2.0 * g1 * g1 * dfac, 2.0 * g1 * g2 * dfac], dim=1)
    de2 = torch.stack([2.0 * g1 * g2 * dfac, f + 2.0 * g2 * g2 * dfac], dim=1)
    Tk = modcov[:, :, 0] + modcov[:, :, 2]
    dcov = torch.zeros((n, G, 3, 3), dtype=torch.float64, device="cuda")
    for i in range(2):
        dcov[:, :, i, 0] = -0.5 * Tk * de1[:, i, None]
        dcov[:, :, i, 1] = 0.5 * Tk * de2[:, i, None]
        dcov[:, :, i, 2] = 0.5 * Tk * de1[:, i, None]
    dcov[:, :, 2, :] = modcov / T[:, None, None]
    img = sb.deriv_images(gpars.reshape(-1, 6), dcov.reshape(-1, 3, 3), G)
    fd, _ = sb.fill_fdiff(gmc, exact=True)
    npix = int(sb.npix[0])
    assert np.all(sb.npix_kept == npix)
    img = img.reshape(n, 6, npix)
    fd = fd.reshape(n, 1, npix)
    ierr = sb.ierr.reshape(n, 1, npix)
    J = img * ierr
    grad = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    grad[:, :5] = -(fd * J[:, 1:6]).sum(dim=2)
    grad[:, 5] = -(fd[:, 0] * J[:, 0]).sum(dim=1) / d[:, 5]
    return grad


def _ad_gradient(sb, pars, model, psf, **kw):
    torch = _torch()
    ad = _autodiff()
    p = torch.from_numpy(pars).cuda().requires_grad_(True)
    ll = ad.loglike(sb, p, model, psf=torch.from_numpy(psf).cuda(), **kw)
    ll.sum().backward()
    return p.grad


@pytest.mark.parametrize("model", ["gauss", "exp", "dev"])
def test_gradient_matches_lm_jacobian(model):
    rng = np.random.RandomState(7)
    sb, pars, psf, _, _ = _make(rng, model, 24, dims=(25, 23), npsf=3, shear=0.05)
    pars[:, 0:2] += 0.05      # away from the optimum: sizeable gradients
    pars[:, 4] *= 1.2
    got = _ad_gradient(sb, pars, model, psf).cpu().numpy()
    ref = _lm_gradient(sb, pars, model, psf).cpu().numpy()
    scale = np.abs(ref).max(axis=1, keepdims=True)
    assert np.all(np.abs(got - ref) <= 1e-10 * scale), np.abs(got - ref).max()


# ------------------------------------------------------- finite differences


def test_value_on_golden_render_loglike(golden):
    """tests/golden/render_loglike.npz: the reference's get_loglike of each
    recorded stamp (exp / bdf with and without psf, masked and kept-zero
    weights, odd shapes) from the kernel's record, npix exact"""
    torch = _torch()
    ad = _autodiff()
    g = golden("render_loglike")
    for name in [str(n) for n in g["names"]]:
        gm = g[name + "_gmix_in"]
        mix = np.stack([gm[k] for k in ("p", "row", "col", "irr", "irc", "icc")], axis=1)
        jac = g[name + "_jac"][0]
        rec = np.array([jac[k] for k in jac.dtype.names])
        sb = StampBatch.from_arrays([g[name + "_image"]], [g[name + "_weight"]], rec[None, :],
                                    [bool(g[name + "_izw"])])
        _, out, status = ad.stamp_loglike_grad(sb, torch.from_numpy(mix[None]).cuda())
        assert int(status[0]) == 0, name
        out = out.cpu().numpy()[0]
        ref = g[name + "_loglike"]
        np.testing.assert_allclose(out[:3], ref[:3], rtol=1e-12, atol=0, err_msg=name)
        assert out[3] == ref[3], name


def test_value_on_golden_c2(golden):
    """tests/golden/c2.npz (inputs rebuilt by helpers/c2_inputs.py): eight
    48x48 'exp' (x) gaussian-psf stamps at two parameter sets, through
    autodiff's own mixture and convolution; the model fill goes through
    tanh / atanh, hence 1e-10 as test_gpu_pixpass holds the kernels to"""
    torch = _torch()
    ad = _autodiff()
    from helpers import c2_inputs as c2
    g = golden("c2")
    pars, moved, jac, images, sigma, _ = c2.stamps()
    weights = np.broadcast_to((1.0 / sigma ** 2)[:, None, None], images.shape).copy()
    sb = StampBatch.from_images(images, weights, jac)
    psf = torch.from_numpy(np.tile([[1.0, 0.0, 0.0, c2.TPSF / 2, 0.0, c2.TPSF / 2]],
                                   (c2.N, 1, 1))).cuda()
    for tag, pp in (("truth", pars), ("moved", moved)):
        d_pp = torch.from_numpy(pp).cuda()
        mix, _ = ad.mixture_from_pars(d_pp, "exp")
        conv, _ = ad.convolve(mix, psf)
        _, out, status = ad.stamp_loglike_grad(sb, conv)
        assert int(status.abs().sum()) == 0
        out = out.cpu().numpy()
        ref = g[tag + "_loglike"]
        np.testing.assert_allclose(out[:, :3], ref[:, :3], rtol=1e-10)
        np.testing.assert_array_equal(out[:, 3], ref[:, 3])
        ll = ad.loglike(sb, d_pp, "exp", psf=psf).cpu().numpy()
        np.testing.assert_allclose(ll, ref[:, 0], rtol=1e-10)


def test_gradient_on_golden_derivs(golden):
    """tests/golden/derivs.npz: the reference's deriv_images (value image and
    [cen1, cen2, g1, g2, T] images) of gauss / exp / dev, without a psf and
    with 1- and 3-gaussian psfs, on a sheared 24x25 stamp.  On an image built
    from that value image, -sum fdiff J formed from the golden images alone
    (flux column: the value image over the flux) against the kernel gradient
    through autodiff, to 1e-10 of the object's largest entry"""
    torch = _torch()
    ad = _autodiff()
    g = golden("derivs")
    nrow, ncol = (int(x) for x in g["dims"])
    jac = g["jac"][0]
    rec = np.array([jac[k] for k in jac.dtype.names])
    # the golden pixel coordinates are the stamp's row-major grid
    rows, cols = np.mgrid[0:nrow, 0:ncol]
    np.testing.assert_allclose(g["v"], (rec[2] * (rows - rec[0]) + rec[3] * (cols - rec[1])).ravel(),
                               rtol=0, atol=1e-14)
    np.testing.assert_allclose(g["u"], (rec[4] * (rows - rec[0]) + rec[5] * (cols - rec[1])).ravel(),
                               rtol=0, atol=1e-14)
    rng = np.random.RandomState(31)
    for name in [str(n) for n in g["names"]]:
        model = name.split("_")[0]
        pars = g[name + "_pars"]
        out = g[name + "_out"]
        model_img = out[0]
        image = 0.9 * model_img + 0.01 * model_img.max() * rng.normal(size=model_img.size)
        ierr = np.full(model_img.size, 1.0 / (0.01 * model_img.max()))
        fdiff = (model_img - image) * ierr
        J = out * ierr[None, :]
        ref = np.empty(6)
        ref[:5] = -(fdiff[None, :] * J[1:6]).sum(axis=1)
        ref[5] = -(fdiff * J[0]).sum() / pars[5]
        sb = StampBatch.from_arrays([image.reshape(nrow, ncol)],
                                    [(ierr * ierr).reshape(nrow, ncol)], rec[None, :], [True])
        psf = None
        if name + "_psf" in g:
            pr = g[name + "_psf"]
            psf = torch.from_numpy(np.stack([pr[k] for k in ("p", "row", "col", "irr", "irc",
                                                             "icc")], axis=1)[None]).cuda()
        p = torch.from_numpy(pars[None, :].copy()).cuda().requires_grad_(True)
        # the composed gaussians are the golden's
        mix, _ = ad.mixture_from_pars(p.detach(), model)
        if psf is not None:
            mix, _ = ad.convolve(mix, psf)
        np.testing.assert_allclose(mix[0].cpu().numpy(), g[name + "_gpars"], rtol=1e-14,
                                   atol=1e-15, err_msg=name)
        ll = ad.loglike(sb, p, model, psf=psf)
        ll.sum().backward()
        got = p.grad[0].cpu().numpy()
        assert np.all(np.abs(got - ref) <= 1e-10 * np.abs(ref).max()), (name, got, ref)


GC_CASES = [("gauss", None, 1, 1), ("turb", None, 1, 2), ("exp", None, 2, 1),
            ("dev", None, 1, 1), ("bdf", None, 2, 2), ("bd", None, 1, 1),
            ("coellip", 3, 1, 1)]


def _window_pixels(sb, mix):
    """(pixel, gaussian) pairs of the listed pixels (ierr > 0) whose chi2 lies
    in the apodisation window (20, 25)"""
    ierr = sb.ierr.cpu().numpy()
    jac = sb.jac.cpu().numpy()
    nwin = 0
    for s in range(sb.n):
        nrow, ncol = int(sb.nrow[s]), int(sb.ncol[s])
        kept = ierr[sb.pix_off[s]:sb.pix_off[s] + nrow * ncol].reshape(nrow, ncol) > 0
        rec = jac[s]
        rows, cols = np.mgrid[0:nrow, 0:ncol]
        v = rec[2] * (rows - rec[0]) + rec[3] * (cols - rec[1])
        u = rec[4] * (rows - rec[0]) + rec[5] * (cols - rec[1])
        for p, r, c, irr, irc, icc in mix[s]:
            det = irr * icc - irc * irc
            dv, du = v - r, u - c
            chi2 = (icc * dv * dv + irr * du * du - 2 * irc * dv * du) / det
            nwin += int(((chi2 > 20) & (chi2 < 25) & kept).sum())
    return nwin


@pytest.mark.parametrize("model,ngauss,nband,nep", GC_CASES)
def test_gradcheck(model, ngauss, nband, nep):
    """central differences (torch.autograd.gradcheck, fp64) of the value
    against the gradient, with respect to pars and to the psf tensor: 17x17 to
    25x25 stamps, sheared jacobians, zero-weight pixels, several epochs and
    bands, and gaussians whose chi2 20-25 window falls on listed pixels.
    Each object's loglike is divided by its largest gradient entry (pars and
    the psf entries of its stamps), so the bound is FD_RTOL of that entry,
    object by object"""
    torch = _torch()
    ad = _autodiff()
    rng = np.random.RandomState(3)
    sb, pars, psf, sobj, sband = _make(rng, model, 3, nep=nep, nband=nband, npsf=2,
                                       shear=0.1, zero_frac=0.05, ragged=True,
                                       ngauss=ngauss)
    pars[:, 0:2] += 0.03
    # these very stamps and mixtures reach the window
    assert _window_pixels(sb, _stamp_mixtures(pars, model, psf, sobj, sband)) > 0
    p = torch.from_numpy(pars).cuda().requires_grad_(True)
    q = torch.from_numpy(psf).cuda().requires_grad_(True)

    def f(pp, qq):
        return ad.loglike(sb, pp, model, psf=qq, stamp_obj=sobj, stamp_band=sband,
                          ngauss=ngauss)

    gp, gq = torch.autograd.grad(f(p, q).sum(), (p, q))
    gp, gq = gp.abs().cpu().numpy(), gq.abs().cpu().numpy()
    scale = np.array([max(gp[o].max(), gq[sobj == o].max()) for o in range(pars.shape[0])])
    d_scale = torch.from_numpy(scale).cuda()
    assert torch.autograd.gradcheck(lambda pp, qq: f(pp, qq) / d_scale, (p, q), eps=1e-6,
                                    atol=FD_RTOL, rtol=0.0, raise_exception=True)


# ------------------------------------------------------- against the fits


# converged to far below the 1e-3 sigma the check resolves (the default ftol
# stops where the step left is ~1e-2 sigma)
TIGHT = {"maxfev": 4000, "ftol": 1.0e-12, "xtol": 1.0e-12}


def _newton_steps(res, sb, model, psf, sobj, sband, prior=None):
    torch = _torch()
    ad = _autodiff()
    ok = np.asarray(res["flags"]) == 0
    pars = np.asarray(res["pars"])
    p = torch.from_numpy(pars).cuda().requires_grad_(True)
    lp = ad.lnprob(sb, p, model, psf=psf, stamp_obj=sobj, stamp_band=sband, prior=prior)
    g, = torch.autograd.grad(lp[torch.from_numpy(ok).cuda()].sum(), p)
    g = g.cpu().numpy()
    cov = np.asarray(res["pars_cov"])
    steps = []
    for i in np.nonzero(ok)[0]:
        step = cov[i] @ g[i]
        steps.append(np.abs(step) / np.sqrt(np.diag(cov[i])))
    return np.array(steps), ok


def test_newton_step_at_lm_solutions_exp():
    from ngmix_amd.lm_batch import LMBatchFitter
    torch = _torch()
    rng = np.random.RandomState(21)
    sb, truth, psf, sobj, sband = _make(rng, "exp", 64, dims=(33, 33), npsf=3)
    guess = truth * rng.uniform(0.95, 1.05, truth.shape)
    res = LMBatchFitter("exp", fit_pars=TIGHT).go(sb, guess, psf=_gm_records(psf))
    steps, ok = _newton_steps(res, sb, "exp", torch.from_numpy(psf).cuda(), sobj, sband)
    assert ok.mean() > 0.9
    assert steps.max() < 1e-3, steps.max()


def test_newton_step_at_lm_solutions_bdf_prior():
    from ngmix_amd.lm_batch import LMBatchFitter
    torch = _torch()
    rng = np.random.RandomState(22)
    sb, truth, psf, sobj, sband = _make(rng, "bdf", 32, nep=2, nband=2, dims=(33, 33),
                                        npsf=2)
    # PriorSimpleSepBatch has no term for bdf's fracdev: the separable batch
    # prior with one middle term, as as_batch_prior builds for PriorBDFSep
    prior = pb.PriorSepBatch(pb.GaussianCen(0.0, 0.0, 0.3, 0.3), pb.GPriorBA(0.3),
                             [pb.Normal(1.0, 1.0), pb.Normal(0.5, 0.3),
                              pb.Normal(100.0, 100.0), pb.Normal(100.0, 100.0)],
                             rows_from_lnprob=True)
    prior.nmid = 1
    guess = truth * rng.uniform(0.95, 1.05, truth.shape)
    res = LMBatchFitter("bdf", prior=prior, fit_pars=TIGHT).go(sb, guess, psf=_gm_records(psf),
                                               stamp_obj=sobj, stamp_band=sband)
    steps, ok = _newton_steps(res, sb, "bdf", torch.from_numpy(psf).cuda(), sobj, sband,
                              prior=prior)
    assert ok.mean() > 0.8
    assert steps.max() < 1e-3, steps.max()


# ------------------------------------------------------- status, determinism


def test_out_of_range_object_isolated_and_deterministic():
    torch = _torch()
    ad = _autodiff()
    rng = np.random.RandomState(9)
    sb, pars, psf, sobj, sband = _make(rng, "bdf", 6, nep=2, nband=2, npsf=2)
    bad = pars.copy()
    bad[3, 2:4] = [0.9, 0.5]      # |g| >= 1

    def run(pp):
        p = torch.from_numpy(pp).cuda().requires_grad_(True)
        q = torch.from_numpy(psf).cuda().requires_grad_(True)
        ll, flags = ad.loglike(sb, p, "bdf", psf=q, stamp_obj=sobj, stamp_band=sband,
                               return_flags=True)
        ll.sum().backward()
        return (ll.detach().cpu().numpy(), p.grad.cpu().numpy(), q.grad.cpu().numpy(),
                flags.cpu().numpy())

    v0, g0, q0, f0 = run(pars)
    v1, g1, q1, f1 = run(bad)
    v2, g2, q2, _ = run(pars)
    assert np.all(f0 == 0) and np.all(np.isfinite(v0)) and np.all(np.isfinite(g0))
    assert np.all(np.isfinite(q0))
    assert f1[3] == _lib.ERR_G_RANGE and np.isnan(v1[3]) and np.all(np.isnan(g1[3]))
    # the psf rows of the flagged object's four stamps are NaN too
    assert np.all(np.isnan(q1[sobj == 3]))
    keep = np.arange(6) != 3
    assert np.all(f1[keep] == 0)
    np.testing.assert_array_equal(v1[keep], v0[keep])
    np.testing.assert_array_equal(g1[keep], g0[keep])
    np.testing.assert_array_equal(q1[sobj != 3], q0[sobj != 3])
    # two runs: the same bits
    np.testing.assert_array_equal(v2, v0)
    np.testing.assert_array_equal(g2, g0)
    np.testing.assert_array_equal(q2, q0)


def test_second_derivative_refused():
    """the kernel gives first derivatives only: differentiating the gradient
    again (create_graph=True, a Hessian-vector product) raises instead of
    silently dropping the kernel's second-order terms"""
    torch = _torch()
    ad = _autodiff()
    rng = np.random.RandomState(12)
    sb, pars, psf, _, _ = _make(rng, "exp", 2, npsf=1)
    p = torch.from_numpy(pars).cuda().requires_grad_(True)
    ll = ad.loglike(sb, p, "exp", psf=torch.from_numpy(psf).cuda())
    with pytest.raises(RuntimeError, match="first derivatives only"):
        torch.autograd.grad(ll.sum(), p, create_graph=True)
    # a plain gradient of the same graph still works
    g, = torch.autograd.grad(ll.sum(), p)
    assert bool(torch.isfinite(g).all())


def test_det_failure_flagged():
    """a convolved gaussian with det <= 0 (negative T): the stamp's status,
    NaN for its object only"""
    torch = _torch()
    ad = _autodiff()
    rng = np.random.RandomState(4)
    sb, pars, psf, sobj, sband = _make(rng, "exp", 4, npsf=1)
    pars[1, 4] = -5.0
    ll, flags = ad.loglike(sb, torch.from_numpy(pars).cuda(), "exp",
                           psf=torch.from_numpy(psf).cuda(), return_flags=True)
    ll, flags = ll.cpu().numpy(), flags.cpu().numpy()
    assert flags[1] in (_lib.ERR_DET_TOO_LOW, _lib.ERR_T_TOO_LOW) and np.isnan(ll[1])
    assert np.all(flags[[0, 2, 3]] == 0) and np.all(np.isfinite(ll[[0, 2, 3]]))


def test_large_batch_matches_lm_jacobian_sample():
    """100k 48x48 'exp' (x) 3-gaussian psf stamps in one call; a seeded sample
    checked as in test_gradient_matches_lm_jacobian"""
    torch = _torch()
    ad = _autodiff()
    n, dims = 100_000, (48, 48)
    g = torch.Generator(device="cuda").manual_seed(5)
    pars = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    pars[:, 0:2] = torch.rand((n, 2), generator=g, device="cuda", dtype=torch.float64) * 0.2 - 0.1
    pars[:, 2:4] = torch.rand((n, 2), generator=g, device="cuda", dtype=torch.float64) * 0.4 - 0.2
    pars[:, 4] = 0.5 + torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    pars[:, 5] = 100.0 + 100 * torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    rng = np.random.RandomState(5)
    psf1 = _psf(rng, 3)
    psf = torch.from_numpy(np.tile(psf1, (n, 1, 1))).cuda()
    images = torch.randn((n,) + dims, generator=g, device="cuda", dtype=torch.float64)
    jac = _jacrec(23.5, 23.5, 0.0)
    sb = StampBatch.from_images(images, torch.full_like(images, 4.0), jac)
    p = pars.clone().requires_grad_(True)
    ll = ad.loglike(sb, p, "exp", psf=psf)
    ll.sum().backward()
    assert bool(torch.isfinite(p.grad).all())
    idx = np.sort(rng.choice(n, 64, replace=False))
    d_idx = torch.from_numpy(idx).cuda()
    sub = sb.select(idx)
    ref = _lm_gradient(sub, pars[d_idx].cpu().numpy(), "exp", np.tile(psf1, (64, 1, 1)))
    got = p.grad[d_idx]
    scale = ref.abs().max(dim=1, keepdim=True).values
    assert bool(((got - ref).abs() <= 1e-10 * scale).all())
