"""
Differentiable batched model images (ngmix_amd.autodiff.render /
stamp_render, backward through csrc/render_grad.hip): the forward against the
reference's recorded images and StampBatch.render, the vector-Jacobian product
against the reference's derivative images, against autodiff.loglike and
against central finite differences; blends, flags, determinism, edge cases
and a 100k-stamp batch.
"""

import numpy as np
import pytest

import ngmix_amd as ngmix
from ngmix_amd import _lib
from ngmix_amd.batch import StampBatch

from test_gpu_autodiff import (GC_CASES, SCALE, _gm_records, _jacrec, _make, _psf,
                               _stamp_mixtures)
from test_gpu_pixpass import assert_pixels

pytestmark = pytest.mark.gpu

# Fast mode's derivative is deriv_images' convention (fexp' taken as fexp),
# not the exact derivative of the exp5_smooth image.  For a generic linear
# functional of the pixels the gap is larger than for loglike (FD_RTOL, whose
# residual weights are small where the model is): up to 2.3e-4 of the largest
# gaussian-level gradient entry in a numpy model of the convention over 40
# random gaussians and weights.  The bound keeps a factor ~4 above it.
FAST_FD_RTOL = 1.0e-3


def _torch():
    import torch
    return torch


def _autodiff():
    from ngmix_amd import autodiff
    return autodiff


def _pix_index(sb, per_stamp):
    """(total_pix,) device int64: per_stamp[s] on every pixel of stamp s
    (packed layouts)"""
    torch = _torch()
    npix = torch.from_numpy(sb.npix).cuda()
    return torch.repeat_interleave(torch.as_tensor(per_stamp, device="cuda"), npix)


def _scale(gp, gq, sobj, nobj):
    return np.array([max(np.abs(gp[o]).max(), np.abs(gq[sobj == o]).max() if gq is not None
                         else 0.0) for o in range(nobj)])


# ------------------------------------------------------------------ forward


def test_forward_on_golden_render_loglike(golden):
    """tests/golden/render_loglike.npz: exact=True equals the reference's fast
    render, the fused default is within test_gpu_pixpass's tolerance, the true
    exp within 1e-14; every mode bit-identical to StampBatch.render"""
    torch = _torch()
    ad = _autodiff()
    g = golden("render_loglike")
    for name in [str(n) for n in g["names"]]:
        gm = g[name + "_gmix_in"]
        mix = np.stack([gm[k] for k in ("p", "row", "col", "irr", "irc", "icc")], axis=1)
        jac = g[name + "_jac"][0]
        rec = np.array([jac[k] for k in jac.dtype.names])
        shape = g[name + "_image"].shape
        sb = StampBatch.from_arrays([g[name + "_image"]], [g[name + "_weight"]], rec[None, :],
                                    [bool(g[name + "_izw"])])
        d_mix = torch.from_numpy(mix[None]).cuda()
        for fast_exp, exact in ((True, True), (True, False), (False, False)):
            im, status = ad.stamp_render(sb, d_mix, fast_exp=fast_exp, exact=exact)
            assert int(status[0]) == 0, name
            im = im.cpu().numpy()
            ref, _ = sb.render(_gm_records(mix[None]), fast_exp=fast_exp, exact=exact)
            np.testing.assert_array_equal(im, ref.cpu().numpy(), err_msg=name)
            if not fast_exp:
                np.testing.assert_allclose(im.reshape(shape), g[name + "_render_exact"],
                                           rtol=1e-14, atol=1e-300, err_msg=name)
            else:
                assert_pixels(im.reshape(shape), g[name + "_render_fast"], exact, err_msg=name)


def test_render_on_golden_c2(golden):
    """tests/golden/c2.npz: the reference's rendered images (minus the base
    they were added to) from the model parameters, through render(psf=...),
    to 1e-10 of the model's peak"""
    torch = _torch()
    ad = _autodiff()
    from helpers import c2_inputs as c2
    g = golden("c2")
    pars, moved, jac, images, sigma, base = c2.stamps()
    weights = np.broadcast_to((1.0 / sigma ** 2)[:, None, None], images.shape).copy()
    sb = StampBatch.from_images(images, weights, jac)
    psf = torch.from_numpy(np.tile([[1.0, 0.0, 0.0, c2.TPSF / 2, 0.0, c2.TPSF / 2]],
                                   (c2.N, 1, 1))).cuda()
    for tag, pp in (("truth", pars), ("moved", moved)):
        im = ad.render(sb, torch.from_numpy(pp).cuda(), "exp", psf=psf)
        im = im.cpu().numpy().reshape(c2.N, -1)
        for i in range(c2.N):
            model = g[tag + "_rendered"][i].ravel() - base[i].ravel()
            np.testing.assert_allclose(im[i], model, rtol=0, atol=1e-10 * np.abs(model).max(),
                                       err_msg="%s %d" % (tag, i))


# ------------------------------------------------------------------ VJP


def test_vjp_on_golden_derivs(golden):
    """tests/golden/derivs.npz: for a seeded upstream image g, pars.grad of
    sum(render * g) against sum g * (the reference's derivative images), the
    flux column from the value image over the flux; 1e-10 of the largest
    entry"""
    torch = _torch()
    ad = _autodiff()
    g = golden("derivs")
    nrow, ncol = (int(x) for x in g["dims"])
    jac = g["jac"][0]
    rec = np.array([jac[k] for k in jac.dtype.names])
    rng = np.random.RandomState(41)
    for name in [str(n) for n in g["names"]]:
        model = name.split("_")[0]
        pars = g[name + "_pars"]
        out = g[name + "_out"]
        up = rng.normal(size=out.shape[1])
        ref = np.empty(6)
        ref[:5] = (up[None, :] * out[1:6]).sum(axis=1)
        ref[5] = (up * out[0]).sum() / pars[5]
        sb = StampBatch.from_arrays([np.zeros((nrow, ncol))], [np.ones((nrow, ncol))],
                                    rec[None, :], [True])
        psf = None
        if name + "_psf" in g:
            pr = g[name + "_psf"]
            psf = torch.from_numpy(np.stack([pr[k] for k in ("p", "row", "col", "irr", "irc",
                                                             "icc")], axis=1)[None]).cuda()
        p = torch.from_numpy(pars[None, :].copy()).cuda().requires_grad_(True)
        im = ad.render(sb, p, model, psf=psf)
        np.testing.assert_allclose(im.detach().cpu().numpy(), out[0], rtol=0,
                                   atol=1e-12 * np.abs(out[0]).max(), err_msg=name)
        (im * torch.from_numpy(up).cuda()).sum().backward()
        got = p.grad[0].cpu().numpy()
        assert np.all(np.abs(got - ref) <= 1e-10 * np.abs(ref).max()), (name, got, ref)


LL_CASES = [("exp", None, 1, 2, 3), ("bdf", None, 2, 2, 2), ("coellip", 3, 1, 1, 1)]


@pytest.mark.parametrize("model,ngauss,nband,nep,npsf", LL_CASES)
def test_loss_matches_loglike(model, ngauss, nband, nep, npsf):
    """-1/2 sum_kept ivar (val - render)^2 in torch (exact=True, the kept mask
    of ignore_zero_weight) against autodiff.loglike: the value to 1e-12
    relative, the gradients (pars and psf) to 1e-10 of each object's largest
    entry.  Ragged shapes, zero-weight pixels, sheared jacobians"""
    torch = _torch()
    ad = _autodiff()
    rng = np.random.RandomState(17)
    sb, pars, psf, sobj, sband = _make(rng, model, 5, nep=nep, nband=nband, npsf=npsf,
                                       shear=0.07, zero_frac=0.1, ragged=True, ngauss=ngauss)
    pars[:, 0:2] += 0.04
    nobj = pars.shape[0]
    kw = dict(stamp_obj=sobj, stamp_band=sband, ngauss=ngauss)

    p1 = torch.from_numpy(pars).cuda().requires_grad_(True)
    q1 = torch.from_numpy(psf).cuda().requires_grad_(True)
    ll = ad.loglike(sb, p1, model, psf=q1, **kw)
    gp1, gq1 = torch.autograd.grad(ll.sum(), (p1, q1))

    p2 = torch.from_numpy(pars).cuda().requires_grad_(True)
    q2 = torch.from_numpy(psf).cuda().requires_grad_(True)
    im = ad.render(sb, p2, model, psf=q2, exact=True, **kw)
    kept = (sb.ierr > 0).to(torch.float64)
    per_pix = -0.5 * kept * sb.ierr ** 2 * (sb.val - im) ** 2
    pix_obj = _pix_index(sb, torch.from_numpy(sobj).cuda())
    loss = torch.zeros(nobj, dtype=torch.float64, device="cuda").index_add(0, pix_obj, per_pix)
    gp2, gq2 = torch.autograd.grad(loss.sum(), (p2, q2))

    np.testing.assert_allclose(loss.detach().cpu().numpy(), ll.detach().cpu().numpy(),
                               rtol=1e-12, atol=0)
    gp1, gq1 = gp1.cpu().numpy(), gq1.cpu().numpy()
    gp2, gq2 = gp2.cpu().numpy(), gq2.cpu().numpy()
    scale = _scale(gp1, gq1, sobj, nobj)
    for o in range(nobj):
        assert np.all(np.abs(gp2[o] - gp1[o]) <= 1e-10 * scale[o]), (o, gp2[o], gp1[o])
        assert np.all(np.abs(gq2[sobj == o] - gq1[sobj == o]) <= 1e-10 * scale[o]), o


def _render_window_pixels(sb, mix):
    """(pixel, gaussian) pairs of the frames whose chi2 lies in (20, 25)"""
    jac = sb.jac.cpu().numpy()
    nwin = 0
    for s in range(sb.n):
        nrow, ncol = int(sb.nrow[s]), int(sb.ncol[s])
        rec = jac[s]
        rows, cols = np.mgrid[0:nrow, 0:ncol]
        v = rec[2] * (rows - rec[0]) + rec[3] * (cols - rec[1])
        u = rec[4] * (rows - rec[0]) + rec[5] * (cols - rec[1])
        for p, r, c, irr, irc, icc in mix[s]:
            det = irr * icc - irc * irc
            dv, du = v - r, u - c
            chi2 = (icc * dv * dv + irr * du * du - 2 * irc * dv * du) / det
            nwin += int(((chi2 > 20) & (chi2 < 25)).sum())
    return nwin


@pytest.mark.parametrize("fast_exp", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("model,ngauss,nband,nep", GC_CASES)
def test_gradcheck(model, ngauss, nband, nep, fast_exp):
    """central differences of a seeded random linear functional of each
    object's pixels, with respect to pars and the psf, divided by the object's
    largest gradient entry: exact mode (the true derivative) to 1e-7, fast
    mode (deriv_images' convention) to FAST_FD_RTOL with the window reached"""
    torch = _torch()
    ad = _autodiff()
    rng = np.random.RandomState(3)
    sb, pars, psf, sobj, sband = _make(rng, model, 3, nep=nep, nband=nband, npsf=2,
                                       shear=0.1, zero_frac=0.05, ragged=True, ngauss=ngauss)
    pars[:, 0:2] += 0.03
    if fast_exp:
        assert _render_window_pixels(sb, _stamp_mixtures(pars, model, psf, sobj, sband)) > 0
    nobj = pars.shape[0]
    w = torch.from_numpy(rng.normal(size=sb.total_pix)).cuda()
    pix_obj = _pix_index(sb, torch.from_numpy(sobj).cuda())
    p = torch.from_numpy(pars).cuda().requires_grad_(True)
    q = torch.from_numpy(psf).cuda().requires_grad_(True)

    def f(pp, qq):
        im = ad.render(sb, pp, model, psf=qq, stamp_obj=sobj, stamp_band=sband,
                       ngauss=ngauss, fast_exp=fast_exp)
        return torch.zeros(nobj, dtype=torch.float64, device="cuda").index_add(
            0, pix_obj, im * w)

    gp, gq = torch.autograd.grad(f(p, q).sum(), (p, q))
    scale = _scale(gp.cpu().numpy(), gq.cpu().numpy(), sobj, nobj)
    d_scale = torch.from_numpy(scale).cuda()
    atol = FAST_FD_RTOL if fast_exp else 1e-7
    assert torch.autograd.gradcheck(lambda pp, qq: f(pp, qq) / d_scale, (p, q), eps=1e-6,
                                    atol=atol, rtol=0.0, raise_exception=True)


PASS2_CASES = {"13x11": (13, 11), "25x25": (25, 25), "off_frame": (25, 25)}


@pytest.mark.parametrize("case", sorted(PASS2_CASES))
def test_vjp_of_the_loglike_residual_is_the_loglike_gradient(case):
    """the fast VJP kernel's gaussian pass is loglike_grad_kernel's pass 2, the
    same text in both files: fed the residual the loglike kernel
    forms -- (val - model) (ierr ierr) with the exact=True fast render as
    model, all weights positive -- the VJP gives the loglike gradient bit for
    bit.  13x11: ragged tiles, one chunk; 25x25: two chunks, the second short;
    off_frame: a gaussian centred above the frame that reaches the first rows
    only (its second chunk is skipped) and one that reaches no tile at all"""
    torch = _torch()
    ad = _autodiff()
    rng = np.random.RandomState(29)
    dims = PASS2_CASES[case]
    # (no shear in the off-frame case: v = SCALE (row - row0) exactly)
    sb, pars, psf, sobj, sband = _make(rng, "exp", 3, dims=dims, npsf=2,
                                       shear=0.0 if case == "off_frame" else 0.05)
    mix = _stamp_mixtures(pars, "exp", psf, sobj, sband)
    if case == "off_frame":
        row0 = sb.jac.cpu().numpy()[:, 0]
        mix[:, 0, 1] = SCALE * (-6.0 - row0)       # 5 sigma = 7.5 pixels: rows 0, 1
        mix[:, 1, 1] = SCALE * (-30.0 - row0)
        mix[:, 0:2, 3] = mix[:, 0:2, 5] = (1.5 * SCALE) ** 2
        mix[:, 0:2, 4] = 0.0
    assert bool((sb.ierr > 0).all())

    g1 = torch.from_numpy(mix).cuda().requires_grad_(True)
    ll, _, st = ad.stamp_loglike_grad(sb, g1)
    assert int(st.abs().sum()) == 0
    want, = torch.autograd.grad(ll.sum(), g1)

    g2 = torch.from_numpy(mix).cuda().requires_grad_(True)
    model, st = ad.stamp_render(sb, g2, fast_exp=True, exact=True)
    assert int(st.abs().sum()) == 0
    r = (sb.val - model.detach()) * (sb.ierr * sb.ierr)
    got, = torch.autograd.grad(model, g2, grad_outputs=r)

    want, got = want.cpu().numpy(), got.cpu().numpy()
    print("%s: largest |vjp - loglike gradient| / largest entry = %.3e"
          % (case, np.abs(got - want).max() / np.abs(want).max()))
    assert np.abs(want).max() > 0
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------ blends


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fused"])
def test_blend_is_the_sum_of_its_parts(exact):
    """an 'exp' and a 'dev' object drawn into the same stamps by concatenating
    their convolved mixtures along G: the image is the sum of the single
    renders, each object's gradient its single-object VJP"""
    torch = _torch()
    ad = _autodiff()
    rng = np.random.RandomState(23)
    n = 6
    sb, pa, psf, _, _ = _make(rng, "exp", n, dims=(32, 30), npsf=3, shear=0.05)
    pb = pa.copy()
    pb[:, 0:2] += rng.uniform(-0.8, 0.8, (n, 2))
    pb[:, 4] *= 2.0
    d_psf = torch.from_numpy(psf).cuda()
    up = torch.from_numpy(rng.normal(size=sb.total_pix)).cuda()

    def conv(pp, model):
        m, _ = ad.mixture_from_pars(pp, model)
        return ad.convolve(m, d_psf)[0]

    a = torch.from_numpy(pa).cuda().requires_grad_(True)
    b = torch.from_numpy(pb).cuda().requires_grad_(True)
    im, st = ad.stamp_render(sb, torch.cat([conv(a, "exp"), conv(b, "dev")], dim=1),
                             exact=exact)
    assert int(st.abs().sum()) == 0
    ga, gb = torch.autograd.grad((im * up).sum(), (a, b))

    a1 = torch.from_numpy(pa).cuda().requires_grad_(True)
    ima, _ = ad.stamp_render(sb, conv(a1, "exp"), exact=exact)
    ga1, = torch.autograd.grad((ima * up).sum(), a1)
    b1 = torch.from_numpy(pb).cuda().requires_grad_(True)
    imb, _ = ad.stamp_render(sb, conv(b1, "dev"), exact=exact)
    gb1, = torch.autograd.grad((imb * up).sum(), b1)

    tot = (ima + imb).detach()
    np.testing.assert_allclose(im.detach().cpu().numpy(), tot.cpu().numpy(), rtol=0,
                               atol=1e-14 * float(tot.abs().max()))
    for got, ref in ((ga, ga1), (gb, gb1)):
        got, ref = got.cpu().numpy(), ref.cpu().numpy()
        scale = np.abs(ref).max(axis=1, keepdims=True)
        assert np.all(np.abs(got - ref) <= 1e-12 * scale), np.abs(got - ref).max()


# ------------------------------------------------------------------ flags


@pytest.mark.parametrize("kind", ["g_range", "zero_psf", "det"])
def test_flagged_object_isolated_and_deterministic(kind):
    torch = _torch()
    ad = _autodiff()
    rng = np.random.RandomState(9)
    sb, pars, psf, sobj, sband = _make(rng, "bdf", 6, nep=2, nband=2, npsf=2)
    bad_p, bad_q = pars.copy(), psf.copy()
    if kind == "g_range":
        bad_p[3, 2:4] = [0.9, 0.5]
        want = (_lib.ERR_G_RANGE,)
    elif kind == "zero_psf":
        bad_q[np.nonzero(sobj == 3)[0][1], :, 0] = 0.0
        want = (_lib.ERR_ZERO_DIV,)
    else:
        bad_p[3, 4] = -5.0
        want = (_lib.ERR_DET_TOO_LOW, _lib.ERR_T_TOO_LOW)
    up = torch.from_numpy(rng.normal(size=sb.total_pix)).cuda()
    pix_obj = _pix_index(sb, torch.from_numpy(sobj).cuda()).cpu().numpy()

    def run(pp, qq):
        p = torch.from_numpy(pp).cuda().requires_grad_(True)
        q = torch.from_numpy(qq).cuda().requires_grad_(True)
        im, flags = ad.render(sb, p, "bdf", psf=q, stamp_obj=sobj, stamp_band=sband,
                              return_flags=True)
        (im * up).sum().backward()
        return (im.detach().cpu().numpy(), p.grad.cpu().numpy(), q.grad.cpu().numpy(),
                flags.cpu().numpy())

    v0, g0, q0, f0 = run(pars, psf)
    v1, g1, q1, f1 = run(bad_p, bad_q)
    v2, g2, q2, f2 = run(bad_p, bad_q)
    assert np.all(f0 == 0) and np.all(np.isfinite(v0)) and np.all(np.isfinite(g0))
    assert np.all(np.isfinite(q0))
    assert f1[3] in want, f1
    assert np.all(np.isnan(v1[pix_obj == 3]))
    assert np.all(np.isnan(g1[3])) and np.all(np.isnan(q1[sobj == 3]))
    keep = np.arange(6) != 3
    assert np.all(f1[keep] == 0)
    np.testing.assert_array_equal(v1[pix_obj != 3], v0[pix_obj != 3])
    np.testing.assert_array_equal(g1[keep], g0[keep])
    np.testing.assert_array_equal(q1[sobj != 3], q0[sobj != 3])
    # two runs: the same bits
    np.testing.assert_array_equal(v2, v1)
    np.testing.assert_array_equal(g2, g1)
    np.testing.assert_array_equal(q2, q1)
    np.testing.assert_array_equal(f2, f1)


def test_stamp_render_refused_gaussian():
    """a det <= 0 gaussian: the stamp's status, zero pixels and a zero gradient
    for that stamp only"""
    torch = _torch()
    ad = _autodiff()
    rng = np.random.RandomState(8)
    sb, pars, psf, sobj, sband = _make(rng, "exp", 3, npsf=1)
    mix = _stamp_mixtures(pars, "exp", psf, sobj, sband)
    mix[1, 2, 3:6] = [1.0, 2.0, 1.0]     # det = -3
    g = torch.from_numpy(mix).cuda().requires_grad_(True)
    im, st = ad.stamp_render(sb, g)
    assert st.cpu().numpy().tolist() == [0, _lib.ERR_DET_TOO_LOW, 0]
    im.sum().backward()
    off, npix = sb.pix_off, sb.npix
    im = im.detach().cpu().numpy()
    assert np.all(im[off[1]:off[1] + npix[1]] == 0.0)
    assert np.all(g.grad[1].cpu().numpy() == 0.0)
    assert bool(torch.isfinite(g.grad).all()) and float(g.grad[0].abs().max()) > 0


# ------------------------------------------------------------------ edges


def test_sum_loss_stride_zero_upstream():
    """image.sum() hands backward a stride-0 expanded gradient"""
    torch = _torch()
    ad = _autodiff()
    rng = np.random.RandomState(2)
    sb, pars, psf, _, _ = _make(rng, "exp", 4, npsf=2)
    p = torch.from_numpy(pars).cuda().requires_grad_(True)
    q = torch.from_numpy(psf).cuda()
    g1, = torch.autograd.grad(ad.render(sb, p, "exp", psf=q).sum(), p)
    ones = torch.ones(sb.total_pix, dtype=torch.float64, device="cuda")
    g2, = torch.autograd.grad((ad.render(sb, p, "exp", psf=q) * ones).sum(), p)
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
    np.testing.assert_array_equal(g1.cpu().numpy(), g2.cpu().numpy())


def test_geometry_only_batch():
    """a StampBatch without pixel data (from_observations_geometry): the same
    image and gradient as a full batch of the same geometry"""
    torch = _torch()
    ad = _autodiff()
    rng = np.random.RandomState(6)
    sb, pars, psf, sobj, sband = _make(rng, "dev", 3, npsf=2, ragged=True)
    jac = sb.jac.cpu().numpy()
    obs = []
    for s in range(sb.n):
        r = jac[s]
        j = ngmix.Jacobian(row=r[0], col=r[1], dvdrow=r[2], dvdcol=r[3], dudrow=r[4],
                           dudcol=r[5])
        obs.append(ngmix.Observation(np.zeros((int(sb.nrow[s]), int(sb.ncol[s]))), jacobian=j))
    geo = StampBatch.from_observations_geometry(obs)
    assert geo.val is None and geo.ierr is None
    up = torch.from_numpy(rng.normal(size=sb.total_pix)).cuda()
    out = []
    for b in (sb, geo):
        p = torch.from_numpy(pars).cuda().requires_grad_(True)
        im = ad.render(b, p, "dev", psf=torch.from_numpy(psf).cuda())
        gp, = torch.autograd.grad((im * up).sum(), p)
        out.append((im.detach().cpu().numpy(), gp.cpu().numpy()))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])


def test_non_packed_layout():
    """stamps stored in reverse order (pix_off not the running sum): the
    image is the packed batch's, stamp by stamp, and so is the gradient"""
    torch = _torch()
    ad = _autodiff()
    rng = np.random.RandomState(10)
    sb, pars, psf, sobj, sband = _make(rng, "exp", 4, npsf=2, dims=(20, 19))
    npix = int(sb.npix[0])
    n = sb.n
    rev = np.arange(n - 1, -1, -1)
    perm = torch.from_numpy((rev[:, None] * npix + np.arange(npix)[None, :]).ravel()).cuda()
    izw = np.ones(n, dtype=bool)
    nb = StampBatch(sb.val[perm], sb.ierr[perm], sb.jac, sb.nrow, sb.ncol, rev * npix, izw)
    assert not nb._packed()
    up = torch.from_numpy(rng.normal(size=sb.total_pix)).cuda()
    mix = torch.from_numpy(_stamp_mixtures(pars, "exp", psf, sobj, sband)).cuda()
    out = []
    for b, u in ((sb, up), (nb, up[perm])):
        g = mix.clone().requires_grad_(True)
        im, st = ad.stamp_render(b, g)
        assert int(st.abs().sum()) == 0
        gg, = torch.autograd.grad((im * u).sum(), g)
        out.append((im.detach(), gg))
    np.testing.assert_array_equal(out[1][0][perm].cpu().numpy(), out[0][0].cpu().numpy())
    np.testing.assert_array_equal(out[1][1].cpu().numpy(), out[0][1].cpu().numpy())
    ref, _ = nb.render(_gm_records(mix.cpu().numpy()))
    np.testing.assert_array_equal(out[1][0].cpu().numpy(), ref.cpu().numpy())


def test_second_derivative_refused():
    torch = _torch()
    ad = _autodiff()
    rng = np.random.RandomState(12)
    sb, pars, psf, _, _ = _make(rng, "exp", 2, npsf=1)
    p = torch.from_numpy(pars).cuda().requires_grad_(True)
    im = ad.render(sb, p, "exp", psf=torch.from_numpy(psf).cuda())
    with pytest.raises(RuntimeError, match="first derivatives only"):
        torch.autograd.grad((im * im).sum(), p, create_graph=True)
    g, = torch.autograd.grad((im * im).sum(), p)
    assert bool(torch.isfinite(g).all())


def test_lds_budget_is_a_clean_error():
    """a mixture too large for the VJP kernel's LDS: the forward renders, the
    backward raises before any launch"""
    torch = _torch()
    ad = _autodiff()
    rng = np.random.RandomState(13)
    G = 600
    sb = StampBatch.from_images(np.zeros((1, 16, 16)), np.ones((1, 16, 16)),
                                _jacrec(7.5, 7.5))
    mix = np.zeros((1, G, 6))
    mix[0, :, 0] = rng.uniform(0.5, 1.0, G)
    mix[0, :, 1:3] = rng.uniform(-0.5, 0.5, (G, 2))
    mix[0, :, 3] = mix[0, :, 5] = rng.uniform(0.3, 1.0, G)
    g = torch.from_numpy(mix).cuda().requires_grad_(True)
    im, st = ad.stamp_render(sb, g)
    assert int(st[0]) == 0 and bool(torch.isfinite(im).all())
    with pytest.raises(ValueError, match="LDS budget"):
        im.sum().backward()


# ------------------------------------------------------------------ scale


def test_large_batch_position_independent():
    """100k 48x48 'exp' (x) 3-gaussian psf stamps in one call: a seeded sample
    of objects' images and kernel gradients (with respect to each stamp's
    gaussians) equals the same objects in a small batch, bit for bit; their
    pars gradients through autograd to 1e-13"""
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
    jac = _jacrec(23.5, 23.5, 0.0)
    sb = StampBatch.from_images(torch.zeros((n,) + dims, dtype=torch.float64, device="cuda"),
                                None, jac)
    up = torch.randn(n * dims[0] * dims[1], generator=g, device="cuda", dtype=torch.float64)
    idx = np.sort(rng.choice(n, 64, replace=False))
    d_idx = torch.from_numpy(idx).cuda()
    sub = sb.select(idx)
    ups = up.reshape(n, -1)[d_idx].reshape(-1)

    def run(b, pp, qq, u):
        mix, _ = ad.mixture_from_pars(pp, "exp")
        mix, _ = ad.convolve(mix, qq)
        gm = mix.detach().requires_grad_(True)
        im, st = ad.stamp_render(b, gm)
        assert int(st.abs().sum()) == 0
        (im * u).sum().backward()
        p = pp.detach().clone().requires_grad_(True)
        pg, = torch.autograd.grad((ad.render(b, p, "exp", psf=qq) * u).sum(), p)
        return im.detach(), gm.grad, pg

    im, gg, pg = run(sb, pars, psf, up)
    assert bool(torch.isfinite(gg).all()) and bool(torch.isfinite(pg).all())
    ims, ggs, pgs = run(sub, pars[d_idx], psf[d_idx], ups)
    np.testing.assert_array_equal(ims.cpu().numpy(),
                                  im.reshape(n, -1)[d_idx].reshape(-1).cpu().numpy())
    np.testing.assert_array_equal(ggs.cpu().numpy(), gg[d_idx].cpu().numpy())
    ref = pg[d_idx].cpu().numpy()
    scale = np.abs(ref).max(axis=1, keepdims=True)
    assert np.all(np.abs(pgs.cpu().numpy() - ref) <= 1e-13 * scale)
