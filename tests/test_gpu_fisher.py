"""
Batched Fisher matrices and parameter covariances (csrc/fisher.hip through
autodiff.stamp_fisher / fisher / covariance), checked against the reference's
derivative images, against the covariances of LMBatchFitter and of the
reference's own fits, against float64 derivatives formed in the test, and for
symmetry, flags, isolation, determinism and scale.
"""
import math

import numpy as np
import pytest

from ngmix_amd import prior_batch as pb
from ngmix_amd.batch import StampBatch
from ngmix_amd.flags import LM_SINGULAR_MATRIX

from test_gpu_autodiff import TIGHT, _gm_records, _jacrec, _make, _psf

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _ad():
    from ngmix_amd import autodiff
    return autodiff


def _norm_err(a, b):
    """max |a - b| / sqrt(diag_i diag_j) over a batch of matrices (of b)"""
    d = np.sqrt(np.abs(np.einsum("nii->ni", b)))
    return np.max(np.abs(a - b) / (d[:, :, None] * d[:, None, :]))


def _true_J(sb, mix, s):
    """float64 d model / d theta (npix, G, 6) of stamp s, the true derivative
    of pnorm exp(-chi2/2) area, by forward-mode AD in torch on the host"""
    torch = _torch()
    nrow, ncol = int(sb.nrow[s]), int(sb.ncol[s])
    jac = sb.jac.cpu().numpy()[s]
    rows, cols = np.mgrid[0:nrow, 0:ncol]
    v = torch.from_numpy((jac[2] * (rows - jac[0]) + jac[3] * (cols - jac[1])).ravel())
    u = torch.from_numpy((jac[4] * (rows - jac[0]) + jac[5] * (cols - jac[1])).ravel())
    area = jac[7] ** 2

    def model(g):
        p, r, c, irr, irc, icc = (g[:, i, None] for i in range(6))
        det = irr * icc - irc * irc
        dv, du = v[None, :] - r, u[None, :] - c
        chi2 = (icc * dv * dv + irr * du * du - 2.0 * irc * dv * du) / det
        return (p / (2.0 * math.pi * torch.sqrt(det)) * torch.exp(-0.5 * chi2) * area).sum(0)

    g = torch.from_numpy(mix[s].cpu().numpy())
    return torch.func.jacfwd(model)(g).numpy()


def _ref_fisher(J, A, w):
    """sum_pix w (J A)(J A)^T: J (npix, G, 6), A (G, 6, K), w (npix,)"""
    X = np.einsum("pga,gak->pk", J, A)
    return np.einsum("p,pk,pl->kl", w, X, X)


# ------------------------------------------------------------------ golden


def test_fisher_on_golden_derivs(golden):
    """tests/golden/derivs.npz: the reference's deriv_images of gauss / exp /
    dev without a psf and with 1- and 3-gaussian psfs.  The reference Fisher
    J diag(ivar) J^T from the golden images alone ([cen1, cen2, g1, g2, T]
    planes, the value image over the flux for the flux column) against
    fisher() at the golden pars, to 1e-10 of the matrix's largest entry"""
    torch = _torch()
    ad = _ad()
    g = golden("derivs")
    nrow, ncol = (int(x) for x in g["dims"])
    jac = g["jac"][0]
    rec = np.array([jac[k] for k in jac.dtype.names])
    for name in [str(n) for n in g["names"]]:
        model = name.split("_")[0]
        pars = g[name + "_pars"]
        out = g[name + "_out"]
        ivar = np.full(out.shape[1], 1.0 / (0.01 * out[0].max()) ** 2)
        J = np.concatenate([out[1:6], out[0:1] / pars[5]])
        ref = np.einsum("p,kp,lp->kl", ivar, J, J)
        sb = StampBatch.from_arrays([out[0].reshape(nrow, ncol)], [ivar.reshape(nrow, ncol)],
                                    rec[None, :], [True])
        psf = None
        if name + "_psf" in g:
            pr = g[name + "_psf"]
            psf = torch.from_numpy(np.stack([pr[k] for k in ("p", "row", "col", "irr", "irc",
                                                             "icc")], axis=1)[None]).cuda()
        p = torch.from_numpy(pars[None, :].copy()).cuda()
        F = ad.fisher(sb, p, model, psf=psf)[0].cpu().numpy()
        assert np.all(np.abs(F - ref) <= 1e-10 * np.abs(ref).max()), (name, F, ref)


# ------------------------------------------------------- against the fits

# The LM's pars_cov0 is inv(J^T J) of MINPACK's LAST jacobian, taken at the
# point one accepted step before the pars it returns.  J moves with the pars
# on the scale of the object (size, centre) or of g (~1), and one sigma of the
# pars is that scale over s/n: a last step of e sigma changes the normalised
# entries by ~ e / (s/n).  TIGHT fits (ftol 1e-12) stop once a step lowers
# chi2 (~ npix ~ 1e3) by a relative 1e-12, i.e. e^2 <~ 1e-9, e <~ 3e-5; at
# s/n ~ 10-40 that is ~ 1e-6.  Measured on MI355X: at most 1.5e-6 (the prior
# case, the lowest s/n); the bound keeps a factor ~3.  The reference's C3
# fits stop at ftol 1e-5 (DEFAULT_LM_PARS): e ~ 1e-1, s/n 85-400, e / (s/n)
# ~ 1e-3.  Measured: 2.1e-3; bound 5e-3.
TOL_TIGHT = 5e-6
TOL_C3 = 5e-3


def _fit_and_compare(model, sb, guess, psf, sobj=None, sband=None, prior=None):
    from ngmix_amd.lm_batch import LMBatchFitter
    torch = _torch()
    ad = _ad()
    res = LMBatchFitter(model, prior=prior, fit_pars=TIGHT).go(
        sb, guess, psf=_gm_records(psf), stamp_obj=sobj, stamp_band=sband)
    ok = np.asarray(res["flags"]) == 0
    assert ok.mean() > 0.8
    p = torch.from_numpy(np.asarray(res["pars"])).cuda()
    cov, flag = ad.covariance(sb, p, model, psf=torch.from_numpy(psf).cuda(), stamp_obj=sobj,
                              stamp_band=sband, prior=prior, return_flags=True)
    assert np.all(flag.cpu().numpy() == 0)
    ref = np.asarray(res["pars_cov0"])[ok]
    err = _norm_err(cov.cpu().numpy()[ok], ref)
    print("%s: normalised |cov - pars_cov0| max %.3g" % (model, err))
    assert err < TOL_TIGHT, err


def test_covariance_matches_lm_exp_psf3():
    rng = np.random.RandomState(41)
    sb, truth, psf, _, _ = _make(rng, "exp", 48, dims=(33, 33), npsf=3)
    guess = truth * rng.uniform(0.95, 1.05, truth.shape)
    _fit_and_compare("exp", sb, guess, psf)


def test_covariance_matches_lm_two_bands_two_epochs():
    rng = np.random.RandomState(42)
    sb, truth, psf, sobj, sband = _make(rng, "exp", 24, nep=2, nband=2, dims=(33, 33),
                                        npsf=2)
    guess = truth * rng.uniform(0.95, 1.05, truth.shape)
    _fit_and_compare("exp", sb, guess, psf, sobj, sband)


def test_covariance_matches_lm_with_prior():
    rng = np.random.RandomState(43)
    sb, truth, psf, _, _ = _make(rng, "exp", 32, dims=(33, 33), npsf=2, noise=0.2)
    prior = pb.PriorSimpleSepBatch(pb.GaussianCen(0.0, 0.0, 0.1, 0.1), pb.GPriorBA(0.2),
                                   pb.Normal(1.0, 0.3), pb.Normal(140.0, 30.0))
    guess = truth * rng.uniform(0.95, 1.05, truth.shape)
    _fit_and_compare("exp", sb, guess, psf, prior=prior)


def test_covariance_at_reference_c3_solutions(golden):
    """tests/golden/lm_c3.npz: the reference's own fits of forty 48x48 'exp'
    objects (gaussian psf): covariance() at its pars against its pars_cov0"""
    torch = _torch()
    ad = _ad()
    g = golden("lm_c3")
    n = g["images"].shape[0]
    weights = np.broadcast_to((1.0 / g["sigma"] ** 2)[:, None, None], g["images"].shape).copy()
    sb = StampBatch.from_images(g["images"], weights, g["jac"])
    psf = torch.from_numpy(np.tile(g["psf_pars"][None, None, :], (n, 1, 1))).cuda()
    cov = ad.covariance(sb, torch.from_numpy(g["pars"]).cuda(), "exp", psf=psf)
    err = _norm_err(cov.cpu().numpy(), g["pars_cov0"])
    print("c3: normalised |cov - pars_cov0| max %.3g" % err)
    assert err < TOL_C3, err


# ------------------------------------------------------------ raw form


def _blend(rng, n=3, dims=(31, 29)):
    """two exp objects drawn into the same stamps (3-gaussian psf): stamps,
    each object's (n, 18, 6) mixture and (n, 18, 6, 6) tangents"""
    torch = _torch()
    ad = _ad()
    pa = np.array([[-0.6, 0.4, 0.1, -0.2, 1.0, 120.0]] * n) + rng.uniform(-0.05, 0.05, (n, 6))
    pb_ = np.array([[0.7, -0.3, -0.2, 0.1, 0.7, 90.0]] * n) + rng.uniform(-0.05, 0.05, (n, 6))
    psf = np.array([_psf(rng, 3) for _ in range(n)])
    jacs = np.array([_jacrec((dims[0] - 1) / 2.0, (dims[1] - 1) / 2.0, 0.05)
                     for _ in range(n)])
    imgs = [rng.normal(size=dims) for _ in range(n)]
    wts = [rng.uniform(0.5, 2.0, size=dims) for _ in range(n)]
    sb = StampBatch.from_arrays(imgs, wts, jacs, [True] * n)
    d_psf = torch.from_numpy(psf).cuda()
    mixes, tans = [], []
    for pars in (pa, pb_):
        (_, _, m, _, _), dm = ad._mixture_tangents(sb, torch.from_numpy(pars).cuda(), "exp",
                                                   d_psf, None, None, None)
        mixes.append(m)
        tans.append(dm)
    return sb, mixes, tans


@pytest.mark.parametrize("fast_exp", [True, False])
def test_blend_blocks(fast_exp):
    """K = 12 over a two-object blend: each diagonal 6x6 block is that
    object's own stamp_fisher to rounding; exact mode: every block against the
    contraction of float64 true derivatives"""
    torch = _torch()
    ad = _ad()
    sb, (ma, mb), (da, db) = _blend(np.random.RandomState(5))
    n, G = ma.shape[0], ma.shape[1]
    mix = torch.cat([ma, mb], dim=1)
    dg = torch.zeros((n, 2 * G, 6, 12), dtype=torch.float64, device="cuda")
    dg[:, :G, :, :6] = da
    dg[:, G:, :, 6:] = db
    F, st = ad.stamp_fisher(sb, mix, dg, fast_exp=fast_exp)
    Fa, _ = ad.stamp_fisher(sb, mix, dg[..., :6], fast_exp=fast_exp)
    Fb, _ = ad.stamp_fisher(sb, mix, dg[..., 6:], fast_exp=fast_exp)
    assert np.all(st.cpu().numpy() == 0)
    F, Fa, Fb = F.cpu().numpy(), Fa.cpu().numpy(), Fb.cpu().numpy()
    for s in range(n):
        scale = np.abs(F[s]).max()
        assert np.abs(F[s, :6, :6] - Fa[s]).max() <= 1e-12 * scale
        assert np.abs(F[s, 6:, 6:] - Fb[s]).max() <= 1e-12 * scale
    if not fast_exp:
        w = sb.ierr.cpu().numpy() ** 2
        A = dg.cpu().numpy()
        for s in range(n):
            J = _true_J(sb, mix, s)
            ref = _ref_fisher(J, A[s], w[sb.pix_off[s]:sb.pix_off[s] + sb.npix[s]])
            assert np.abs(F[s] - ref).max() <= 1e-12 * np.abs(ref).max(), s


def test_exact_mode_matches_true_derivative():
    """fast_exp=False against float64 true derivatives, sheared, ragged
    stamps with zero-weight pixels, 1e-12 relative"""
    torch = _torch()
    ad = _ad()
    rng = np.random.RandomState(8)
    sb, pars, psf, _, _ = _make(rng, "dev", 4, npsf=2, shear=0.1, zero_frac=0.1, ragged=True)
    d_psf = torch.from_numpy(psf).cuda()
    (_, _, mix, _, _), dm = ad._mixture_tangents(sb, torch.from_numpy(pars).cuda(), "dev",
                                                 d_psf, None, None, None)
    F, st = ad.stamp_fisher(sb, mix, dm, fast_exp=False)
    F = F.cpu().numpy()
    w = sb.ierr.cpu().numpy() ** 2
    A = dm.cpu().numpy()
    for s in range(sb.n):
        ref = _ref_fisher(_true_J(sb, mix, s), A[s],
                          w[sb.pix_off[s]:sb.pix_off[s] + sb.npix[s]])
        assert np.abs(F[s] - ref).max() <= 1e-12 * np.abs(ref).max(), s
    # fisher() is stamp_fisher of the same tangents
    Fo = ad.fisher(sb, torch.from_numpy(pars).cuda(), "dev", psf=d_psf, fast_exp=False)
    assert np.array_equal(Fo.cpu().numpy(), F)


def test_weights():
    """weight = ierr^2 passed explicitly gives the default bits (the kernel
    takes sqrt of ierr^2 either way); a Poisson weight 1 / model against the
    float64 contraction"""
    torch = _torch()
    ad = _ad()
    rng = np.random.RandomState(9)
    sb, pars, psf, _, _ = _make(rng, "exp", 3, npsf=3, zero_frac=0.1)
    d_psf = torch.from_numpy(psf).cuda()
    (_, _, mix, _, _), dm = ad._mixture_tangents(sb, torch.from_numpy(pars).cuda(), "exp",
                                                 d_psf, None, None, None)
    for fast in (True, False):
        F0, _ = ad.stamp_fisher(sb, mix, dm, fast_exp=fast)
        F1, _ = ad.stamp_fisher(sb, mix, dm, weight=sb.ierr ** 2, fast_exp=fast)
        assert torch.equal(F0, F1)
    img, _ = ad.stamp_render(sb, mix, fast_exp=False)
    w = 1.0 / (img + 1.0)
    F, _ = ad.stamp_fisher(sb, mix, dm, weight=w, fast_exp=False)
    F, w, A = F.cpu().numpy(), w.cpu().numpy(), dm.cpu().numpy()
    for s in range(sb.n):
        ref = _ref_fisher(_true_J(sb, mix, s), A[s],
                          w[sb.pix_off[s]:sb.pix_off[s] + sb.npix[s]])
        assert np.abs(F[s] - ref).max() <= 1e-12 * np.abs(ref).max(), s


# ------------------------------------------------------------ structure


@pytest.mark.parametrize("model,nband,nep,ngauss", [("exp", 1, 1, None), ("bdf", 2, 2, None),
                                                    ("bd", 3, 1, None),
                                                    ("coellip", 1, 1, 6)])
def test_symmetric_psd_ragged(model, nband, nep, ngauss):
    """symmetric to the bit and positive semidefinite, on ragged sheared
    stamps; bdf / bd multi-band and coellip with 6 gaussians (K = 16)"""
    torch = _torch()
    ad = _ad()
    rng = np.random.RandomState(11)
    sb, pars, psf, sobj, sband = _make(rng, model, 5, nep=nep, nband=nband, npsf=2,
                                       shear=0.1, zero_frac=0.05, ragged=True, ngauss=ngauss)
    F, flag = ad.fisher(sb, torch.from_numpy(pars).cuda(), model,
                        psf=torch.from_numpy(psf).cuda(), stamp_obj=sobj, stamp_band=sband,
                        ngauss=ngauss, return_flags=True)
    assert np.all(flag.cpu().numpy() == 0)
    assert F.shape == (5, pars.shape[1], pars.shape[1])
    assert torch.equal(F, F.transpose(1, 2))
    ev = torch.linalg.eigvalsh(F)
    assert bool((ev >= -1e-12 * ev.abs().max(dim=1, keepdim=True).values).all())
    # fisher() of the stamps one by one, summed in stamp order: the same bits
    d_psf = torch.from_numpy(psf).cuda()
    (_, _, mix, _, _), dm = ad._mixture_tangents(sb, torch.from_numpy(pars).cuda(), model,
                                                 d_psf, sobj, sband, ngauss)
    Fs, _ = ad.stamp_fisher(sb, mix, dm)
    for o in range(5):
        tot = None
        for s in np.nonzero(sobj == o)[0]:
            tot = Fs[s] if tot is None else tot + Fs[s]
        assert torch.equal(tot, F[o])


def test_padded_gaussians():
    """mixed G in one batch: a stamp padded with zero-flux gaussians of zero
    tangent gives the unpadded matrix, bit for bit"""
    torch = _torch()
    ad = _ad()
    sb, (ma, _), (da, _) = _blend(np.random.RandomState(6))
    n, G = ma.shape[0], ma.shape[1]
    pad = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 1.0], dtype=torch.float64, device="cuda")
    mix = torch.cat([ma, pad.expand(n, 5, 6)], dim=1)
    dg = torch.cat([da, da.new_zeros((n, 5, 6, 6))], dim=1)
    F0, _ = ad.stamp_fisher(sb, ma, da)
    F1, _ = ad.stamp_fisher(sb, mix, dg)
    assert torch.equal(F0, F1)


def test_refusals():
    """K = 17 and a mixture too large for the LDS are refused before launch"""
    torch = _torch()
    ad = _ad()
    rng = np.random.RandomState(12)
    sb, pars, psf, _, _ = _make(rng, "gauss", 2, npsf=1)
    mix = torch.zeros((2, 1, 6), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="K must be 1..16"):
        ad.stamp_fisher(sb, mix, torch.zeros((2, 1, 6, 17), dtype=torch.float64,
                                             device="cuda"))
    big = torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], dtype=torch.float64,
                       device="cuda").expand(2, 1000, 6).contiguous()
    with pytest.raises(ValueError, match="LDS budget"):
        ad.stamp_fisher(sb, big, torch.zeros((2, 1000, 6, 3), dtype=torch.float64,
                                             device="cuda"))


def test_flags_isolated_and_deterministic():
    """an object with |g| >= 1 and one whose convolved gaussian the norms
    refuse get NaN and their flag; the others are bitwise the same with or
    without them, and two runs give the same bits"""
    from ngmix_amd import _lib
    torch = _torch()
    ad = _ad()
    rng = np.random.RandomState(13)
    sb, pars, psf, _, _ = _make(rng, "exp", 6, npsf=2)
    bad = pars.copy()
    bad[1, 2] = 0.9
    bad[1, 3] = 0.9
    bad[4, 4] = -2.0   # negative T: a convolved gaussian of negative det
    d_psf = torch.from_numpy(psf).cuda()
    F, flag = ad.fisher(sb, torch.from_numpy(bad).cuda(), "exp", psf=d_psf, return_flags=True)
    F2, flag2 = ad.fisher(sb, torch.from_numpy(bad).cuda(), "exp", psf=d_psf,
                          return_flags=True)
    assert torch.equal(flag, flag2)
    assert np.array_equal(F.cpu().numpy(), F2.cpu().numpy(), equal_nan=True)
    flag = flag.cpu().numpy()
    assert flag[1] == _lib.ERR_G_RANGE and flag[4] != 0
    assert np.all(flag[[0, 2, 3, 5]] == 0)
    F = F.cpu().numpy()
    assert np.all(np.isnan(F[[1, 4]]))
    Fg = ad.fisher(sb, torch.from_numpy(pars).cuda(), "exp", psf=d_psf).cpu().numpy()
    assert np.array_equal(F[[0, 2, 3, 5]], Fg[[0, 2, 3, 5]])
    cov, cflag = ad.covariance(sb, torch.from_numpy(bad).cuda(), "exp", psf=d_psf,
                               return_flags=True)
    assert np.array_equal(cflag.cpu().numpy(), flag)
    assert np.all(np.isnan(cov.cpu().numpy()[[1, 4]]))
    assert np.all(np.isfinite(cov.cpu().numpy()[[0, 2, 3, 5]]))


def test_singular_matrix_flagged():
    """a parameter the model does not depend on (a second band's flux with no
    stamp in that band) makes the matrix singular: NaN and LM_SINGULAR_MATRIX"""
    torch = _torch()
    ad = _ad()
    rng = np.random.RandomState(14)
    sb, pars, psf, sobj, sband = _make(rng, "exp", 3, npsf=2)
    pars2 = np.concatenate([pars, pars[:, 5:6]], axis=1)
    cov, flag = ad.covariance(sb, torch.from_numpy(pars2).cuda(), "exp",
                              psf=torch.from_numpy(psf).cuda(), return_flags=True)
    assert np.all(flag.cpu().numpy() == LM_SINGULAR_MATRIX)
    assert bool(torch.isnan(cov).all())


def test_large_batch_matches_sub_batch():
    """100k 48x48 stamps: a sub-batch of them gives the same bits"""
    torch = _torch()
    ad = _ad()
    rng = np.random.RandomState(15)
    n, dims = 100_000, (48, 48)
    g = torch.Generator(device="cuda").manual_seed(15)

    def uni(shape, lo, hi):
        return lo + (hi - lo) * torch.rand(shape, generator=g, device="cuda",
                                           dtype=torch.float64)

    pars = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    pars[:, 0:2] = uni((n, 2), -0.2, 0.2)
    pars[:, 2:4] = uni((n, 2), -0.3, 0.3)
    pars[:, 4] = uni(n, 0.5, 3.0)
    pars[:, 5] = uni(n, 50.0, 500.0)
    images = torch.randn((n,) + dims, generator=g, device="cuda", dtype=torch.float64)
    sb = StampBatch.from_images(images, uni((n,) + dims, 0.5, 2.0), _jacrec(23.5, 23.5, 0.05))
    psf = torch.from_numpy(np.tile(_psf(rng, 3)[None], (n, 1, 1))).cuda()
    F = ad.fisher(sb, pars, "exp", psf=psf)
    assert bool(torch.isfinite(F).all())
    idx = np.sort(rng.choice(n, 64, replace=False))
    d_idx = torch.from_numpy(idx).cuda()
    Fs = ad.fisher(sb.select(idx), pars[d_idx], "exp", psf=psf[d_idx])
    assert torch.equal(F[d_idx], Fs)
