"""Host checks of ngmix_amd.autodiff: the torch mixture construction and
convolution against the host GMix classes, and the refusal of a host-loop
prior when a gradient is asked for."""
import numpy as np
import pytest
import torch

import ngmix_amd as ngmix
from ngmix_amd import autodiff
from ngmix_amd.gexceptions import GMixRangeError
from ngmix_amd.gmix import GMix, GMixModel, GMixCoellip


def _rows(model, n, rng, ngauss=None):
    base = np.column_stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n),
                            rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n)])
    if model == "coellip":
        T = rng.uniform(0.05, 3.0, (n, ngauss))
        F = rng.uniform(1.0, 100.0, (n, ngauss))
        pars = np.column_stack([base, T, F])
    else:
        T = rng.uniform(-0.2, 3.0, n)
        F = rng.uniform(-5.0, 500.0, n)
        extra = []
        if model == "bdf":
            extra = [rng.uniform(-0.2, 1.2, n)]
        elif model == "bd":
            extra = [rng.uniform(-1.0, 1.0, n), rng.uniform(-0.2, 1.2, n)]
        pars = np.column_stack([base, T] + extra + [F])
    # edges: g = 0 exactly, |g| just below 1, |g| >= 1, fracdev 0 and 1
    pars[0, 2:4] = 0.0
    pars[1, 2:4] = [0.6, -0.79]
    pars[2, 2:4] = [0.8, 0.6]
    pars[3, 2:4] = [1.2, 0.0]
    if model == "bdf":
        pars[4, 5], pars[5, 5] = 0.0, 1.0
    if model == "bd":
        pars[4, 6], pars[5, 6] = 0.0, 1.0
    return pars


def _host(pars, model):
    if model == "coellip":
        return GMixCoellip(pars)
    return GMixModel(pars, model)


CASES = [("gauss", None), ("turb", None), ("exp", None), ("dev", None), ("bdf", None),
         ("bd", None)] + [("coellip", k) for k in range(1, 6)]


@pytest.mark.parametrize("model,ngauss", CASES)
def test_mixture_from_pars_matches_host(model, ngauss):
    rng = np.random.RandomState(11 + (ngauss or 0))
    pars = _rows(model, 40, rng, ngauss)
    mix, bad = autodiff.mixture_from_pars(torch.from_numpy(pars), model, ngauss=ngauss)
    assert mix.dtype == torch.float64 and mix.device.type == "cpu"
    mix = mix.numpy()
    bad = bad.numpy()
    for i in range(pars.shape[0]):
        try:
            ref = _host(pars[i], model).get_full_pars().reshape(-1, 6)
        except (GMixRangeError, ZeroDivisionError):
            assert bad[i], (model, i)
            assert np.all(np.isnan(mix[i]))
            continue
        assert not bad[i], (model, i)
        np.testing.assert_allclose(mix[i], ref, rtol=1e-15, atol=0.0)


@pytest.mark.parametrize("model,ngauss", [("exp", None), ("bdf", None), ("bd", None),
                                          ("coellip", 3), ("gauss", None)])
def test_convolve_matches_host(model, ngauss):
    rng = np.random.RandomState(5)
    n = 20
    pars = _rows(model, n, rng, ngauss)[6:]
    pars[:, 2:4] *= 0.5
    n = pars.shape[0]
    npsf = 3
    psf = np.zeros((n, npsf, 6))
    psf[:, :, 0] = rng.uniform(0.1, 1.0, (n, npsf))
    psf[:, :, 1:3] = rng.uniform(-0.05, 0.05, (n, npsf, 2))
    T = rng.uniform(0.1, 1.0, (n, npsf))
    e = rng.uniform(-0.1, 0.1, (n, npsf, 2))
    psf[:, :, 3] = 0.5 * T * (1 - e[..., 0])
    psf[:, :, 4] = 0.5 * T * e[..., 1]
    psf[:, :, 5] = 0.5 * T * (1 + e[..., 0])
    psf[0, :, 0] = [0.5, -0.5, 0.0]   # zero flux: the host's ZeroDivisionError
    mix, mbad = autodiff.mixture_from_pars(torch.from_numpy(pars), model, ngauss=ngauss)
    conv, cbad = autodiff.convolve(mix, torch.from_numpy(psf))
    conv = conv.numpy()
    for i in range(n):
        gm = _host(pars[i], model)
        pg = GMix(pars=psf[i].reshape(-1))
        try:
            ref = gm.convolve(pg).get_full_pars().reshape(-1, 6)
        except (GMixRangeError, ZeroDivisionError):
            assert bool(cbad[i])
            assert np.all(np.isnan(conv[i]))
            continue
        assert not bool(cbad[i]) and not bool(mbad[i])
        # (1e-15 of each column's scale: a sum like o.irc + q.irc cancels, and
        # tanh / atanh / pow may round differently in torch and the C library)
        np.testing.assert_allclose(conv[i], ref, rtol=1e-15,
                                   atol=1e-15 * np.abs(ref).max(axis=0).max())


def test_mixture_is_differentiable():
    """torch carries gradients through the mixture, g = 0 included (the slope
    of e = 2g / (1 + g^2) there is 2)"""
    pars = torch.tensor([[0.1, -0.2, 0.0, 0.0, 1.3, 0.4, 20.0]], dtype=torch.float64,
                        requires_grad=True)
    mix, _ = autodiff.mixture_from_pars(pars, "bdf")
    irr = mix[0, :, 3].sum()
    irr.backward()
    assert torch.all(torch.isfinite(pars.grad))
    # d irr / d g1 at g = 0 is -2 * sum(T_i / 2)
    assert pars.grad[0, 2].item() == pytest.approx(-2.0 * mix[0, :, 3].sum().item(),
                                                   rel=1e-12)


def test_bad_rows_do_not_touch_good_rows():
    pars = torch.tensor([[0.0, 0.0, 0.1, 0.2, 1.0, 5.0],
                         [0.0, 0.0, 1.5, 0.2, 1.0, 5.0]], dtype=torch.float64)
    mix2, bad2 = autodiff.mixture_from_pars(pars, "exp")
    mix1, _ = autodiff.mixture_from_pars(pars[:1], "exp")
    assert bad2.tolist() == [False, True]
    assert torch.equal(mix2[0], mix1[0])


def test_host_loop_prior_refuses_gradient():
    """a prior only the host loop evaluates has no gradient: a clear error,
    before any stamp is touched"""

    class HostPrior(object):
        def fill_fdiff(self, pars, fdiff):
            fdiff[0] = pars[0]
            return 1

        def get_lnprob_scalar(self, pars):
            return -0.5 * pars[0] ** 2

    pars = torch.zeros((2, 6), dtype=torch.float64, requires_grad=True)

    class NoStamps(object):
        device = torch.device("cpu")
        n = 2

    with pytest.raises(TypeError, match="no gradient"):
        autodiff.lnprob(NoStamps(), pars, "exp", prior=HostPrior())


def test_no_new_top_level_names():
    assert not hasattr(ngmix, "loglike_grad")
    assert not hasattr(ngmix, "mixture_from_pars")
