"""Host checks of autodiff.stamp_fisher / fisher / covariance: the argument
and layout checks run before any stamp is touched or any kernel launched."""
import numpy as np
import pytest
import torch

import ngmix_amd as ngmix
from ngmix_amd import _lib, autodiff


class NoStamps(object):
    """stands in for a StampBatch: any use beyond n / device fails"""
    device = torch.device("cpu")

    def __init__(self, n):
        self.n = n


def _z(*shape):
    return torch.zeros(shape, dtype=torch.float64)


def test_names_exported():
    for name in ("stamp_fisher", "fisher", "covariance"):
        assert name in autodiff.__all__
        assert not hasattr(ngmix, name)
    assert "ngmix_fisher_batch" in _lib.SIGNATURES


@pytest.mark.parametrize("gshape,dshape,match", [
    ((2, 3), (2, 3, 6, 4), "nstamps, G, 6"),
    ((2, 3, 5), (2, 3, 6, 4), "nstamps, G, 6"),
    ((3, 2, 6), (3, 2, 6, 4), "one mixture per stamp"),
    ((2, 0, 6), (2, 0, 6, 4), "at least one gaussian"),
    ((2, 3, 6), (2, 3, 6), "nstamps, G, 6, K"),
    ((2, 3, 6), (2, 2, 6, 4), "nstamps, G, 6, K"),
    ((2, 3, 6), (2, 3, 5, 4), "nstamps, G, 6, K"),
    ((2, 3, 6), (2, 3, 6, 17), "K must be 1..16"),
    ((2, 3, 6), (2, 3, 6, 0), "K must be 1..16"),
])
def test_stamp_fisher_shape_checks(gshape, dshape, match):
    with pytest.raises(ValueError, match=match):
        autodiff.stamp_fisher(NoStamps(2), _z(*gshape), _z(*dshape))


def test_stamp_fisher_device_check():
    class MetaStamps(NoStamps):
        device = torch.device("meta")

    with pytest.raises(ValueError, match="device"):
        autodiff.stamp_fisher(MetaStamps(1), _z(1, 2, 6), _z(1, 2, 6, 3))


def test_stamp_fisher_weight_checks():
    class Stamps(NoStamps):
        total_pix = 20
        pix_off = np.array([0, 10])
        npix = np.array([10, 10])

    with pytest.raises(ValueError, match="weight: a flat tensor"):
        autodiff.stamp_fisher(Stamps(2), _z(2, 1, 6), _z(2, 1, 6, 3), weight=_z(2, 10))
    with pytest.raises(ValueError, match="the stamps span 20"):
        autodiff.stamp_fisher(Stamps(2), _z(2, 1, 6), _z(2, 1, 6, 3), weight=_z(19))


@pytest.mark.parametrize("func", [autodiff.fisher, autodiff.covariance])
@pytest.mark.parametrize("kw,match", [
    (dict(model="exp", pars=np.zeros((2, 5))), "5 shape columns"),
    (dict(model="bdf", pars=np.zeros((2, 7)), stamp_band=[0, 1]), "one flux per band"),
    (dict(model="coellip", pars=np.zeros((2, 7))), "coellip needs"),
    (dict(model="exp", pars=np.zeros((3, 6))), "stamp_obj is needed"),
    (dict(model="exp", pars=np.zeros((2, 6)), stamp_obj=[1, 0]), "non-decreasing"),
    (dict(model="exp", pars=np.zeros((2, 6)), stamp_band=[0, -1]), "non-negative band"),
    (dict(model="nomodel", pars=np.zeros((2, 6))), "model"),
    (dict(model="coellip", pars=np.ones((2, 18))), "at most 16 parameters"),
])
def test_layout_checks(func, kw, match):
    kw = dict(kw)
    pars = torch.from_numpy(kw.pop("pars"))
    model = kw.pop("model")
    with pytest.raises((ValueError, KeyError), match=match):
        func(NoStamps(2), pars, model, **kw)


def test_pars_device_check():
    class MetaStamps(NoStamps):
        device = torch.device("meta")

    with pytest.raises(ValueError, match="device"):
        autodiff.fisher(MetaStamps(1), torch.zeros((1, 6), dtype=torch.float64), "exp")


def test_psf_shape_check():
    with pytest.raises(ValueError, match="psf"):
        autodiff.covariance(NoStamps(2), torch.ones((2, 6), dtype=torch.float64), "exp",
                            psf=torch.ones((2, 6), dtype=torch.float64))
