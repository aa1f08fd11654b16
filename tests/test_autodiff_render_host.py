"""Host checks of autodiff.render / autodiff.stamp_render: the argument and
layout checks run before any stamp is touched or any kernel launched."""
import numpy as np
import pytest
import torch

import ngmix_amd as ngmix
from ngmix_amd import autodiff


class NoStamps(object):
    """stands in for a StampBatch: any use beyond n / device fails"""
    device = torch.device("cpu")

    def __init__(self, n):
        self.n = n


def test_names_exported():
    assert "render" in autodiff.__all__ and "stamp_render" in autodiff.__all__
    assert not hasattr(ngmix, "stamp_render")


@pytest.mark.parametrize("shape,match", [((2, 3), "nstamps, G, 6"),
                                         ((2, 3, 5), "nstamps, G, 6"),
                                         ((3, 2, 6), "one mixture per stamp"),
                                         ((2, 0, 6), "at least one gaussian")])
def test_stamp_render_shape_checks(shape, match):
    with pytest.raises(ValueError, match=match):
        autodiff.stamp_render(NoStamps(2), torch.zeros(shape, dtype=torch.float64))


def test_stamp_render_device_check():
    class MetaStamps(NoStamps):
        device = torch.device("meta")

    with pytest.raises(ValueError, match="device"):
        autodiff.stamp_render(MetaStamps(1), torch.zeros((1, 2, 6), dtype=torch.float64))


@pytest.mark.parametrize("kw,match", [
    (dict(model="exp", pars=np.zeros((2, 5))), "5 shape columns"),
    (dict(model="bdf", pars=np.zeros((2, 7)), stamp_band=[0, 1]), "one flux per band"),
    (dict(model="coellip", pars=np.zeros((2, 7))), "coellip needs"),
    (dict(model="exp", pars=np.zeros((3, 6))), "stamp_obj is needed"),
    (dict(model="exp", pars=np.zeros((2, 6)), stamp_obj=[1, 0]), "non-decreasing"),
    (dict(model="exp", pars=np.zeros((2, 6)), stamp_band=[0, -1]), "non-negative band"),
    (dict(model="nomodel", pars=np.zeros((2, 6))), "model"),
])
def test_render_layout_checks(kw, match):
    kw = dict(kw)
    pars = torch.from_numpy(kw.pop("pars"))
    model = kw.pop("model")
    with pytest.raises((ValueError, KeyError), match=match):
        autodiff.render(NoStamps(2), pars, model, **kw)


def test_render_pars_device_check():
    class MetaStamps(NoStamps):
        device = torch.device("meta")

    with pytest.raises(ValueError, match="device"):
        autodiff.render(MetaStamps(1), torch.zeros((1, 6), dtype=torch.float64), "exp")


def test_render_psf_shape_check():
    with pytest.raises(ValueError, match="psf"):
        autodiff.render(NoStamps(2), torch.ones((2, 6), dtype=torch.float64), "exp",
                        psf=torch.ones((2, 6), dtype=torch.float64))
