"""
ngmix_amd.metacal without a device: the public names, argument errors, the
paths that are not served, container shapes, and the C entry's refusals.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import ngmix_amd as ngmix
from ngmix_amd import _lib, metacal
from helpers import metacal_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _obs(shape=(16, 16), psf_shape=(15, 15), seed=0, noise=False, psf=True):
    rng = np.random.RandomState(seed)
    jac = ngmix.Jacobian(row=(shape[0] - 1) / 2 + 0.2, col=(shape[1] - 1) / 2 - 0.3,
                         dvdrow=0.5, dvdcol=0.02, dudrow=-0.01, dudcol=0.52)
    pjac = ngmix.Jacobian(row=(psf_shape[0] - 1) / 2, col=(psf_shape[1] - 1) / 2,
                          dvdrow=0.5, dvdcol=0.02, dudrow=-0.01, dudcol=0.52)
    eye = np.eye(2)
    im = M.gaussian_stamp(shape, jac.get_data().view("f8"), 0.9 * eye, 50.0)
    im = im + rng.normal(scale=1e-3, size=shape)
    pim = M.gaussian_stamp(psf_shape, pjac.get_data().view("f8"), 0.45 * eye, 1.0)
    pobs = ngmix.Observation(pim, weight=np.full(psf_shape, 1e6), jacobian=pjac)
    return ngmix.Observation(im, weight=np.full(shape, 1e6), jacobian=jac,
                             psf=pobs if psf else None,
                             noise=rng.normal(scale=1e-3, size=shape) if noise else None)


def test_module_is_exported():
    assert ngmix.metacal is metacal
    for name in ("MetacalBatch", "get_all_metacal", "METACAL_TYPES", "METACAL_MINIMAL_TYPES"):
        assert name in metacal.__all__ and hasattr(metacal, name)
    assert metacal.METACAL_MINIMAL_TYPES == ["noshear", "1p", "1m", "2p", "2m"]
    assert "interpolant differs" in metacal.__doc__.lower()


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ngmix_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+ngmix_metacal_spectrum_batch\s*\(", header)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ngmix_metacal_spectrum_batch")
    assert len(_lib.SIGNATURES["ngmix_metacal_spectrum_batch"][1]) == 19
    assert "metacal.hip" in _lib._makefile_list("SRCS")


def test_c_entry_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert M.cabi_refusals(L, _lib.ERR_BAD_ARG) == []
    assert "metacal_spectrum" in L.ngmix_last_error().decode()


@pytest.mark.parametrize("psf", ["gauss", "azgauss", "dilate", object()])
def test_psfs_that_rest_on_galsim_are_not_implemented(psf):
    with pytest.raises(NotImplementedError, match="galsim"):
        metacal.get_all_metacal(_obs(), psf=psf, rng=np.random.RandomState(1))
    with pytest.raises(NotImplementedError, match="galsim"):
        metacal.MetacalBatch(None, None, psf=psf)


def test_argument_errors():
    rng = np.random.RandomState(1)
    with pytest.raises(ValueError, match="bad metacal psf"):
        metacal.get_all_metacal(_obs(), psf="blah", rng=rng)
    with pytest.raises(ValueError, match="bad metacal type"):
        metacal.get_all_metacal(_obs(), types=["noshear", "3p"], rng=rng)
    with pytest.raises(NotImplementedError, match="shearing the psf"):
        metacal.get_all_metacal(_obs(), types=["1p_psf"], rng=rng)
    with pytest.raises(ValueError, match="Observation, ObsList"):
        metacal.get_all_metacal(3, rng=rng)
    with pytest.raises(ValueError, match="rng"):
        metacal.get_all_metacal(_obs())
    with pytest.raises(ValueError, match="psf observation"):
        metacal.get_all_metacal(_obs(psf=False), rng=rng)
    with pytest.raises(ValueError, match="obs.noise"):
        metacal.get_all_metacal(_obs(), rng=rng, use_noise_image=True)
    with pytest.raises(ValueError, match="square"):
        metacal.get_all_metacal(_obs(shape=(12, 17)), rng=rng)
    o = _obs()
    pj = o.psf.jacobian
    o.psf.jacobian = ngmix.Jacobian(row=pj.row0, col=pj.col0, dvdrow=0.4, dvdcol=0.0, dudrow=0.0,
                                    dudcol=0.4)
    with pytest.raises(ValueError, match="same jacobian"):
        metacal.get_all_metacal(o, rng=rng)
    with pytest.raises(ValueError, match="StampBatch"):
        metacal.MetacalBatch(None, None, target_sigma=np.ones(2))
    with pytest.raises(ValueError, match="unit circle"):
        metacal._check_shears(np.array([[0.8, 0.7]]))


def test_type_shears_and_fitgauss_sigma():
    np.testing.assert_array_equal(
        metacal._type_shears(["noshear", "1p", "1m", "2p", "2m"], 0.02),
        [[0, 0], [0.02, 0], [-0.02, 0], [0, 0.02], [0, -0.02]])
    rng = np.random.RandomState(4)
    irr, icc = rng.uniform(0.1, 0.4, size=(2, 50))
    irc = rng.uniform(-0.05, 0.05, size=50)
    np.testing.assert_allclose(metacal.fitgauss_sigma(irr, irc, icc),
                               M.fitgauss_sigma(irr, irc, icc), rtol=1e-15)
    # the reference's own steps: e2mom, eigenvalues, the dilation and its cap
    for a, b, c in zip(irr, irc, icc):
        T = a + c
        dil = np.sqrt(np.linalg.eigvalsh([[a, b], [b, c]]).max() / (T / 2.0))
        dil = min(1.0 + 2 * (dil - 1.0), 1.1)
        assert metacal.fitgauss_sigma(a, b, c) == pytest.approx(np.sqrt(T * dil / 2.0), rel=1e-13)


def test_containers_are_flattened_and_rebuilt():
    a, b, c = _obs(seed=1), _obs(seed=2), _obs(seed=3)
    flat, rebuild = metacal._flatten(a)
    assert flat == [a] and rebuild([b]) is b
    ol = ngmix.ObsList()
    ol.append(a)
    ol.append(b)
    flat, rebuild = metacal._flatten(ol)
    out = rebuild([c, a])
    assert isinstance(out, ngmix.ObsList) and len(out) == 2 and out[0] is c and out[1] is a
    mb = ngmix.MultiBandObsList()
    mb.append(ol)
    ol2 = ngmix.ObsList()
    ol2.append(c)
    mb.append(ol2)
    flat, rebuild = metacal._flatten(mb)
    assert len(flat) == 3 and flat[2] is c
    out = rebuild([c, b, a])
    assert isinstance(out, ngmix.MultiBandObsList) and [len(x) for x in out] == [2, 1]
    assert out[0][0] is c and out[0][1] is b and out[1][0] is a


def test_get_all_metacal_needs_the_device_and_keeps_the_container():
    """without a GPU the call fails loudly, as every compute entry of the
    package does; with one, every type holds a container like the input's"""
    mb = ngmix.MultiBandObsList()
    for band in range(2):
        ol = ngmix.ObsList()
        for epoch in range(2 - band):
            ol.append(_obs(seed=10 * band + epoch, noise=True))
        mb.append(ol)
    rng = np.random.RandomState(8)
    if not _has_gpu():
        with pytest.raises(RuntimeError, match="GPU"):
            metacal.get_all_metacal(mb, rng=rng)
        return
    res = metacal.get_all_metacal(mb, rng=rng, use_noise_image=True)
    assert list(res) == metacal.METACAL_MINIMAL_TYPES
    for t, out in res.items():
        assert isinstance(out, ngmix.MultiBandObsList) and [len(x) for x in out] == [2, 1]
        for ol_in, ol_out in zip(mb, out):
            for o_in, o_out in zip(ol_in, ol_out):
                assert o_out.image.shape == o_in.image.shape
                assert np.all(np.isfinite(o_out.image)) and o_out.meta["metacal_flags"] == 0
                np.testing.assert_array_equal(o_out.weight, o_in.weight / 2)
                np.testing.assert_array_equal(o_out.weight_orig, o_in.weight)
                assert o_out.psf.jacobian.row0 == 7.0 and o_out.psf.jacobian.col0 == 7.0
                assert o_out.jacobian.row0 == o_in.jacobian.row0
                assert np.all(o_out.psf.weight == 1.0 / (o_in.psf.image.max() / 50000.0) ** 2)
    one = metacal.get_all_metacal(mb[0][0], rng=rng, fixnoise=False, types=["noshear", "2m"])
    assert list(one) == ["noshear", "2m"] and isinstance(one["2m"], ngmix.Observation)
    np.testing.assert_array_equal(one["2m"].weight, mb[0][0].weight)
