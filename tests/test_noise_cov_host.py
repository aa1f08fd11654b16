"""Host-side checks of the noise-image sandwich covariance routes: what is
refused before anything reaches a device."""
import numpy as np
import pytest

import ngmix_amd as ngmix
from ngmix_amd.noise_cov import NOISE_MISSING, noise_of_observations


def _obs(noise=True):
    rng = np.random.RandomState(0)
    im = rng.normal(size=(17, 17))
    jac = ngmix.DiagonalJacobian(row=8.0, col=8.0, scale=0.263)
    return ngmix.Observation(im, weight=np.ones_like(im), jacobian=jac,
                             noise=rng.normal(size=im.shape) if noise else None)


def test_go_many_missing_noise_image_raises():
    """Fitter(use_noise_image=True).go_many needs ob.noise everywhere: the
    per-object route's ValueError, before any launch"""
    objs = [_obs(), _obs(noise=False)]
    fitter = ngmix.fitting.Fitter(model="exp", use_noise_image=True)
    with pytest.raises(ValueError, match=NOISE_MISSING):
        fitter.go_many(objs, np.tile([0.0, 0.0, 0.0, 0.0, 0.5, 10.0], (2, 1)))


def test_noise_of_observations_order():
    """flatten_observations' stamp order: objects, then bands, then epochs"""
    a, b, c = _obs(), _obs(), _obs()
    b.noise = b.noise + 1.0
    c.noise = c.noise + 2.0
    ol = ngmix.ObsList()
    ol.append(b)
    ol.append(c)
    mb = ngmix.MultiBandObsList()
    mb.append(ol)
    out = noise_of_observations([a, mb])
    assert len(out) == 3
    for got, ob in zip(out, (a, b, c)):
        np.testing.assert_array_equal(got, ob.noise)
    with pytest.raises(ValueError, match=NOISE_MISSING):
        noise_of_observations([a, _obs(noise=False)])


def test_lm_batch_fitter_noise_image_not_for_coellip():
    from ngmix_amd.lm_batch import LMBatchFitter
    with pytest.raises(ValueError):
        LMBatchFitter("coellip", ngauss=2, use_noise_image=True)
