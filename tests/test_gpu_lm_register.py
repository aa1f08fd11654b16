"""
The register instantiation of the lmder step (csrc/lm_core.hpp's one text under
lm_core_reg.hpp's fixed_dim<N>: what fits of 6-8 parameters run) against the
run-time instantiation of the same text (lm_advance_kernel<14, false>), both on
the device in one process: the STATE RECORDS are compared after every lock-step
round, byte for byte over their live part -- one full wave plus a one-lane
tail, lmder with eager and lazy jacobians, forward differences, bounds with
prior rows, poor guesses (rejected steps, several lmpar iterations).
"""
import numpy as np
import pytest

from ngmix_amd import _lib
from ngmix_amd.lm_batch import LMBatchFitter

from test_gpu_lm_team import _assert_same_rounds, _census_has, _multiband, _rounds

pytestmark = pytest.mark.gpu

NOBJ = 65   # WAVE + 1


def _bounded_prior(nband):
    from ngmix_amd import prior_batch as pb
    return pb.PriorSimpleSepBatch(
        pb.GaussianCen(0.0, 0.0, 0.3, 0.3), pb.GPriorBA(0.3),
        pb.Normal(0.6, 0.5, bounds=[0.05, 4.0]),
        [pb.Normal(120.0, 200.0, bounds=[1.0, None])] +
        [pb.TwoSidedErf(-1.0e3, 1.0, 1.0e5, 10.0)] * (nband - 1))


@pytest.mark.parametrize("nband", [1, 2, 3])
@pytest.mark.parametrize("case", ["lmder_eager", "lmder_lazy_bounds", "lmdif"])
def test_register_step_equals_generic_step_on_the_device(nband, case, monkeypatch):
    """'exp' over 1 / 2 / 3 bands: lm_advance_kernel<6 / 7 / 8, true> against
    lm_advance_kernel<14, false>, 65 fits"""
    monkeypatch.delenv("NGMIX_LM_TEAM_MIN", raising=False)
    monkeypatch.delenv("NGMIX_LM_GENERIC", raising=False)
    n = 5 + nband
    rng = np.random.RandomState(700 + 10 * nband + len(case))
    sb, psf, guess, sobj, sband = _multiband(NOBJ, nband, "exp", rng)
    guess[::4, 4:] *= 1.6                      # poor guesses: rejected steps, lmpar iterations
    guess[::6, 2:4] = 0.4, -0.3
    guess[NOBJ - 1, 4] *= 2.5                  # the tail lane's fit too
    bounded = case == "lmder_lazy_bounds"
    prior = _bounded_prior(nband) if bounded else None

    def make():
        f = LMBatchFitter("exp", prior=prior, analytic_jacobian=case != "lmdif")
        f.lazy_jacobian = case == "lmder_lazy_bounds"
        return f

    def go(f):
        return f.go(sb, guess, psf=psf, stamp_obj=sobj, stamp_band=sband)
    _lib.launch_census(reset=True)
    rr, sr = _rounds(make(), go, True)
    seen = _lib.launch_census(reset=True)
    assert _census_has(seen, "lm_advance_kernel<%d, true>" % n), seen
    assert not _census_has(seen, "lm_advance_kernel<14, false>") and not _census_has(seen, "team")
    rg, sg = _rounds(make(), go, False)
    seen = _lib.launch_census(reset=True)
    assert _census_has(seen, "lm_advance_kernel<14, false>"), seen
    assert not _census_has(seen, "lm_advance_kernel<%d," % n) and not _census_has(seen, "team"), seen
    _assert_same_rounds(sr, sg)
    assert np.all(sr[-1]["bounded"] == int(bounded))
    assert np.all(sr[-1]["mode"] == {"lmder_eager": 0, "lmdif": 1, "lmder_lazy_bounds": 2}[case])
    for k in ("flags", "nfev", "njev", "ier", "pars", "pars_cov", "lnprob"):
        np.testing.assert_array_equal(rr[k], rg[k], err_msg=k)
    # the fits did something: most converge, and not all in the same number of
    # evaluations (the poor guesses take rejected steps)
    assert np.mean(rr["flags"] == 0) > 0.7
    assert rr["nfev"].max() > rr["nfev"].min()
