"""
The sheared pre-psf moments on the device (DESIGN.md 3.21;
csrc/prepsf_shear.hip through PrePSFMom.measure_arrays_sheared and
metacal.metacal_moments_batch / _many) against the dense longdouble reference
of tests/helpers/prepsf_shear_reference.py, under the bound its float64
restatement sets (TWIN_TOL = 4 x the float64 gap, relative to each sum's
largest term); against measure_arrays at g = 0 (1e-10 of each quantity's scale,
the figure test_gpu_prepsfmom.py holds measure_arrays to); and for what must
hold to the bit: the two layouts of g, batches cut in two, repeated calls, the
neighbours of flagged stamps, the response computed by hand.
"""
import numpy as np
import pytest

from ngmix_amd import flags as ngflags
from ngmix_amd import metacal, prepsfmom
from ngmix_amd.batch import StampBatch
from ngmix_amd.jacobian import Jacobian
from ngmix_amd.observation import Observation
from helpers import prepsf_shear_reference as ps

pytestmark = pytest.mark.gpu

CASES = [(d, p, n, k, a) for (d, p, n) in ps.SHAPES for k in ps.KINDS for a in ps.AP_RADS]
ROWS_OF_70 = (0, 1, 69)


def sums14(mom, cov):
    out = [mom[..., 2 + a] for a in range(4)]
    out += [cov[..., 2 + a, 2 + b] for a in range(4) for b in range(a, 4)]
    return np.stack(out, axis=-1)


def run(c, m, g, sel=slice(None)):
    mom, cov, fl, kernels, D = m.measure_arrays_sheared(
        c["images"][sel], c["weights"][sel], c["cen"][sel], ps.DERIV, c["psfs"][sel],
        c["pcen"][sel], g)
    return sums14(mom, cov), fl


@pytest.mark.parametrize("dim,pdim,n,kind,ap_rad", CASES)
def test_kernel_against_longdouble(dim, pdim, n, kind, ap_rad):
    rows_of = ROWS_OF_70 if n == 70 else None
    ref = ps.reference(dim, pdim, n, kind, ap_rad, rows_of=rows_of)
    c = ps.case(dim, pdim, n)
    m = ps.measure_of(kind, dim, ap_rad)
    idx = list(rows_of or range(n))
    for name, g in (("types", ps.type_shears()), ("galshear", c["shears"][:, None, :])):
        sums, fl = run(c, m, g)
        assert not fl.any() and np.all(np.isfinite(sums))
        sub = {k: v[idx] for k, v in ref[name].items()}
        gap = ps.gap(sums[idx], sub)
        print("%s dim %d/%d %s ap %.1f: kernel gap %.3g (allowed %.3g)"
              % (name, dim, pdim, kind, ap_rad, gap, ps.TWIN_TOL))
        assert gap <= ps.TWIN_TOL


@pytest.mark.parametrize("dim,pdim,n,kind,ap_rad", CASES)
def test_zero_shear_is_measure_arrays(dim, pdim, n, kind, ap_rad):
    c = ps.case(dim, pdim, n)
    m = ps.measure_of(kind, dim, ap_rad)
    mom, cov, fl, _, D = m.measure_arrays_sheared(c["images"], c["weights"], c["cen"], ps.DERIV,
                                                  c["psfs"], c["pcen"], np.zeros((1, 2)))
    wmom, wcov, _, wD = m.measure_arrays(c["images"], c["weights"], c["cen"], ps.DERIV, c["psfs"],
                                         c["pcen"])
    assert D == wD and not fl.any()
    for i in range(n):
        for got, want in ((mom[i, 0, 2:], wmom[i, 2:]), (cov[i, 0, 2:, 2:], wcov[i, 2:, 2:])):
            assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    assert np.all(np.isnan(mom[:, 0, :2])) and np.all(cov[:, 0, 0, 0] == 1)


def test_bits_do_not_depend_on_layout_batch_or_run():
    dim, pdim, n = ps.SHAPES[0]
    c = ps.case(dim, pdim, n)
    for kind in ps.KINDS:
        m = ps.measure_of(kind, dim, 1.5)
        whole, fl = run(c, m, ps.type_shears())
        again, _ = run(c, m, ps.type_shears())
        assert np.array_equal(whole, again)
        tiled, _ = run(c, m, np.tile(ps.type_shears(), (n, 1, 1)))
        assert np.array_equal(whole, tiled)
        a, _ = run(c, m, ps.type_shears(), slice(0, 35))
        b, _ = run(c, m, ps.type_shears(), slice(35, 70))
        assert np.array_equal(np.concatenate([a, b]), whole)
        back, _ = run(c, m, ps.type_shears(), slice(None, None, -1))
        assert np.array_equal(back[::-1], whole)


def test_flagged_stamps_are_nan_and_leave_their_neighbours_alone():
    dim, pdim, n = ps.SHAPES[1]
    c = ps.case(dim, pdim, n)
    m = ps.measure_of("pgauss", dim, 1.5)
    _, D, rows, cols, wgt, fk = ps.plan_of(m, dim, pdim)
    g = c["shears"][:, None, :].copy()
    clean, fl = run(c, m, g)
    assert not fl.any()
    g[0, 0] = 0.6, 0.0                       # leaves the band
    bad = dict(c, psfs=c["psfs"].copy())
    bad["psfs"][2] = 0.0                     # through the amplitude floor: 0 / 0
    sums, fl = run(bad, m, g)
    assert fl[:, 0].tolist() == [ngflags.METACAL_BAND_LIMIT, 0, ngflags.METACAL_BAND_LIMIT]
    assert np.all(np.isnan(sums[[0, 2]])) and np.array_equal(sums[1], clean[1])
    for i in (0, 2):
        ref, rfl, _ = ps.sheared_sums(bad["images"][i], bad["weights"][i], bad["cen"][i], ps.DERIV,
                                      bad["psfs"][i], bad["pcen"][i], g[i, 0], rows, cols, wgt,
                                      fk, D, 1.5)
        assert rfl == 1 and np.all(np.isnan(ref))
    # a kernel that reaches the Nyquist row is out of the band under |g| = 0.3
    scale = np.sqrt(abs(ps.DERIV[0] * ps.DERIV[3] - ps.DERIV[1] * ps.DERIV[2]))
    wide = ps.measure_of("pgauss", dim, 1.5, fwhm=3.6 * scale)
    sums, fl = run(c, wide, np.array([[0.3 * np.cos(0.4), 0.3 * np.sin(0.4)]]))
    assert np.all(fl == ngflags.METACAL_BAND_LIMIT) and np.all(np.isnan(sums))
    # go_metacal_batch: NaN rows, the flag in both columns
    res = m.go_metacal_batch(bad["images"], bad["weights"], bad["cen"], ps.DERIV, bad["psfs"],
                             bad["pcen"])
    for t in ps.TYPES:
        assert res[t]["mcal_flags"].tolist() == [0, 0, ngflags.METACAL_BAND_LIMIT]
        assert res[t]["flags"][2] & ngflags.METACAL_BAND_LIMIT and res[t]["flags"][1] == 0
        assert np.all(np.isnan(res[t]["e"][2])) and np.isnan(res[t]["flux"][2])


def _jacs(cen):
    n = cen.shape[0]
    det = ps.DERIV[0] * ps.DERIV[3] - ps.DERIV[1] * ps.DERIV[2]
    out = np.zeros((n, 8))
    out[:, 0:2] = cen
    out[:, 2:6] = ps.DERIV
    out[:, 6], out[:, 7] = det, np.sqrt(abs(det))
    return out


def test_metacal_moments_batch_response_is_the_one_computed_by_hand():
    dim, pdim, n = ps.SHAPES[0]
    c = ps.case(dim, pdim, n)
    m = ps.measure_of("pgauss", dim, 1.5)
    sb = StampBatch.from_images(c["images"], c["weights"], _jacs(c["cen"]))
    psb = StampBatch.from_images(c["psfs"], None, _jacs(c["pcen"]))
    res = metacal.metacal_moments_batch(sb, psb, m, step=ps.STEP)
    assert list(res) == list(ps.TYPES)
    resp = metacal.shear_response(res, step=ps.STEP, key="e")
    gamma = metacal.mean_shear(resp)
    assert not resp["flags"].any()
    assert np.all(np.isfinite(resp["R"])) and np.all(np.isfinite(gamma))
    # by hand, from the arrays (the weights are 16 where positive: ierr^2 is exact)
    w = np.where(c["weights"] > 0, c["weights"], 0.0)
    mom, cov, fl, _, _ = m.measure_arrays_sheared(c["images"], w, c["cen"], ps.DERIV, c["psfs"],
                                                  c["pcen"], ps.type_shears())
    e = mom[:, :, 2:4] / mom[:, :, 4:5]
    R = np.stack([(e[:, 1] - e[:, 2]) / (2 * ps.STEP), (e[:, 3] - e[:, 4]) / (2 * ps.STEP)], axis=2)
    assert np.array_equal(resp["g"], e[:, 0]) and np.array_equal(resp["R"], R)
    assert np.array_equal(gamma, np.linalg.solve(R.mean(axis=0), e[:, 0].mean(axis=0)))
    for i, t in enumerate(ps.TYPES):
        assert np.array_equal(res[t]["sums"][:, 2:], mom[:, i, 2:])
        assert np.array_equal(res[t]["mcal_flags"], fl[:, i])
    # what it checks of its inputs
    with pytest.raises(ValueError, match="one psf stamp"):
        metacal.metacal_moments_batch(sb, psb.select(np.arange(3)), m)
    other = _jacs(c["pcen"])
    other[5, 2] *= 1.01
    with pytest.raises(ValueError, match="derivatives"):
        metacal.metacal_moments_batch(sb, StampBatch.from_images(c["psfs"], None, other), m)


def test_metacal_moments_many_is_the_batch_row_by_row():
    m = ps.measure_of("ksigma", 17, 1.5)
    obs, rows = [], []
    for dim, pdim, n in (ps.SHAPES[1], (16, 16, 4)):
        c = ps.case(dim, pdim, n)
        c["weights"] = np.where(c["weights"] > 0, c["weights"], 0.0)
        res = ps.measure_of("ksigma", 17, 1.5).go_metacal_batch(
            c["images"], c["weights"], c["cen"], ps.DERIV, c["psfs"], c["pcen"], step=ps.STEP)
        for i in range(n):
            def jac(cen):
                return Jacobian(row=cen[0], col=cen[1], dvdrow=ps.DERIV[0], dvdcol=ps.DERIV[1],
                                dudrow=ps.DERIV[2], dudcol=ps.DERIV[3])
            psf = Observation(c["psfs"][i], jacobian=jac(c["pcen"][i]))
            obs.append(Observation(c["images"][i], weight=c["weights"][i], jacobian=jac(c["cen"][i]),
                                   psf=psf))
            rows.append((res, i))
    order = [4, 0, 5, 1, 6, 2, 3]            # the two shapes interleaved
    many = metacal.metacal_moments_many([obs[k] for k in order], m, step=ps.STEP)
    assert len(many) == len(order)
    for got, k in zip(many, order):
        res, i = rows[k]
        assert list(got) == list(ps.TYPES)
        for t in ps.TYPES:
            for key in ("sums", "sums_cov", "flux", "T", "e"):
                assert np.array_equal(got[t][key], res[t][key][i], equal_nan=True), (t, key)
            assert got[t]["flags"] == res[t]["flags"][i]
            assert got[t]["mcal_flags"] == res[t]["mcal_flags"][i] == 0


def test_gap_to_the_image_route_is_reported():
    """metacal images (truncated to the stamp, reconvolved), then measure_arrays
    on them with its second taper: a finding, printed, not a bound"""
    dim, pdim, n = ps.SHAPES[2][0], ps.SHAPES[2][1], 8
    c = ps.case(dim, pdim, n)
    m = ps.measure_of("pgauss", dim, 1.5)
    sb = StampBatch.from_images(c["images"], np.where(c["weights"] > 0, c["weights"], 0.0),
                                _jacs(c["cen"]))
    psb = StampBatch.from_images(c["psfs"], None, _jacs(c["pcen"]))
    res = metacal.metacal_moments_batch(sb, psb, m, step=ps.STEP)
    both = metacal.MetacalBatch(sb, psb, rng=np.random.RandomState(3)).get_all(
        step=ps.STEP, fixnoise=False)
    worst = 0.0
    for t in ps.TYPES:
        d = both[t]
        pjac = d["psf_stamps"].jac[:, 0:2].cpu().numpy()
        mom, _, _, _ = m.measure_arrays(
            d["stamps"].val.reshape(n, dim, dim), np.full((n, dim, dim), 16.0), c["cen"], ps.DERIV,
            d["psf_stamps"].val.reshape(n, pdim, pdim), pjac)
        e2 = mom[:, 2:4] / mom[:, 4:5]
        gap = np.nanmax(np.abs(e2 - res[t]["e"]))
        fgap = np.nanmax(np.abs(mom[:, 5] / res[t]["sums"][:, 5] - 1))
        worst = max(worst, gap)
        print("%s: image route against sheared modes: |delta e| <= %.3g, |delta flux| / flux <= %.3g"
              % (t, gap, fgap))
    assert np.isfinite(worst)
