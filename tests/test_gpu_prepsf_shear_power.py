"""
The covariance of the sheared pre-psf moments from a noise image on the device
(prepsf_shear_sums_kernel<NOISE, true> through
PrePSFMom(use_noise_image=True).measure_arrays_sheared(noise_images=),
go_metacal_batch and metacal.metacal_moments_many) against the dense longdouble
reference of tests/helpers/prepsf_shear_power_reference.py under its counted bound;
against the host twins; at g = 0 against measure_arrays on the device; and what
must hold to the bit: the moment sums beside the forms without the noise image,
the two layouts of g, a NaN's isolation, the catalogue route against
go_metacal_batch(noise_images=) (metacal_moments_batch takes a StampBatch, which
holds no noise images, and keeps its parameters).
"""
import numpy as np
import pytest

from ngmix_amd import _lib, metacal, prepsfmom
from ngmix_amd.batch import StampBatch
from ngmix_amd.jacobian import Jacobian
from ngmix_amd.observation import Observation
from helpers import prepsf_shear_power_reference as pw

pytestmark = pytest.mark.gpu

CASES = [(d, p, n, k, a) for (d, p, n) in pw.SHAPES for k in pw.KINDS for a in (0.0, 1.5)]
SEED = 0x5EEDF00D1234


def sums14(mom, cov):
    out = [mom[..., 2 + a] for a in range(4)]
    out += [cov[..., 2 + a, 2 + b] for a in range(4) for b in range(a, 4)]
    return np.stack(out, axis=-1)


def measure(kind, dim, ap_rad, power=True):
    return prepsfmom.PrePSFMom(pw.measure_of(kind, dim, ap_rad).fwhm, kind, ap_rad=ap_rad,
                               use_noise_image=power)


def run(c, m, g, power, noise=None):
    mom, cov, fl, _, _ = m.measure_arrays_sheared(
        c["images"], c["weights"], c["cen"], pw.DERIV, c["psfs"], c["pcen"], g, noise=noise,
        noise_images=power)
    return sums14(mom, cov), fl


def inputs(dim, pdim, n):
    return pw.case(dim, pdim, n), pw.power_planes(dim, pdim, n), pw.noise_planes(dim, pdim, n)


@pytest.mark.parametrize("fixnoise", [False, True])
@pytest.mark.parametrize("dim,pdim,n,kind,ap_rad", CASES)
def test_kernel_against_longdouble(dim, pdim, n, kind, ap_rad, fixnoise):
    ref = pw.reference(dim, pdim, n, kind, ap_rad, fixnoise)
    c, power, field = inputs(dim, pdim, n)
    m = measure(kind, dim, ap_rad)
    bound = pw.c_round(dim, pdim)
    for name, g in (("types", pw.type_shears()), ("galshear", c["shears"][:, None, :])):
        sums, fl = run(c, m, g, power, field if fixnoise else None)
        assert not fl.any() and np.all(np.isfinite(sums))
        ratio = pw.worst_ratio(sums[..., 4:], ref[name])
        print("%s dim %d/%d %s ap %.1f fixnoise %d: kernel %.4g units (bound %.0f)"
              % (name, dim, pdim, kind, ap_rad, fixnoise, ratio, bound))
        assert ratio <= bound


@pytest.mark.parametrize("dim,pdim,n", pw.SHAPES[::2])
def test_kernel_against_host_twins(dim, pdim, n):
    """the twin runs the kernel's text in the kernel's order and differs from it
    through sincos and hypot alone: the covariance sums under the bound of
    either, the moment sums under that of the forms without the noise image"""
    from helpers import prepsf_shear_noise_reference as pn
    c, power, field = inputs(dim, pdim, n)
    for kind in pw.KINDS:
        m = measure(kind, dim, 1.5)
        _, D, rows, cols, wgt, fk = pw.plan_of(m, dim, pdim)
        for fixnoise in (False, True):
            ref = pw.reference(dim, pdim, n, kind, 1.5, fixnoise)
            mref = pn.reference(dim, pdim, n, kind, 1.5) if fixnoise else None
            for name, g in (("types", pw.type_shears()), ("galshear", c["shears"][:, None, :])):
                sums, fl = run(c, m, g, power, field if fixnoise else None)
                st, twin, tfl = pw.call_host(_lib.lib(), _lib.ptr, c, power,
                                             pw.turned(field) if fixnoise else None, g, rows, cols,
                                             wgt, fk, D, 1.5)
                assert st == _lib.OK and not fl.any() and not tfl.any()
                gap = float(np.max(np.abs(sums[..., 4:] - twin[..., 4:]) /
                                   (pw.EPS * ref[name]["absum"].astype(np.float64))))
                print("%s dim %d/%d %s fixnoise %d: kernel against twin %.4g units"
                      % (name, dim, pdim, kind, fixnoise, gap))
                assert gap <= pw.c_round(dim, pdim)
                if mref is not None:
                    scale = mref[name]["scale"][..., :4].astype(np.float64)
                    assert np.all(np.abs(sums[..., :4] - twin[..., :4]) <= 2 * pn.TWIN_TOL * scale)


@pytest.mark.parametrize("dim,pdim,n,kind,ap_rad", CASES[::2] + CASES[1::4])
def test_g0_is_measure_arrays_on_the_device(dim, pdim, n, kind, ap_rad):
    """at g = 0 the covariance sums are those of measure_arrays(..., noise_images)
    with use_noise_image=True -- the reference's -- under the bound"""
    c, power, _ = inputs(dim, pdim, n)
    m = measure(kind, dim, ap_rad)
    _, cov, _, _ = m.measure_arrays(c["images"], c["weights"], c["cen"], pw.DERIV, c["psfs"],
                                    c["pcen"], power)
    want = sums14(np.zeros((n, 6)), cov)[:, 4:]
    sums, fl = run(c, m, np.zeros((1, 2)), power)
    ref = pw.reference(dim, pdim, n, kind, ap_rad, False)["types"]
    assert not fl.any()
    gap = float(np.max(np.abs(sums[:, 0, 4:] - want) /
                       (pw.EPS * ref["absum"][:, 0].astype(np.float64))))
    print("g = 0 dim %d/%d %s ap %.1f: kernel against measure_arrays %.4g units (bound %.0f)"
          % (dim, pdim, kind, ap_rad, gap, pw.c_round(dim, pdim)))
    assert gap <= pw.c_round(dim, pdim)


@pytest.mark.parametrize("dim,pdim,n", pw.SHAPES)
def test_moment_sums_are_those_without_the_noise_image(dim, pdim, n):
    c, power, field = inputs(dim, pdim, n)
    g = pw.type_shears()
    for kind in pw.KINDS:
        m, m0 = measure(kind, dim, 1.5), measure(kind, dim, 1.5, power=False)
        for noise in (None, field, metacal.DeviceNoise(SEED, np.arange(n) + 40)):
            a, fl = run(c, m, g, power, noise)
            b, fl0 = run(c, m0, g, None, noise)
            assert not fl.any() and not fl0.any()
            assert np.array_equal(a[..., :4], b[..., :4])
            assert not np.any(a[..., 4:] == b[..., 4:])
            tiled, _ = run(c, m, np.tile(g, (n, 1, 1)), power, noise)
            assert np.array_equal(tiled, a)


def test_nan_in_a_noise_image_flags_its_own_stamp():
    dim, pdim, n = pw.SHAPES[2]
    c, power, field = inputs(dim, pdim, n)
    m = measure("pgauss", dim, 1.5)
    for noise in (None, field):
        clean, fl = run(c, m, pw.type_shears(), power, noise)
        bad = power.copy()
        bad[1, 3, 4] = np.nan
        sums, fl = run(c, m, pw.type_shears(), bad, noise)
        assert (fl != 0).tolist() == [[False] * 5, [True] * 5, [False] * 5]
        assert np.all(fl[1] == metacal.METACAL_BAND_LIMIT)
        assert np.all(np.isnan(sums[1])) and np.array_equal(sums[[0, 2]], clean[[0, 2]])


def _jacs(cen):
    det = pw.DERIV[0] * pw.DERIV[3] - pw.DERIV[1] * pw.DERIV[2]
    out = np.zeros((cen.shape[0], 8))
    out[:, 0:2] = cen
    out[:, 2:6] = pw.DERIV
    out[:, 6], out[:, 7] = det, np.sqrt(abs(det))
    return out


def test_many_objects_are_the_batch_row_by_row():
    m = prepsfmom.PGaussMom(pw.measure_of("pgauss", 16, 1.5).fwhm, use_noise_image=True)
    white = prepsfmom.PGaussMom(m.fwhm)
    obs, want = [], []
    for dim, pdim, n in ((16, 9, 2), (12, 12, 2)):
        c, power, _ = inputs(dim, pdim, n)
        c["weights"] = np.where(c["weights"] > 0, c["weights"], 0.0)
        res = m.go_metacal_batch(c["images"], c["weights"], c["cen"], pw.DERIV, c["psfs"],
                                 c["pcen"], step=pw.STEP, noise_images=power)
        for i in range(n):
            def jac(cen):
                return Jacobian(row=cen[0], col=cen[1], dvdrow=pw.DERIV[0], dvdcol=pw.DERIV[1],
                                dudrow=pw.DERIV[2], dudcol=pw.DERIV[3])
            psf = Observation(c["psfs"][i], jacobian=jac(c["pcen"][i]))
            obs.append(Observation(c["images"][i], weight=c["weights"][i], noise=power[i],
                                   jacobian=jac(c["cen"][i]), psf=psf))
            want.append((res, i))
    order = [2, 0, 3, 1]                     # the two shapes interleaved
    many = metacal.metacal_moments_many([obs[k] for k in order], m, step=pw.STEP)
    plain = metacal.metacal_moments_many([obs[k] for k in order], white, step=pw.STEP)
    for got, old, k in zip(many, plain, order):
        res, i = want[k]
        for t in pw.TYPES:
            for key in ("sums", "sums_cov", "flux", "flux_err", "T", "T_err", "e", "e_err", "s2n"):
                assert np.array_equal(got[t][key], res[t][key][i], equal_nan=True), (t, key)
            assert got[t]["flags"] == res[t]["flags"][i]
            assert got[t]["mcal_flags"] == res[t]["mcal_flags"][i] == 0
            assert np.array_equal(got[t]["sums"], old[t]["sums"], equal_nan=True)
            assert np.all(got[t]["e_err"] != old[t]["e_err"])
    # one plane as the fixnoise field and as the power estimate
    both = metacal.metacal_moments_many([obs[k] for k in order], m, step=pw.STEP, fixnoise=True,
                                        use_noise_image=True)
    field = metacal.metacal_moments_many([obs[k] for k in order], white, step=pw.STEP,
                                         fixnoise=True, use_noise_image=True)
    for a, b in zip(both, field):
        assert np.array_equal(a["1p"]["sums"], b["1p"]["sums"], equal_nan=True)
        assert np.all(a["1p"]["e_err"] != b["1p"]["e_err"])
    # shear_response takes the batch result as it is
    c, power, _ = inputs(16, 9, 3)
    w = np.where(c["weights"] > 0, c["weights"], 0.0)
    res = m.go_metacal_batch(c["images"], w, c["cen"], pw.DERIV, c["psfs"], c["pcen"],
                             step=pw.STEP, noise_images=power)
    resp = metacal.shear_response(res, step=pw.STEP, key="e")
    assert not resp["flags"].any() and np.all(np.isfinite(resp["R"]))
    # a StampBatch holds no noise images: metacal_moments_batch says what is missing
    sb = StampBatch.from_images(c["images"], w, _jacs(c["cen"]))
    psb = StampBatch.from_images(c["psfs"], None, _jacs(c["pcen"]))
    with pytest.raises(ValueError, match="obs.noise must be set"):
        metacal.metacal_moments_batch(sb, psb, m, step=pw.STEP)
