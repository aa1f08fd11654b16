"""
The dense reference of psf='dilate-exact' (tests/helpers/
metacal_dilate_reference.py) held to what can be known without it: the identity
at g = 0, d = 1, the closed form for gaussians, the keep rule, and its own
longdouble form.  No GPU.
"""
import numpy as np
import pytest

from helpers import metacal_dilate_reference as D
from helpers import metacal_reference as M


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("shape,psf_shape", [((16, 16), (16, 16)), ((12, 17), (11, 11)),
                                             ((15, 15), (12, 9))])
@pytest.mark.parametrize("kind", [D.IMAGE, D.PSF])
def test_identity_at_zero_shear_and_unit_dilation(shape, psf_shape, kind):
    """step 6 of the definition: at g = 0, d = 1 the image and the psf come back
    as they went in, minus the Nyquist row and column of their transforms --
    for ANY image and psf, here random ones"""
    rng = np.random.RandomState(shape[0] + 100 * psf_shape[1])
    image = rng.normal(size=shape)
    psf = rng.uniform(0.5, 1.5, size=psf_shape)         # (no zero of its transform in the band)
    psf[psf_shape[0] // 2, psf_shape[1] // 2] += 40.0
    jac = M.jac_record((shape[0] - 1) / 2 + 0.3, (shape[1] - 1) / 2 - 0.4, *M._DERIVS[1])
    pcen = ((psf_shape[0] - 1) / 2 - 0.2, (psf_shape[1] - 1) / 2 + 0.1)
    out, flag = D.metacal_image(image, psf, jac, pcen, (0.0, 0.0), 1.0, kind)
    pout, pflag = D.target_psf_image(psf, jac, pcen, (0.0, 0.0), 1.0, kind)
    assert flag == 0 and pflag == 0
    err, perr = _rel(out, D.drop_nyquist(image)), _rel(pout, D.drop_nyquist(psf))
    print("identity %s %s %s: image %.3g, psf %.3g of the peak" % (shape, psf_shape, kind, err, perr))
    # rounding alone: a sum of n terms is off by at most n eps of its largest
    # partial sum; three such transforms and the inverse one meet in a mode
    bound = 4 * max(shape[0] * shape[1], psf_shape[0] * psf_shape[1]) * np.finfo(np.float64).eps
    assert err <= bound and perr <= bound


def test_closed_form_for_gaussians():
    """O^(q) of point-sampled gaussians (psf sigma = 2 px, object wider, 64 x 64)
    against G^_obj+psf(k') / G^_psf(k') G^_psf(k_t) Pi(q) / Pi(q_t) on the modes
    with max(|q_r|, |q_c|) <= 2, relative to the largest |O^|: both kinds, the
    four jacobians of device_case, five shears.  Measured: CLOSED_FORM_MEASURED;
    the bound is eight times that (aliasing there is below 1e-12; a figure above
    1e-8 would mean that the reference is wrong)"""
    worst = 0.0
    for deriv in M._DERIVS:
        image, psf, jac, pcen, ocov, pcov = D.closed_form_case(deriv)
        for g in D.CLOSED_FORM_SHEARS:
            for kind in (D.IMAGE, D.PSF):
                _, dil, _ = D.shear_spec(g, kind)
                got, kept = D.spectrum(image, psf, jac, pcen, g, dil, kind)
                want, low = D.closed_form_spectrum(jac, ocov, pcov, g, dil, kind)
                assert low.sum() == 41 * 41
                # (at |g| = 0.01 every such mode is kept; at (0.2, -0.1), d = 1.45, the
                # target frequency of some leaves the band: those are zero by the
                # keep rule and the closed form does not speak of them)
                if abs(g[0]) + abs(g[1]) <= 0.01:
                    assert kept[low].all()
                assert kept[low].sum() >= 25 * 25 and np.all(got[low & ~kept] == 0)
                low &= kept
                err = float(np.abs(got - want)[low].max() / np.abs(want).max())
                print("closed form: deriv %s g %s %s: %.3g of the largest mode"
                      % (deriv, g, kind, err))
                worst = max(worst, err)
    print("closed form: largest deviation %.3g of the largest mode (bound %.3g)"
          % (worst, 8 * D.CLOSED_FORM_MEASURED))
    assert worst <= 8 * D.CLOSED_FORM_MEASURED
    assert 8 * D.CLOSED_FORM_MEASURED < 1e-8


@pytest.mark.parametrize("shape,per_axis", [((12, 17), (7, 11)), ((20, 20), (13, 13))])
def test_modes_whose_target_frequency_leaves_the_band_are_zero(shape, per_axis):
    """d = 1.6 at g = 0: a mode is kept where 1.6 |q| < pi on both axes -- fft
    numbers |k| < n / 3.2 -- and every other mode is exactly zero"""
    rng = np.random.RandomState(3)
    image = rng.normal(size=shape)
    psf = M.gaussian_stamp((11, 11), M.jac_record(5.2, 4.9, *M._DERIVS[0]), 0.12 * np.eye(2), 1.0)
    jac = M.jac_record((shape[0] - 1) / 2, (shape[1] - 1) / 2, *M._DERIVS[0])
    for kind in (D.IMAGE, D.PSF):
        spec, kept = D.spectrum(image, psf, jac, (5.2, 4.9), (0.0, 0.0), 1.6, kind)
        assert kept.sum() == per_axis[0] * per_axis[1]
        k = [np.abs(np.fft.fftfreq(n) * n) for n in shape]
        want = (k[0][:, None] < shape[0] / 3.2) & (k[1][None, :] < shape[1] / 3.2)
        assert np.array_equal(kept, want)
        assert np.all(spec[~kept] == 0) and np.all(spec[kept] != 0)
    # the psf's own spectrum: the same rule on the psf stamp's grid (11: |k| < 3.44)
    pspec, pkept = D.psf_spectrum(psf, jac, (5.2, 4.9), (0.0, 0.0), 1.6, D.IMAGE)
    assert pkept.sum() == 7 * 7 and np.all(pspec[~pkept] == 0)
    # a shear moves the band of the psf kind's target, not of its image frequency
    _, k0 = D.spectrum(image, psf, jac, (5.2, 4.9), (0.0, 0.0), 1.1, D.PSF)
    _, k1 = D.spectrum(image, psf, jac, (5.2, 4.9), (0.2, 0.1), 1.1, D.PSF)
    assert (k0 != k1).any()


def test_zero_psf_is_flagged_and_nan():
    case = D.device_case((16, 16), (16, 16), 1)
    args = (case["psfs"][0] * 0, case["jacs"][0], case["pjacs"][0][0:2], (0.01, 0.0), 1.02)
    for kind in (D.IMAGE, D.PSF):
        out, flag = D.metacal_image(case["images"][0], *args, kind)
        assert flag == 1 and np.all(np.isnan(out))


def test_type_and_shear_specs():
    assert D.type_spec("noshear", 0.01) == ((0.0, 0.0), 1.02, D.IMAGE)
    assert D.type_spec("2m", 0.01) == ((0.0, -0.01), 1.02, D.IMAGE)
    assert D.type_spec("1m_psf", 0.02) == ((-0.02, 0.0), 1.04, D.PSF)
    g, d, kind = D.shear_spec((0.3, -0.4), D.PSF)
    assert g == (0.3, -0.4) and d == pytest.approx(2.0) and kind == D.PSF
    assert len(D.TYPES) == 9 and D.TYPES[:5] == M.TYPES


def test_float64_against_longdouble():
    """the float64 form against the longdouble one over the device tests'
    stamps, relative to each stamp's peak: held to D.F64_VS_LONGDOUBLE"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("np.longdouble is no wider than float64 here")
    worst = 0.0
    for shape, psf_shape, n in D.DEVICE_SHAPES:
        ld = D.device_reference(shape, psf_shape, n)
        f8 = D.device_reference(shape, psf_shape, n, dtype=np.float64)
        for name in ld:
            for key in ("images", "psf_images", "fixnoise_images"):
                if ld[name][key] is None:
                    continue
                for a, b in zip(f8[name][key], ld[name][key]):
                    assert np.all(np.isfinite(a))
                    worst = max(worst, float(np.abs(a - b.astype(np.float64)).max()
                                             / np.abs(b).max()))
    print("float64 against longdouble: largest deviation %.3g of a stamp's peak" % worst)
    assert worst <= D.F64_VS_LONGDOUBLE
