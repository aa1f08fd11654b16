"""
The sheared pre-psf moments without a GPU: the dense
longdouble reference (tests/helpers/prepsf_shear_reference.py) against itself
in float64, at g = 0 and against analytic gaussian moments, and the host twin
ngmix_prepsf_shear_sums_host -- the kernel's per-mode code in the kernel's
summation order -- against the reference, with its refusals and flags.  No
kernel is launched here.

The gaussian kernels are built with the fast exponential in numpy
(helpers.host_fexp): the package evaluates it on the device.  The kernels are
inputs of the reference and of the twin alike.
"""
import numpy as np
import pytest

from ngmix_amd import _lib, flags, metacal, prepsfmom
from helpers import prepsf_shear_reference as ps

CASES = [(d, p, n, k, a) for (d, p, n) in ps.SHAPES for k in ps.KINDS for a in ps.AP_RADS]
# of the 70 stamps the dense reference is taken at three; the twin runs all
ROWS_OF_70 = (0, 1, 69)


@pytest.fixture(autouse=True, scope="module")
def host_kernels():
    """gaussian kernels from the numpy fast exponential while this module runs;
    nothing built with it is left behind"""
    saved = prepsfmom._fexp
    prepsfmom._KERNELS.clear()
    ps._CACHE.clear()
    prepsfmom._fexp = ps.host_fexp
    yield
    prepsfmom._fexp = saved
    prepsfmom._KERNELS.clear()
    ps._CACHE.clear()


def rows_of(n):
    return ROWS_OF_70 if n == 70 else None


def picked(ref, n):
    idx = list(rows_of(n) or range(n))
    return idx, {k: v[idx] for k, v in ref.items()}


def twin(dim, pdim, n, kind, ap_rad, g):
    c = ps.case(dim, pdim, n)
    _, D, rows, cols, wgt, fk = ps.plan_of(ps.measure_of(kind, dim, ap_rad), dim, pdim)
    st, sums, fl = ps.call_host(_lib.lib(), _lib.ptr, c, g, rows, cols, wgt, fk, D, ap_rad)
    assert st == _lib.OK, _lib.last_error()
    return sums, fl


def test_host_fexp_is_the_fast_exponential():
    x = -np.linspace(0.0, 12.49, 500)
    assert np.abs(ps.host_fexp(x) / np.exp(x) - 1).max() < 5e-6


@pytest.mark.parametrize("dim,pdim,n,kind,ap_rad", CASES)
def test_float64_against_longdouble(dim, pdim, n, kind, ap_rad):
    ref = ps.reference(dim, pdim, n, kind, ap_rad, rows_of=rows_of(n))
    f64 = ps.reference(dim, pdim, n, kind, ap_rad, dtype=np.float64, rows_of=rows_of(n))
    for name in ("types", "galshear"):
        idx, sub = picked(ref[name], n)
        assert not sub["flags"].any()
        gap = ps.gap(f64[name]["sums"][idx], sub)
        print("%s dim %d/%d %s ap %.1f: float64 gap %.3g (recorded %.3g)"
              % (name, dim, pdim, kind, ap_rad, gap, ps.F64_VS_LONGDOUBLE))
        assert gap <= ps.F64_VS_LONGDOUBLE


@pytest.mark.parametrize("dim,pdim,n,kind,ap_rad", CASES)
def test_host_twin_against_longdouble(dim, pdim, n, kind, ap_rad):
    ref = ps.reference(dim, pdim, n, kind, ap_rad, rows_of=rows_of(n))
    c = ps.case(dim, pdim, n)
    for name, g in (("types", ps.type_shears()), ("galshear", c["shears"][:, None, :])):
        sums, fl = twin(dim, pdim, n, kind, ap_rad, g)
        assert not fl.any() and np.all(np.isfinite(sums))
        idx, sub = picked(ref[name], n)
        gap = ps.gap(sums[idx], sub)
        print("%s dim %d/%d %s ap %.1f: host twin gap %.3g (allowed %.3g)"
              % (name, dim, pdim, kind, ap_rad, gap, ps.TWIN_TOL))
        assert gap <= ps.TWIN_TOL


@pytest.mark.parametrize("dtype", [np.longdouble, np.float64])
def test_reference_at_zero_shear_is_its_unsheared_form_to_the_bit(dtype):
    for dim, pdim, n in ps.SHAPES[1:]:
        c = ps.case(dim, pdim, n)
        for kind in ps.KINDS:
            _, D, rows, cols, wgt, fk = ps.plan_of(ps.measure_of(kind, dim, 1.5), dim, pdim)
            args = (c["images"][0], c["weights"][0], c["cen"][0], ps.DERIV, c["psfs"][0],
                    c["pcen"][0])
            a, fa, _ = ps.sheared_sums(*args, (0.0, 0.0), rows, cols, wgt, fk, D, 1.5, dtype)
            b, fb, _ = ps.unsheared_sums(*args, rows, cols, wgt, fk, D, 1.5, dtype)
            assert fa == fb == 0
            # (not tobytes(): the padding of an 80-bit longdouble is not part of its value)
            assert np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def test_twin_at_zero_shear_does_not_see_the_shear_map():
    """k' = k exactly at g = 0: whatever J is, the twin's noshear sums are
    those of a run whose other types differ"""
    a, _ = twin(17, 11, 3, "ksigma", 1.5, ps.type_shears())
    b, _ = twin(17, 11, 3, "ksigma", 1.5, np.array([[0.0, 0.0], [0.2, -0.1]]))
    assert np.array_equal(a[:, 0], b[:, 0])


def test_response_of_a_round_gaussian_is_the_analytic_one():
    image, weight, psf = ps.physics_case()
    m = prepsfmom.PGaussMom(ps.PHYS_FWHM)
    _, D, rows, cols, wgt, fk = ps.plan_of(m, ps.PHYS_DIM, ps.PHYS_DIM)
    e = []
    for g in ps.type_shears():
        s, fl, _ = ps.sheared_sums(image, weight, ps.PHYS_CEN, ps.DERIV, psf, ps.PHYS_PCEN, g,
                                   rows, cols, wgt, fk, D, m.ap_rad)
        assert fl == 0
        e.append([float(s[0] / s[2]), float(s[1] / s[2])])
    got = ps.response(e)
    want = ps.response([ps.analytic_pgauss_e(g) for g in ps.type_shears()])
    gap = np.abs(got - want).max()
    print("R reference\n%s\nR analytic\n%s\nlargest difference %.4g (measured %.4g, allowed %.4g)"
          % (got, want, gap, ps.PHYS_MEASURED, ps.PHYSICS_BOUND))
    assert abs(want[0, 0] - 1) < 0.1 and want[0, 1] == 0     # a response of order one
    assert gap <= ps.PHYSICS_BOUND


def test_a_stamp_does_not_depend_on_its_batch():
    dim, pdim, n = 17, 11, 3
    c = ps.case(dim, pdim, n)
    _, D, rows, cols, wgt, fk = ps.plan_of(ps.measure_of("pgauss", dim, 1.5), dim, pdim)
    L = _lib.lib()
    g = c["shears"][:, None, :]
    _, whole, _ = ps.call_host(L, _lib.ptr, c, g, rows, cols, wgt, fk, D, 1.5)
    for i in (2, 0, 1):
        one = {k: v[i:i + 1] for k, v in c.items()}
        _, s, _ = ps.call_host(L, _lib.ptr, one, g[i:i + 1], rows, cols, wgt, fk, D, 1.5)
        assert np.array_equal(s[0], whole[i])
    # (T, 2) and (N, T, 2) with equal rows
    _, a, _ = ps.call_host(L, _lib.ptr, c, ps.type_shears(), rows, cols, wgt, fk, D, 1.5)
    _, b, _ = ps.call_host(L, _lib.ptr, c, np.tile(ps.type_shears(), (n, 1, 1)), rows, cols, wgt,
                           fk, D, 1.5)
    assert np.array_equal(a, b)


def test_band_limit_and_zero_psf_are_flagged_nan():
    dim, pdim, n = 16, 16, 3
    c = ps.case(dim, pdim, n)
    L = _lib.lib()
    scale = np.sqrt(abs(ps.DERIV[0] * ps.DERIV[3] - ps.DERIV[1] * ps.DERIV[2]))
    # a kernel that reaches the Nyquist row: every mode is kept, none doubled
    m = ps.measure_of("pgauss", dim, 1.5, fwhm=3.6 * scale)
    _, D, rows, cols, wgt, fk = ps.plan_of(m, dim, pdim)
    assert np.all(wgt == 1) and (rows == D // 2).any()
    g = np.array([[0.3 * np.cos(0.4), 0.3 * np.sin(0.4)]])
    st, sums, fl = ps.call_host(L, _lib.ptr, c, g, rows, cols, wgt, fk, D, 1.5)
    assert st == _lib.OK and np.all(fl == 1) and np.all(np.isnan(sums))
    ref, rfl, _ = ps.sheared_sums(c["images"][0], c["weights"][0], c["cen"][0], ps.DERIV,
                                  c["psfs"][0], c["pcen"][0], g[0], rows, cols, wgt, fk, D, 1.5)
    assert rfl == 1 and np.all(np.isnan(ref))
    # one stamp of a batch leaves the band (|g| = 0.6), one has a psf of zeros:
    # both NaN and flagged as the reference has them, the third to the bit
    m = ps.measure_of("pgauss", dim, 1.5)
    _, D, rows, cols, wgt, fk = ps.plan_of(m, dim, pdim)
    g = np.zeros((n, 1, 2))
    g[:, 0] = c["shears"]
    _, clean, _ = ps.call_host(L, _lib.ptr, c, g, rows, cols, wgt, fk, D, 1.5)
    g[0, 0] = 0.6, 0.0
    bad = dict(c, psfs=c["psfs"].copy())
    bad["psfs"][2] = 0.0
    st, sums, fl = ps.call_host(L, _lib.ptr, bad, g, rows, cols, wgt, fk, D, 1.5)
    assert st == _lib.OK and fl[:, 0].tolist() == [1, 0, 1]
    assert np.all(np.isnan(sums[[0, 2]])) and np.array_equal(sums[1], clean[1])
    for i in (0, 2):
        ref, rfl, _ = ps.sheared_sums(bad["images"][i], bad["weights"][i], bad["cen"][i], ps.DERIV,
                                      bad["psfs"][i], bad["pcen"][i], g[i, 0], rows, cols, wgt,
                                      fk, D, 1.5)
        assert rfl == 1 and np.all(np.isnan(ref))


def test_refusals():
    dim, pdim, n = 17, 11, 3
    c = ps.case(dim, pdim, n)
    _, D, rows, cols, wgt, fk = ps.plan_of(ps.measure_of("ksigma", dim, 1.5), dim, pdim)
    L = _lib.lib()
    g = ps.type_shears()
    for host in (True, False):      # the device entry refuses the same calls before a launch
        def call(**over):
            return ps.call_host(L, _lib.ptr, c, over.pop("g", g), rows, cols, wgt, fk, D, 1.5,
                                host=host, **over)
        for name in ("images", "weights", "psf", "cen", "psf_cen", "g_host", "mrow", "mcol",
                     "wgt", "fk", "sums", "flags"):
            assert call(**{name: None})[0] == _lib.ERR_BAD_ARG, name
            assert "required" in _lib.last_error()
        for name in ("ntypes", "nmodes", "dim", "pdim", "fft_dim"):
            for v in (0, -3):
                assert call(**{name: v})[0] == _lib.ERR_BAD_ARG, name
        assert call(n=-1)[0] == _lib.ERR_BAD_ARG
        for gbad in ([1.0, 0.0], [0.8, 0.7], [np.nan, 0.0]):
            gb = g.copy()
            gb[3] = gbad
            assert call(g=gb)[0] == _lib.ERR_BAD_ARG
            assert "unit circle" in _lib.last_error()
        assert call(deriv=(0.2, 0.1, 0.4, 0.2))[0] == _lib.ERR_BAD_ARG       # det = 0
        assert call(dim=120, pdim=100)[0] == _lib.ERR_BAD_ARG
        assert "LDS" in _lib.last_error()
        assert call(n=1 << 30, ntypes=5)[0] == _lib.ERR_BAD_ARG
        assert "one launch" in _lib.last_error()
        # refused calls write nothing
        st, sums, fl = call(dim=0)
        assert np.all(sums == -7.0) and np.all(fl == -7)
        # nothing to do: no pointer is read
        st, _, _ = call(n=0, images=None, weights=None, psf=None, cen=None, psf_cen=None, sums=None,
                        flags=None, mrow=None, mcol=None, wgt=None, fk=None)
        assert st == _lib.OK
    # without a taper
    st, sums, fl = ps.call_host(L, _lib.ptr, c, g, rows, cols, wgt, fk, D, 0.0)
    assert st == _lib.OK and not fl.any()


def test_what_is_not_served_says_so():
    m = prepsfmom.PGaussMom(1.2)
    z = np.zeros((2, 16, 16))
    cen = np.full((2, 2), 7.5)
    deriv = (0.263, 0.0, 0.0, 0.263)
    g = ps.type_shears()
    with pytest.raises(NotImplementedError, match="no_psf"):
        m.measure_arrays_sheared(z, z + 1, cen, deriv, None, None, g)
    noisy = prepsfmom.PGaussMom(1.2, use_noise_image=True)
    with pytest.raises(NotImplementedError, match="use_noise_image"):
        noisy.measure_arrays_sheared(z, z + 1, cen, deriv, z, cen, g)
    with pytest.raises(NotImplementedError, match="fixnoise"):
        m.go_metacal_batch(z, z + 1, cen, deriv, z, cen, fixnoise=True)
    with pytest.raises(NotImplementedError, match="fixnoise"):
        metacal.metacal_moments_batch(None, None, m, fixnoise=True)
    with pytest.raises(NotImplementedError, match="fixnoise"):
        metacal.metacal_moments_many([], m, fixnoise=True)
    for call in (lambda: m.go_metacal_batch(z, z + 1, cen, deriv, z, cen, types=["1p_psf"]),
                 lambda: metacal.metacal_moments_batch(None, None, m, types=["noshear", "1m_psf"]),
                 lambda: metacal.metacal_moments_many([], m, types=["2p_psf"])):
        with pytest.raises(NotImplementedError, match="psf"):
            call()
    with pytest.raises(ValueError, match="unit circle"):
        m.measure_arrays_sheared(z, z + 1, cen, deriv, z, cen, np.array([[0.8, 0.7]]))
    with pytest.raises(ValueError):
        metacal.metacal_moments_batch(None, None, object())
    assert metacal.metacal_moments_many([], m) == []


def test_the_flag_bit_is_new_and_named():
    bit = flags.METACAL_BAND_LIMIT
    assert metacal.METACAL_BAND_LIMIT == bit and bit & (bit - 1) == 0
    others = [v for k, v in vars(flags).items() if k.isupper() and isinstance(v, int)
              and k != "METACAL_BAND_LIMIT"]
    assert bit not in others and bit > max(others)
    assert bit not in (metacal.METACAL_PSF_FIT_FAILURE, metacal.METACAL_NONFINITE)
    assert flags.NONPOS_FLUX == 4 and flags.ZERO_DOF == 1 << 15           # nothing renumbered
    assert "band limit" in flags.get_flags_str(bit | flags.NONPOS_FLUX)


def test_empty_batch_needs_no_device():
    m = prepsfmom.KSigmaMom(1.2)
    z = np.zeros((0, 16, 16))
    mom, cov, fl, kernels, D = m.measure_arrays_sheared(
        z, z, np.zeros((0, 2)), (0.263, 0.0, 0.0, 0.263), z, np.zeros((0, 2)), ps.type_shears())
    assert mom.shape == (0, 5, 6) and cov.shape == (0, 5, 6, 6) and fl.shape == (0, 5) and D == 64
