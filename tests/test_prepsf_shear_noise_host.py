"""
The fixnoise term of the sheared pre-psf moments without a
GPU: the dense longdouble reference (tests/helpers/prepsf_shear_noise_reference.py)
against itself in float64, the host twin ngmix_prepsf_shear_fixnoise_sums_host
-- the kernel's per-mode code in the kernel's summation order -- against the
reference, the turning identity (which does not use the restatement), its
refusals and flags, and the rules of the Python keywords.  No kernel is
launched here.

The gaussian kernels are built with the fast exponential in numpy
(helpers.host_fexp), as in test_prepsf_shear_host.py.
"""
import numpy as np
import pytest

from ngmix_amd import _lib, metacal, prepsfmom
from helpers import prepsf_shear_reference as ps
from helpers import prepsf_shear_noise_reference as pn

CASES = [(d, p, n, k, a) for (d, p, n) in pn.SHAPES for k in pn.KINDS for a in pn.AP_RADS]
# of the 70 stamps the dense reference is taken at three; the twin runs all
ROWS_OF_70 = (0, 1, 69)


@pytest.fixture(autouse=True, scope="module")
def host_kernels():
    """gaussian kernels from the numpy fast exponential while this module runs;
    nothing built with it is left behind"""
    saved = prepsfmom._fexp
    prepsfmom._KERNELS.clear()
    ps._CACHE.clear()
    pn._CACHE.clear()
    prepsfmom._fexp = ps.host_fexp
    yield
    prepsfmom._fexp = saved
    prepsfmom._KERNELS.clear()
    ps._CACHE.clear()
    pn._CACHE.clear()


def rows_of(n):
    return ROWS_OF_70 if n == 70 else None


def picked(ref, n):
    idx = list(rows_of(n) or range(n))
    return idx, {k: v[idx] for k, v in ref.items()}


def setup_of(dim, pdim, n, kind, ap_rad):
    c = pn.case(dim, pdim, n)
    _, D, rows, cols, wgt, fk = pn.plan_of(pn.measure_of(kind, dim, ap_rad), dim, pdim)
    return c, pn.turned(pn.noise_planes(dim, pdim, n)), (rows, cols, wgt, fk, D, ap_rad)


def twin(dim, pdim, n, kind, ap_rad, g):
    c, nt, plan = setup_of(dim, pdim, n, kind, ap_rad)
    st, sums, fl = pn.call_host(_lib.lib(), _lib.ptr, c, nt, g, *plan)
    assert st == _lib.OK, _lib.last_error()
    return sums, fl


@pytest.mark.parametrize("dim,pdim,n,kind,ap_rad", CASES)
def test_float64_against_longdouble(dim, pdim, n, kind, ap_rad):
    ref = pn.reference(dim, pdim, n, kind, ap_rad, rows_of=rows_of(n))
    f64 = pn.reference(dim, pdim, n, kind, ap_rad, dtype=np.float64, rows_of=rows_of(n))
    for name in ("types", "galshear"):
        idx, sub = picked(ref[name], n)
        assert not sub["flags"].any()
        gap = pn.gap(f64[name]["sums"][idx], sub)
        print("%s dim %d/%d %s ap %.1f: float64 gap %.4g (recorded %.3g)"
              % (name, dim, pdim, kind, ap_rad, gap, pn.F64_VS_LONGDOUBLE))
        assert gap <= pn.F64_VS_LONGDOUBLE


@pytest.mark.parametrize("dim,pdim,n,kind,ap_rad", CASES)
def test_host_twin_against_longdouble(dim, pdim, n, kind, ap_rad):
    ref = pn.reference(dim, pdim, n, kind, ap_rad, rows_of=rows_of(n))
    c = pn.case(dim, pdim, n)
    for name, g in (("types", pn.type_shears()), ("galshear", c["shears"][:, None, :])):
        sums, fl = twin(dim, pdim, n, kind, ap_rad, g)
        assert not fl.any() and np.all(np.isfinite(sums))
        idx, sub = picked(ref[name], n)
        gap = pn.gap(sums[idx], sub)
        print("%s dim %d/%d %s ap %.1f: host twin gap %.4g (allowed %.3g)"
              % (name, dim, pdim, kind, ap_rad, gap, pn.TWIN_TOL))
        assert gap <= pn.TWIN_TOL


def test_the_noise_term_is_not_small():
    """the reference's sums move by many times the bound when the plane goes
    in: the comparisons above see the term"""
    dim, pdim, n = pn.SHAPES[1]
    with_noise = pn.reference(dim, pdim, n, "pgauss", 1.5)["types"]
    without = ps.reference(dim, pdim, n, "pgauss", 1.5)["types"]
    moved = np.abs(with_noise["sums"][..., :4] - without["sums"][..., :4]) / with_noise["scale"][..., :4]
    assert float(moved.max()) > 1e4 * pn.TWIN_TOL


@pytest.mark.parametrize("kind", pn.KINDS)
def test_zero_noise_plane_leaves_the_moments_and_doubles_the_variance_terms(kind):
    """moment sums to the bit those of ngmix_prepsf_shear_sums_host; covariance
    sums as step 5 has them"""
    dim, pdim, n = pn.SHAPES[2]
    c, nt, plan = setup_of(dim, pdim, n, kind, 1.5)
    rows, cols, wgt, fk, D, ap = plan
    L = _lib.lib()
    for g in (pn.type_shears(), c["shears"][:, None, :]):
        _, plain, pfl = ps.call_host(L, _lib.ptr, c, g, *plan)
        st, sums, fl = pn.call_host(L, _lib.ptr, c, np.zeros_like(nt), g, *plan)
        assert st == _lib.OK and not fl.any() and not pfl.any()
        assert np.array_equal(sums[..., :4], plain[..., :4])
        for i in range(n):
            for t in range(g.shape[-2]):
                gt = g[t] if g.ndim == 2 else g[i, t]
                ref, rfl, scale, _ = pn.fixnoise_sums(
                    c["images"][i], c["weights"][i], np.zeros((dim, dim)), c["cen"][i], pn.DERIV,
                    c["psfs"][i], c["pcen"][i], gt, rows, cols, wgt, fk, D, ap)
                assert rfl == 0
                assert np.all(np.abs(sums[i, t, 4:] - ref[4:]) <= pn.TWIN_TOL * scale[4:])
                assert np.all(sums[i, t, [4, 8, 11, 13]] > plain[i, t, [4, 8, 11, 13]])


def test_turning_identity():
    """conformal J with a flip, a psf stamp symmetric under rot90, centres at
    the stamps' own: the noise term of N at g (the new entry minus the existing
    one) is the image term of N at -g (the existing entry); so with image = N
    the moment sums of 1p and 1m agree, and those of 2p and 2m"""
    L = _lib.lib()
    for dim, pdim, n in ((16, 16, 2), (17, 11, 2)):
        c, planes, deriv = pn.turning_case(dim, pdim, n)
        for kind in pn.KINDS:
            m = pn.measure_of(kind, dim, 1.5)
            _, D, rows, cols, wgt, fk = pn.plan_of(m, dim, pdim, deriv=deriv)
            plan = (rows, cols, wgt, fk, D, 1.5)
            g = np.concatenate([pn.type_shears(), [[0.21, -0.17]]])
            st, both, fl = pn.call_host(L, _lib.ptr, c, pn.turned(planes), g, *plan, deriv=deriv)
            assert st == _lib.OK and not fl.any()
            _, image_term, fl1 = ps.call_host(L, _lib.ptr, c, g, *plan, deriv=deriv)
            _, mirrored, fl2 = ps.call_host(L, _lib.ptr, c, -g, *plan, deriv=deriv)
            assert not fl1.any() and not fl2.any()
            noise_term = both[..., :4] - image_term[..., :4]
            worst = 0.0
            for i in range(n):
                for t in range(g.shape[0]):
                    _, rfl, scale, _ = pn.fixnoise_sums(
                        planes[i], c["weights"][i], planes[i], c["cen"][i], deriv, c["psfs"][i],
                        c["pcen"][i], g[t], rows, cols, wgt, fk, D, 1.5)
                    assert rfl == 0
                    scale = scale[:4].astype(np.float64)
                    assert np.all(np.abs(image_term[i, t, :4]) > 0)
                    d = np.abs(noise_term[i, t] - mirrored[i, t, :4]) / scale
                    worst = max(worst, float(d.max()))
                    assert np.all(d <= 2 * pn.TWIN_TOL)
                    if t in (1, 3):      # 1p against 1m, 2p against 2m
                        d = np.abs(both[i, t, :4] - both[i, t + 1, :4]) / scale
                        worst = max(worst, float(d.max()))
                        assert np.all(d <= 2 * pn.TWIN_TOL)
            print("turning identity dim %d/%d %s: largest gap %.3g (allowed %.3g)"
                  % (dim, pdim, kind, worst, 2 * pn.TWIN_TOL))


def test_a_stamp_does_not_depend_on_its_batch():
    dim, pdim, n = 17, 11, 3
    c, nt, plan = setup_of(dim, pdim, n, "pgauss", 1.5)
    L = _lib.lib()
    g = c["shears"][:, None, :]
    _, whole, _ = pn.call_host(L, _lib.ptr, c, nt, g, *plan)
    for i in (2, 0, 1):
        one = {k: v[i:i + 1] for k, v in c.items()}
        _, s, _ = pn.call_host(L, _lib.ptr, one, nt[i:i + 1], g[i:i + 1], *plan)
        assert np.array_equal(s[0], whole[i])
    _, a, _ = pn.call_host(L, _lib.ptr, c, nt, pn.type_shears(), *plan)
    _, b, _ = pn.call_host(L, _lib.ptr, c, nt, np.tile(pn.type_shears(), (n, 1, 1)), *plan)
    assert np.array_equal(a, b)


def test_a_nan_noise_pixel_flags_only_its_own_stamp():
    dim, pdim, n = 17, 11, 3
    c, nt, plan = setup_of(dim, pdim, n, "ksigma", 1.5)
    L = _lib.lib()
    _, clean, _ = pn.call_host(L, _lib.ptr, c, nt, pn.type_shears(), *plan)
    bad = nt.copy()
    bad[1, 0, 0] = np.nan          # a corner the taper holds at zero: still not finite
    bad[2, 8, 9] = np.inf
    st, sums, fl = pn.call_host(L, _lib.ptr, c, bad, pn.type_shears(), *plan)
    assert st == _lib.OK and fl.tolist() == [[0] * 5, [1] * 5, [1] * 5]
    assert np.all(np.isnan(sums[1:])) and np.array_equal(sums[0], clean[0])


def test_band_limit_through_the_turned_frequency():
    """a kept mode whose k' stays inside the band while q' leaves it: the plain
    entry measures the stamp, the fixnoise entry flags it, as the reference does"""
    dim, pdim, n = 16, 16, 2
    c = pn.case(dim, pdim, n)
    nt = pn.turned(pn.noise_planes(dim, pdim, n))
    D = 64
    # one mode on the row axis, just inside the band; its turned partner lies on
    # the column axis.  g1 > 0 stretches one axis and shrinks the other
    rows, cols = np.array([D // 2 - 1, 0]), np.array([0, 3])
    wgt, fk = np.ones(2), np.ones((4, 2))
    L = _lib.lib()
    found = 0
    for g in ([0.1, 0.0], [-0.1, 0.0]):
        g = np.array([g])
        _, plain, pfl = ps.call_host(L, _lib.ptr, c, g, rows, cols, wgt, fk, D, 1.5)
        st, sums, fl = pn.call_host(L, _lib.ptr, c, nt, g, rows, cols, wgt, fk, D, 1.5)
        ref, rfl, _, _ = pn.fixnoise_sums(
            c["images"][0], c["weights"][0], pn.noise_planes(dim, pdim, n)[0], c["cen"][0],
            pn.DERIV, c["psfs"][0], c["pcen"][0], g[0], rows, cols, wgt, fk, D, 1.5)
        assert st == _lib.OK and np.all(fl == rfl)
        if rfl and not pfl.any():
            found += 1
            assert np.all(np.isnan(sums)) and np.all(np.isfinite(plain))
    assert found == 1


def test_refusals():
    dim, pdim, n = 17, 11, 3
    c, nt, plan = setup_of(dim, pdim, n, "ksigma", 1.5)
    L = _lib.lib()
    g = pn.type_shears()
    for host in (True, False):      # the device entry refuses the same calls before a launch
        def call(**over):
            return pn.call_host(L, _lib.ptr, c, over.pop("noise", nt), over.pop("g", g), *plan,
                                host=host, **over)
        for name in ("images", "weights", "psf", "noise_turned", "cen", "psf_cen", "g_host",
                     "mrow", "mcol", "wgt", "fk", "sums", "flags"):
            assert call(**{name: None})[0] == _lib.ERR_BAD_ARG, name
            assert "required" in _lib.last_error()
        assert call(noise_turned=None)[0] == _lib.ERR_BAD_ARG
        assert "noise_turned" in _lib.last_error()
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
        # 100^2 + 100^2 doubles fit the 160 KB; with a second plane of 100^2 they do not
        assert call(dim=100, pdim=100)[0] == _lib.ERR_BAD_ARG
        assert "LDS" in _lib.last_error() and "noise" in _lib.last_error()
        assert call(n=1 << 30, ntypes=5)[0] == _lib.ERR_BAD_ARG
        assert "one launch" in _lib.last_error()
        # refused calls write nothing
        for over in (dict(dim=0), dict(noise_turned=None), dict(dim=100, pdim=100)):
            st, sums, fl = call(**over)
            assert st == _lib.ERR_BAD_ARG and np.all(sums == -7.0) and np.all(fl == -7)
        # nothing to do: no pointer is read
        st, _, _ = call(n=0, images=None, weights=None, psf=None, noise_turned=None, cen=None,
                        psf_cen=None, sums=None, flags=None, mrow=None, mcol=None, wgt=None,
                        fk=None)
        assert st == _lib.OK
    # the existing entry still takes 100 / 100 (checked before its launch: the g is bad)
    gb = g.copy()
    gb[0] = 1.0, 0.0
    st, _, _ = ps.call_host(L, _lib.ptr, c, gb, *plan, host=False, dim=100, pdim=100)
    assert st == _lib.ERR_BAD_ARG and "unit circle" in _lib.last_error()
    # without a taper
    st, sums, fl = pn.call_host(L, _lib.ptr, c, nt, g, *plan[:-1], 0.0)
    assert st == _lib.OK and not fl.any()


def test_the_entries_are_declared_with_one_more_argument():
    sig = _lib.SIGNATURES
    plain = sig["ngmix_prepsf_shear_sums_batch"][1]
    assert len(plain) == 26 and len(sig["ngmix_prepsf_shear_sums_host"][1]) == 25
    assert sig["ngmix_prepsf_shear_fixnoise_sums_batch"][1] == plain[:3] + [plain[0]] + plain[3:]
    assert sig["ngmix_prepsf_shear_fixnoise_sums_host"][1] == \
        sig["ngmix_prepsf_shear_fixnoise_sums_batch"][1][:-1]


def test_python_argument_rules():
    m = prepsfmom.PGaussMom(1.2)
    z = np.zeros((2, 16, 16))
    cen = np.full((2, 2), 7.5)
    deriv = (0.263, 0.0, 0.0, 0.263)
    # fixnoise=True with no noise source: not served, said before anything else is looked at
    for call in (lambda: m.go_metacal_batch(z, z + 1, cen, deriv, z, cen, fixnoise=True),
                 lambda: m.go_metacal_batch(None, None, None, None, None, None, types=["bad"],
                                            fixnoise=True),
                 lambda: metacal.metacal_moments_batch(None, None, object(), fixnoise=True),
                 lambda: metacal.metacal_moments_many([], object(), types=["bad"], fixnoise=True)):
        with pytest.raises(NotImplementedError, match="fixnoise"):
            call()
    # a noise source with fixnoise=False, or two of them
    for kw in (dict(noise=z), dict(noise_seed=3), dict(noise=metacal.DeviceNoise(3)),
               dict(fixnoise=True, noise=z, noise_seed=3),
               dict(fixnoise=True, noise=z, ids=np.arange(2))):
        with pytest.raises(ValueError):
            m.go_metacal_batch(z, z + 1, cen, deriv, z, cen, **kw)
        with pytest.raises(ValueError):
            metacal.metacal_moments_batch(None, None, m, **kw)
    for kw in (dict(noise_seed=3), dict(use_noise_image=True),
               dict(fixnoise=True, noise_seed=3, use_noise_image=True),
               dict(fixnoise=True, use_noise_image=True, ids=[])):
        with pytest.raises(ValueError):
            metacal.metacal_moments_many([], m, **kw)
    # with a source the other checks come next, and an empty catalogue is empty
    with pytest.raises(ValueError):
        metacal.metacal_moments_batch(None, None, object(), fixnoise=True, noise_seed=3)
    with pytest.raises(NotImplementedError, match="psf"):
        metacal.metacal_moments_batch(None, None, m, types=["1p_psf"], fixnoise=True, noise_seed=3)
    assert metacal.metacal_moments_many([], m, fixnoise=True, noise_seed=3) == []
    assert metacal.metacal_moments_many([], m, fixnoise=True, use_noise_image=True) == []
    # the new keywords come last and default to today's behaviour
    import inspect
    names = list(inspect.signature(metacal.metacal_moments_batch).parameters)
    assert names == ["stamps", "psf_stamps", "measure", "step", "types", "fixnoise", "noise",
                     "noise_seed", "ids"]
    names = list(inspect.signature(metacal.metacal_moments_many).parameters)
    assert names == ["list_of_obs", "measure", "step", "types", "fixnoise", "noise_seed", "ids",
                     "use_noise_image"]
    names = list(inspect.signature(m.go_metacal_batch).parameters)
    assert names[:13] == ["images", "weights", "cen", "deriv", "psf_images", "psf_cen", "step",
                          "types", "fixnoise", "noise", "noise_seed", "ids", "noise_ierr"]
    assert list(inspect.signature(m.measure_arrays_sheared).parameters)[6:8] == ["g", "noise"]


def test_empty_batch_with_noise_needs_no_device():
    m = prepsfmom.KSigmaMom(1.2)
    z = np.zeros((0, 16, 16))
    mom, cov, fl, kernels, D = m.measure_arrays_sheared(
        z, z, np.zeros((0, 2)), (0.263, 0.0, 0.0, 0.263), z, np.zeros((0, 2)), pn.type_shears(),
        noise=z)
    assert mom.shape == (0, 5, 6) and cov.shape == (0, 5, 6, 6) and fl.shape == (0, 5) and D == 64
