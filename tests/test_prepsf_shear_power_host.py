"""
The covariance of the sheared pre-psf moments from a noise image (DESIGN.md
3.28; use_noise_image=True on the metacal route) without a GPU: the host twins
ngmix_prepsf_shear_power_sums_host and ngmix_prepsf_shear_fixnoise_power_sums_host
-- the kernel's per-mode code in the kernel's summation order -- against the
dense longdouble reference of tests/helpers/prepsf_shear_power_reference.py
under its counted bound; at g = 0 against the unsheared measurement's own
stages; the turning identity; the moment sums to the bit; the statistics the
feature exists for; and the refusals.  No kernel is launched here.

The gaussian kernels are built with the fast exponential in numpy
(helpers.host_fexp), as in test_prepsf_shear_host.py.
"""
import numpy as np
import pytest

from ngmix_amd import _lib, metacal, prepsfmom
from helpers import prepsf_shear_reference as ps
from helpers import prepsf_shear_noise_reference as pn
from helpers import prepsf_shear_power_reference as pw

CASES = [(d, p, n, k, a) for (d, p, n) in pw.SHAPES for k in pw.KINDS for a in (0.0, 1.5)]


@pytest.fixture(autouse=True, scope="module")
def host_kernels():
    """gaussian kernels from the numpy fast exponential while this module runs;
    nothing built with it is left behind"""
    saved = prepsfmom._fexp
    prepsfmom._KERNELS.clear()
    prepsfmom._fexp = ps.host_fexp
    yield
    prepsfmom._fexp = saved
    prepsfmom._KERNELS.clear()
    pw._CACHE.clear()


def setup_of(dim, pdim, n, kind, ap_rad):
    c = pw.case(dim, pdim, n)
    _, D, rows, cols, wgt, fk = pw.plan_of(pw.measure_of(kind, dim, ap_rad), dim, pdim)
    return (c, pw.power_planes(dim, pdim, n), pw.turned(pw.noise_planes(dim, pdim, n)),
            (rows, cols, wgt, fk, D, ap_rad))


def twin(dim, pdim, n, kind, ap_rad, g, fixnoise, **kw):
    c, power, nt, plan = setup_of(dim, pdim, n, kind, ap_rad)
    st, sums, fl = pw.call_host(_lib.lib(), _lib.ptr, c, power, nt if fixnoise else None, g, *plan,
                                **kw)
    assert st == _lib.OK, _lib.last_error()
    return sums, fl


@pytest.mark.parametrize("fixnoise", [False, True])
@pytest.mark.parametrize("dim,pdim,n,kind,ap_rad", CASES)
def test_host_twins_against_longdouble(dim, pdim, n, kind, ap_rad, fixnoise):
    ref = pw.reference(dim, pdim, n, kind, ap_rad, fixnoise)
    c = pw.case(dim, pdim, n)
    bound = pw.c_round(dim, pdim)
    for name, g in (("types", pw.type_shears()), ("galshear", c["shears"][:, None, :])):
        sums, fl = twin(dim, pdim, n, kind, ap_rad, g, fixnoise)
        assert not ref[name]["flags"].any() and not fl.any() and np.all(np.isfinite(sums))
        ratio = pw.worst_ratio(sums[..., 4:], ref[name])
        print("%s dim %d/%d %s ap %.1f fixnoise %d: host twin %.4g units (bound %.0f)"
              % (name, dim, pdim, kind, ap_rad, fixnoise, ratio, bound))
        assert ratio <= bound


def test_the_noise_image_is_seen():
    """the covariance sums move by many times the bound between the weight map's
    white level and the plane's power, and between two planes"""
    dim, pdim, n = pw.SHAPES[2]
    c, power, nt, plan = setup_of(dim, pdim, n, "pgauss", 1.5)
    ref = pw.reference(dim, pdim, n, "pgauss", 1.5, False)["types"]
    L = _lib.lib()
    _, white, _ = pw.call_host(L, _lib.ptr, c, None, None, pw.type_shears(), *plan, base=True)
    _, a, _ = pw.call_host(L, _lib.ptr, c, power, None, pw.type_shears(), *plan)
    _, b, _ = pw.call_host(L, _lib.ptr, c, power[::-1], None, pw.type_shears(), *plan)
    tol = pw.c_round(dim, pdim) * pw.EPS * ref["absum"].astype(np.float64)
    assert np.all(np.abs(a[..., 4:] - white[..., 4:]) > 1e3 * tol)
    assert np.all(np.abs(a[[0, 2]][..., 4:] - b[[0, 2]][..., 4:]) > 1e3 * tol[[0, 2]])


def _unsheared_power_cov(m, c, power, dim, pdim):
    """the ten covariance sums of PrePSFMom.measure_arrays(..., noise_images)
    with use_noise_image=True, from that method's own stages run on the host:
    _transform_at_modes of the stamps, psf stamps and noise images and the
    (stamp, mode) sums in their torch form (_sums_torch, the check of
    ngmix_prepsf_sums_batch) -- measure_arrays itself needs a device (the GPU
    suite makes this comparison with it)"""
    import torch
    n = c["images"].shape[0]
    D = int(max(dim, pdim) * m.pad_factor)
    kernels = prepsfmom._kernels(m.kind, D, float(m.fwhm), pw.DERIV, float(m.fwhm_smooth))
    plan = prepsfmom._mode_plan(kernels, "cpu")
    nc = plan["ucols"].size

    def modes(t):
        at = (torch.arange(n) * nc)[:, None] + torch.from_numpy(
            plan["irow"].astype(np.int64) * (n * nc) + plan["icol"].astype(np.int64))[None, :]
        return t.reshape(-1)[at]
    kim = prepsfmom._transform_at_modes(c["images"], D, m.ap_rad, kernels, "cpu")
    kpsf = prepsfmom._transform_at_modes(c["psfs"], D, 0, kernels, "cpu")
    kn = prepsfmom._transform_at_modes(power, D, 0, kernels, "cpu")
    max_amp = torch.from_numpy(np.abs(c["psfs"].reshape(n, -1).sum(axis=1)))
    fk = torch.from_numpy(np.stack([kernels[k][plan["keep"]] for k in ("fkp", "fkc", "fkr", "fkf")]))
    df2 = (1 / D) ** 2
    sums = prepsfmom._sums_torch(
        modes(kim[0]), modes(kim[1]), modes(kpsf[0]), modes(kpsf[1]), None, modes(kn[0]),
        modes(kn[1]), None, (D / dim) ** 2, max_amp, None, None, torch.from_numpy(plan["irow"]),
        torch.from_numpy(plan["icol"]), fk, torch.from_numpy(plan["wgt"]), df2, df2 * df2)
    return sums.numpy()[:, 4:]


@pytest.mark.parametrize("dim,pdim,n,kind,ap_rad", CASES[::2] + CASES[1::4])
def test_g0_is_the_unsheared_measurement(dim, pdim, n, kind, ap_rad):
    """at g = 0 the sheared frequency is the mode's own (d00 = d01 = d11 = 0
    exactly) and the covariance sums are those of measure_arrays with
    use_noise_image=True, the reference's, under the bound of the twins (no
    centre phase enters a covariance sum)"""
    c, power, _, plan = setup_of(dim, pdim, n, kind, ap_rad)
    m = prepsfmom.PrePSFMom(pw.measure_of(kind, dim, ap_rad).fwhm, kind, ap_rad=ap_rad,
                            use_noise_image=True)
    want = _unsheared_power_cov(m, c, power, dim, pdim)
    g = np.zeros((1, 2))
    sums, fl = twin(dim, pdim, n, kind, ap_rad, g, False)
    ref = pw.reference(dim, pdim, n, kind, ap_rad, False)["types"]
    sub = {k: v[:, :1] for k, v in ref.items()}
    assert not fl.any()
    ratio = pw.worst_ratio(sums[..., 4:], sub)
    ratio_m = pw.worst_ratio(want[:, None, :], sub)
    gap = float(np.max(np.abs(sums[:, 0, 4:] - want) /
                       (pw.EPS * sub["absum"][:, 0].astype(np.float64))))
    print("g = 0 dim %d/%d %s ap %.1f: twin %.4g, measure_arrays' stages %.4g, between them %.4g "
          "units (bound %.0f)" % (dim, pdim, kind, ap_rad, ratio, ratio_m, gap,
                                  pw.c_round(dim, pdim)))
    assert gap <= pw.c_round(dim, pdim)


def test_turning_identity():
    """|DTFT[rot90(N, 1)](q_r, q_c)| = |N^(q_c, -q_r)| for random planes at random
    in-band frequencies, to a few ulp of sum |N|: why the fixnoise term's power
    is read from the un-turned plane"""
    rng = np.random.RandomState(31)
    worst = 0.0
    for dim in (9, 12, 16):
        plane = rng.normal(size=(dim, dim))
        q = rng.uniform(-np.pi, np.pi, size=(2, 40))
        qr, qc = q[0].astype(np.longdouble), q[1].astype(np.longdouble)
        zero = np.zeros(2, dtype=np.longdouble)
        for dtype in (np.longdouble, np.float64):
            a = np.abs(pn._dtft(np.rot90(plane, 1).astype(dtype), zero.astype(dtype),
                                qr.astype(dtype), qc.astype(dtype)))
            b = np.abs(pn._dtft(plane.astype(dtype), zero.astype(dtype), qc.astype(dtype),
                                (-qr).astype(dtype)))
            ulp = float(np.finfo(dtype).eps) * np.abs(plane).sum()
            worst = max(worst, float(np.max(np.abs(a - b)) / ulp)) if dtype is np.float64 else worst
            assert np.all(np.abs(a - b) <= 8 * ulp)
        # and not at the frequencies a mistaken turn would read
        wrong = np.abs(pn._dtft(plane.astype(np.longdouble), zero, qc, qr))
        assert np.max(np.abs(a - wrong.astype(np.float64))) > 0.1
    print("turning identity: largest float64 gap %.3g ulp of sum |N| (allowed 8)" % worst)


def test_the_fixnoise_power_is_the_turned_planes():
    """what the fixnoise power entry adds to the covariance sums of the power
    entry (the twins' difference) is the second term of the definition taken
    from a LITERAL turned copy rot90(N, 1) read at q' -- the twin reads the
    un-turned plane at (q'_c, -q'_r) and holds no such copy"""
    dim, pdim, n = pw.SHAPES[0]
    c, power, nt, plan = setup_of(dim, pdim, n, "ksigma", 1.5)
    rows, cols, wgt, fk, D, _ = plan
    L = _lib.lib()
    g = np.array([[0.21, -0.17]])
    _, both, _ = pw.call_host(L, _lib.ptr, c, power, nt, g, *plan)
    _, first, _ = pw.call_host(L, _lib.ptr, c, power, None, g, *plan)
    for i in range(n):
        ks, qs = pw.frequencies(pw.DERIV, g[0], rows, cols, D)
        lit = pw.plane_power(np.rot90(power[i], 1), qs[0], qs[1])       # a literal turned copy
        want, fl, absum = pw.cov_sums(None, lit, c["psfs"][i], c["pcen"][i], ks, qs, wgt, fk, D,
                                      dim, np.abs(power[i]).sum())
        assert fl == 0
        second = both[i, 0, 4:] - first[i, 0, 4:]
        # two twins' errors and the subtraction of two sums of about twice the size
        tol = 4 * pw.c_round(dim, pdim) * pw.EPS * absum.astype(np.float64)
        assert np.all(np.abs(second - want.astype(np.float64)) <= tol)


@pytest.mark.parametrize("dim,pdim,n", pw.SHAPES)
def test_moment_sums_are_those_without_the_noise_image(dim, pdim, n):
    L = _lib.lib()
    for kind in pw.KINDS:
        c, power, nt, plan = setup_of(dim, pdim, n, kind, 1.5)
        for g in (pw.type_shears(), c["shears"][:, None, :]):
            for fix in (None, nt):
                st, with_power, fl = pw.call_host(L, _lib.ptr, c, power, fix, g, *plan)
                st0, base, fl0 = pw.call_host(L, _lib.ptr, c, None, fix, g, *plan, base=True)
                assert st == st0 == _lib.OK and not fl.any() and not fl0.any()
                assert np.array_equal(with_power[..., :4], base[..., :4])
                assert not np.any(with_power[..., 4:] == base[..., 4:])
                # the weights are not read
                st, again, _ = pw.call_host(L, _lib.ptr, c, power, fix, g, *plan, weights=None)
                assert st == _lib.OK and np.array_equal(again, with_power)


def test_a_stamp_does_not_depend_on_its_batch_and_a_nan_stays_home():
    dim, pdim, n = pw.SHAPES[2]
    c, power, nt, plan = setup_of(dim, pdim, n, "pgauss", 1.5)
    L = _lib.lib()
    g = pw.type_shears()
    for fix in (None, nt):
        _, whole, _ = pw.call_host(L, _lib.ptr, c, power, fix, g, *plan)
        _, tiled, _ = pw.call_host(L, _lib.ptr, c, power, fix, np.tile(g, (n, 1, 1)), *plan)
        assert np.array_equal(whole, tiled)
        one = {k: v[2:3] for k, v in c.items()}
        _, s, _ = pw.call_host(L, _lib.ptr, one, power[2:3], None if fix is None else fix[2:3], g,
                               *plan)
        assert np.array_equal(s[0], whole[2])
        bad = power.copy()
        bad[1, 0, dim - 1] = np.nan
        st, sums, fl = pw.call_host(L, _lib.ptr, c, bad, fix, g, *plan)
        assert st == _lib.OK and fl.tolist() == [[0] * 5, [1] * 5, [0] * 5]
        assert np.all(np.isnan(sums[1])) and np.array_equal(sums[[0, 2]], whole[[0, 2]])
        bad[1, 0, dim - 1] = np.inf
        st, sums, fl = pw.call_host(L, _lib.ptr, c, bad, fix, g, *plan)
        assert fl.tolist() == [[0] * 5, [1] * 5, [0] * 5] and np.all(np.isnan(sums[1]))


def test_errors_of_correlated_noise():
    """The reason for the feature.  256 stamps of 16 x 16 carry stationary
    correlated noise (white noise on 18 x 18 through a fixed 3 x 3 kernel); the
    noise image of each is an independent realisation.  The expected power is
    closed form, and through the longdouble reference gives the expected
    covariance C0.  Per diagonal covariance sum the per-stamp ratio to C0 has
    sample mean m and scatter s: |m - 1| < 5 s / sqrt(256) for the noise-image
    path, with and without fixnoise -- and NOT for the white-noise path at the
    pixel variance (weight = 1 / variance), on the ff sum at least."""
    dim, n = pw.STAT_DIM, pw.STAT_N
    rng = np.random.RandomState(77)
    cen = np.array([7.3, 7.8])
    psf = pw.gaussian_stamp(dim, (7.5, 7.5), pw.DERIV, 0.3 ** 2 * np.eye(2), 1.0)
    gal = pw.gaussian_stamp(dim, cen, pw.DERIV, (0.3 ** 2 + 0.35 ** 2) * np.eye(2), 100.0)
    images = gal[None] + pw.correlated_noise(rng, n, dim)
    power = pw.correlated_noise(rng, n, dim)
    field = pw.turned(pw.correlated_noise(rng, n, dim))
    xi = pw.autocorrelation()
    var = xi[0, 0]
    assert abs(power.var() / var - 1) < 0.05
    c = dict(images=images, psfs=np.tile(psf, (n, 1, 1)), weights=np.full((n, dim, dim), 1 / var),
             cen=np.tile(cen, (n, 1)), pcen=np.full((n, 2), 7.5))
    m = pw.measure_of("pgauss", dim, 1.5)
    _, D, rows, cols, wgt, fk = pw.plan_of(m, dim, dim)
    plan = (rows, cols, wgt, fk, D, 1.5)
    g = np.array([[0.0, 0.0], [0.2, -0.1]])
    L = _lib.lib()
    diag = [0, 4, 7, 9]                   # pp, cc, rr, ff among the ten
    for fix in (None, field):
        st, sums, fl = pw.call_host(L, _lib.ptr, c, power, fix, g, *plan)
        st0, white, fl0 = pw.call_host(L, _lib.ptr, c, None, fix, g, *plan, base=True)
        assert st == st0 == _lib.OK and not fl.any() and not fl0.any()
        for t in range(g.shape[0]):
            ks, qs = pw.frequencies(pw.DERIV, g[t], rows, cols, D)
            ek = pw.expected_power(ks[0], ks[1], dim, xi)
            eq = None if fix is None else pw.expected_power(qs[1], -qs[0], dim, xi)
            c0, rfl, _ = pw.cov_sums(ek, eq, psf, (7.5, 7.5), ks, qs, wgt, fk, D, dim, 1.0)
            assert rfl == 0
            c0 = c0.astype(np.float64)[diag]
            ratio = sums[:, t, 4:][:, diag] / c0
            mean, s = ratio.mean(axis=0), ratio.std(axis=0, ddof=1)
            wratio = white[:, t, 4:][:, diag] / c0
            wmean, ws = wratio.mean(axis=0), wratio.std(axis=0, ddof=1)
            print("fixnoise %d g %s: noise image m - 1 = %s, 5 s / 16 = %s; white m - 1 = %s"
                  % (fix is not None, g[t], np.round(mean - 1, 4), np.round(5 * s / 16, 4),
                     np.round(wmean - 1, 4)))
            assert np.all(np.abs(mean - 1) < 5 * s / np.sqrt(n))
            # the white level fails the criterion on ff -- by its own scatter (one
            # weight map: none) and by the scatter of the estimate it would replace
            assert not abs(wmean[3] - 1) < 5 * ws[3] / np.sqrt(n)
            assert not abs(wmean[3] - 1) < 5 * s[3] / np.sqrt(n)


def test_refusals():
    m = prepsfmom.PGaussMom(1.2, use_noise_image=True)
    plain = prepsfmom.PGaussMom(1.2)
    z = np.zeros((2, 16, 16))
    cen = np.full((2, 2), 7.5)
    deriv = (0.263, 0.0, 0.0, 0.263)
    g = pw.type_shears()
    # before anything is uploaded or launched: these raise where there is no device
    with pytest.raises(ValueError, match="obs.noise must be set when use_noise_image=True"):
        m.measure_arrays_sheared(z, z + 1, cen, deriv, z, cen, g)
    with pytest.raises(ValueError, match="obs.noise must be set when use_noise_image=True"):
        m.go_metacal_batch(z, z + 1, cen, deriv, z, cen)
    # (callers of the route as it was, which refused the option, still catch it)
    with pytest.raises(NotImplementedError, match="use_noise_image"):
        m.measure_arrays_sheared(z, z + 1, cen, deriv, z, cen, g)
    with pytest.raises(ValueError, match="use_noise_image=False"):
        plain.measure_arrays_sheared(z, z + 1, cen, deriv, z, cen, g, noise_images=z)
    with pytest.raises(ValueError, match="use_noise_image=False"):
        plain.go_metacal_batch(z, z + 1, cen, deriv, z, cen, noise_images=z)
    for bad in (np.zeros((2, 16, 15)), np.zeros((3, 16, 16)), np.zeros((2, 17, 17)),
                np.zeros((2, 256))):
        with pytest.raises(ValueError, match="one 16 x 16 plane per stamp"):
            m.measure_arrays_sheared(z, z + 1, cen, deriv, z, cen, g, noise_images=bad)
    # no_psf stays refused, and the empty batch needs no device
    with pytest.raises(NotImplementedError, match="no_psf"):
        m.measure_arrays_sheared(z, z + 1, cen, deriv, None, None, g, noise_images=z)
    e = np.zeros((0, 16, 16))
    mom, cov, fl, _, D = m.measure_arrays_sheared(e, e, np.zeros((0, 2)), deriv, e,
                                                  np.zeros((0, 2)), g, noise_images=e)
    assert mom.shape == (0, 5, 6) and cov.shape == (0, 5, 6, 6) and fl.shape == (0, 5) and D == 64
    # the catalogue route: the measure's switch asks for every observation's noise image
    from ngmix_amd.jacobian import Jacobian
    from ngmix_amd.observation import Observation
    jac = Jacobian(row=7.5, col=7.5, dvdrow=0.263, dvdcol=0.0, dudrow=0.0, dudcol=0.263)
    psf = Observation(np.ones((16, 16)), jacobian=jac)
    obs = [Observation(z[0] + 1, weight=z[0] + 1, jacobian=jac, psf=psf, noise=z[0]),
           Observation(z[0] + 1, weight=z[0] + 1, jacobian=jac, psf=psf)]
    with pytest.raises(ValueError, match="obs.noise must be set when use_noise_image=True"):
        metacal.metacal_moments_many(obs, m)
    assert metacal.metacal_moments_many([], m) == []
    # the C ABI: both entries, host twin and device entry (which refuses before a launch)
    dim, pdim, n = pw.SHAPES[2]
    c, power, nt, plan = setup_of(dim, pdim, n, "ksigma", 1.5)
    L = _lib.lib()
    for host in (True, False):
        for fix in (None, nt):
            def call(**over):
                return pw.call_host(L, _lib.ptr, c, power, fix, over.pop("g", g), *plan, host=host,
                                    **over)
            assert call(noise_power=None)[0] == _lib.ERR_BAD_ARG
            assert "noise_power is required" in _lib.last_error()
            for name in ("images", "psf", "cen", "psf_cen", "g_host", "mrow", "fk", "sums", "flags"):
                assert call(**{name: None})[0] == _lib.ERR_BAD_ARG, name
                assert "required" in _lib.last_error()
            if fix is not None:
                assert call(noise_turned=None)[0] == _lib.ERR_BAD_ARG
                assert "noise_turned" in _lib.last_error()
            assert call(dim=0)[0] == _lib.ERR_BAD_ARG and call(n=-1)[0] == _lib.ERR_BAD_ARG
            gb = g.copy()
            gb[2] = 0.8, 0.7
            assert call(g=gb)[0] == _lib.ERR_BAD_ARG
            assert "unit circle" in _lib.last_error()
            # over the 160 KB of LDS: 20424 doubles of planes.  Three planes of 82^2 fit
            # (20172), of 83^2 do not; with the fixnoise plane four of 71^2 fit, of 72^2
            # do not; the forms without the noise image still take those shapes
            over, fits = (72, 71) if fix is not None else (83, 82)
            st, sums, fl = call(dim=over, pdim=over)
            assert st == _lib.ERR_BAD_ARG and "LDS" in _lib.last_error()
            assert "noise-power plane" in _lib.last_error()
            assert np.all(sums == -7.0) and np.all(fl == -7)          # nothing was written
            assert call(dim=over, pdim=over, base=True, g=gb)[0] == _lib.ERR_BAD_ARG
            assert "unit circle" in _lib.last_error()                 # (its last check: it fits)
            assert call(dim=fits, pdim=fits, g=gb)[0] == _lib.ERR_BAD_ARG
            assert "unit circle" in _lib.last_error()
            st, _, _ = call(n=0, images=None, weights=None, psf=None, noise_power=None, cen=None,
                            psf_cen=None, sums=None, flags=None, mrow=None, mcol=None, wgt=None,
                            fk=None, **({} if fix is None else dict(noise_turned=None)))
            assert st == _lib.OK


def test_the_entries_are_declared_with_one_more_argument():
    sig = _lib.SIGNATURES
    plain = sig["ngmix_prepsf_shear_sums_batch"][1]
    fix = sig["ngmix_prepsf_shear_fixnoise_sums_batch"][1]
    assert sig["ngmix_prepsf_shear_power_sums_batch"][1] == plain[:3] + [plain[0]] + plain[3:]
    assert sig["ngmix_prepsf_shear_fixnoise_power_sums_batch"][1] == fix[:4] + [fix[0]] + fix[4:]
    for name in ("ngmix_prepsf_shear_power_sums", "ngmix_prepsf_shear_fixnoise_power_sums"):
        assert sig[name + "_host"][1] == sig[name + "_batch"][1][:-1]
    import inspect
    m = prepsfmom.PGaussMom(1.2)
    assert list(inspect.signature(m.measure_arrays_sheared).parameters)[7:] == \
        ["noise", "noise_ierr", "noise_images"]
    assert list(inspect.signature(m.go_metacal_batch).parameters)[-1] == "noise_images"
    # metacal_moments_batch keeps its parameters: a StampBatch holds no noise images
    assert "noise_images" not in inspect.signature(metacal.metacal_moments_batch).parameters
