"""
The fixnoise term of the sheared pre-psf moments on the device (DESIGN.md 3.22;
prepsf_shear_sums_kernel<true> through PrePSFMom.measure_arrays_sheared(noise=)
and metacal.metacal_moments_batch / _many) against the dense longdouble
reference of tests/helpers/prepsf_shear_noise_reference.py, under the bound its
float64 restatement sets (TWIN_TOL = 4 x the float64 gap, relative to each
sum's largest term); against the host twin; the turning identity, which does
not use the restatement; and what must hold to the bit: the two layouts of g,
batches cut in two and reversed, repeated draws, the two ways to send the same
planes, the catalogue route, and fixnoise=False beside the new code.
"""
import numpy as np
import pytest

from ngmix_amd import _lib, metacal
from ngmix_amd.batch import StampBatch
from ngmix_amd.jacobian import Jacobian
from ngmix_amd.observation import Observation
from helpers import prepsf_shear_reference as ps
from helpers import prepsf_shear_noise_reference as pn

pytestmark = pytest.mark.gpu

CASES = [(d, p, n, k, a) for (d, p, n) in pn.SHAPES for k in pn.KINDS for a in pn.AP_RADS]
ROWS_OF_70 = (0, 1, 69)
SEED = 0x5EEDF00D1234


def sums14(mom, cov):
    out = [mom[..., 2 + a] for a in range(4)]
    out += [cov[..., 2 + a, 2 + b] for a in range(4) for b in range(a, 4)]
    return np.stack(out, axis=-1)


def run(c, m, g, noise, sel=slice(None), deriv=pn.DERIV):
    mom, cov, fl, kernels, D = m.measure_arrays_sheared(
        c["images"][sel], c["weights"][sel], c["cen"][sel], deriv, c["psfs"][sel], c["pcen"][sel],
        g, noise=None if noise is None else noise[sel])
    return sums14(mom, cov), fl


def _jacs(cen):
    n = cen.shape[0]
    det = pn.DERIV[0] * pn.DERIV[3] - pn.DERIV[1] * pn.DERIV[2]
    out = np.zeros((n, 8))
    out[:, 0:2] = cen
    out[:, 2:6] = pn.DERIV
    out[:, 6], out[:, 7] = det, np.sqrt(abs(det))
    return out


def batches(c):
    sb = StampBatch.from_images(c["images"], np.where(c["weights"] > 0, c["weights"], 0.0),
                                _jacs(c["cen"]))
    return sb, StampBatch.from_images(c["psfs"], None, _jacs(c["pcen"]))


def same(a, b, keys=("sums", "sums_cov", "flux", "T", "e", "flags", "mcal_flags")):
    for t in pn.TYPES:
        for key in keys:
            assert np.array_equal(a[t][key], b[t][key], equal_nan=True), (t, key)


def rows(res, idx):
    return {t: {k: v[idx] for k, v in res[t].items() if isinstance(v, np.ndarray)
                and v.shape[:1] == res[t]["flags"].shape} for t in res}


@pytest.mark.parametrize("dim,pdim,n,kind,ap_rad", CASES)
def test_kernel_against_longdouble(dim, pdim, n, kind, ap_rad):
    rows_of = ROWS_OF_70 if n == 70 else None
    ref = pn.reference(dim, pdim, n, kind, ap_rad, rows_of=rows_of)
    c, noise = pn.case(dim, pdim, n), pn.noise_planes(dim, pdim, n)
    m = pn.measure_of(kind, dim, ap_rad)
    idx = list(rows_of or range(n))
    for name, g in (("types", pn.type_shears()), ("galshear", c["shears"][:, None, :])):
        sums, fl = run(c, m, g, noise)
        assert not fl.any() and np.all(np.isfinite(sums))
        sub = {k: v[idx] for k, v in ref[name].items()}
        gap = pn.gap(sums[idx], sub)
        print("%s dim %d/%d %s ap %.1f: kernel gap %.4g (allowed %.3g)"
              % (name, dim, pdim, kind, ap_rad, gap, pn.TWIN_TOL))
        assert gap <= pn.TWIN_TOL


@pytest.mark.parametrize("dim,pdim,n", pn.SHAPES[1:3])
def test_kernel_against_host_twin(dim, pdim, n):
    """the twin runs the kernel's text in the kernel's order and differs from it
    through sincos and hypot alone; each is within TWIN_TOL of the exact value,
    so the two are within twice that of each other"""
    c, noise = pn.case(dim, pdim, n), pn.noise_planes(dim, pdim, n)
    for kind in pn.KINDS:
        m = pn.measure_of(kind, dim, 1.5)
        _, D, mrows, mcols, wgt, fk = pn.plan_of(m, dim, pdim)
        ref = pn.reference(dim, pdim, n, kind, 1.5)
        for name, g in (("types", pn.type_shears()), ("galshear", c["shears"][:, None, :])):
            sums, fl = run(c, m, g, noise)
            st, twin, tfl = pn.call_host(_lib.lib(), _lib.ptr, c, pn.turned(noise), g, mrows,
                                         mcols, wgt, fk, D, 1.5)
            assert st == _lib.OK and not fl.any() and not tfl.any()
            gap = float(np.max(np.abs(sums - twin) / ref[name]["scale"].astype(np.float64)))
            print("%s dim %d/%d %s: kernel against twin %.4g" % (name, dim, pdim, kind, gap))
            assert gap <= 2 * pn.TWIN_TOL


def test_turning_identity_on_the_device():
    for dim, pdim, n in ((16, 16, 2), (17, 11, 2)):
        c, planes, deriv = pn.turning_case(dim, pdim, n)
        for kind in pn.KINDS:
            m = pn.measure_of(kind, dim, 1.5)
            _, D, mrows, mcols, wgt, fk = pn.plan_of(m, dim, pdim, deriv=deriv)
            g = np.concatenate([pn.type_shears(), [[0.21, -0.17]]])
            both, fl = run(c, m, g, planes, deriv=deriv)
            image_term, fl1 = run(c, m, g, None, deriv=deriv)
            mirrored, fl2 = run(c, m, -g, None, deriv=deriv)
            assert not fl.any() and not fl1.any() and not fl2.any()
            noise_term = both[..., :4] - image_term[..., :4]
            worst = 0.0
            for i in range(n):
                for t in range(g.shape[0]):
                    _, rfl, scale, _ = pn.fixnoise_sums(
                        planes[i], c["weights"][i], planes[i], c["cen"][i], deriv, c["psfs"][i],
                        c["pcen"][i], g[t], mrows, mcols, wgt, fk, D, 1.5)
                    scale = scale[:4].astype(np.float64)
                    d = np.abs(noise_term[i, t] - mirrored[i, t, :4]) / scale
                    worst = max(worst, float(d.max()))
                    assert rfl == 0 and np.all(d <= 2 * pn.TWIN_TOL)
                    if t in (1, 3):      # 1p against 1m, 2p against 2m: no response of the sums
                        d = np.abs(both[i, t, :4] - both[i, t + 1, :4]) / scale
                        worst = max(worst, float(d.max()))
                        assert np.all(d <= 2 * pn.TWIN_TOL)
            print("turning identity dim %d/%d %s: largest gap %.3g (allowed %.3g)"
                  % (dim, pdim, kind, worst, 2 * pn.TWIN_TOL))


def test_bits_do_not_depend_on_layout_of_g():
    dim, pdim, n = pn.SHAPES[0]
    c, noise = pn.case(dim, pdim, n), pn.noise_planes(dim, pdim, n)
    for kind in pn.KINDS:
        m = pn.measure_of(kind, dim, 1.5)
        whole, fl = run(c, m, pn.type_shears(), noise)
        tiled, _ = run(c, m, np.tile(pn.type_shears(), (n, 1, 1)), noise)
        assert not fl.any() and np.array_equal(whole, tiled)
        plain, _ = run(c, m, pn.type_shears(), None)
        assert not np.array_equal(whole[..., :4], plain[..., :4])


def test_seeded_field_does_not_depend_on_the_batching():
    """35 + 35 = 70, the reversed order and a second call, to the bit, through
    metacal_moments_batch(noise_seed=, ids=); the planes sent un-turned are the
    DeviceNoise route to the bit"""
    dim, pdim, n = pn.SHAPES[0]
    c = pn.case(dim, pdim, n)
    m = pn.measure_of("pgauss", dim, 1.5)
    sb, psb = batches(c)
    ids = np.arange(n, dtype=np.int64) * 7 + 1000
    kw = dict(step=pn.STEP, fixnoise=True, noise_seed=SEED)
    whole = metacal.metacal_moments_batch(sb, psb, m, ids=ids, **kw)
    assert list(whole) == list(pn.TYPES)
    same(whole, metacal.metacal_moments_batch(sb, psb, m, ids=ids, **kw))
    for idx in (np.arange(35), np.arange(35, 70), np.arange(n)[::-1]):
        part = metacal.metacal_moments_batch(sb.select(idx), psb.select(idx), m, ids=ids[idx], **kw)
        same(part, rows(whole, idx))
    # ids default to the positions
    same(metacal.metacal_moments_batch(sb, psb, m, **kw),
         metacal.metacal_moments_batch(sb, psb, m, ids=np.arange(n), **kw))
    other = metacal.metacal_moments_batch(sb, psb, m, ids=ids, step=pn.STEP, fixnoise=True,
                                          noise_seed=SEED + 1)
    assert not np.array_equal(other["1p"]["sums"], whole["1p"]["sums"])
    # the same field as un-turned planes, and as a DeviceNoise
    mc = metacal.MetacalBatch(sb, psb, target_sigma=np.full(n, 0.4))
    planes = mc.device_noise(SEED, ids)
    for noise in (planes, planes.cpu().numpy(), metacal.DeviceNoise(SEED, ids)):
        same(whole, metacal.metacal_moments_batch(sb, psb, m, step=pn.STEP, fixnoise=True,
                                                  noise=noise))


def test_fixnoise_false_is_unchanged_beside_the_new_code():
    dim, pdim, n = pn.SHAPES[1]
    c = pn.case(dim, pdim, n)
    m = pn.measure_of("ksigma", dim, 1.5)
    sb, psb = batches(c)
    before = metacal.metacal_moments_batch(sb, psb, m, step=pn.STEP)
    with_noise = metacal.metacal_moments_batch(sb, psb, m, step=pn.STEP, fixnoise=True,
                                               noise_seed=SEED)
    after = metacal.metacal_moments_batch(sb, psb, m, step=pn.STEP, fixnoise=False)
    same(before, after)
    assert not np.array_equal(before["noshear"]["sums"], with_noise["noshear"]["sums"])
    # ... and they are the sums of the plain entry
    w = np.where(c["weights"] > 0, c["weights"], 0.0)
    mom, cov, fl, _, _ = m.measure_arrays_sheared(c["images"], w, c["cen"], pn.DERIV, c["psfs"],
                                                  c["pcen"], pn.type_shears())
    for i, t in enumerate(pn.TYPES):
        assert np.array_equal(after[t]["sums"][:, 2:], mom[:, i, 2:])
        assert np.array_equal(after[t]["sums_cov"][:, 2:, 2:], cov[:, i, 2:, 2:])


def test_metacal_moments_many_with_noise_images_is_the_batch_row_by_row():
    m = pn.measure_of("ksigma", 17, 1.5)
    obs, want = [], []
    for dim, pdim, n in (pn.SHAPES[1], pn.SHAPES[2]):
        c, noise = pn.case(dim, pdim, n), pn.noise_planes(dim, pdim, n)
        c["weights"] = np.where(c["weights"] > 0, c["weights"], 0.0)
        res = m.go_metacal_batch(c["images"], c["weights"], c["cen"], pn.DERIV, c["psfs"],
                                 c["pcen"], step=pn.STEP, fixnoise=True, noise=noise)
        for i in range(n):
            def jac(cen):
                return Jacobian(row=cen[0], col=cen[1], dvdrow=pn.DERIV[0], dvdcol=pn.DERIV[1],
                                dudrow=pn.DERIV[2], dudcol=pn.DERIV[3])
            psf = Observation(c["psfs"][i], jacobian=jac(c["pcen"][i]))
            obs.append(Observation(c["images"][i], weight=c["weights"][i], noise=noise[i],
                                   jacobian=jac(c["cen"][i]), psf=psf))
            want.append((res, i))
    order = [3, 0, 4, 1, 2]                  # the two shapes interleaved
    many = metacal.metacal_moments_many([obs[k] for k in order], m, step=pn.STEP, fixnoise=True,
                                        use_noise_image=True)
    plain = metacal.metacal_moments_many([obs[k] for k in order], m, step=pn.STEP)
    for got, old, k in zip(many, plain, order):
        res, i = want[k]
        for t in pn.TYPES:
            for key in ("sums", "sums_cov", "flux", "T", "e"):
                assert np.array_equal(got[t][key], res[t][key][i], equal_nan=True), (t, key)
            assert got[t]["flags"] == res[t]["flags"][i]
            assert got[t]["mcal_flags"] == res[t]["mcal_flags"][i] == 0
            assert not np.array_equal(got[t]["sums"], old[t]["sums"])
    # seeded: a row does not depend on the catalogue around it once it has its id
    ids = np.array([11, 12, 13, 14, 15])
    seeded = metacal.metacal_moments_many([obs[k] for k in order], m, step=pn.STEP, fixnoise=True,
                                          noise_seed=SEED, ids=ids)
    alone = metacal.metacal_moments_many([obs[order[2]]], m, step=pn.STEP, fixnoise=True,
                                         noise_seed=SEED, ids=ids[2:3])
    for t in pn.TYPES:
        assert np.array_equal(seeded[2][t]["sums"], alone[0][t]["sums"], equal_nan=True)


def test_nan_noise_pixel_flags_its_own_stamp():
    dim, pdim, n = pn.SHAPES[1]
    c, noise = pn.case(dim, pdim, n), pn.noise_planes(dim, pdim, n)
    m = pn.measure_of("pgauss", dim, 1.5)
    clean, fl = run(c, m, pn.type_shears(), noise)
    bad = noise.copy()
    bad[1, 3, 4] = np.nan
    sums, fl = run(c, m, pn.type_shears(), bad)
    assert (fl != 0).tolist() == [[False] * 5, [True] * 5, [False] * 5]
    assert np.all(fl[1] == metacal.METACAL_BAND_LIMIT)
    assert np.all(np.isnan(sums[1])) and np.array_equal(sums[[0, 2]], clean[[0, 2]])


def test_response_is_finite_and_the_recovered_response_is_reported():
    """shear_response / mean_shear take the result; the response recovered from
    an ensemble of noisy round gaussians with and without fixnoise is a finding,
    printed, not a bound (none exists for it)"""
    dim, n, scale = 32, 64, 0.263
    deriv = (scale, 0.0, 0.0, scale)
    rng = np.random.RandomState(12)
    cen = (dim - 1) / 2 + rng.uniform(-0.5, 0.5, size=(n, 2))
    pcen = np.full((n, 2), (dim - 1) / 2.0)
    eye = np.eye(2)
    images = np.stack([pn.gaussian_stamp(dim, cen[i], deriv, (0.5 ** 2 + 0.4 ** 2) * eye, 100.0)
                       for i in range(n)])
    sigma = 0.02 * images.max()
    images = images + rng.normal(scale=sigma, size=images.shape)
    psfs = np.stack([pn.gaussian_stamp(dim, pcen[i], deriv, 0.4 ** 2 * eye, 1.0) for i in range(n)])

    def jacs(cen):
        out = np.zeros((n, 8))
        out[:, 0:2] = cen
        out[:, 2:6] = deriv
        out[:, 6], out[:, 7] = scale * scale, scale
        return out
    sb = StampBatch.from_images(images, np.full(images.shape, 1 / sigma ** 2), jacs(cen))
    psb = StampBatch.from_images(psfs, None, jacs(pcen))
    from ngmix_amd import prepsfmom
    m = prepsfmom.PGaussMom(1.2)
    for fixnoise in (False, True):
        res = metacal.metacal_moments_batch(sb, psb, m, step=pn.STEP, fixnoise=fixnoise,
                                            noise_seed=SEED if fixnoise else None)
        resp = metacal.shear_response(res, step=pn.STEP, key="e")
        assert not resp["flags"].any()
        assert np.all(np.isfinite(resp["R"])) and np.all(np.isfinite(resp["g"]))
        assert np.all(np.isfinite(metacal.mean_shear(resp)))
        R = resp["R"].mean(axis=0)
        print("fixnoise=%s: mean response of %d noisy round gaussians R11 %.5f R22 %.5f, "
              "scatter of R11 %.4f (noiseless analytic 1.019)"
              % (fixnoise, n, R[0, 0], R[1, 1], resp["R"][:, 0, 0].std()))
