"""
Stamps whose weight map is ONE value (NGMIX_STAMP_UNIFORM_IERR): the fused
loglike / fill_fdiff / model_s2n_sum kernels read ierr[pix_off] once instead of
streaming the map.

  * detection: the flag is a fact about the data -- set by the pass that counts
    the kept pixels, compared here with a numpy recomputation from the ierr the
    batch holds (bit patterns equal to the first's, that value finite and > 0);
  * equality: every output with the fast path is torch.equal to the same call
    with StampBatch.stream_ierr = True (the kernels then read every weight map
    as before), over full-tile, ragged, masked, mixed, failing and empty cases.
"""
import numpy as np
import pytest

from ngmix_amd import _lib

pytestmark = pytest.mark.gpu

U = _lib.STAMP_UNIFORM_IERR
SCALE = 0.263


def expected_flags(sb):
    """the uniform bit of every stamp, recomputed on the host from sb.ierr"""
    ierr = sb.ierr.cpu().numpy()
    out = np.zeros(sb.n, dtype=bool)
    for i in range(sb.n):
        e = ierr[sb.pix_off[i]:sb.pix_off[i] + sb.npix[i]]
        bits = e.view(np.int64)
        out[i] = bool(np.all(bits == bits[0]) and np.isfinite(e[0]) and e[0] > 0.0)
    return out


def got_flags(sb):
    host = (sb.flags & U) != 0
    # every device table carries the same bits
    tab = sb.stamp_table(3).cpu().numpy().reshape(-1).view(_lib.STAMP_DTYPE)
    np.testing.assert_array_equal((tab["flags"] & U) != 0, host)
    np.testing.assert_array_equal(tab["flags"] & _lib.STAMP_IGNORE_ZERO_WEIGHT,
                                  sb.flags & _lib.STAMP_IGNORE_ZERO_WEIGHT)
    return host


def mixtures(n, seed, model="exp"):
    from ngmix_amd.batch import GMixBatch
    rng = np.random.RandomState(seed)
    npars = 7 if model == "bdf" else 6
    pars = np.zeros((n, npars))
    pars[:, 0:2] = rng.uniform(-0.5, 0.5, size=(n, 2)) * SCALE
    pars[:, 2:4] = np.clip(rng.normal(scale=0.1, size=(n, 2)), -0.45, 0.45)
    pars[:, 4] = rng.uniform(0.3, 1.5, size=n)
    if model == "bdf":
        pars[:, 5] = rng.uniform(0.1, 0.9, size=n)
    pars[:, -1] = rng.uniform(50, 500, size=n)
    psfpars = np.tile([0.0, 0.0, 0.0, 0.0, 0.27, 1.0], (n, 1))
    gm0, _ = GMixBatch.from_pars(pars, model)
    psf, _ = GMixBatch.from_pars(psfpars, "gauss")
    gm, _ = gm0.convolve(psf)
    return gm


def ragged_batch(shapes, ierr_of, izw=True, seed=3):
    """stamps of the given shapes; ierr_of(i, npix, rng) -> the stamp's ierr"""
    import torch
    from ngmix_amd.batch import StampBatch
    rng = np.random.RandomState(seed)
    n = len(shapes)
    nrow = np.array([s[0] for s in shapes])
    ncol = np.array([s[1] for s in shapes])
    npix = nrow * ncol
    off = np.concatenate([[0], np.cumsum(npix)[:-1]]).astype(np.int64)
    val = rng.normal(size=int(npix.sum()))
    ierr = np.concatenate([np.asarray(ierr_of(i, int(npix[i]), rng), dtype="f8")
                           for i in range(n)])
    jac = np.zeros((n, 8))
    for i, s in enumerate(shapes):
        jac[i] = [(s[0] - 1) / 2, (s[1] - 1) / 2, SCALE, 0.0, 0.0, SCALE, SCALE ** 2, SCALE]
    return StampBatch(torch.from_numpy(val).cuda(), torch.from_numpy(ierr).cuda(),
                      torch.from_numpy(jac).cuda(), nrow, ncol, off, izw)


def mixed_ierr(i, npix, rng):
    """by stamp index: uniform / a full weight map / masked / one pixel off"""
    kind = i % 4
    if kind == 0:
        return np.full(npix, 0.5 + 0.01 * i)
    if kind == 1:
        return rng.uniform(0.5, 2.0, size=npix)
    if kind == 2:
        e = np.full(npix, 1.25)
        e[rng.choice(npix, size=max(1, npix // 7), replace=False)] = 0.0
        return e
    e = np.full(npix, 0.75)
    e[npix // 2] = np.nextafter(0.75, 1.0)
    return e


# ------------------------------------------------------------------ detection
def test_flag_cases():
    n, npix = 12, 48 * 48

    def ierr_of(i, npix, rng):
        e = np.full(npix, 1.0 / 3.0)
        if i == 1:
            e[0] = 0.5                    # the first pixel differs
        elif i == 2:
            e[npix // 2 + 5] = 0.5        # a middle one
        elif i == 3:
            e[-1] = np.nextafter(e[-1], 1.0)   # the last, by one ulp
        elif i == 4:
            e[17] = 0.0                   # one zero-weight pixel
        elif i == 5:
            e[:] = 0.0                    # nothing listed ...
            e[3] = 1.0                    # ... but one pixel (a stamp must keep one)
        elif i == 6:
            e[100] = np.nan
        elif i == 7:
            e[:] = np.inf
        elif i == 8:
            e[:] = np.nan
        elif i == 9:
            e[40] = -e[40]
        elif i == 10:
            e[:] = 7.0                    # another uniform value
        return e

    sb = ragged_batch([(48, 48)] * n, ierr_of)
    got = got_flags(sb)
    want = np.zeros(n, dtype=bool)
    want[[0, 10, 11]] = True
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, expected_flags(sb))
    assert sb.npix_kept[4] == npix - 1 and sb.npix_kept[0] == npix


def test_flag_all_zero_and_keep_zero():
    # ignore_zero_weight off: every pixel is listed, but a zero is not a weight
    # map of one positive value
    def ierr_of(i, npix, rng):
        e = np.full(npix, 2.0)
        if i == 1:
            e[5] = 0.0
        elif i == 2:
            e[:] = 0.0                    # all-zero ierr
        elif i == 3:
            e[:] = -0.0
        return e
    sb = ragged_batch([(16, 16)] * 4, ierr_of, izw=False)
    got = got_flags(sb)
    np.testing.assert_array_equal(got, [True, False, False, False])
    np.testing.assert_array_equal(got, expected_flags(sb))
    assert not sb.any_masked


def test_flag_mixed_ragged():
    shapes = [(48, 48), (17, 23), (32, 32), (8, 16), (33, 9), (64, 64), (20, 17), (13, 15),
              (8, 8), (5, 70), (48, 48), (40, 24)]
    sb = ragged_batch(shapes, mixed_ierr)
    got = got_flags(sb)
    np.testing.assert_array_equal(got, expected_flags(sb))
    np.testing.assert_array_equal(got, np.arange(len(shapes)) % 4 == 0)
    assert sb.any_masked


def test_flag_select_prep_em():
    sb = ragged_batch([(24, 24)] * 9 + [(17, 23)] * 3, mixed_ierr)
    sel = sb.select([11, 0, 3, 4, 4, 2, 8])
    np.testing.assert_array_equal(got_flags(sel), expected_flags(sel))
    np.testing.assert_array_equal(got_flags(sel), got_flags(sb)[[11, 0, 3, 4, 4, 2, 8]])
    em, _ = sb.prep_em()
    np.testing.assert_array_equal(got_flags(em), expected_flags(em))
    np.testing.assert_array_equal(got_flags(em), got_flags(sb))


def test_flag_builders():
    import torch
    from ngmix_amd.batch import StampBatch
    rng = np.random.RandomState(8)
    n, nrow, ncol = 8, 16, 24
    images = rng.normal(size=(n, nrow, ncol))
    weights = np.empty((n, nrow, ncol))
    for i in range(n):
        weights[i] = mixed_ierr(i, nrow * ncol, rng).reshape(nrow, ncol) ** 2
    weights[5] = -1.0       # no positive weight, ignore_zero_weight off below
    jac = np.tile([7.5, 11.5, SCALE, 0.0, 0.0, SCALE, SCALE ** 2, SCALE], (n, 1))
    izw = np.array([True] * 5 + [False] + [True] * 2)
    want = np.arange(n) % 4 == 0
    for sb in (StampBatch.from_stacked(images, weights, jac, izw),
               StampBatch.from_stacked(torch.from_numpy(images), torch.from_numpy(weights),
                                       jac, izw),
               StampBatch.from_arrays(list(images), list(weights), list(jac), list(izw)),
               StampBatch.from_images(images, weights, jac[0], izw)):
        got = got_flags(sb)
        np.testing.assert_array_equal(got, expected_flags(sb))
        np.testing.assert_array_equal(got, want)
        # (the table the host-side builders upload themselves)
        tab = sb.stamp_table(1).cpu().numpy().reshape(-1).view(_lib.STAMP_DTYPE)
        np.testing.assert_array_equal((tab["flags"] & U) != 0, want)
    # no weight map at all: unit weights
    sb = StampBatch.from_images(images)
    assert got_flags(sb).all() and expected_flags(sb).all()


def test_rescan_weights():
    sb = ragged_batch([(16, 16)] * 4, lambda i, npix, rng: np.full(npix, 1.5))
    gm = mixtures(4, 2)
    assert got_flags(sb).all()
    a, _ = sb.loglike(gm.clone())
    sb.ierr[sb.pix_off[1] + 7] = 0.0
    sb.ierr[sb.pix_off[2] + 255] = 3.0
    sb.rescan_weights()
    np.testing.assert_array_equal(got_flags(sb), [True, False, False, True])
    np.testing.assert_array_equal(got_flags(sb), expected_flags(sb))
    assert sb.npix_kept[1] == 255 and sb.any_masked
    check_equal(sb, gm)
    b, _ = sb.loglike(gm.clone())
    assert float(b[1, 3]) == 255.0 and float(a[1, 3]) == 256.0
    assert bool(b[0, 0] == a[0, 0]) and bool(b[2, 0] != a[2, 0])


# ------------------------------------------------------------------- equality
def check_equal(sb, gm, no_skip=False, expect_status=None):
    """loglike (four columns and status), fill_fdiff and model_s2n_sum: the
    fast path against the same call with every weight map streamed"""
    import torch
    res = []
    for stream in (False, True):
        sb.stream_ierr = stream
        out = torch.zeros((sb.n, 4), dtype=torch.float64, device=sb.device)
        out, st = sb.loglike(gm.clone(), out=out, no_skip=no_skip)
        fd, stf = sb.fill_fdiff(gm.clone(), no_skip=no_skip)
        s2n = torch.zeros(sb.n, dtype=torch.float64, device=sb.device)
        s2n, sts = sb.model_s2n_sum(gm.clone(), out=s2n)
        torch.cuda.synchronize()
        res.append((out, st, fd, stf, s2n, sts))
    sb.stream_ierr = False
    for a, b, name in zip(res[0], res[1], ("loglike", "status", "fdiff", "fdiff status",
                                             "s2n", "s2n status")):
        assert torch.equal(a, b), name
    if expect_status is not None:
        np.testing.assert_array_equal(res[0][1].cpu().numpy(), expect_status)
    else:
        assert int(res[0][1].abs().sum()) == 0
        assert bool(torch.isfinite(res[0][0]).all())
    return res[0]


def uniform_c2(n, seed=4, shape=(48, 48)):
    """the flagship's kind of batch: one noise level per stamp"""
    import torch
    from ngmix_amd.batch import StampBatch
    rng = np.random.RandomState(seed)
    npix = shape[0] * shape[1]
    val = torch.from_numpy(rng.normal(size=n * npix)).cuda()
    sig = torch.from_numpy(rng.uniform(0.5, 2.0, size=n)).cuda()
    ierr = (1.0 / sig)[:, None].expand(n, npix).contiguous().reshape(-1)
    jac = np.tile([(shape[0] - 1) / 2, (shape[1] - 1) / 2, SCALE, 0.0, 0.0, SCALE,
                   SCALE ** 2, SCALE], (n, 1))
    return StampBatch(val, ierr, torch.from_numpy(jac).cuda(), np.full(n, shape[0]),
                      np.full(n, shape[1]), np.arange(n, dtype=np.int64) * npix, True)


@pytest.mark.parametrize("no_skip", [False, True])
def test_equal_c2(no_skip):
    n = 512
    sb = uniform_c2(n)
    assert got_flags(sb).all() and not sb.any_masked
    gm = mixtures(n, 5)
    out = check_equal(sb, gm, no_skip=no_skip)[0]
    assert float(out[:, 2].min()) > 0.0
    # the tracked-load diagnostic takes the compiler-tracked path: same bits
    sb.tracked_loads = True
    out_t = check_equal(sb, gm, no_skip=no_skip)[0]
    sb.tracked_loads = False
    import torch
    assert torch.equal(out, out_t)


def test_equal_mixed_masked():
    n = 256
    sb = ragged_batch([(48, 48)] * n, mixed_ierr)
    assert sb.any_masked and got_flags(sb).sum() == n // 4
    check_equal(sb, mixtures(n, 6))


def test_equal_ragged():
    shapes = [(48, 48), (17, 23), (32, 32), (8, 16), (33, 9), (64, 64), (20, 17), (13, 15),
              (8, 8), (5, 70), (47, 48), (40, 24)] * 8
    sig = np.random.RandomState(1).uniform(0.5, 2.0, size=len(shapes))
    sb = ragged_batch(shapes, lambda i, npix, r: np.full(npix, 1.0 / sig[i]))
    assert got_flags(sb).all()
    check_equal(sb, mixtures(len(shapes), 7))
    # ... and with real weight maps and masks among them
    sb = ragged_batch(shapes, mixed_ierr)
    check_equal(sb, mixtures(len(shapes), 7))


def test_equal_64x64x16():
    n = 96
    sb = uniform_c2(n, shape=(64, 64))
    gm = mixtures(n, 9, model="bdf")
    assert gm.ngauss == 16 and got_flags(sb).all()
    check_equal(sb, gm)


def test_equal_empty_mixture():
    from ngmix_amd.batch import GMixBatch
    sb = ragged_batch([(48, 48)] * 6 + [(17, 23)] * 2, mixed_ierr)
    check_equal(sb, GMixBatch.empty(sb.n, 0))


def test_equal_failed_norms():
    n = 64
    sb = uniform_c2(n)
    gm = mixtures(n, 10)
    rec = gm.to_numpy()
    bad = [3, 17, 40]
    for i in bad:
        rec["det"][i, 2] = 1e-250     # the norms refuse this stamp
        rec["norm_set"][i] = 0
    from ngmix_amd.batch import GMixBatch
    gm = GMixBatch.from_numpy(rec)
    want = np.zeros(n, dtype=np.int32)
    want[bad] = _lib.ERR_DET_TOO_LOW
    check_equal(sb, gm, expect_status=want)


def test_equal_100k():
    n = 100000
    sb = uniform_c2(n)
    assert got_flags(sb).all()
    check_equal(sb, mixtures(n, 11))


def test_exact_does_not_depend_on_flag():
    import torch
    n = 64
    sb = uniform_c2(n)
    gm = mixtures(n, 12)
    a, sa = sb.loglike(gm.clone(), exact=True)
    fa, _ = sb.fill_fdiff(gm.clone(), exact=True)
    sb.stream_ierr = True
    b, sbt = sb.loglike(gm.clone(), exact=True)
    fb, _ = sb.fill_fdiff(gm.clone(), exact=True)
    # the same data in a batch whose stamps are not flagged
    sb2 = uniform_c2(n)
    assert torch.equal(sb2.ierr, sb.ierr) and torch.equal(sb2.val, sb.val)
    sb2.flags = sb2.flags & ~np.int32(U)
    sb2._stamp_tables = {}
    c, sc = sb2.loglike(gm.clone(), exact=True)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(sa, sbt) and torch.equal(fa, fb)
    assert torch.equal(a, c) and torch.equal(sa, sc)
    # ... and the fused fast path agrees with the exact kernels to rounding
    sb.stream_ierr = False
    f, _ = sb.loglike(gm.clone())
    np.testing.assert_allclose(f.cpu().numpy()[:, :3], a.cpu().numpy()[:, :3], rtol=1e-10)
