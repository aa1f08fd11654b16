"""
GPU tests of the fused pixel kernels' ADDRESSING.  The
kernels launched for batches of mixtures of at most 8 gaussians unroll the pair
loop over the gaussian index: bit g of a tile's mask is tested on the scalar
unit and record g is read at a compile-time LDS offset; the lane's tile number
and the address of its box share one register.  Larger mixtures, and stamps
whose gaussians do not share a centre, run the generic loop.  The arithmetic is
the same everywhere, so what can go wrong is an address: a record read at the
wrong offset, a tile offset after a row wrap, a look-ahead past the last tile
that loads, a box tested against the wrong tile.

  * fused default == itself under NGMIX_BATCH_NO_SKIP and under
    NGMIX_BATCH_TRACKED_LOADS, bit for bit (the tracked path addresses its
    pixels through ordinary per-lane loads: an independent addressing);
  * fused default against the exact kernels, with the tolerances of
    tests/test_gpu_pixpass.py (PIX_RTOL / FUSED_ELEM_RTOL per pixel, 1e-11 on
    the sums);
  * a render into an existing image leaves the lines no gaussian reaches
    bit-identical to what they held.
Batches of at most 64 stamps.
"""
import types

import numpy as np
import pytest

from ngmix_amd import _lib

pytestmark = pytest.mark.gpu

SCALE = 0.263
PIX_RTOL = 2e-13          # tests/test_gpu_pixpass.py: per pixel, of the stamp's peak
FUSED_ELEM_RTOL = 1e-10   # ... and elementwise on values that are no cancellation residue
SUM_RTOL = 1e-11          # ... fused against exact sums

# complete 8x8 tilings (loglike / s2n), complete 4x16 tilings (render / fdiff), ragged
SHAPES_8x8 = [(8, 8), (8, 16), (16, 8), (24, 40), (40, 24), (48, 48)]
SHAPES_4x16 = [(4, 16), (8, 32), (12, 48), (48, 48)]
SHAPES_RAGGED = [(13, 21), (47, 50)]
ALL_SHAPES = SHAPES_8x8 + SHAPES_4x16[:3] + SHAPES_RAGGED
NGAUSS = [1, 2, 6, 8, 9, 16, 33]


def _mixtures(rng, shapes, ng, same_centre, cen_pix=3.0, sigma_pix=(0.7, 3.0)):
    """(n, ng) records, norms unset, sizes in pixels of each stamp's scale"""
    n = len(shapes)
    gm = np.zeros((n, ng), dtype=_lib.GAUSS2D_DTYPE)
    sig = rng.uniform(sigma_pix[0], sigma_pix[1], size=(n, ng)) * SCALE
    T = 2.0 * sig ** 2
    e1 = rng.uniform(-0.5, 0.5, size=(n, ng))
    e2 = rng.uniform(-0.5, 0.5, size=(n, ng))
    cshape = (n, 1) if same_centre else (n, ng)
    gm["p"] = rng.uniform(0.5, 5.0, size=(n, ng))
    gm["row"] = np.broadcast_to(rng.uniform(-cen_pix, cen_pix, size=cshape) * SCALE, (n, ng))
    gm["col"] = np.broadcast_to(rng.uniform(-cen_pix, cen_pix, size=cshape) * SCALE, (n, ng))
    gm["irr"], gm["irc"], gm["icc"] = T / 2 * (1 - e1), T / 2 * e2, T / 2 * (1 + e1)
    gm["det"] = gm["irr"] * gm["icc"] - gm["irc"] ** 2
    for f in ("drr", "drc", "dcc", "norm", "pnorm"):
        gm[f] = np.nan
    return gm


def _jacobians(rng, shapes, sheared=True):
    """row0 / col0 differ per stamp; a sheared matrix"""
    jac = np.zeros((len(shapes), 8))
    for i, (nr, nc) in enumerate(shapes):
        a, d = SCALE * (1 + rng.uniform(-0.05, 0.05)), SCALE * (1 + rng.uniform(-0.05, 0.05))
        b, c = (rng.uniform(-0.03, 0.03, size=2) if sheared else (0.0, 0.0))
        det = a * d - b * c
        jac[i] = [(nr - 1) / 2 + rng.uniform(-1.5, 1.5), (nc - 1) / 2 + rng.uniform(-1.5, 1.5),
                  a, b, c, d, det, np.sqrt(abs(det))]
    return jac


def _data(rng, shapes, weights="mixed"):
    imgs = [rng.normal(size=sh) for sh in shapes]
    wts = []
    for i, sh in enumerate(shapes):
        if weights == "uniform" or (weights == "mixed" and i % 2 == 0):
            wts.append(np.full(sh, rng.uniform(0.5, 2.0)))       # one value: not streamed
        else:
            wts.append(rng.uniform(0.5, 2.0, size=sh))           # a real weight map
    return imgs, wts


def _gmix(gmh, ngs=None):
    """device mixtures; ngs: gaussians per stamp (a ragged layout) or None"""
    import torch
    from ngmix_amd.batch import GMixBatch
    if ngs is None:
        return GMixBatch.from_numpy(gmh)
    recs = np.concatenate([gmh[i, :k] for i, k in enumerate(ngs)]) if sum(ngs) else \
        np.zeros(1, dtype=_lib.GAUSS2D_DTYPE)
    flat = np.ascontiguousarray(recs).view(np.float64).reshape(-1, 13)
    return types.SimpleNamespace(n=len(ngs), ngauss=np.asarray(ngs, dtype=np.int64),
                                 data=torch.from_numpy(flat.copy()).cuda())


def _run(imgs, wts, jac, gmh, ngs=None, base=None, **kw):
    """loglike, fdiff, render (into `base`), s2n of one batch as numpy arrays.
    kw: tracked=True, no_skip=True, exact=True"""
    import torch
    from ngmix_amd.batch import StampBatch
    sb = StampBatch.from_arrays(imgs, wts, list(jac), [True] * len(imgs))
    sb.tracked_loads = bool(kw.get("tracked"))
    flags = dict(no_skip=bool(kw.get("no_skip")), exact=bool(kw.get("exact")))
    ll, st = sb.loglike(_gmix(gmh, ngs), **flags)
    fd, sf = sb.fill_fdiff(_gmix(gmh, ngs), **flags)
    image = torch.from_numpy(base).cuda() if base is not None else \
        torch.zeros(sb.total_pix, dtype=torch.float64, device="cuda")
    im, sr = sb.render(_gmix(gmh, ngs), image=image, **flags)
    s2, ss = sb.model_s2n_sum(_gmix(gmh, ngs), exact=flags["exact"])
    torch.cuda.synchronize()
    sts = [t.cpu().numpy() for t in (st, sf, sr, ss)]
    for s in sts[1:]:
        np.testing.assert_array_equal(s, sts[0])
    return dict(ll=ll.cpu().numpy(), fd=fd.cpu().numpy(), im=im.cpu().numpy(),
                s2=s2.cpu().numpy(), status=sts[0], sb=sb)


def _assert_same_bits(a, b, what):
    np.testing.assert_array_equal(a["status"], b["status"])
    ok = a["status"] == 0     # (a stamp that raised has no sums: its rows are not written)
    for k in ("ll", "fd", "im", "s2"):
        x, y = a[k], b[k]
        if k in ("ll", "s2"):
            x, y = np.ascontiguousarray(x[ok]), np.ascontiguousarray(y[ok])
        assert np.array_equal(x.view(np.int64), y.view(np.int64)), (what, k)


def _assert_pixels(got, ref, scale, msg):
    np.testing.assert_allclose(got, ref, rtol=PIX_RTOL, atol=PIX_RTOL * scale, err_msg=msg)
    big = np.abs(ref) > 1e-3 * scale
    if big.any():
        np.testing.assert_allclose(got[big], ref[big], rtol=FUSED_ELEM_RTOL, atol=0, err_msg=msg)


def _assert_fused_is_exact(f, x, imgs, wts, ok=None):
    """the fused default against the exact kernels, stamp by stamp"""
    sb = f["sb"]
    np.testing.assert_array_equal(f["status"], x["status"])
    koff = sb.kept_offsets()
    for i in range(sb.n):
        if ok is not None and not ok[i]:
            continue
        a, b = int(sb.pix_off[i]), int(sb.pix_off[i] + sb.npix[i])
        mscale = max(np.abs(x["im"][a:b]).max(), 1e-300)
        _assert_pixels(f["im"][a:b], x["im"][a:b], mscale, "render %d" % i)
        ka, kb = int(koff[i]), int(koff[i] + sb.npix_kept[i])
        rfd = x["fd"][ka:kb]
        _assert_pixels(f["fd"][ka:kb], rfd,
                       mscale * np.sqrt(max(wts[i].max(), 0.0)) + np.abs(rfd).max(), "fdiff %d" % i)
        assert f["ll"][i, 3] == x["ll"][i, 3]
        np.testing.assert_allclose(f["ll"][i, 0], x["ll"][i, 0], rtol=SUM_RTOL, atol=0)
        np.testing.assert_allclose(f["ll"][i, 2], x["ll"][i, 2], rtol=SUM_RTOL, atol=0)
        # s2n_numer = sum(val * model * ivar) has mixed signs: sum|terms| bounds it
        wk = np.where(wts[i] > 0, wts[i], 0.0)
        aa = float((imgs[i] ** 2 * wk).sum())
        assert abs(f["ll"][i, 1] - x["ll"][i, 1]) <= SUM_RTOL * np.sqrt(aa * x["ll"][i, 2]) + 1e-300
        np.testing.assert_allclose(f["s2"][i], x["s2"][i], rtol=SUM_RTOL, atol=0)


def _union_box(gm, j):
    """union over a stamp's gaussians of the pixel ranges where chi2 < 25 is possible:
    |r - cen_r| <= 5 sigma_r, |c - cen_c| <= 5 sigma_c (the covariance mapped to pixels)"""
    a, b, c, d = j[2], j[3], j[4], j[5]
    det = a * d - b * c
    rr, ru, cr, cu = d / det, -b / det, -c / det, a / det
    var_r = rr * rr * gm["irr"] + 2 * rr * ru * gm["irc"] + ru * ru * gm["icc"]
    var_c = cr * cr * gm["irr"] + 2 * cr * cu * gm["irc"] + cu * cu * gm["icc"]
    cen_r = j[0] + rr * gm["row"] + ru * gm["col"]
    cen_c = j[1] + cr * gm["row"] + cu * gm["col"]
    hr, hc = 5 * np.sqrt(var_r), 5 * np.sqrt(var_c)
    return ((cen_r - hr).min(), (cen_r + hr).max(), (cen_c - hc).min(), (cen_c + hc).max())


def _check_all(imgs, wts, jac, gmh, ngs=None, ok=None, base=None):
    f = _run(imgs, wts, jac, gmh, ngs, base=base)
    _assert_same_bits(f, _run(imgs, wts, jac, gmh, ngs, base=base, no_skip=True), "no_skip")
    _assert_same_bits(f, _run(imgs, wts, jac, gmh, ngs, base=base, tracked=True), "tracked")
    x = _run(imgs, wts, jac, gmh, ngs, base=base, exact=True)
    _assert_fused_is_exact(f, x, imgs, wts, ok)
    return f


@pytest.mark.parametrize("same_centre", [True, False], ids=["shared_centre", "own_centres"])
@pytest.mark.parametrize("ng", NGAUSS)
def test_shapes_and_mixture_sizes(ng, same_centre):
    """every shape (one tile with only look-ahead behind it, a row wrap after one
    tile or none, ntx != nty, ragged) at every mixture size: both sides of the
    unrolled / generic switch (8 | 9, and shared centre | own centres), the chunked
    ballot, ng > 32"""
    rng = np.random.RandomState(100 * ng + same_centre)
    shapes = ALL_SHAPES + [(48, 48)]
    imgs, wts = _data(rng, shapes)
    jac = _jacobians(rng, shapes)
    gmh = _mixtures(rng, shapes, ng, same_centre)
    f = _check_all(imgs, wts, jac, gmh)
    assert np.all(f["status"] == 0)
    assert np.abs(f["im"]).max() > 0


def test_mixed_ngauss_empty_mixture_and_failing_norms():
    """one batch whose stamps have 0 .. 8 gaussians (the unrolled kernels) and one
    with up to 33 (the generic ones); a stamp whose norms fail reports its status
    and leaves the others alone"""
    rng = np.random.RandomState(77)
    shapes = [(48, 48), (8, 8), (24, 40), (13, 21), (16, 8), (48, 48), (40, 24), (8, 16)]
    imgs, wts = _data(rng, shapes)
    jac = _jacobians(rng, shapes)
    for ngs in ([6, 0, 8, 3, 1, 2, 7, 5], [6, 0, 33, 3, 9, 16, 1, 8]):
        gmh = _mixtures(rng, shapes, max(ngs), True)
        gmh["det"][5, 1] = 1e-250      # stamp 5 raises (det too low)
        f = _check_all(imgs, wts, jac, gmh, ngs=ngs, ok=[i != 5 for i in range(len(shapes))])
        want = [0] * len(shapes)
        want[5] = _lib.ERR_DET_TOO_LOW
        assert list(f["status"]) == want
        # an empty mixture: model == 0
        sb = f["sb"]
        a, b = int(sb.pix_off[1]), int(sb.pix_off[1] + sb.npix[1])
        assert np.all(f["im"][a:b] == 0.0)
        np.testing.assert_allclose(f["ll"][1, 0], -0.5 * (imgs[1] ** 2 * wts[1]).sum(), rtol=1e-13)
        # the same stamps alone give the same bits: nothing leaks between stamps
        keep = [i for i in range(len(shapes)) if i != 5]
        g = _run([imgs[i] for i in keep], [wts[i] for i in keep], jac[keep], gmh[keep],
                 ngs=[ngs[i] for i in keep])
        assert np.array_equal(g["ll"].view(np.int64), f["ll"][keep].view(np.int64))


@pytest.mark.parametrize("ng", [6, 9])
def test_centres_outside_and_in_corners_unreached_lines_keep_their_bits(ng):
    """a centre 10 pixels outside the stamp (the render's line skip trims whole
    bands, so its tile walk starts past tile 0), in a corner, far away (nothing
    reached); the render into an existing image leaves every pixel of a line no
    gaussian reaches bit-identical -- NaN payloads and -0.0 included"""
    rng = np.random.RandomState(500 + ng)
    shapes = [(48, 48)] * 6 + [(12, 48), (8, 32), (47, 50), (40, 24)]
    n = len(shapes)
    imgs, wts = _data(rng, shapes)
    jac = _jacobians(rng, shapes, sheared=False)
    gmh = _mixtures(rng, shapes, ng, True, cen_pix=0.5, sigma_pix=(0.6, 1.6))
    cens = [(34.0, 0.0), (-34.0, 3.0), (23.0, 23.0), (-23.5, -23.5), (0.0, 34.0), (400.0, 0.0),
            (16.0, 0.0), (0.0, -26.0), (33.5, -10.0), (-30.0, 0.0)]
    for i, (dr, dc) in enumerate(cens):
        gmh["row"][i] += dr * jac[i, 2]
        gmh["col"][i] += dc * jac[i, 5]
    tot = sum(a * b for a, b in shapes)
    base = rng.normal(size=tot)
    f = _check_all(imgs, wts, jac, gmh, base=base.copy())
    assert np.all(f["status"] == 0)
    # values whose bits an `x + 0.0` would change
    base[::7] = -0.0
    base.view(np.int64)[3::11] = 0x7FF8000000000123
    f = _run(imgs, wts, jac, gmh, base=base.copy())
    sb = f["sb"]
    nlines = 0
    for i, (nr, nc) in enumerate(shapes):
        a = int(sb.pix_off[i])
        got = f["im"][a:a + nr * nc].reshape(nr, nc)
        was = base[a:a + nr * nc].reshape(nr, nc)
        rmin, rmax, cmin, cmax = _union_box(gmh[i], jac[i])
        for r in range(nr):
            for c0 in range(0, nc, 16):
                # a line (16 pixels of one row) more than a pixel away from the union of
                # the chi2 < 25 boxes: certainly unreached, whatever the boxes' rounding
                if r < rmin - 1 or r > rmax + 1 or c0 + 15 < cmin - 1 or c0 > cmax + 1:
                    assert np.array_equal(got[r, c0:c0 + 16].view(np.int64),
                                          was[r, c0:c0 + 16].view(np.int64)), (i, r, c0)
                    nlines += 1
    assert nlines > 400     # of 814: most of these stamps is out of reach
    assert np.array_equal(f["im"][int(sb.pix_off[5]):int(sb.pix_off[5]) + 2304].view(np.int64),
                          base[int(sb.pix_off[5]):int(sb.pix_off[5]) + 2304].view(np.int64))


@pytest.mark.parametrize("ng", [2, 16])
def test_masked_and_uniform_weight_stamps_in_one_batch(ng):
    """uniform-weight stamps (ierr not streamed), real weight maps and a stamp
    with zero weights (fill_fdiff's ranks) side by side"""
    rng = np.random.RandomState(900 + ng)
    shapes = [(48, 48), (24, 40), (16, 8), (13, 21), (12, 48), (48, 48), (8, 8)]
    imgs, wts = _data(rng, shapes, weights="mixed")
    wts[1][rng.uniform(size=shapes[1]) < 0.2] = 0.0
    wts[4][:, 5:9] = 0.0
    wts[5][7, :] = -1.0
    jac = _jacobians(rng, shapes)
    gmh = _mixtures(rng, shapes, ng, True)
    f = _check_all(imgs, wts, jac, gmh)
    assert np.all(f["status"] == 0)
    sb = f["sb"]
    assert sb.any_masked and sb.any_uniform
    assert list(sb.npix_kept) == [int((w > 0).sum()) for w in wts]
    # and the same batch with every weight map uniform / none uniform
    for kind in ("uniform", "real"):
        imgs2, wts2 = _data(rng, shapes, weights=kind)
        f2 = _check_all(imgs2, wts2, jac, gmh)
        assert f2["sb"].any_uniform == (kind == "uniform")
