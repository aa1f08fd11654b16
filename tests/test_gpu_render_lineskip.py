"""
GPU tests of the fused render's line skip: image lines
(16 pixels of one row, 128 bytes) that the union of the stamp's chi2 < 25 boxes
does not reach are neither read nor written.

  * render == render(no_skip=True) bit for bit (NGMIX_BATCH_NO_SKIP makes every
    box full, so that build moves every byte), into zeros and into random
    non-zero images, over the shapes and mixtures that take every path of the
    kernel;
  * unreached lines keep their bits, whatever they hold (-0.0, NaN payloads);
  * an overwriting render still writes every pixel;
  * the compiler-tracked load path equals the hand-counted one.
"""
import numpy as np
import pytest

from ngmix_amd import _lib

pytestmark = pytest.mark.gpu

SCALE = 0.263
LINE = 16  # pixels per 128-byte line = columns of the render's 4x16 tile


def _gauss_records(p, row, col, irr, irc, icc):
    """(n, ngauss) gauss2d records with norms unset"""
    gm = np.zeros(np.shape(p), dtype=_lib.GAUSS2D_DTYPE)
    gm["p"], gm["row"], gm["col"] = p, row, col
    gm["irr"], gm["irc"], gm["icc"] = irr, irc, icc
    gm["det"] = gm["irr"] * gm["icc"] - gm["irc"] ** 2
    return gm


def _small_mixtures(rng, n, ng, sigma_pix=(0.8, 2.5), cen_pix=4.0, same_centre=True):
    """mixtures a few pixels wide (sigma in pixels), centres within cen_pix
    pixels of the jacobian centre"""
    sig = rng.uniform(sigma_pix[0], sigma_pix[1], size=(n, ng)) * SCALE
    T = 2.0 * sig ** 2
    e1 = rng.uniform(-0.4, 0.4, size=(n, ng))
    e2 = rng.uniform(-0.4, 0.4, size=(n, ng))
    shape = (n, 1) if same_centre else (n, ng)
    row = np.broadcast_to(rng.uniform(-cen_pix, cen_pix, size=shape) * SCALE, (n, ng))
    col = np.broadcast_to(rng.uniform(-cen_pix, cen_pix, size=shape) * SCALE, (n, ng))
    return _gauss_records(rng.uniform(0.5, 5.0, size=(n, ng)), row, col,
                          T / 2 * (1 - e1), T / 2 * e2, T / 2 * (1 + e1))


def _geometry(shapes, offdiag=True):
    import torch
    from ngmix_amd.batch import StampBatch
    n = len(shapes)
    nrow = np.array([sh[0] for sh in shapes])
    ncol = np.array([sh[1] for sh in shapes])
    pix_off = np.concatenate([[0], np.cumsum(nrow * ncol)[:-1]]).astype(np.int64)
    jac = np.zeros((n, 8))
    for i, sh in enumerate(shapes):
        if offdiag:
            det = 0.263 * 0.27 + 1e-4
            jac[i] = [(sh[0] - 1) / 2, (sh[1] - 1) / 2, 0.263, 0.01, -0.01, 0.27,
                      det, np.sqrt(det)]
        else:
            jac[i] = [(sh[0] - 1) / 2, (sh[1] - 1) / 2, SCALE, 0.0, 0.0, SCALE,
                      SCALE ** 2, SCALE]
    sb = StampBatch(None, None, torch.from_numpy(jac).cuda(), nrow, ncol, pix_off, True)
    return sb, jac


def _assert_skip_equals_noskip(sb, gmh, expect_status=None):
    """into zeros and into random non-zero values: bit for bit, same status"""
    import torch
    from ngmix_amd.batch import GMixBatch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    rnd = torch.randn(sb.total_pix, generator=gen, device="cuda", dtype=torch.float64)
    rnd = torch.where(rnd == 0.0, torch.ones_like(rnd), rnd) * 3.0
    for x in (torch.zeros_like(rnd), rnd):
        a, sa = sb.render(GMixBatch.from_numpy(gmh), image=x.clone())
        b, sn = sb.render(GMixBatch.from_numpy(gmh), image=x.clone(), no_skip=True)
        torch.cuda.synchronize()
        assert torch.equal(sa, sn)
        if expect_status is not None:
            assert list(sa.cpu().numpy()) == list(expect_status)
        assert torch.equal(a, b)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    return a, x


def test_c2_shaped_batch():
    """4096 stamps of 48x48, 'exp' (x) gaussian psf as the benchmark draws them"""
    import torch
    from ngmix_amd.batch import StampBatch, GMixBatch
    n = 4096
    rng = np.random.RandomState(1000)
    pars = np.zeros((n, 6))
    pars[:, 0:2] = rng.uniform(-0.5, 0.5, size=(n, 2)) * SCALE
    pars[:, 2:4] = np.clip(rng.normal(scale=0.1, size=(n, 2)), -0.45, 0.45)
    pars[:, 4] = rng.uniform(0.3, 1.5, size=n) * 1.02
    pars[:, 5] = rng.uniform(50.0, 500.0, size=n)
    gm0, _ = GMixBatch.from_pars(pars, "exp")
    psf, _ = GMixBatch.from_pars(np.tile([0.0, 0.0, 0.0, 0.0, 0.27, 1.0], (n, 1)), "gauss")
    gm, _ = gm0.convolve(psf)
    assert int(gm.set_norms().abs().sum()) == 0
    jac = np.array([23.5, 23.5, SCALE, 0.0, 0.0, SCALE, SCALE ** 2, SCALE])
    sb = StampBatch.from_images(torch.zeros((n, 48, 48), dtype=torch.float64, device="cuda"),
                                None, jac)
    out, x = _assert_skip_equals_noskip(sb, gm.to_numpy(), expect_status=[0] * n)
    assert not torch.equal(out, x)


@pytest.mark.parametrize("same_centre", [True, False])
def test_mixed_shapes_offdiagonal_jacobian(same_centre):
    """complete 4x16 tilings (the hand-counted load path) and ragged shapes (the
    compiler-tracked one), non-diagonal jacobian; gaussians of one centre (the
    shared-centre evaluator) and of different centres (the general one)"""
    rng = np.random.RandomState(31)
    shapes = [(48, 48)] * 5 + [(17, 23), (32, 32), (8, 16), (33, 9), (64, 64), (4, 16),
                               (5, 40), (48, 20)]
    sb, _ = _geometry(shapes)
    gmh = _small_mixtures(rng, len(shapes), 4, same_centre=same_centre)
    _assert_skip_equals_noskip(sb, gmh, expect_status=[0] * len(shapes))
    # and the wide, sometimes nasty mixtures of the other pixel tests
    gmw = _small_mixtures(rng, len(shapes), 4, sigma_pix=(0.3, 9.0), cen_pix=6.0,
                          same_centre=same_centre)
    gmw["p"][1, 0] = -0.7
    _assert_skip_equals_noskip(sb, gmw, expect_status=[0] * len(shapes))


def test_partly_and_wholly_outside_the_stamp():
    import torch
    rng = np.random.RandomState(32)
    shapes = [(48, 48)] * 6 + [(17, 23)] * 3
    sb, _ = _geometry(shapes, offdiag=False)
    n = len(shapes)
    gmh = _small_mixtures(rng, n, 3, cen_pix=1.0)
    # centres, in pixels from the stamp centre: over an edge, over a corner,
    # far outside (no pixel reached: the union is empty), and one gaussian of
    # the mixture outside while the others stay inside
    for i, (dr, dc) in enumerate([(-24.0, 0.0), (23.0, 25.0), (300.0, -5.0), (0.0, -400.0),
                                  (-1e6, 1e6), (22.0, -22.0), (9.0, 0.5), (40.0, 40.0),
                                  (-8.0, 11.0)]):
        gmh["row"][i] += dr * SCALE
        gmh["col"][i] += dc * SCALE
    gmh["row"][5, 1] += 200.0 * SCALE
    out, x = _assert_skip_equals_noskip(sb, gmh, expect_status=[0] * n)
    off = [int(o) for o in sb.pix_off]
    # wholly outside: the image as it was
    assert torch.equal(out[off[2]:off[5]].view(torch.int64), x[off[2]:off[5]].view(torch.int64))
    assert torch.equal(out[off[7]:off[8]].view(torch.int64), x[off[7]:off[8]].view(torch.int64))
    assert not torch.equal(out[off[0]:off[1]], x[off[0]:off[1]])
    assert not torch.equal(out[off[5]:off[6]], x[off[5]:off[6]])


def test_degenerate_gaussian_makes_the_union_full():
    """rho^2 >= 1 - 1e-6: gauss_pixel_box returns full_box() and every line of
    that stamp is reached, whatever the other gaussians' boxes are"""
    rng = np.random.RandomState(33)
    shapes = [(48, 48), (48, 48), (17, 23), (32, 32)]
    sb, _ = _geometry(shapes, offdiag=False)
    gmh = _small_mixtures(rng, len(shapes), 3, cen_pix=2.0)
    for i in (0, 2):
        s2 = (3.0 * SCALE) ** 2
        gmh["irr"][i, 1], gmh["icc"][i, 1] = s2, s2
        gmh["irc"][i, 1] = s2 * 0.9999996
        gmh["det"][i, 1] = gmh["irr"][i, 1] * gmh["icc"][i, 1] - gmh["irc"][i, 1] ** 2
    _assert_skip_equals_noskip(sb, gmh, expect_status=[0] * len(shapes))


def test_empty_mixture_and_raising_stamp_leave_the_image_alone():
    import torch
    from ngmix_amd.batch import GMixBatch
    shapes = [(48, 48), (48, 48), (17, 23)]
    sb, _ = _geometry(shapes, offdiag=False)
    x = torch.arange(sb.total_pix, dtype=torch.float64, device="cuda") - 100.5
    # ngauss = 0
    for no_skip in (False, True):
        im, st = sb.render(GMixBatch.empty(len(shapes), 0), image=x.clone(), no_skip=no_skip)
        assert int(st.abs().sum()) == 0
        assert torch.equal(im.view(torch.int64), x.view(torch.int64))
    # a stamp that raises: its status, and its image untouched
    rng = np.random.RandomState(34)
    gmh = _small_mixtures(rng, len(shapes), 3)
    gmh["det"][1, 2] = 1e-250
    expect = [0, _lib.ERR_DET_TOO_LOW, 0]
    _assert_skip_equals_noskip(sb, gmh, expect_status=expect)
    im, st = sb.render(GMixBatch.from_numpy(gmh), image=x.clone())
    torch.cuda.synchronize()
    assert list(st.cpu().numpy()) == expect
    a, b = int(sb.pix_off[1]), int(sb.pix_off[2])
    assert torch.equal(im[a:b].view(torch.int64), x[a:b].view(torch.int64))
    assert not torch.equal(im[:a], x[:a])


# ------------------------------------------------------ unreached lines: bits

def _cpu_union_boxes(gmh, jac):
    """gauss_pixel_box (csrc/device_utils.hpp) and the union of the boxes per
    stamp, in numpy from the device's own drr / drc / dcc; also the smallest
    distance of any box edge to an integer (the kernel's rcp / rsq arithmetic
    agrees with IEEE's to ~1e-10: a margin of 1e-6 makes the integer boxes equal)"""
    n, ng = gmh.shape
    boxes = np.zeros((n, 4), dtype=np.int64)
    margin = np.inf
    for i in range(n):
        a, b, c, d = jac[i, 2], jac[i, 3], jac[i, 4], jac[i, 5]
        det = a * d - b * c
        rr, ru, cr, cu = d / det, -b / det, -c / det, a / det
        rmin = cmin = 1 << 30
        rmax = cmax = -(1 << 30)
        for g in gmh[i]:
            dcc, drr, drc = g["dcc"], g["drr"], g["drc"]
            detq = dcc * drr - drc * drc
            assert dcc > 0 and drr > 0 and detq > 0 and drc * drc < (1 - 1e-6) * dcc * drr
            var_v, var_u, cov = drr / detq, dcc / detq, drc / detq
            var_r = rr * rr * var_v + 2 * rr * ru * cov + ru * ru * var_u
            var_c = cr * cr * var_v + 2 * cr * cu * cov + cu * cu * var_u
            cen_r = jac[i, 0] + (rr * g["row"] + ru * g["col"])
            cen_c = jac[i, 1] + (cr * g["row"] + cu * g["col"])
            hr = 5 * np.sqrt(var_r) * (1 + 1e-6) + 1e-6
            hc = 5 * np.sqrt(var_c) * (1 + 1e-6) + 1e-6
            edges = np.array([cen_r - hr, cen_r + hr, cen_c - hc, cen_c + hc])
            margin = min(margin, np.abs(edges - np.round(edges)).min())
            r0, r1 = int(np.ceil(edges[0])), int(np.floor(edges[1]))
            c0, c1 = int(np.ceil(edges[2])), int(np.floor(edges[3]))
            if r0 <= r1 and c0 <= c1:
                rmin, rmax = min(rmin, r0), max(rmax, r1)
                cmin, cmax = min(cmin, c0), max(cmax, c1)
        boxes[i] = [rmin, rmax, cmin, cmax]
    return boxes, margin


# what an `image += 0.0` would not leave alone, and what it would
_EXOTIC = np.array([0x8000000000000000,   # -0.0
                    0x7FF0000000ABCDEF,   # a signalling NaN with a payload
                    0x7FF8000000123456,   # a quiet NaN with a payload
                    0xFFF0000000000000,   # -inf
                    0xDEADBEEFCAFEF00D,   # finite, recognisable
                    0x0000000000000000], dtype=np.uint64).view(np.int64)


@pytest.mark.parametrize("shapes", [[(48, 48)] * 24 + [(64, 64)] * 4 + [(32, 32)] * 4,
                                    [(17, 23), (33, 9), (24, 16), (40, 50), (21, 70), (48, 20),
                                     (19, 40), (30, 30)] * 3])
def test_unreached_lines_keep_their_bits(shapes):
    """every stamp, no exception: the lines outside the union of the boxes
    (computed here on the CPU) hold the bits they held, -0.0 and NaN payloads
    included; pixels of reached lines outside the union box got + 0.0, which
    leaves a non-zero finite value's bits alone too"""
    import torch
    from ngmix_amd.batch import GMixBatch
    rng = np.random.RandomState(35)
    n = len(shapes)
    sb, jac = _geometry(shapes)
    gmh = _small_mixtures(rng, n, 3, sigma_pix=(0.5, 0.9), cen_pix=1.5)
    # the first stamps: nothing of the mixture on the stamp (an empty union)
    gmh["row"][0] += 500.0 * SCALE
    gm = GMixBatch.from_numpy(gmh)
    assert int(gm.set_norms().abs().sum()) == 0
    boxes, margin = _cpu_union_boxes(gm.to_numpy(), jac)
    assert margin > 1e-6, "a box edge on an integer: draw other mixtures"

    before = np.zeros(sb.total_pix, dtype=np.int64)
    unreached = np.zeros(sb.total_pix, dtype=bool)
    outside = np.zeros(sb.total_pix, dtype=bool)
    for i, (nr, nc) in enumerate(shapes):
        rmin, rmax, cmin, cmax = boxes[i]
        rows, cols = np.arange(nr)[:, None], np.arange(nc)[None, :]
        c0 = (cols // LINE) * LINE   # first column of the pixel's line
        reached = (rows >= rmin) & (rows <= rmax) & (c0 <= cmax) & (c0 + LINE - 1 >= cmin)
        inbox = (rows >= rmin) & (rows <= rmax) & (cols >= cmin) & (cols <= cmax)
        assert not reached.all(), "stamp %d has no unreached line" % i
        assert i == 0 or inbox.any()
        k = np.arange(nr * nc).reshape(nr, nc)
        fill = np.where(reached, (1.0 + (k + 1) * 2.0 ** -30).view(np.int64),
                        _EXOTIC[k % len(_EXOTIC)])
        sl = slice(int(sb.pix_off[i]), int(sb.pix_off[i]) + nr * nc)
        before[sl] = fill.reshape(-1)
        unreached[sl] = ~reached.reshape(-1)
        outside[sl] = ~inbox.reshape(-1)

    x = torch.from_numpy(before).cuda().view(torch.float64)
    im, st = sb.render(gm, image=x)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    after = im.view(torch.int64).cpu().numpy()
    assert unreached.sum() > 0 and (outside & ~unreached).sum() > 0
    np.testing.assert_array_equal(after[unreached], before[unreached])
    np.testing.assert_array_equal(after[outside], before[outside])
    # ... and the render did happen
    assert np.any(after[~outside] != before[~outside])
    for i in range(1, n):
        sl = slice(int(sb.pix_off[i]), int(sb.pix_off[i]) + shapes[i][0] * shapes[i][1])
        assert np.any(after[sl] != before[sl])


def test_overwrite_still_writes_every_pixel():
    """a fresh render (NGMIX_BATCH_RENDER_OVERWRITE) of small mixtures over a
    poisoned allocator block: all finite, bit for bit the render into zeros"""
    import torch
    from ngmix_amd.batch import GMixBatch
    rng = np.random.RandomState(36)
    shapes = [(48, 48)] * 6 + [(17, 23), (32, 32), (8, 16), (33, 9), (64, 64)]
    sb, _ = _geometry(shapes)
    gmh = _small_mixtures(rng, len(shapes), 3, sigma_pix=(0.6, 1.5), cen_pix=3.0)
    gmh["row"][2] += 400.0 * SCALE   # an empty union
    zeros = torch.zeros(sb.total_pix, dtype=torch.float64, device="cuda")
    a, sa = sb.render(GMixBatch.from_numpy(gmh), image=zeros)
    torch.cuda.synchronize()
    junk = torch.full((sb.total_pix,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    del junk
    b, sbt = sb.render(GMixBatch.from_numpy(gmh))
    torch.cuda.synchronize()
    assert int(sa.abs().sum()) == 0 and int(sbt.abs().sum()) == 0
    assert bool(torch.isfinite(b).all())
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    off = sb.pix_off
    assert float(b[off[2]:off[3]].abs().max()) == 0.0
    assert float(b[off[0]:off[1]].abs().max()) > 0.0


def test_tracked_equals_untracked_loads():
    """render into a non-zero image: the compiler-tracked load path
    (NGMIX_BATCH_TRACKED_LOADS) equals the hand-counted one bit for bit"""
    import torch
    from ngmix_amd.batch import GMixBatch
    rng = np.random.RandomState(37)
    shapes = [(48, 48)] * 8 + [(64, 64), (32, 32), (16, 16)]
    gmh = np.concatenate([_small_mixtures(rng, 6, 4), _small_mixtures(
        rng, len(shapes) - 6, 4, sigma_pix=(1.0, 8.0), same_centre=False)])
    res = []
    for tracked in (False, True):
        sb, _ = _geometry(shapes)
        sb.tracked_loads = tracked
        x = torch.randn(sb.total_pix, generator=torch.Generator(device="cuda").manual_seed(11),
                        device="cuda", dtype=torch.float64) + 5.0
        im, st = sb.render(GMixBatch.from_numpy(gmh), image=x)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0
        res.append(im)
    assert torch.equal(res[0].view(torch.int64), res[1].view(torch.int64))
