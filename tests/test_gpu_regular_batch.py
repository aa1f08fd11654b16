"""
Regular batches (NGMIX_BATCH_REGULAR): every stamp one shape, one ngauss, one
flag word, pixels packed, mixtures stamp-major, nothing masked.  The fused
loglike / render / fill_fdiff / model_s2n_sum kernels then run instantiations
that read no stamp record and ask for the jacobian, the gaussian records and
the first tiles at once.

  * equality: every output, the status and the written-back mixtures of the
    regular path are array_equal to the same StampBatch with
    general_kernels = True (the bit cleared: the kernels that read the stamp
    records), over the shapes that reach each branch of the tile loop, the
    unrolled and generic pair loops, one and several staging rounds, uniform
    weights and weight maps, norms set and not set on entry, a failing mixture;
  * dispatch: ngmix_launch_census_regular counts the launches that took the
    path; batches that are not regular must not, with unchanged results;
  * the fact: StampBatch.regular_bits from host arrays (no GPU), and
    ngmix_batch_create / ngmix_batch_upload for the C API.
"""
import ctypes

import numpy as np
import pytest

from ngmix_amd import _lib

SCALE = 0.263
REG = _lib.BATCH_REGULAR
SHIFT = _lib.BATCH_REGULAR_STAMP_FLAGS_SHIFT
IZW = _lib.STAMP_IGNORE_ZERO_WEIGHT
UNI = _lib.STAMP_UNIFORM_IERR


# ------------------------------------------------------------------ builders
def jacobians(rng, n, nrow, ncol):
    """random WCS with sub-pixel centres; stamp 1 rotated, stamp 2 flipped (det < 0)"""
    jac = np.zeros((n, 8))
    for i in range(n):
        a = SCALE * (1.0 + 0.05 * rng.uniform(-1, 1))
        m = np.array([[a, 0.02 * rng.uniform(-1, 1)], [0.02 * rng.uniform(-1, 1), a]])
        if i == 1:
            c, s = np.cos(0.6), np.sin(0.6)
            m = np.array([[c, -s], [s, c]]) * a
        if i == 2:
            m[1] = -m[1]
        det = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
        jac[i] = [(nrow - 1) / 2 + rng.uniform(-0.5, 0.5), (ncol - 1) / 2 + rng.uniform(-0.5, 0.5),
                  m[0, 0], m[0, 1], m[1, 0], m[1, 1], det, np.sqrt(abs(det))]
    return jac


def mixtures_host(rng, n, ng, off_centre):
    """(n, ng) gauss2d records with norm_set == 0; one centre per stamp, the last
    gaussian moved off it when off_centre"""
    g = np.zeros((n, ng), dtype=_lib.GAUSS2D_DTYPE)
    cen = rng.uniform(-0.5, 0.5, size=(n, 1, 2)) * SCALE
    g["p"] = rng.uniform(0.2, 2.0, size=(n, ng))
    g["row"] = cen[:, :, 0]
    g["col"] = cen[:, :, 1]
    if off_centre:
        g["row"][:, -1] += 0.31
        g["col"][:, -1] -= 0.17
    g["irr"] = rng.uniform(0.04, 0.6, size=(n, ng))
    g["icc"] = rng.uniform(0.04, 0.6, size=(n, ng))
    g["irc"] = rng.uniform(-0.5, 0.5, size=(n, ng)) * np.sqrt(g["irr"] * g["icc"])
    g["det"] = g["irr"] * g["icc"] - g["irc"] ** 2
    return g


def stamps(rng, n, nrow, ncol, weights, izw=True, gap_at=None):
    """weights: 'uniform' (one value per stamp) or 'maps'"""
    import torch
    from ngmix_amd.batch import StampBatch
    npix = nrow * ncol
    off = np.arange(n, dtype=np.int64) * npix
    if gap_at is not None:
        off[gap_at:] += 8
    total = int(off[-1] + npix)
    val = rng.normal(size=total)
    ierr = np.ones(total)
    for i in range(n):
        ierr[off[i]:off[i] + npix] = (0.5 + 0.01 * i) if weights == "uniform" else \
            rng.uniform(0.5, 2.0, size=npix)
    return StampBatch(torch.from_numpy(val).cuda(), torch.from_numpy(ierr).cuda(),
                      torch.from_numpy(jacobians(rng, n, nrow, ncol)).cuda(),
                      np.full(n, nrow), np.full(n, ncol), off, izw)


def run_all(sb, gmh, preset, image0, no_skip=False):
    """every fused pixel pass of one batch: {name: numpy array}
    (no_skip: the diagnostic that evaluates every pair; model_s2n_sum has none)"""
    import torch
    from ngmix_amd.batch import GMixBatch
    res = {}

    def fresh():
        gm = GMixBatch.from_numpy(gmh)
        if preset:
            gm.set_norms()
        return gm

    def keep(name, out, status, gm):
        res[name] = out.cpu().numpy()
        res[name + ".status"] = status.cpu().numpy()
        res[name + ".gm"] = gm.data.cpu().numpy().view(np.int64)

    # (a stamp that fails leaves its output record as it was: zeros here)
    gm = fresh()
    keep("loglike", *sb.loglike(gm, out=torch.zeros((sb.n, 4), dtype=torch.float64,
                                                    device="cuda"),
                                 no_skip=no_skip), gm)
    gm = fresh()
    keep("render+", *sb.render(gm, image=image0.clone(), no_skip=no_skip), gm)
    gm = fresh()
    if sb._packed():
        keep("render=", *sb.render(gm, no_skip=no_skip), gm)
    else:
        # (render(image=None) sizes its image for packed stamps)
        keep("render=", *sb.render(gm, image=torch.zeros_like(image0), no_skip=no_skip), gm)
    gm = fresh()
    keep("fdiff", *sb.fill_fdiff(gm, no_skip=no_skip), gm)
    gm = fresh()
    keep("s2n", *sb.model_s2n_sum(gm, out=torch.zeros(sb.n, dtype=torch.float64,
                                                     device="cuda")), gm)
    torch.cuda.synchronize()
    return res


def both_paths(sb, gmh, preset, expect_regular=True, seed=5, no_skip=False):
    """the same calls on the regular and on the general kernels; returns the
    regular path's results after asserting that they are the general path's"""
    import torch
    # (the image spans the stamps where they lie, gaps included)
    extent = int((sb.pix_off + sb.npix).max())
    image0 = torch.from_numpy(np.random.RandomState(seed).normal(size=extent)).cuda()
    assert not sb.general_kernels
    _lib.regular_launches(reset=True)
    got = run_all(sb, gmh, preset, image0, no_skip)
    assert _lib.regular_launches(reset=True) == (5 if expect_regular else 0)
    sb.general_kernels = True
    try:
        want = run_all(sb, gmh, preset, image0, no_skip)
        assert _lib.regular_launches(reset=True) == 0
    finally:
        sb.general_kernels = False
    assert sorted(got) == sorted(want)
    for name in want:
        # (bit patterns: NaNs and signed zeros count)
        a, b = got[name], want[name]
        if a.dtype == np.float64:
            a, b = a.view(np.int64), b.view(np.int64)
        assert np.array_equal(a, b), name
    return got


# ------------------------------------------------------------------ equality
# 16x16: complete tiles for 8x8 and 4x16, exactly the four look-ahead sets;
# 8x16: fewer tiles than register sets (sentinel loads); 24x16: a group of four
# and a remainder of two; 10x13: ragged, the compiler-tracked path
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(16, 16), (8, 16), (24, 16), (10, 13)])
@pytest.mark.parametrize("weights", ["uniform", "maps"])
def test_regular_equals_general(shape, weights):
    rng = np.random.RandomState(100 + shape[0] + (7 if weights == "maps" else 0))
    n = 64
    sb = stamps(rng, n, shape[0], shape[1], weights)
    word = IZW | (UNI if weights == "uniform" else 0)
    for ng in (1, 6, 8, 9, 16):
        assert sb.regular_bits(ng) == REG | (word << SHIFT)
        for off_centre in (False, True):
            gmh = mixtures_host(rng, n, ng, off_centre)
            # (only the kernels of mixtures of at most 8 gaussians have a regular
            # form: larger regular batches run the general kernels)
            got = both_paths(sb, gmh, preset=True, expect_regular=ng <= 8)
            assert not got["loglike.status"].any()
            if ng in (6, 9):
                # norm_set == 0 on entry: the norms are set and written back
                got = both_paths(sb, gmh, preset=False, expect_regular=ng <= 8)
                assert not got["loglike.status"].any()
                back = got["loglike.gm"].view(np.float64).reshape(-1).view(_lib.GAUSS2D_DTYPE)
                assert np.all(back["norm_set"] == 1)


@pytest.mark.gpu
def test_regular_equals_general_48x48_and_many_rounds():
    rng = np.random.RandomState(48)
    sb = stamps(rng, 64, 48, 48, "uniform")
    both_paths(sb, mixtures_host(rng, 64, 6, False), preset=True)
    both_paths(sb, mixtures_host(rng, 64, 6, True), preset=False)
    # more than one staging round of 64 gaussians
    sb = stamps(rng, 64, 16, 16, "maps")
    both_paths(sb, mixtures_host(rng, 64, 70, True), preset=True, expect_regular=False)
    both_paths(sb, mixtures_host(rng, 64, 70, False), preset=False, expect_regular=False)
    # the no-skip diagnostic (every gaussian staged with the full box) and the
    # compiler-tracked load path stay regular
    both_paths(sb, mixtures_host(rng, 64, 6, False), preset=True, no_skip=True)
    both_paths(sb, mixtures_host(rng, 64, 8, True), preset=False, no_skip=True)
    sb.tracked_loads = True
    both_paths(sb, mixtures_host(rng, 64, 6, False), preset=True)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(16, 16), (10, 13)])
def test_failing_mixture(shape):
    """the third gaussian of stamp 5 has det <= 0: the same status, the same
    partial write-back (gaussians 0 and 1 normalised, the rest untouched), and
    a zero-filled stamp from the overwriting render"""
    rng = np.random.RandomState(9)
    n, ng = 64, 6
    sb = stamps(rng, n, shape[0], shape[1], "uniform")
    gmh = mixtures_host(rng, n, ng, False)
    gmh["irc"][5, 2] = 2.0 * np.sqrt(gmh["irr"][5, 2] * gmh["icc"][5, 2])
    gmh["det"][5, 2] = gmh["irr"][5, 2] * gmh["icc"][5, 2] - gmh["irc"][5, 2] ** 2
    got = both_paths(sb, gmh, preset=False)
    for name in ("loglike", "render+", "render=", "fdiff", "s2n"):
        status = got[name + ".status"]
        assert status[5] != 0 and not np.delete(status, 5).any(), name
        back = got[name + ".gm"].view(np.float64).reshape(-1).view(
            _lib.GAUSS2D_DTYPE).reshape(n, ng)
        assert list(back["norm_set"][5]) == [1, 1, 0, 0, 0, 0]
        assert np.all(np.delete(back["norm_set"], 5, axis=0) == 1)
    npix = shape[0] * shape[1]
    assert not got["render="][5 * npix:6 * npix].any()
    assert got["render="][4 * npix:5 * npix].any()


# ------------------------------------------------------------------ dispatch
def _loglike_exact(sb, gmh):
    from ngmix_amd.batch import GMixBatch
    gm = GMixBatch.from_numpy(gmh)
    gm.set_norms()
    out, _ = sb.loglike(gm, exact=True)
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mixed shapes", "masked", "mixed weights", "gap"])
def test_batches_that_are_not_regular(kind):
    import torch
    from ngmix_amd.batch import StampBatch
    rng = np.random.RandomState(31)
    n, ng = 64, 6
    if kind == "mixed shapes":
        shapes = [(16, 16)] * (n - 1) + [(16, 24)]
        nrow = np.array([s[0] for s in shapes])
        ncol = np.array([s[1] for s in shapes])
        npix = nrow * ncol
        off = np.concatenate([[0], np.cumsum(npix)[:-1]]).astype(np.int64)
        jac = np.concatenate([jacobians(rng, n - 1, 16, 16), jacobians(rng, 1, 16, 24)])
        sb = StampBatch(torch.from_numpy(rng.normal(size=int(npix.sum()))).cuda(),
                        torch.from_numpy(rng.uniform(0.5, 2.0, size=int(npix.sum()))).cuda(),
                        torch.from_numpy(jac).cuda(), nrow, ncol, off, True)
    elif kind == "gap":
        sb = stamps(rng, n, 16, 16, "uniform", gap_at=17)
    else:
        sb = stamps(rng, n, 16, 16, "uniform")
        a = int(sb.pix_off[9])
        if kind == "masked":
            sb.ierr[a + 37] = 0.0
        else:
            sb.ierr[a:a + 256] = torch.from_numpy(rng.uniform(0.5, 2.0, size=256)).cuda()
        sb.rescan_weights()
    assert sb.regular_bits(ng) == 0
    gmh = mixtures_host(rng, n, ng, False)
    got = both_paths(sb, gmh, preset=True, expect_regular=False)
    assert not got["loglike.status"].any()
    np.testing.assert_allclose(got["loglike"][:, :3], _loglike_exact(sb, gmh)[:, :3], rtol=1e-10)


@pytest.mark.gpu
def test_per_stamp_ngauss_is_not_regular():
    """a ragged mixture layout through the C ABI: general kernels, and each
    stamp's record equal to that stamp evaluated on its own"""
    import torch
    from ngmix_amd.batch import GMixBatch
    rng = np.random.RandomState(77)
    n = 64
    sb = stamps(rng, n, 16, 16, "maps")
    ngs = np.where(np.arange(n) % 2 == 0, 6, 3)
    assert sb.regular_bits(ngs) == 0
    assert sb.regular_bits(np.full(n, 6)) == sb.regular_bits(6) != 0
    full = mixtures_host(rng, n, 6, False)
    flat = np.concatenate([full[i, :ngs[i]] for i in range(n)])
    gm = GMixBatch(torch.from_numpy(flat.view(np.float64).reshape(-1, 13).copy()).cuda(),
                   n, 6)
    b = sb._batch(ngs)
    assert not b.flags & REG
    out = torch.empty((n, 4), dtype=torch.float64, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    _lib.regular_launches(reset=True)
    _lib.check(_lib.lib().ngmix_loglike_batch(
        ctypes.byref(b), ctypes.c_void_p(gm.data.data_ptr()), ctypes.c_void_p(out.data_ptr()),
        ctypes.c_void_p(status.data_ptr()), None), "loglike")
    torch.cuda.synchronize()
    assert _lib.regular_launches(reset=True) == 0
    assert not status.cpu().numpy().any()
    for ng in (6, 3):
        pick = np.flatnonzero(ngs == ng)
        one, _ = sb.select(pick).loglike(GMixBatch.from_numpy(full[pick, :ng].copy()))
        assert np.array_equal(out.cpu().numpy()[pick], one.cpu().numpy())


@pytest.mark.gpu
def test_launcher_refuses_a_contradicted_bit():
    import torch
    from ngmix_amd.batch import GMixBatch
    rng = np.random.RandomState(2)
    sb = stamps(rng, 64, 16, 16, "uniform")
    gm = GMixBatch.from_numpy(mixtures_host(rng, 64, 6, False))
    out = torch.empty((64, 4), dtype=torch.float64, device="cuda")
    status = torch.empty(64, dtype=torch.int32, device="cuda")
    for field, value in (("any_masked", 1), ("max_npix", 255), ("max_nrow", 0)):
        b = sb._batch(6)
        assert b.flags & REG
        setattr(b, field, value)
        st = _lib.lib().ngmix_loglike_batch(
            ctypes.byref(b), ctypes.c_void_p(gm.data.data_ptr()), ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(status.data_ptr()), None)
        assert st == _lib.ERR_BAD_ARG, field


@pytest.mark.gpu
def test_cabi_store_sets_and_clears_the_bit():
    L = _lib.lib()
    rng = np.random.RandomState(4)
    n, ng, dim = 8, 3, 16
    nrow = np.full(n, dim, dtype=np.int32)
    ncol = np.full(n, dim, dtype=np.int32)
    jac = np.zeros(n, dtype=_lib.JACOBIAN_DTYPE)
    jac[:] = (7.5, 7.5, SCALE, 0.0, 0.0, SCALE, SCALE ** 2, SCALE)
    images = rng.normal(size=n * dim * dim)
    maps = rng.uniform(0.5, 2.0, size=n * dim * dim)

    def bits(pb, weights):
        _lib.check(L.ngmix_batch_upload(pb, _lib.ptr(images),
                                        None if weights is None else _lib.ptr(weights),
                                        _lib.ptr(jac), None), "upload")
        f = pb.contents.flags
        return f & REG, (f & _lib.BATCH_REGULAR_STAMP_FLAGS) >> SHIFT

    pb = ctypes.POINTER(_lib.Batch)()
    assert L.ngmix_batch_create(ctypes.byref(pb), n, _lib.ptr(nrow), _lib.ptr(ncol), ng, 1) == 0
    try:
        assert pb.contents.flags & REG == 0          # nothing uploaded yet
        assert bits(pb, maps) == (REG, IZW)
        assert bits(pb, None) == (REG, IZW | UNI)    # unit weights
        masked = maps.copy()
        masked[5 * dim * dim + 3] = 0.0
        assert bits(pb, masked) == (0, 0)
        mixed = maps.copy()
        mixed[:dim * dim] = 2.0                      # one uniform stamp among maps
        assert bits(pb, mixed) == (0, 0)
        assert bits(pb, maps) == (REG, IZW)          # ... and set again
    finally:
        assert L.ngmix_batch_free(pb) == 0
    # mixed shapes; no gaussians
    ncol2 = ncol.copy()
    ncol2[3] = 24
    for args in ((nrow, ncol2, ng), (nrow, ncol, 0)):
        pb = ctypes.POINTER(_lib.Batch)()
        assert L.ngmix_batch_create(ctypes.byref(pb), n, _lib.ptr(args[0]), _lib.ptr(args[1]),
                                    args[2], 0) == 0
        try:
            npix = int((args[0].astype(np.int64) * args[1]).sum())
            _lib.check(L.ngmix_batch_upload(pb, _lib.ptr(rng.normal(size=npix)),
                                            _lib.ptr(rng.uniform(0.5, 2.0, size=npix)),
                                            _lib.ptr(jac), None), "upload")
            assert pb.contents.flags & (REG | _lib.BATCH_REGULAR_STAMP_FLAGS) == 0
        finally:
            assert L.ngmix_batch_free(pb) == 0


# ------------------------------------------------------------------ the fact (no GPU)
class _HostTensor(object):
    """what StampBatch reads of a tensor when it is handed host facts"""

    def __init__(self, n):
        self.shape = (n, 8)
        self.device = "cpu"


def _host_batch(nrow, ncol, off, izw, kept=None, uniform=None):
    from ngmix_amd.batch import StampBatch
    n = len(nrow)
    npix = np.asarray(nrow, dtype=np.int64) * np.asarray(ncol)
    return StampBatch(None, _HostTensor(n), _HostTensor(n), nrow, ncol, off, izw,
                      npix_kept=npix if kept is None else kept,
                      uniform_ierr=np.zeros(n, dtype=bool) if uniform is None else uniform)


def test_stamp_batch_derives_the_bit(monkeypatch):
    from ngmix_amd.batch import StampBatch
    # (the device table itself is not needed to establish the fact)
    monkeypatch.setattr(StampBatch, "_make_table", lambda self, *a: object())
    n = 12
    dim = np.full(n, 16)
    off = np.arange(n, dtype=np.int64) * 256
    ok = _host_batch(dim, dim, off, True)
    assert ok.regular_bits(6) == REG | (IZW << SHIFT)
    assert ok.regular_bits(1) == REG | (IZW << SHIFT)
    assert ok.regular_bits(np.full(n, 6)) == REG | (IZW << SHIFT)
    assert ok.regular_bits(0) == 0
    assert ok.regular_bits(np.where(np.arange(n) == 4, 5, 6)) == 0
    assert _host_batch(dim, dim, off, False).regular_bits(6) == REG
    uni = np.ones(n, dtype=bool)
    assert _host_batch(dim, dim, off, True, uniform=uni).regular_bits(6) == \
        REG | ((IZW | UNI) << SHIFT)
    # mixed uniform and non-uniform weights; mixed ignore_zero_weight
    uni[3] = False
    assert _host_batch(dim, dim, off, True, uniform=uni).regular_bits(6) == 0
    assert _host_batch(dim, dim, off, np.arange(n) != 2).regular_bits(6) == 0
    # a masked stamp
    kept = np.full(n, 256)
    kept[7] = 255
    assert _host_batch(dim, dim, off, True, kept=kept).regular_bits(6) == 0
    # mixed shapes (packed all the same), a gap, another order
    ncol = dim.copy()
    ncol[-1] = 24
    assert _host_batch(dim, ncol, off, True).regular_bits(6) == 0
    gap = off.copy()
    gap[5:] += 8
    assert _host_batch(dim, dim, gap, True).regular_bits(6) == 0
    assert _host_batch(dim, dim, off[::-1].copy(), True).regular_bits(6) == 0


class _NoDevice(object):
    """stands in for the library where a builder converts the weights on the
    device: the fact under test comes from the host arrays alone"""

    @staticmethod
    def ngmix_weight_to_ierr_batch(*args):
        return 0


class _Here(object):
    def __init__(self, dev):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def test_builders_from_host_arrays_derive_the_bit(monkeypatch):
    """from_stacked / from_arrays count the kept pixels and find the uniform
    weight maps in the host weights; the bit follows from those"""
    import torch
    from ngmix_amd import batch as B
    monkeypatch.setattr(B, "_require_cuda", lambda device: torch.device("cpu"))
    monkeypatch.setattr(B, "_on_device", _Here)
    monkeypatch.setattr(B, "_stream", lambda: None)
    monkeypatch.setattr(B._lib, "lib", lambda: _NoDevice)
    rng = np.random.RandomState(6)
    n, dim = 6, 16
    jac = np.tile([7.5, 7.5, SCALE, 0.0, 0.0, SCALE, SCALE ** 2, SCALE], (n, 1))
    images = rng.normal(size=(n, dim, dim))
    maps = rng.uniform(0.5, 2.0, size=(n, dim, dim))
    flat = np.full((n, dim, dim), 0.25)
    masked = maps.copy()
    masked[2, 3, 4] = 0.0
    mixed = maps.copy()
    mixed[0] = 0.25

    def stacked(w):
        return B.StampBatch.from_stacked(images, w, jac)

    def arrays(w):
        return B.StampBatch.from_arrays(list(images), list(w), list(jac), np.ones(n, dtype=bool))

    for build in (stacked, arrays):
        assert build(maps).regular_bits(1) == REG | (IZW << SHIFT)
        assert build(maps).regular_bits(6) == REG | (IZW << SHIFT)
        assert build(flat).regular_bits(1) == REG | ((IZW | UNI) << SHIFT)
        assert build(masked).regular_bits(1) == 0
        assert build(mixed).regular_bits(1) == 0
    ragged = [images[0], images[1][:, :12]]
    sb = B.StampBatch.from_arrays(ragged, [np.ones_like(a) for a in ragged], list(jac[:2]),
                                  np.ones(2, dtype=bool))
    assert sb.regular_bits(1) == 0
