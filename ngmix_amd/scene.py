"""
Many objects and ONE frame: what the private-stamp kernels cannot do
(DESIGN.md section 3.15).

    frame, status = scene.render_scene((nrow, ncol), gm, jacobians)
    sb = scene.cut_stamps(frame, weight, r_lo, c_lo, 32, 32, jacobians)

render_scene draws N mixtures, each with a jacobian of its own (row0 / col0 in
frame pixel coordinates), into one image: a kernel finds every object's
chi2 < 25 pixel box and the frame tiles (4 rows x 16 columns) it covers, the
(tile, object) pairs are sorted on the device, and one wave per tile adds its
objects in ascending index.  The result has the bits of rendering the objects
one after the other into a frame-sized stamp with StampBatch.render(fast_exp=
True, exact=True); no atomics, so two runs give the same bits.  Only the fast
exp is built: its chi2 < 25 gate is what makes the binning exact.

cut_stamps cuts N (ragged) windows out of a frame and a weight frame that are
already on the device into a StampBatch, pixels outside the frame masked.

    sb, status = scene.cut_deblended_stamps(frame, weight, r_lo, c_lo, 32, 32, jacobians, gm)
    res = scene.fit_deblended(frame, weight, r_lo, c_lo, 32, 32, jacobians, guess, "exp", psf=psf)

cut_deblended_stamps is cut_stamps with the models of every object but the
window's owner subtracted, over the renderer's tile lists and in its order of
summation: bit for bit cut(frame) - cut(render_scene(all objects but the
owner)).  fit_deblended alternates it with the lock-step LM fitter: every object
is fitted alone on a stamp from which its neighbours' models of the previous
pass are gone.

torch does the plumbing (the binning of _tile_pairs); the pixel work is HIP
(csrc/scene.hip).
"""
import numpy as np

from . import _lib
from .batch import GMixBatch, StampBatch, _dptr, _on_device, _require_cuda, _stream, _torch

__all__ = ["render_scene", "cut_stamps", "cut_deblended_stamps", "fit_deblended"]

TILE_H = 4      # csrc/scene.hip: SCENE_TH, SCENE_TW
TILE_W = 16
MAX_PAIRS = 2 ** 31 - 1


def _tile_pairs(tile_lo_r, tile_hi_r, tile_lo_c, tile_hi_c, ntx, nty, max_pairs=None,
                total=None):
    """
    The (tile -> object) list of a frame of nty x ntx tiles: object i covers
    the tiles ty in [tile_lo_r[i], tile_hi_r[i]], tx in [tile_lo_c[i],
    tile_hi_c[i]] (inclusive; hi < lo: none), tile (ty, tx) = ty * ntx + tx.
    The arguments are (N,) int64 tensors, on any device.

    Returns (pair_obj, tile_start): the objects of tile 0 in ascending order,
    then those of tile 1, ... (int64), and the ntiles + 1 offsets of the tiles'
    slices.  Reading the pair count back is the one host synchronisation; it
    is checked against max_pairs (default 2^31 - 1) before anything of that
    size is allocated.  total: the pair count, for a caller that has the
    ranges on the host already (no read-back then).
    """
    torch = _torch()
    dev = tile_lo_r.device
    n = int(tile_lo_r.shape[0])
    ntiles = int(ntx) * int(nty)
    i64 = dict(dtype=torch.int64, device=dev)
    nr = torch.clamp(tile_hi_r - tile_lo_r + 1, min=0)
    nc = torch.clamp(tile_hi_c - tile_lo_c + 1, min=0)
    cnt = (nr * nc).to(torch.int64)
    if total is None:
        total = int(cnt.sum()) if n else 0
    limit = MAX_PAIRS if max_pairs is None else int(max_pairs)
    if total > limit:
        raise ValueError("scene: %d (tile, object) pairs exceed max_pairs = %d"
                         % (total, limit))
    if total == 0:
        return torch.zeros(0, **i64), torch.zeros(ntiles + 1, **i64)
    obj = torch.repeat_interleave(torch.arange(n, **i64), cnt, output_size=total)
    start = torch.cumsum(cnt, 0) - cnt
    k = torch.arange(total, **i64) - start[obj]
    ncs = nc.to(torch.int64)[obj]
    kr = torch.div(k, ncs, rounding_mode="floor")
    ty = tile_lo_r.to(torch.int64)[obj] + kr
    tx = tile_lo_c.to(torch.int64)[obj] + (k - kr * ncs)
    key, _ = torch.sort((ty * int(ntx) + tx) * n + obj)
    tile = torch.div(key, n, rounding_mode="floor")
    pair_obj = key - tile * n
    counts = torch.bincount(tile, minlength=ntiles)
    tile_start = torch.cat([torch.zeros(1, **i64), torch.cumsum(counts, 0)])
    return pair_obj, tile_start


def _frame_shape(shape):
    try:
        nrow, ncol = (int(s) for s in shape)
    except (TypeError, ValueError):
        raise ValueError("scene: shape must be (nrow, ncol)")
    if nrow < 1 or ncol < 1:
        raise ValueError("scene: the frame needs nrow * ncol > 0, got %r" % (tuple(shape),))
    return nrow, ncol


def _jacobian_count(jacobians):
    """how many jacobians the argument holds (host work only); None: one
    Jacobian object, shared by every object"""
    torch = _torch()
    if hasattr(jacobians, "get_data"):
        return None
    if isinstance(jacobians, (list, tuple)):
        return len(jacobians)
    if isinstance(jacobians, torch.Tensor):
        if jacobians.ndim != 2 or jacobians.shape[1] != 8:
            raise ValueError("scene: a jacobian tensor must be (N, 8)")
        return int(jacobians.shape[0])
    arr = np.asarray(jacobians)
    if arr.dtype.names is not None:
        return int(arr.size)
    if arr.size % 8:
        raise ValueError("scene: jacobian records are 8 doubles each")
    return int(arr.size // 8)


def _check_jacobians(jacobians, n, who):
    if jacobians is None:
        raise ValueError("%s: jacobians are required (frame coordinates)" % who)
    count = _jacobian_count(jacobians)
    if count is not None and count != n:
        raise ValueError("%s: %d jacobians for %d objects" % (who, count, n))


def _jacobian_tensor(jacobians, n, dev):
    if n == 0:
        return _torch().zeros((0, 8), dtype=_torch().float64, device=dev)
    return StampBatch._jacobian_tensor(jacobians, n, 0, 0, dev)


def _scene_lists(nrow, ncol, rec, G, n, jac, max_pairs, boxes_to_host=False):
    """scene_boxes_kernel and the binning on (n * G, 13) gaussian records and an
    (n, 8) jacobian tensor.  Returns (gev, status, boxes, pair_obj, tile_start):
    boxes (n, 8) int32 on the device, or (boxes_to_host) a numpy copy that came
    over with the pair count, in the same read-back"""
    torch = _torch()
    dev = rec.device
    L = _lib.lib()
    ntx = (ncol + TILE_W - 1) // TILE_W
    nty = (nrow + TILE_H - 1) // TILE_H
    boxes = torch.empty((n, 8), dtype=torch.int32, device=dev)
    gev = torch.empty((n * G, 8), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    with _on_device(dev):
        st = L.ngmix_scene_boxes(_dptr(rec), G, _dptr(jac), n, nrow, ncol, _dptr(gev),
                                 _dptr(boxes), _dptr(status), _stream())
    _lib.check(st, "ngmix_scene_boxes")
    if boxes_to_host:
        hb = boxes.cpu().numpy()
        b = torch.from_numpy(hb.astype(np.int64)).to(dev) if n else boxes.to(torch.int64)
        total = int((np.clip(hb[:, 5] - hb[:, 4] + 1, 0, None).astype(np.int64) *
                     np.clip(hb[:, 7] - hb[:, 6] + 1, 0, None)).sum())
    else:
        hb = None
        b = boxes.to(torch.int64)
        total = None
    pair_obj, tile_start = _tile_pairs(b[:, 4], b[:, 5], b[:, 6], b[:, 7], ntx, nty, max_pairs,
                                       total)
    return gev, status, (hb if boxes_to_host else boxes), pair_obj, tile_start


def _render_records(nrow, ncol, rec, G, n, jac, image, max_pairs, boxes_to_host=False):
    """the scene kernels on (n * G, 13) gaussian records and an (n, 8) jacobian
    tensor; adds into image (None: a fresh frame).  Returns (frame, status,
    boxes): boxes as _scene_lists returns them"""
    torch = _torch()
    dev = rec.device
    gev, status, boxes, pair_obj, tile_start = _scene_lists(nrow, ncol, rec, G, n, jac,
                                                            max_pairs, boxes_to_host)
    fresh = image is None
    frame = torch.empty((nrow, ncol), dtype=torch.float64, device=dev) if fresh else image
    npairs = int(pair_obj.shape[0])
    with _on_device(dev):
        st = _lib.lib().ngmix_scene_render(_dptr(gev), G, _dptr(jac), _dptr(pair_obj), npairs,
                                           _dptr(tile_start), nrow, ncol, _dptr(frame),
                                           int(fresh), _stream())
    _lib.check(st, "ngmix_scene_render")
    return frame, status, boxes


def _check_image(image, nrow, ncol, who):
    torch = _torch()
    if image is None:
        return
    if not isinstance(image, torch.Tensor) or image.ndim != 2 or \
            tuple(image.shape) != (nrow, ncol):
        raise ValueError("%s: image must be a (%d, %d) tensor" % (who, nrow, ncol))
    if image.dtype != torch.float64:
        raise ValueError("%s: image must be float64" % who)


def render_scene(shape, gm, jacobians, image=None, max_pairs=None, fast_exp=True):
    """
    Draw the n mixtures of gm into one frame.

    shape: (nrow, ncol) of the frame
    gm: GMixBatch of n objects x G gaussians (already convolved with their
        psf); norms are set lazily, in place, as StampBatch.render sets them
    jacobians: n jacobian records / Jacobian objects ((n, 8) array or tensor,
        a structured array, a list), or one Jacobian object for all; row0 /
        col0 are in FRAME pixel coordinates and may lie outside the frame
    image: (nrow, ncol) contiguous float64 device tensor to add into, in
        place; None: a fresh frame
    max_pairs: refuse (ValueError naming the count) more (tile, object) pairs
        than this; default 2^31 - 1

    Returns (frame, status): status (n,) int32 is 0, or the code of the norms'
    refusal (_lib.ERR_*); a refused object is left out of the frame.

    Order of summation (part of the interface): per object m = sum over its
    gaussians in order from 0.0, pixel = pixel + m, objects in ascending index,
    starting from image's value or 0.0.  So rendering objects 0..k and then
    k+1..n-1 into image= of the first result gives the bits of one call.
    """
    nrow, ncol = _frame_shape(shape)
    if not fast_exp:
        raise ValueError("render_scene: only fast_exp=True is built: the chi2 < 25 gate of "
                         "the fast exp is what makes the tile binning exact")
    if not isinstance(gm, GMixBatch):
        raise ValueError("render_scene: gm must be a GMixBatch")
    if gm.ngauss < 1:
        raise ValueError("render_scene: at least one gaussian per object")
    _check_jacobians(jacobians, gm.n, "render_scene")
    _check_image(image, nrow, ncol, "render_scene")
    dev = _require_cuda(gm.device)
    if image is not None and (image.device != dev or not image.is_contiguous()):
        raise ValueError("render_scene: image must be contiguous, on the mixtures' device")
    jac = _jacobian_tensor(jacobians, gm.n, dev)
    frame, status, _ = _render_records(nrow, ncol, gm.data, gm.ngauss, gm.n, jac, image,
                                       max_pairs)
    return frame, status


def _window_arrays(r_lo, c_lo, nrow, ncol, who="cut_stamps"):
    """(r_lo, c_lo, nrow, ncol) as (N,) host arrays, checked"""
    r_lo = np.atleast_1d(np.asarray(r_lo)).reshape(-1)
    n = r_lo.shape[0]
    c_lo = np.atleast_1d(np.asarray(c_lo)).reshape(-1)
    if c_lo.shape[0] != n:
        raise ValueError("%s: r_lo and c_lo must have one entry per window" % who)
    out = []
    for name, a in (("nrow", nrow), ("ncol", ncol)):
        a = np.asarray(a)
        if a.ndim == 0:
            a = np.full(n, int(a))
        a = a.reshape(-1)
        if a.shape[0] != n:
            raise ValueError("%s: %s must be an int or one entry per window" % (who, name))
        if np.any(a <= 0):
            raise ValueError("%s: window %d has a non-positive shape (%s = %d)"
                             % (who, int(np.argmax(a <= 0)), name, int(a[np.argmax(a <= 0)])))
        out.append(a.astype(np.int64))
    lim = 2 ** 31 - 1
    for a in (r_lo, c_lo):
        if n and np.any(np.abs(a.astype(np.int64)) > lim - out[0].max() - out[1].max()):
            raise ValueError("%s: window origins must fit 32 bits" % who)
    return r_lo.astype(np.int64), c_lo.astype(np.int64), out[0], out[1]


def _gather(frame, win_host, pix_off_host, total, mode):
    """frame_gather_kernel: the windows win_host (N, 4) int32 of the (R, C)
    float64 device tensor frame, packed at pix_off_host"""
    torch = _torch()
    dev = frame.device
    n = win_host.shape[0]
    out = torch.empty(total, dtype=torch.float64, device=dev)
    win_host = np.ascontiguousarray(win_host, dtype=np.int32)
    win = torch.from_numpy(win_host).to(dev)
    off = torch.from_numpy(np.ascontiguousarray(pix_off_host, dtype=np.int64)).to(dev)
    with _on_device(dev):
        st = _lib.lib().ngmix_frame_gather(_dptr(frame), int(frame.shape[0]), int(frame.shape[1]),
                                           _dptr(win), _lib.ptr(win_host), _dptr(off), n,
                                           int(mode), _dptr(out), _stream())
    _lib.check(st, "ngmix_frame_gather")
    return out


def _cut_arguments(frame, weight, r_lo, c_lo, nrow, ncol, jacobians, who="cut_stamps"):
    """cut_stamps' arguments, checked on the host; the windows as (N,) arrays"""
    torch = _torch()
    if not isinstance(frame, torch.Tensor) or frame.ndim != 2:
        raise ValueError("%s: frame must be a 2-d device tensor" % who)
    if frame.shape[0] < 1 or frame.shape[1] < 1:
        raise ValueError("%s: the frame needs nrow * ncol > 0" % who)
    if isinstance(weight, torch.Tensor) and weight.ndim != 0:
        if tuple(weight.shape) != tuple(frame.shape):
            raise ValueError("%s: weight must be a scalar or have the frame's shape" % who)
    r_lo, c_lo, wr, wc = _window_arrays(r_lo, c_lo, nrow, ncol, who)
    _check_jacobians(jacobians, r_lo.shape[0], who)
    return r_lo, c_lo, wr, wc


def _cut(frame, weight, windows, jacobians, ignore_zero_weight, values):
    """the StampBatch of the checked windows: values(frame, win, off, total)
    gives the packed pixel values, everything else is cut_stamps'"""
    torch = _torch()
    r_lo, c_lo, wr, wc = windows
    n = r_lo.shape[0]
    dev = _require_cuda(frame.device)
    frame = frame.to(torch.float64).contiguous()
    if isinstance(weight, torch.Tensor) and weight.ndim == 2:
        wframe = weight.to(device=dev, dtype=torch.float64).contiguous()
    else:
        wframe = torch.full(tuple(frame.shape), float(weight), dtype=torch.float64, device=dev)
    npix = wr * wc
    off = np.concatenate([[0], np.cumsum(npix)[:-1]]).astype(np.int64) if n else \
        np.zeros(0, dtype=np.int64)
    total = int(npix.sum())
    win = np.stack([r_lo, c_lo, wr, wc], axis=1) if n else np.zeros((0, 4), dtype=np.int64)
    val = values(frame, win, off, total)
    ierr = _gather(wframe, win, off, total, 1)
    jac = _jacobian_tensor(jacobians, n, dev).clone()
    jac[:, 0] -= torch.from_numpy(r_lo.astype(np.float64)).to(dev)
    jac[:, 1] -= torch.from_numpy(c_lo.astype(np.float64)).to(dev)
    return StampBatch(val, ierr, jac, wr, wc, off, ignore_zero_weight)


def cut_stamps(frame, weight, r_lo, c_lo, nrow, ncol, jacobians, ignore_zero_weight=True):
    """
    Cut N windows out of a frame that is already on the device into a
    StampBatch.

    frame: (R, C) device tensor; weight: the same shape, or a scalar (float32
        is widened by torch first: the frame is small)
    r_lo, c_lo: (N,) first row / column of each window, in frame pixel indices;
        a window may cross the frame's edge or lie outside it: pixels outside
        the frame get value 0.0 and weight 0.0 (masked)
    nrow, ncol: ints, or (N,) arrays for ragged windows
    jacobians: as render_scene's, in FRAME coordinates; the batch stores
        row0 - r_lo, col0 - c_lo
    ierr = sqrt(max(w, 0)) as the other builders (pixels_nb.py:49-52); npix_kept
    and the uniform-weight flags come from the count pass over the cut-out
    weights on the device (StampBatch.rescan_weights), never assumed.
    """
    windows = _cut_arguments(frame, weight, r_lo, c_lo, nrow, ncol, jacobians)
    return _cut(frame, weight, windows, jacobians, ignore_zero_weight,
                lambda f, win, off, total: _gather(f, win, off, total, 0))


def _window_items(r_lo, c_lo, wr, wc, nrow, ncol, device=None, max_items=MAX_PAIRS):
    """
    The work items of scene_cut_minus_kernel: every (window, frame tile) pair
    that overlaps inside the (nrow, ncol) frame, window after window, a
    window's tiles in ascending order; (nitems, 2) int32 on `device` (torch; a
    CPU device serves as well).  r_lo, c_lo, wr, wc: (N,) host arrays.  The
    count comes from the host arrays and is checked against max_items (the
    launch grid's limit) before anything of that size is allocated.
    """
    torch = _torch()
    ntx = (int(ncol) + TILE_W - 1) // TILE_W
    r_lo, c_lo, wr, wc = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (r_lo, c_lo, wr, wc))
    n = r_lo.shape[0]
    ra, rb = np.maximum(r_lo, 0), np.minimum(r_lo + wr, int(nrow)) - 1
    ca, cb = np.maximum(c_lo, 0), np.minimum(c_lo + wc, int(ncol)) - 1
    hit = (rb >= ra) & (cb >= ca)
    ty_lo, tx_lo = ra // TILE_H, ca // TILE_W
    nr = np.where(hit, rb // TILE_H - ty_lo + 1, 0)
    nc = np.where(hit, cb // TILE_W - tx_lo + 1, 0)
    cnt = nr * nc
    total = int(cnt.sum())
    if total > int(max_items):
        raise ValueError("scene: %d (window, tile) items exceed the limit of %d"
                         % (total, int(max_items)))
    i64 = dict(dtype=torch.int64, device=device)
    if total == 0:
        return torch.zeros((0, 2), dtype=torch.int32, device=device)
    t_cnt, t_nc, t_ty, t_tx = (torch.from_numpy(a).to(device) for a in (cnt, nc, ty_lo, tx_lo))
    w = torch.repeat_interleave(torch.arange(n, **i64), t_cnt, output_size=total)
    k = torch.arange(total, **i64) - (torch.cumsum(t_cnt, 0) - t_cnt)[w]
    ncs = t_nc[w]
    kr = torch.div(k, ncs, rounding_mode="floor")
    tile = (t_ty[w] + kr) * ntx + t_tx[w] + (k - kr * ncs)
    return torch.stack([w, tile], dim=1).to(torch.int32).contiguous()


def _check_owner(owner, n, m):
    """owner as an (n,) int32 host array with entries in [-1, m)"""
    if owner is None:
        if m != n:
            raise ValueError("cut_deblended_stamps: owner=None needs one object per window "
                             "(%d objects, %d windows)" % (m, n))
        return np.arange(n, dtype=np.int32)
    if _torch().is_tensor(owner):
        owner = owner.detach().cpu().numpy()
    owner = np.asarray(owner)
    if owner.size and owner.dtype.kind not in "iu":
        raise ValueError("cut_deblended_stamps: owner must have an integer dtype, got %s"
                         % owner.dtype)
    owner = owner.reshape(-1)
    if owner.shape[0] != n:
        raise ValueError("cut_deblended_stamps: %d owners for %d windows" % (owner.shape[0], n))
    owner = owner.astype(np.int64)
    bad = (owner < -1) | (owner >= m)
    if np.any(bad):
        i = int(np.argmax(bad))
        raise ValueError("cut_deblended_stamps: owner %d of window %d is outside [-1, %d)"
                         % (int(owner[i]), i, m))
    return owner.astype(np.int32)


def cut_deblended_stamps(frame, weight, r_lo, c_lo, nrow, ncol, jacobians, gm,
                         gm_jacobians=None, owner=None, max_pairs=None,
                         ignore_zero_weight=True):
    """
    cut_stamps with the models of every object but the window's owner
    subtracted from the values.

    frame, weight, r_lo, c_lo, nrow, ncol, jacobians, ignore_zero_weight:
        cut_stamps' arguments, for N windows
    gm: GMixBatch of M objects x G gaussians (already convolved with their
        psf); norms are set lazily, in place, as render_scene sets them
    gm_jacobians: the M objects' jacobians, in frame coordinates, as
        render_scene's; None: M == N and they are `jacobians`
    owner: (N,) integers in [-1, M): the object each window keeps; -1: none (a
        residual stamp); several windows may share an owner.  None: arange(N),
        which needs M == N
    max_pairs: as render_scene's

    Returns (StampBatch, status): status (M,) int32 as render_scene's; a
    refused object is left out of every subtraction.

    Only the values differ from cut_stamps: ierr, npix_kept, the uniform-weight
    flags and the stored jacobians come from the same code.  The values
    (csrc/scene.hip, scene_cut_minus_kernel): a pixel p of window s inside the
    frame is frame[p] - nbr, where nbr = 0.0 and then nbr = nbr + m_j(p) over
    the objects j != owner[s] of p's frame tile in ascending index, m_j
    render_scene's per-object sum.  So window s is, bit for bit,
    cut_stamps(frame)[s] - cut_stamps(render_scene(all objects but owner[s]))[s],
    and two calls give the same bits.
    """
    torch = _torch()
    windows = _cut_arguments(frame, weight, r_lo, c_lo, nrow, ncol, jacobians,
                             "cut_deblended_stamps")
    n = windows[0].shape[0]
    if not isinstance(gm, GMixBatch):
        raise ValueError("cut_deblended_stamps: gm must be a GMixBatch")
    if gm.ngauss < 1:
        raise ValueError("cut_deblended_stamps: at least one gaussian per object")
    m, G = gm.n, gm.ngauss
    if gm_jacobians is None:
        if m != n:
            raise ValueError("cut_deblended_stamps: gm_jacobians=None needs one object per "
                             "window (%d objects, %d windows)" % (m, n))
        gm_jacobians = jacobians
    _check_jacobians(gm_jacobians, m, "cut_deblended_stamps")
    owner = _check_owner(owner, n, m)
    if frame.device != gm.device:
        raise ValueError("cut_deblended_stamps: the frame must be on the mixtures' device (%s)"
                         % gm.device)
    dev = _require_cuda(gm.device)
    nr, nc = int(frame.shape[0]), int(frame.shape[1])
    gjac = _jacobian_tensor(gm_jacobians, m, dev)
    gev, status, _, pair_obj, tile_start = _scene_lists(nr, nc, gm.data, G, m, gjac, max_pairs)
    items = _window_items(windows[0], windows[1], windows[2], windows[3], nr, nc, dev)

    def values(f, win_host, off_host, total):
        out = torch.empty(total, dtype=torch.float64, device=dev)
        win_host = np.ascontiguousarray(win_host, dtype=np.int32)
        win = torch.from_numpy(win_host).to(dev)
        own = torch.from_numpy(owner).to(dev)
        off = torch.from_numpy(np.ascontiguousarray(off_host, dtype=np.int64)).to(dev)
        with _on_device(dev):
            st = _lib.lib().ngmix_scene_cut_minus(
                _dptr(f), nr, nc, _dptr(gev), G, _dptr(gjac), m, _dptr(pair_obj),
                int(pair_obj.shape[0]), _dptr(tile_start), _dptr(win), _lib.ptr(win_host),
                _dptr(own), _lib.ptr(owner), _dptr(off), n, _dptr(items), int(items.shape[0]),
                _dptr(out), total, _stream())
        _lib.check(st, "ngmix_scene_cut_minus")
        return out

    return _cut(frame, weight, windows, jacobians, ignore_zero_weight, values), status


def fit_deblended(frame, weight, r_lo, c_lo, nrow, ncol, jacobians, guess, model, psf=None,
                  prior=None, niter=3, fitter=None):
    """
    Fit the objects of a crowded frame, one band, one window per object: each
    pass cuts every object's window with the current models of all the others
    subtracted (cut_deblended_stamps) and fits every object alone on it with
    the lock-step LM fitter.

    frame, weight, r_lo, c_lo, nrow, ncol, jacobians: cut_stamps' arguments,
        window i and jacobian i belonging to object i
    guess: (nobj, npars) starting parameters, as LMBatchFitter.go's, one flux
    model: the model of GMixBatch.from_pars and LMBatchFitter
    psf: GMixBatch with one mixture per object, or None
    prior: LMBatchFitter's
    niter: passes, >= 1
    fitter: anything with LMBatchFitter's go(stamps, guess, psf=); None:
        LMBatchFitter(model, prior=prior)

    Pass 1 subtracts the guess's models.  The update is Jacobi-style: every
    object sees its neighbours as the previous pass left them, so a pass is one
    batch and the result does not depend on the order of the objects.  An
    object whose fit ends with flags != 0 keeps its previous parameters for the
    next pass's subtraction; an object whose mixture is refused is left out of
    the subtractions and flagged in deblend_status.

    Returns the last pass's result dict, plus deblend_niter, deblend_dpars
    (niter, nobj): the largest absolute parameter change of each object in each
    pass, and deblend_status (nobj,) int32: 0, or the code (_lib.ERR_*) with
    which the last pass's mixture of the object was refused (by from_pars,
    convolve or the norms, the first of them): that object was in no
    subtraction of that pass.
    """
    niter = int(niter)
    if niter < 1:
        raise ValueError("fit_deblended: niter must be at least 1, got %d" % niter)
    windows = _cut_arguments(frame, weight, r_lo, c_lo, nrow, ncol, jacobians, "fit_deblended")
    pars = np.array(np.atleast_2d(guess), dtype=np.float64)
    nobj = pars.shape[0]
    if windows[0].shape[0] != nobj:
        raise ValueError("fit_deblended: %d windows for %d objects"
                         % (windows[0].shape[0], nobj))
    if psf is not None and (not isinstance(psf, GMixBatch) or psf.n != nobj):
        raise ValueError("fit_deblended: psf must be a GMixBatch with one mixture per object")
    if fitter is None:
        from .lm_batch import LMBatchFitter
        fitter = LMBatchFitter(model, prior=prior)
    dev = _require_cuda(frame.device)
    dpars = np.zeros((niter, nobj))
    res = None
    for k in range(niter):
        gm, status = GMixBatch.from_pars(pars, model, device=dev)
        if psf is not None:
            gm, st = gm.convolve(psf)
            status = _torch().where(status != 0, status, st)
        sb, st = cut_deblended_stamps(frame, weight, windows[0], windows[1], windows[2],
                                      windows[3], jacobians, gm)
        status = _torch().where(status != 0, status, st)
        res = fitter.go(sb, pars, psf=psf)
        ok = np.asarray(res["flags"]) == 0
        new = np.where(ok[:, None], np.asarray(res["pars"], dtype=np.float64), pars)
        dpars[k] = np.abs(new - pars).max(axis=1) if nobj else 0.0
        pars = new
    res = dict(res)
    res["deblend_niter"] = niter
    res["deblend_dpars"] = dpars
    res["deblend_status"] = status.cpu().numpy().astype(np.int32)
    return res
