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

    ne = scene.normal_equations(frame, weight, jacobians, pars, "exp", psf=psf)
    cov = scene.joint_covariance(frame, weight, jacobians, pars, "exp", psf=psf)
    res = scene.fit_joint(frame, weight, jacobians, guess, "exp", psf=psf)

normal_equations gives the Gauss-Newton blocks of the whole frame at once
(csrc/scene_normal.hip): every object's own block and
gradient, and the cross block of every pair of objects that share a tile and
whose boxes meet, each object with a jacobian of its own.  joint_covariance
inverts them per group of connected objects (the covariance of an object
marginalised over its neighbours), and fit_joint is a Levenberg-Marquardt fit of
all the objects of a frame together over them.

    sol = scene.solve_normal(ne, lam=1e-3)
    res = scene.fit_joint(frame, weight, jacobians, guess, "exp", psf=psf, large_groups="cg")

solve_normal solves (F + lam diag F) delta = grad over those blocks, every
group as one system, by preconditioned conjugate gradients on the device
(csrc/scene_solve.hip): the operator over the block rows
and the CG updates are HIP, no atomics, and a group's bits depend on that group
alone.  fit_joint(large_groups="cg") steps the groups that are too large for a
dense solve with it, instead of with their own blocks only.

    ne = scene.normal_equations_frames(frames, weights, jacobians, pars, "exp", psf=psfs,
                                       frame_band=[0, 1, 1], prior=prior)
    res = scene.fit_joint_frames(frames, weights, jacobians, guess, "exp", psf=psfs,
                                 frame_band=[0, 1, 1], prior=prior)

normal_equations_frames, joint_covariance_frames and fit_joint_frames are the
same over a LIST of frames (several bands, several epochs per band, each image
with its own shape, jacobians and psf) and with a prior: pars hold the shape
parameters and one flux per band (DESIGN.md section 3.18;
csrc/scene_normal_frames.hip).  The one-frame calls above are their case F = 1,
one band, no prior, on the same code (_Frames.one); only the kernel entry is
chosen by the case (_scene_normal).

torch does the plumbing (the binning of _tile_pairs, the row lists of
_block_rows, the dense solves of the groups); the pixel work and the sparse
solve are HIP (csrc/scene.hip, csrc/scene_normal.hip,
csrc/scene_normal_frames.hip, csrc/scene_solve.hip).
"""
import numpy as np

from . import _lib
from .batch import GMixBatch, StampBatch, _dptr, _on_device, _require_cuda, _stream, _torch

__all__ = ["render_scene", "cut_stamps", "cut_deblended_stamps", "fit_deblended",
           "normal_equations", "joint_covariance", "fit_joint", "solve_normal",
           "normal_equations_frames", "joint_covariance_frames", "fit_joint_frames"]

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


# ------------------------------------------------ normal equations of a frame
# (the one-frame API; it runs as the case F = 1, one band, no prior of the
# frames' code further down: _Frames.one, _frames_model, _normal_frames)

NORMAL_KMAX = 8          # csrc/scene_normal.hip: SN_KT
LAMBDA_FLOOR = 1.0e-9    # fit_joint: no damping factor goes below this


def _scene_pairs(pair_obj, tile_start, boxes, n, max_pairs=None):
    """
    The pairs (a, b), a < b, of objects that share a frame tile AND whose
    clipped boxes intersect, from the (tile -> object) lists of _tile_pairs
    (any device): every tile with n_t objects gives n_t (n_t - 1) / 2
    candidates (never an N x N array), which are made unique and then tested
    against boxes (n, >= 4) [rmin, rmax, cmin, cmax, ...].  The candidate count
    is checked against max_pairs (default 2^31 - 1) before anything of that
    size is allocated.  Returns (P, 2) int64, sorted by (a, b).
    """
    torch = _torch()
    dev = pair_obj.device
    i64 = dict(dtype=torch.int64, device=dev)
    E = int(pair_obj.shape[0])
    limit = MAX_PAIRS if max_pairs is None else int(max_pairs)
    if E == 0:
        return torch.zeros((0, 2), **i64)
    cnt = tile_start[1:] - tile_start[:-1]
    total = int((cnt * (cnt - 1)).sum()) // 2
    if total > limit:
        raise ValueError("scene: %d candidate object pairs exceed max_pairs = %d"
                         % (total, limit))
    if total == 0:
        return torch.zeros((0, 2), **i64)
    tile = torch.repeat_interleave(torch.arange(cnt.shape[0], **i64), cnt, output_size=E)
    later = cnt[tile] - 1 - (torch.arange(E, **i64) - tile_start[tile])
    first = torch.repeat_interleave(torch.arange(E, **i64), later, output_size=total)
    second = first + 1 + torch.arange(total, **i64) - (torch.cumsum(later, 0) - later)[first]
    key = torch.unique(pair_obj[first] * int(n) + pair_obj[second])
    a = torch.div(key, int(n), rounding_mode="floor")
    b = key - a * int(n)
    bx = boxes.to(device=dev, dtype=torch.int64)
    meet = (torch.maximum(bx[a, 0], bx[b, 0]) <= torch.minimum(bx[a, 1], bx[b, 1])) & \
        (torch.maximum(bx[a, 2], bx[b, 2]) <= torch.minimum(bx[a, 3], bx[b, 3]))
    return torch.stack([a[meet], b[meet]], dim=1)


def _components(n, a, b):
    """labels (n,) int64 of the connected components of the graph with edges
    (a[i], b[i]) on n nodes: every node gets the smallest index of its component
    (host arrays; hooking to the smaller root, then pointer jumping)"""
    label = np.arange(n, dtype=np.int64)
    a = np.asarray(a, dtype=np.int64)
    b = np.asarray(b, dtype=np.int64)
    for _ in range(n + 1):
        la, lb = label[a], label[b]
        m = np.minimum(la, lb)
        new = label.copy()
        np.minimum.at(new, la, m)
        np.minimum.at(new, lb, m)
        for _ in range(64):
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, label):
            break
        label = new
    return label


def _scene_groups(pair_obj, tile_start, n):
    """
    The connected components of the tile-sharing graph, on the host: objects in
    one tile's list are connected.  pair_obj, tile_start: host int64 arrays.
    Returns (group (n,) int64, tile_group (ntiles,) int64): groups numbered
    0, 1, ... by their smallest member (an object in no tile is a group of its
    own), and the group of every tile (-1: a tile without objects).
    """
    group, tile_group = _scene_groups_frames([(pair_obj, tile_start)], n)
    return group, tile_group[0]


def _tile_chain(pair_obj, tile_start):
    """the edges (a, b) of a chain through each tile's list, which connects what
    the tile's n_t^2 pairs connect (host int64 arrays)"""
    E = pair_obj.shape[0]
    same = np.ones(max(E - 1, 0), dtype=bool)
    ends = tile_start[1:-1]
    ends = ends[(ends > 0) & (ends < E)]
    same[ends - 1] = False
    idx = np.nonzero(same)[0]
    return pair_obj[idx], pair_obj[idx + 1]


def _scene_groups_frames(lists, n):
    """
    _scene_groups over several frames: lists = [(pair_obj, tile_start), ...],
    one (tile -> object) list per frame (host int64 arrays), all over the same
    n objects.  The groups are the connected components of the UNION of the
    frames' tile-sharing graphs, numbered by their smallest member.  Returns
    (group (n,) int64, [tile_group of frame 0, of frame 1, ...]): every tile
    with objects, in any frame, belongs to exactly one group.
    """
    lists = [(np.asarray(po, dtype=np.int64), np.asarray(ts, dtype=np.int64))
             for po, ts in lists]
    edges = [_tile_chain(po, ts) for po, ts in lists]
    label = _components(n, np.concatenate([e[0] for e in edges]),
                        np.concatenate([e[1] for e in edges]))
    _, group = np.unique(label, return_inverse=True)
    group = group.astype(np.int64).reshape(-1)
    tile_groups = []
    for po, ts in lists:
        cnt = np.diff(ts)
        tile_group = np.full(cnt.shape[0], -1, dtype=np.int64)
        has = cnt > 0
        tile_group[has] = group[po[ts[:-1][has]]]
        tile_groups.append(tile_group)
    return group, tile_groups


def _segment_sums(values, seg, nseg):
    """sums of values (host float64) per segment id seg (>= 0; < 0: left out),
    added in a fixed order: a stable sort by segment, then np.add.reduceat"""
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    seg = np.asarray(seg, dtype=np.int64).reshape(-1)
    out = np.zeros(nseg, dtype=np.float64)
    keep = seg >= 0
    values, seg = values[keep], seg[keep]
    if values.shape[0] == 0:
        return out
    order = np.argsort(seg, kind="stable")
    seg, values = seg[order], values[order]
    starts = np.concatenate([[0], np.nonzero(np.diff(seg))[0] + 1])
    out[seg[starts]] = np.add.reduceat(values, starts)
    return out


def _tile_sums(x):
    """the sum of the (nrow, ncol) tensor x over every 4 x 16 frame tile,
    (nty * ntx,) in tile order"""
    nrow, ncol = int(x.shape[0]), int(x.shape[1])
    ntx = (ncol + TILE_W - 1) // TILE_W
    nty = (nrow + TILE_H - 1) // TILE_H
    pad = x.new_zeros((nty * TILE_H, ntx * TILE_W))
    pad[:nrow, :ncol] = x
    return pad.reshape(nty, TILE_H, ntx, TILE_W).sum(dim=(1, 3)).reshape(-1)


class _GroupLayout(object):
    """
    How the objects of a frame fall into dense per-group systems.  group: (N,)
    host labels 0 .. ngroups - 1.  A group of up to max_group objects is one
    system of (size K) unknowns, its members in ascending index; the systems
    are bucketed by size (1, 2, 4, ... up to max_group), a bucket's smaller
    groups padded with identity blocks.  The members of a larger group are
    systems of one object each (their own blocks only): oversized.
    """

    def __init__(self, group, max_group):
        group = np.asarray(group, dtype=np.int64).reshape(-1)
        n = group.shape[0]
        max_group = int(max_group)
        if max_group < 1:
            raise ValueError("scene: max_group must be at least 1, got %d" % max_group)
        size = np.bincount(group, minlength=(int(group.max()) + 1 if n else 0))
        order = np.argsort(group, kind="stable")
        start = np.concatenate([[0], np.cumsum(size)[:-1]]) if size.shape[0] else size
        slot = np.empty(n, dtype=np.int64)
        slot[order] = np.arange(n) - start[group[order]]
        self.n = n
        self.oversized = size[group] > max_group if n else np.zeros(0, dtype=bool)
        # the system of every object: a group, or (oversized) the object itself
        sys_of = np.where(self.oversized, size.shape[0] + np.arange(n), group)
        self.slot = np.where(self.oversized, 0, slot)
        sys_size = np.where(self.oversized, 1, size[group] if n else 0)
        widths = []
        w = 1
        while w < max_group:
            widths.append(w)
            w *= 2
        widths.append(max_group)
        self.buckets = []     # (width m, objects (host), row of each in the bucket, nrows)
        self.bucket_of = np.full(n, -1, dtype=np.int64)
        self.row = np.zeros(n, dtype=np.int64)
        lo = 0
        for m in widths:
            objs = np.nonzero((sys_size > lo) & (sys_size <= m))[0]
            lo = m
            if objs.shape[0] == 0:
                continue
            ids, row = np.unique(sys_of[objs], return_inverse=True)
            self.bucket_of[objs] = len(self.buckets)
            self.row[objs] = row.reshape(-1)
            self.buckets.append((m, objs, row.reshape(-1), ids.shape[0]))

    def dense(self, F_self, pairs, F_cross):
        """the buckets' matrices [(nrows, m K, m K) tensor, ...] from the blocks:
        F_self (N, K, K), pairs (P, 2), F_cross (P, K, K) tensors on one device;
        a pair across two systems (an oversized group's) is left out"""
        torch = _torch()
        dev = F_self.device
        K = int(F_self.shape[1])
        pa = pairs[:, 0].cpu().numpy() if pairs.shape[0] else np.zeros(0, dtype=np.int64)
        pb = pairs[:, 1].cpu().numpy() if pairs.shape[0] else np.zeros(0, dtype=np.int64)
        inside = ~self.oversized[pa] & ~self.oversized[pb] if pa.shape[0] else \
            np.zeros(0, dtype=bool)
        out = []
        for k, (m, objs, row, nrows) in enumerate(self.buckets):
            M = torch.zeros((nrows, m, K, m, K), dtype=F_self.dtype, device=dev)
            used = torch.zeros((nrows, m), dtype=torch.bool, device=dev)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
            r, sl, o = t(row), t(self.slot[objs]), t(objs)
            M[r, sl, :, sl, :] = F_self[o]
            used[r, sl] = True
            sel = np.nonzero(inside & (self.bucket_of[pa] == k))[0] if pa.shape[0] else pa
            if sel.shape[0]:
                ra, sa, sb = t(self.row[pa[sel]]), t(self.slot[pa[sel]]), t(self.slot[pb[sel]])
                C = F_cross[t(sel)]
                M[ra, sa, :, sb, :] = C
                M[ra, sb, :, sa, :] = C.transpose(1, 2)
            M = M.reshape(nrows, m * K, m * K)
            # identity in the slots that no object fills
            pad = (~used).to(F_self.dtype)[:, :, None].expand(nrows, m, K)
            out.append(M + torch.diag_embed(pad.reshape(nrows, m * K)))
        return out

    def blocks(self, mats, K):
        """every object's K x K diagonal block of its system's matrix: (N, K, K)"""
        torch = _torch()
        dev = mats[0].device if mats else None
        res = None
        for (m, objs, row, nrows), M in zip(self.buckets, mats):
            if res is None:
                res = torch.zeros((self.n, K, K), dtype=M.dtype, device=dev)
            M5 = M.reshape(nrows, m, K, m, K)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
            r, sl = t(row), t(self.slot[objs])
            res[t(objs)] = M5[r, sl, :, sl, :]
        return res

    def gather(self, vec, k):
        """bucket k's right-hand sides (nrows, m K) from per-object rows (N, K)"""
        torch = _torch()
        m, objs, row, nrows = self.buckets[k]
        K = int(vec.shape[1])
        dev = vec.device
        out = torch.zeros((nrows, m, K), dtype=vec.dtype, device=dev)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        out[t(row), t(self.slot[objs])] = vec[t(objs)]
        return out.reshape(nrows, m * K)

    def scatter(self, sols, K, like):
        """per-object rows (N, K) from the buckets' solutions [(nrows, m K), ...]"""
        torch = _torch()
        res = torch.zeros((self.n, K), dtype=like.dtype, device=like.device)
        for (m, objs, row, nrows), x in zip(self.buckets, sols):
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(like.device)  # noqa: E731
            res[t(objs)] = x.reshape(nrows, m, K)[t(row), t(self.slot[objs])]
        return res

    def per_object(self, values, k):
        """bucket k's per-system values (nrows, ...) at its objects"""
        m, objs, row, nrows = self.buckets[k]
        return objs, values[_torch().from_numpy(np.ascontiguousarray(row)).to(values.device)]


def _joint_arguments(frame, weight, jacobians, pars, model, psf, who):
    """the arguments every joint call shares, checked on the host before a
    device is asked for.  Returns (pars tensor (N, K) float64 on the frame's
    device, model name)"""
    from . import autodiff
    torch = _torch()
    if not isinstance(frame, torch.Tensor) or frame.ndim != 2:
        raise ValueError("%s: frame must be a 2-d device tensor" % who)
    if frame.shape[0] < 1 or frame.shape[1] < 1:
        raise ValueError("%s: the frame needs nrow * ncol > 0" % who)
    if frame.dtype != torch.float64:
        raise ValueError("%s: frame must be float64" % who)
    if isinstance(weight, torch.Tensor) and weight.ndim != 0:
        if tuple(weight.shape) != tuple(frame.shape):
            raise ValueError("%s: weight must be None, a scalar or have the frame's shape" % who)
        if weight.device != frame.device:
            raise ValueError("%s: weight must be on the frame's device (%s)"
                             % (who, frame.device))
    if isinstance(pars, torch.Tensor):
        if pars.device != frame.device:
            raise ValueError("%s: pars must be on the frame's device (%s)" % (who, frame.device))
        p = pars.detach().to(torch.float64)
    else:
        p = torch.from_numpy(np.array(pars, dtype=np.float64))
    if p.ndim != 2:
        raise ValueError("%s: pars must be (nobj, npars)" % who)
    n, K = int(p.shape[0]), int(p.shape[1])
    name = autodiff._model_name(model)
    if K > NORMAL_KMAX:
        raise ValueError("%s: at most %d parameters per object (one band), got K = %d"
                         % (who, NORMAL_KMAX, K))
    if name == "coellip" or K != autodiff._NLOC[name]:
        raise ValueError("%s: model '%s' with one flux needs %s parameters, got %d"
                         % (who, name, autodiff._NLOC.get(name, "at most 8"), K))
    _check_jacobians(jacobians, n, who)
    if psf is not None:
        if isinstance(psf, GMixBatch):
            if psf.n != n:
                raise ValueError("%s: psf must hold one mixture per object" % who)
            if psf.device != frame.device:
                raise ValueError("%s: psf must be on the frame's device (%s)"
                                 % (who, frame.device))
        elif isinstance(psf, torch.Tensor):
            if psf.ndim != 3 or psf.shape[0] != n or psf.shape[2] != 6:
                raise ValueError("%s: psf: (nobj, ngauss_psf, 6) tensor or a GMixBatch" % who)
            if psf.device != frame.device:
                raise ValueError("%s: psf must be on the frame's device (%s)"
                                 % (who, frame.device))
        else:
            raise ValueError("%s: psf: (nobj, ngauss_psf, 6) tensor or a GMixBatch" % who)
    return p, name


def _weight_frame(frame, weight):
    """(the weight frame for the kernel, or None for w = 1; max(w, 0) as a
    tensor or the float 1.0)"""
    torch = _torch()
    if weight is None:
        return None, 1.0
    if isinstance(weight, torch.Tensor) and weight.ndim == 2:
        w = weight.detach().to(torch.float64).contiguous()
    else:
        if float(weight) == 1.0:
            return None, 1.0
        w = torch.full(tuple(frame.shape), float(weight), dtype=torch.float64,
                       device=frame.device)
    return w, torch.clamp(w, min=0.0)


def _render_fresh(nrow, ncol, gev, G, jac, pair_obj, tile_start):
    """a fresh frame of _scene_lists' records and lists (render_scene's bits)"""
    torch = _torch()
    dev = gev.device
    model = torch.empty((nrow, ncol), dtype=torch.float64, device=dev)
    with _on_device(dev):
        st = _lib.lib().ngmix_scene_render(_dptr(gev), G, _dptr(jac), _dptr(pair_obj),
                                           int(pair_obj.shape[0]), _dptr(tile_start), nrow, ncol,
                                           _dptr(model), 1, _stream())
    _lib.check(st, "ngmix_scene_render")
    return model


def _public(res):
    return {k: v for k, v in res.items() if not k.startswith("_")}


def normal_equations(frame, weight, jacobians, pars, model, psf=None, ngauss=None,
                     max_pairs=None):
    """
    The Gauss-Newton normal equations of a frame at pars, one band, no prior:
    with r = frame - render_scene(objects at pars) (computed here), w =
    max(weight, 0) and J_a = d model_a / d pars_a (deriv_images' convention, as
    autodiff.fisher(fast_exp=True)),
        F_self[a] = sum w J_a J_a^T   over a's clipped box, symmetric to the bit
        grad[a]   = sum w r J_a       (minus half the gradient of chi2)
        F_cross[p] = sum w J_a J_b^T  over box_a n box_b, (a, b) = pairs[p].

    frame: (nrow, ncol) float64 device tensor; weight: None (1), a scalar, or a
        tensor of the frame's shape (negative and zero weights drop out)
    jacobians: as render_scene's, one per object, in FRAME coordinates
    pars: (N, K) array or tensor, the model's parameters with one flux, K <= 8
    psf: GMixBatch or (N, P, 6) tensor with one mixture per object, or None
    max_pairs: refuse (ValueError naming the count) more (tile, object) pairs,
        or more candidate object pairs, than this; default 2^31 - 1

    Returns a dict of device tensors: F_self (N, K, K), grad (N, K), pairs
    (P, 2) int64 with a < b sorted by (a, b): the objects that share a frame
    tile and whose boxes intersect, F_cross (P, K, K), group (N,) int64: the
    connected components of the tile-sharing graph, numbered by their smallest
    member, chi2_group (ngroups,): sum w r^2 over the tiles of each group (every
    tile with objects belongs to exactly one group; summed in a fixed order),
    status (N,) int32: 0 or the code (_lib.ERR_*) with which the object was
    refused.  A refused object is left out of the model; its F_self and grad
    are NaN, it is in no pair, and every other object's numbers are bit for bit
    those of the catalogue without it.  No atomics: two calls give the same
    bits (csrc/scene_normal.hip).
    """
    fs = _Frames.one(frame, weight, jacobians, pars, model, psf, "normal_equations")
    return _public(_normal_frames(fs, fs.pars, ngauss, max_pairs))


def _own_inverse(F, bad):
    """(the inverse of every K x K block by Cholesky, not positive definite)"""
    torch = _torch()
    eye = torch.eye(F.shape[1], dtype=F.dtype, device=F.device).expand_as(F)
    L, info = torch.linalg.cholesky_ex(torch.where(bad[:, None, None], eye, F))
    return torch.cholesky_inverse(L), (info != 0) & ~bad


def _covariance(ne, max_group):
    """joint_covariance from a _normal_frames result"""
    from .flags import LM_SINGULAR_MATRIX
    torch = _torch()
    F = ne["F_self"]
    n, K = int(F.shape[0]), int(F.shape[1])
    dev = F.device
    layout = _GroupLayout(ne["_group"], max_group)
    flag = ne["status"].clone()
    bad = flag != 0
    eye = torch.eye(K, dtype=F.dtype, device=dev).expand_as(F)
    mats = layout.dense(torch.where(bad[:, None, None], eye, F), ne["pairs"], ne["F_cross"])
    inv, sing = [], torch.zeros(n, dtype=torch.bool, device=dev)
    for k, M in enumerate(mats):
        L, info = torch.linalg.cholesky_ex(M)
        inv.append(torch.cholesky_inverse(L))
        objs, failed = layout.per_object(info != 0, k)
        sing[torch.from_numpy(objs).to(dev)] = failed
    cov = layout.blocks(inv, K) if n else F.clone()
    sing = sing & ~bad
    cov = torch.where((bad | sing)[:, None, None], torch.full_like(cov, float("nan")), cov)
    flag = torch.where(sing, torch.full_like(flag, LM_SINGULAR_MATRIX), flag)
    joint_status = torch.from_numpy(layout.oversized.astype(np.int32)).to(dev)
    return dict(pars_cov=cov, flags=flag, group=ne["group"], joint_status=joint_status)


def joint_covariance(frame, weight, jacobians, pars, model, psf=None, ngauss=None,
                     max_pairs=None, max_group=16):
    """
    The covariance of every object of a frame marginalised over its neighbours:
    per group of connected objects (normal_equations' group) the dense
    (n_g K) x (n_g K) matrix of the group's F_self and F_cross blocks is
    inverted by Cholesky (groups bucketed by size, padded with identity) and
    each object gets its own K x K diagonal block of the inverse.
    LMBatchFitter's pars_cov0 convention: not rescaled by chi2 / dof.  For an
    isolated object this is autodiff.covariance of its pixels.

    Arguments as normal_equations; max_group: the objects of a larger group get
    the inverse of their own block alone, and joint_status 1.

    Returns a dict of device tensors: pars_cov (N, K, K), flags (N,) int32 as
    autodiff.covariance's (the refusal's code; a matrix that is not positive
    definite: NaN for every object of that group and flags.LM_SINGULAR_MATRIX),
    group (N,) int64, joint_status (N,) int32 (1: own block only).
    """
    _GroupLayout(np.zeros(0, dtype=np.int64), max_group)
    fs = _Frames.one(frame, weight, jacobians, pars, model, psf, "joint_covariance")
    return _covariance(_normal_frames(fs, fs.pars, ngauss, max_pairs), max_group)


def _joint_step(ne, layout, lam):
    """(delta (N, K), predicted decrease delta^T g per object's system (N,),
    solved (N,) bool) of (F + lam diag F) delta = g per system; lam: (N,) host,
    equal over a system's objects"""
    torch = _torch()
    F, g = ne["F_self"], ne["grad"]
    n, K = int(F.shape[0]), int(F.shape[1])
    dev = F.device
    bad = ne["status"] != 0
    eye = torch.eye(K, dtype=F.dtype, device=dev).expand_as(F)
    mats = layout.dense(torch.where(bad[:, None, None], eye, F), ne["pairs"], ne["F_cross"])
    g0 = torch.where(bad[:, None], torch.zeros_like(g), g)
    d_lam = torch.from_numpy(lam).to(dev)
    sols = []
    pred = torch.zeros(n, dtype=F.dtype, device=dev)
    solved = torch.zeros(n, dtype=torch.bool, device=dev)
    for k, M in enumerate(mats):
        rhs = layout.gather(g0, k)
        lam_k = layout.gather(d_lam[:, None].expand(n, K).contiguous(), k)
        D = torch.diagonal(M, dim1=1, dim2=2)
        L, info = torch.linalg.cholesky_ex(M + torch.diag_embed(lam_k * D))
        x = torch.cholesky_solve(rhs[:, :, None], L)[:, :, 0]
        ok = info == 0
        x = torch.where(ok[:, None], x, torch.zeros_like(x))
        sols.append(x)
        objs, p = layout.per_object((x * rhs).sum(dim=1), k)
        o = torch.from_numpy(objs).to(dev)
        pred[o] = p
        solved[o] = layout.per_object(ok, k)[1]
    delta = layout.scatter(sols, K, g) if n else g.clone()
    return delta, pred, solved & ~bad


# ------------------------------------------- conjugate gradients over the blocks

def _block_rows(pairs, n):
    """
    The row lists of the block-sparse matrix of n objects whose off-diagonal
    blocks are `pairs` (P, 2) (an integer tensor, on any device; a < b in every
    pair): object a gets one entry per pair that contains it, in ascending
    neighbour index.  Returns (row_start (n + 1,) int64, row_ent (2 P, 2)
    int32): the entries of object a are row_ent[row_start[a]:row_start[a + 1]],
    each (neighbour, code) with code = p when a is the first member of pair p
    (the block as stored) and -1 - p when it is the second (the block
    transposed).  One stable sort of 2 P keys; never an N x N array.
    """
    torch = _torch()
    dev = pairs.device
    n, P = int(n), int(pairs.shape[0])
    i64 = dict(dtype=torch.int64, device=dev)
    if P == 0:
        return torch.zeros(n + 1, **i64), torch.zeros((0, 2), dtype=torch.int32, device=dev)
    a, b = pairs[:, 0].to(torch.int64), pairs[:, 1].to(torch.int64)
    p = torch.arange(P, **i64)
    owner, nbr, code = torch.cat([a, b]), torch.cat([b, a]), torch.cat([p, -1 - p])
    _, order = torch.sort(owner * n + nbr, stable=True)
    row_ent = torch.stack([nbr[order], code[order]], dim=1).to(torch.int32).contiguous()
    counts = torch.bincount(owner, minlength=n)
    return torch.cat([torch.zeros(1, **i64), torch.cumsum(counts, 0)]), row_ent


def _group_segments(group, keep=None):
    """
    The objects sorted by group: group (n,) integer labels (a tensor, on any
    device), keep: None or an (n,) bool tensor, the objects that take part.
    Returns (seg_order (m,) int64, seg_start (ngroups + 1,) int64, index (n,)
    int64): the labels in ascending order are groups 0 .. ngroups - 1, index is
    every object's group, and group G's members that take part are
    seg_order[seg_start[G]:seg_start[G + 1]] in ascending index (a group of
    which no member takes part is an empty segment).
    """
    torch = _torch()
    dev = group.device
    i64 = dict(dtype=torch.int64, device=dev)
    if int(group.shape[0]) == 0:
        return torch.zeros(0, **i64), torch.zeros(1, **i64), torch.zeros(0, **i64)
    uniq, index = torch.unique(group.to(torch.int64), return_inverse=True)
    ngroups = int(uniq.shape[0])
    order = torch.argsort(index, stable=True)
    if keep is not None:
        order = order[keep[order]]
        counts = torch.bincount(index[keep], minlength=ngroups)
    else:
        counts = torch.bincount(index, minlength=ngroups)
    return order, torch.cat([torch.zeros(1, **i64), torch.cumsum(counts, 0)]), index


def _block_matvec(F_self, F_cross, row_start, row_ent, lam, x, want_xy=False):
    """ngmix_scene_block_matvec on contiguous float64 device tensors: y (n, K),
    and (want_xy) the per-object x . y (n,)"""
    torch = _torch()
    dev = F_self.device
    n, K = int(F_self.shape[0]), int(F_self.shape[1])
    y = torch.empty((n, K), dtype=torch.float64, device=dev)
    xy = torch.empty(n, dtype=torch.float64, device=dev) if want_xy else None
    with _on_device(dev):
        st = _lib.lib().ngmix_scene_block_matvec(
            _dptr(F_self), _dptr(F_cross), n, int(F_cross.shape[0]), K, _dptr(row_start),
            _dptr(row_ent), int(row_ent.shape[0]), _dptr(lam), _dptr(x), _dptr(y), _dptr(xy),
            _stream())
    _lib.check(st, "ngmix_scene_block_matvec")
    return (y, xy) if want_xy else y


_SOLVE_KEYS = ("F_self", "grad", "pairs", "F_cross", "group", "status")


def _solve_arguments(ne, lam, tol, maxiter, check_every, who):
    """solve_normal's arguments, checked on the host before a device is asked
    for.  Returns lam as an (N,) host array"""
    torch = _torch()
    if not hasattr(ne, "keys") or any(k not in ne for k in _SOLVE_KEYS):
        raise ValueError("%s: ne must be a dict with %s" % (who, ", ".join(_SOLVE_KEYS)))
    for k in _SOLVE_KEYS:
        if not isinstance(ne[k], torch.Tensor):
            raise ValueError("%s: ne['%s'] must be a tensor" % (who, k))
        if ne[k].device != ne["F_self"].device:
            raise ValueError("%s: ne['%s'] must be on the device of F_self (%s)"
                             % (who, k, ne["F_self"].device))
    F, C, pairs = ne["F_self"], ne["F_cross"], ne["pairs"]
    if F.ndim != 3 or F.shape[1] != F.shape[2]:
        raise ValueError("%s: F_self must be (N, K, K)" % who)
    n, K = int(F.shape[0]), int(F.shape[1])
    if K < 1 or K > NORMAL_KMAX:
        raise ValueError("%s: K must be 1..%d parameters per object, got %d"
                         % (who, NORMAL_KMAX, K))
    if tuple(ne["grad"].shape) != (n, K):
        raise ValueError("%s: grad must be (%d, %d)" % (who, n, K))
    if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int64:
        raise ValueError("%s: pairs must be (P, 2) int64" % who)
    if tuple(C.shape) != (int(pairs.shape[0]), K, K):
        raise ValueError("%s: F_cross must be (%d, %d, %d)" % (who, int(pairs.shape[0]), K, K))
    for k in ("F_self", "grad", "F_cross"):
        if ne[k].dtype != torch.float64:
            raise ValueError("%s: %s must be float64" % (who, k))
    for k in ("group", "status"):
        if tuple(ne[k].shape) != (n,) or ne[k].dtype.is_floating_point:
            raise ValueError("%s: %s must be (%d,) integers" % (who, k, n))
    if isinstance(lam, torch.Tensor):
        lam = lam.detach().cpu().numpy()
    try:
        lam = np.asarray(lam, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: lam must be a scalar or an (N,) array" % who)
    if lam.ndim == 0:
        lam = np.full(n, float(lam))
    if lam.shape != (n,):
        raise ValueError("%s: lam must be a scalar or have one entry per object (%d)" % (who, n))
    if not np.all(np.isfinite(lam)) or np.any(lam < 0.0):
        raise ValueError("%s: lam must be finite and >= 0" % who)
    _cg_arguments(tol, maxiter, who, "tol", "maxiter")
    if int(check_every) < 1:
        raise ValueError("%s: check_every must be at least 1, got %d" % (who, int(check_every)))
    return lam


def _cg_arguments(tol, maxiter, who, tol_name, maxiter_name):
    if not (float(tol) >= 0.0) or not np.isfinite(float(tol)):
        raise ValueError("%s: %s must be finite and >= 0" % (who, tol_name))
    if int(maxiter) < 1:
        raise ValueError("%s: %s must be at least 1, got %d" % (who, maxiter_name, int(maxiter)))


def _solve(ne, lam, tol, maxiter, check_every, only=None):
    """solve_normal on checked arguments; lam (N,) host, equal over a group;
    only: None, or an (N,) host bool array: the objects that take part (whole
    groups), the others are left out as refused objects are"""
    torch = _torch()
    F, g, pairs, C = ne["F_self"], ne["grad"], ne["pairs"], ne["F_cross"]
    dev = _require_cuda(F.device)
    n, K = int(F.shape[0]), int(F.shape[1])
    f64 = dict(dtype=torch.float64, device=dev)
    if n == 0:
        return dict(delta=torch.zeros((0, K), **f64),
                    cg_iter=torch.zeros(0, dtype=torch.int64, device=dev),
                    cg_converged=torch.zeros(0, dtype=torch.bool, device=dev),
                    cg_failed=torch.zeros(0, dtype=torch.bool, device=dev),
                    cg_resid=torch.zeros(0, **f64))
    take = ne["status"] == 0
    if only is not None:
        take = take & torch.from_numpy(np.ascontiguousarray(only, dtype=bool)).to(dev)
    eye = torch.eye(K, **f64).expand(n, K, K)
    Fu = torch.where(take[:, None, None], F, eye).contiguous()
    gu = torch.where(take[:, None], g, torch.zeros_like(g)).contiguous()
    if int(pairs.shape[0]) and int(take.sum()) < n:
        inside = take[pairs[:, 0]] & take[pairs[:, 1]]
        pairs, C = pairs[inside], C[inside]
    C = C.contiguous()
    row_start, row_ent = _block_rows(pairs, n)
    seg_order, seg_start, index = _group_segments(ne["group"], take)
    ngroups = int(seg_start.shape[0]) - 1
    obj_group = torch.where(take, index, torch.full_like(index, -1)).to(torch.int32)
    d_lam = torch.from_numpy(np.ascontiguousarray(lam, dtype=np.float64)).to(dev)
    own = Fu + d_lam[:, None, None] * torch.diag_embed(torch.diagonal(Fu, dim1=1, dim2=2))
    Minv, sing = _own_inverse(own, ~take)
    # an own block that is not positive definite: NaN, so the group's first
    # r^T Minv r is not finite and the group is failed before it iterates
    Minv = torch.where(sing[:, None, None], torch.full_like(Minv, float("nan")),
                       Minv).contiguous()
    x, r, p, z, q = (torch.zeros((n, K), **f64) for _ in range(5))
    part = torch.zeros(n, **f64)
    gscal = torch.zeros((ngroups, 4), **f64)
    grec = torch.zeros((ngroups, 4), dtype=torch.int32, device=dev)
    L = _lib.lib()
    spent, init = 0, 1
    while True:
        k = min(int(check_every), int(maxiter) - spent)
        with _on_device(dev):
            st = L.ngmix_scene_pcg(
                _dptr(Fu), _dptr(C), n, int(C.shape[0]), K, _dptr(row_start), _dptr(row_ent),
                int(row_ent.shape[0]), _dptr(d_lam), _dptr(Minv), _dptr(gu), _dptr(obj_group),
                _dptr(seg_order), int(seg_order.shape[0]), _dptr(seg_start), ngroups, _dptr(x),
                _dptr(r), _dptr(p), _dptr(z), _dptr(q), _dptr(part), _dptr(gscal), _dptr(grec),
                float(tol), init, k, _stream())
        _lib.check(st, "ngmix_scene_pcg")
        spent, init = spent + k, 0
        # the one read-back per check_every iterations
        if bool(grec[:, 0].cpu().numpy().all()) or spent >= int(maxiter):
            break
    done, failed = grec[index, 0] != 0, grec[index, 2] != 0
    rz, rz0 = gscal[index, 0], gscal[index, 1]
    resid = torch.where(rz0 > 0.0, torch.sqrt(torch.clamp(rz, min=0.0) / rz0),
                        torch.where(failed, torch.full_like(rz, float("nan")),
                                    torch.zeros_like(rz)))
    return dict(delta=torch.where(take[:, None], x, torch.zeros_like(x)),
                cg_iter=torch.where(take, grec[index, 1].to(torch.int64),
                                    torch.zeros_like(index)),
                cg_converged=take & done & ~failed, cg_failed=take & failed,
                cg_resid=torch.where(take, resid, torch.zeros_like(resid)))


def solve_normal(ne, lam=0.0, tol=1e-8, maxiter=200, check_every=8):
    """
    Solve (F + lam diag F) delta = grad over the blocks of normal_equations,
    every group of connected objects as one system, by block-Jacobi
    preconditioned conjugate gradients on the device (csrc/scene_solve.hip;
    DESIGN.md section 3.17): what a group too large for a dense solve steps
    with.  F is the block-sparse symmetric matrix of F_self and F_cross.

    ne: a normal_equations result, or any dict of device tensors with F_self
        (N, K, K), grad (N, K), pairs (P, 2) int64 (a < b), F_cross (P, K, K),
        group (N,) and status (N,)
    lam: the damping factor, a scalar or an (N,) array that is equal over a
        group (a group takes its members' largest)
    tol: a group has converged when r^T M^-1 r <= tol^2 times its starting
        value, r the (recurred) residual and M the preconditioner: the own
        blocks (F_aa + lam diag F_aa)
    maxiter: iterations at most (block-Jacobi is a weak preconditioner for a
        frame that percolates into one group: DESIGN.md section 3.17 measured 701
        iterations to tol = 1e-8 on 29,970 connected objects)
    check_every: the host reads the groups' done flags back once per this many
        iterations (the only synchronisation) and stops when all are done

    Returns a dict of device tensors: delta (N, K), cg_iter (N,) int64: the
    iterations of the object's group, cg_converged (N,) bool, cg_failed (N,)
    bool: breakdown, p^T A p <= 0 or a scalar that is not finite (the matrix is
    not positive definite to rounding; also an own block that Cholesky refuses),
    cg_resid (N,): sqrt(r^T M^-1 r / its starting value) of the object's group.
    A group with a zero right-hand side has delta = 0 after 0 iterations.  A
    group that is done is frozen on the device: its bits depend neither on the
    other groups nor on check_every.  An object with status != 0 (NaN blocks)
    gets delta = 0 and converged False, is in no row list and no sum, and leaves
    every other object's bits those of the catalogue without it.  No atomics:
    two calls give the same bits.
    """
    lam = _solve_arguments(ne, lam, tol, maxiter, check_every, "solve_normal")
    dev = _require_cuda(ne["F_self"].device)
    n = int(lam.shape[0])
    if n:
        group = np.asarray(ne["_group"]) if "_group" in ne else ne["group"].cpu().numpy()
        _, index = np.unique(group, return_inverse=True)
        g_lam = np.zeros(int(index.max()) + 1)
        np.maximum.at(g_lam, index.reshape(-1), lam)
        lam = g_lam[index.reshape(-1)]
    with _on_device(dev):
        return _solve(ne, lam, float(tol), int(maxiter), int(check_every))


def fit_joint(frame, weight, jacobians, guess, model, psf=None, maxiter=50, tol=1e-6,
              lambda0=1e-3, max_group=16, large_groups="jacobi", cg_tol=1e-8, cg_maxiter=200):
    """
    Fit all the objects of a frame together (a joint, MOF-style fit), ONE band
    and NO prior: Levenberg-Marquardt over normal_equations, with one damping
    factor lambda per group of connected objects.

    frame, weight, jacobians, psf: normal_equations' arguments
    guess: (N, K) starting parameters, the model's with one flux, K <= 8
    maxiter: iterations; each makes one normal_equations call and one trial
        render_scene (every loop here is bounded by it)
    tol: a group has converged when an accepted step's predicted decrease
        delta^T g is at most tol.  The unit is chi2, so the default 1e-6 is far
        below any statistical meaning
    lambda0: the starting lambda; it never goes below scene.LAMBDA_FLOOR
    max_group: the objects of a larger group step with their own blocks only
        (block-Jacobi) and carry joint_status 1 -- with large_groups="jacobi"
    large_groups: "jacobi", or "cg": a group of more than max_group objects
        steps with solve_normal's delta at the group's lambda (conjugate
        gradients over all of its blocks, to cg_tol, cg_maxiter iterations at
        most); its predicted decrease is delta^T g summed in a fixed order, and
        a solve that failed or did not converge counts as a system that cannot
        be solved.  Such objects carry joint_status 2.  Groups of up to
        max_group objects take the dense solve either way, with the same bits.
        pars_cov of a joint_status 2 object is still the inverse of its own
        block: its marginal covariance would take K solves per object

    Per iteration the groups are those of the current parameters.  Every group
    that has not converged solves (F + lambda diag F) delta = g over its dense
    system; the trial parameters of all groups are rendered into one frame, and
    a group accepts its step when chi2 = sum w r^2 over ITS CURRENT TILES
    decreases: lambda <- lambda / 10; otherwise, or when a trial object is
    refused or the system cannot be solved, lambda <- 10 lambda and the group
    keeps its parameters.  The decision ignores what the trial's grown boxes add
    outside those tiles (inside another group's tiles or in empty ones); the
    next iteration's groups see it.  When groups merge, the merged group takes
    its members' largest lambda and converges anew.

    Returns a dict of host arrays: pars (N, K), pars_cov (N, K, K):
    joint_covariance at pars, bit for bit, pars_err (N, K), flags (N,) int32
    (joint_covariance's; flags.MAXITER for an object of a group that did not
    converge), group (N,), niter (N,): the iterations the object's group took
    part in, converged (N,) bool, joint_status (N,), chi2: sum w r^2 of the
    whole frame at pars, recomputed, lambda (N,), and cg_iter (N,): the
    conjugate-gradient iterations spent on the object's groups, all LM
    iterations together (0 with large_groups="jacobi").
    """
    kw = _fit_keywords("fit_joint", maxiter, tol, lambda0, max_group, large_groups, cg_tol,
                       cg_maxiter)
    fs = _Frames.one(frame, weight, jacobians, guess, model, psf, "fit_joint")
    return _fit_loop(fs, fs.pars, **kw)


def _fit_keywords(who, maxiter, tol, lambda0, max_group, large_groups, cg_tol, cg_maxiter):
    """fit_joint's keywords, checked on the host; as _fit_loop takes them"""
    maxiter = int(maxiter)
    if maxiter < 1:
        raise ValueError("%s: maxiter must be at least 1, got %d" % (who, maxiter))
    if not (float(tol) >= 0.0) or not (float(lambda0) > 0.0):
        raise ValueError("%s: tol must be >= 0 and lambda0 > 0" % who)
    if large_groups not in ("jacobi", "cg"):
        raise ValueError("%s: large_groups must be 'jacobi' or 'cg', got %r"
                         % (who, large_groups))
    _cg_arguments(cg_tol, cg_maxiter, who, "cg_tol", "cg_maxiter")
    _GroupLayout(np.zeros(0, dtype=np.int64), max_group)
    return dict(maxiter=maxiter, tol=float(tol), lambda0=float(lambda0), max_group=max_group,
                cg=large_groups == "cg", cg_tol=float(cg_tol), cg_maxiter=int(cg_maxiter))


def _fit_loop(problem, pars, maxiter, tol, lambda0, max_group, cg, cg_tol, cg_maxiter):
    """fit_joint's Levenberg-Marquardt loop, one lambda per group, over a
    problem (_Frames) that gives normal(pars), trial(ne, trial, ngroups) and
    chi2(ne)"""
    from .flags import MAXITER
    torch = _torch()
    dev = pars.device
    n, K = int(pars.shape[0]), int(pars.shape[1])
    lam = np.full(n, float(lambda0))
    conv = np.zeros(n, dtype=bool)
    niter = np.zeros(n, dtype=np.int64)
    cg_iter = np.zeros(n, dtype=np.int64)
    for _ in range(maxiter):
        ne = problem.normal(pars)
        group = ne["_group"]
        ngroups = int(group.max()) + 1 if n else 0
        ok_obj = ne["status"].cpu().numpy() == 0
        # a group is at rest when all of its (fittable) members have converged
        g_lam = np.zeros(ngroups)
        np.maximum.at(g_lam, group, lam)
        g_rest = np.ones(ngroups, dtype=bool)
        np.logical_and.at(g_rest, group, conv | ~ok_obj)
        lam = g_lam[group]
        conv = np.where(ok_obj, g_rest[group], False)
        active = ~g_rest[group] & ok_obj
        if not active.any():
            break
        niter[active] += 1
        layout = _GroupLayout(group, max_group)
        delta, pred, solved = _joint_step(ne, layout, lam)
        big = layout.oversized & active if cg else np.zeros(n, dtype=bool)
        if big.any():
            sol = _solve(ne, lam, float(cg_tol), int(cg_maxiter), 8, only=big)
            d_big = torch.from_numpy(big).to(dev)
            delta = torch.where(d_big[:, None], sol["delta"], delta)
            solved = torch.where(d_big, sol["cg_converged"], solved)
            cg_iter[big] += sol["cg_iter"].cpu().numpy()[big]
        d_active = torch.from_numpy(active).to(dev)
        trial = torch.where(d_active[:, None], pars + delta, pars)
        new, trial_flag = problem.trial(ne, trial, ngroups)
        old = ne["chi2_group"].cpu().numpy()
        refused = np.zeros(ngroups, dtype=bool)
        np.logical_or.at(refused, group, (trial_flag.cpu().numpy() != 0) & ok_obj)
        unsolved = np.zeros(ngroups, dtype=bool)
        np.logical_or.at(unsolved, group, ~solved.cpu().numpy() & ok_obj)
        accept_g = (new < old) & ~refused & ~unsolved
        if big.any():
            # delta^T g of a group: per object in ascending parameter, then the
            # group's objects in ascending index
            dg = (delta * ne["grad"]).cpu().numpy()
            pred_b = np.zeros(n)
            for k in range(K):
                pred_b = pred_b + np.where(big, dg[:, k], 0.0)
            pred_g = np.zeros(ngroups)
            np.add.at(pred_g, group, pred_b)
            pred_o = np.where(big, pred_g[group], pred.cpu().numpy())
        elif layout.oversized.any() and not cg:
            # block-Jacobi members step one by one but are judged with their group
            pred_g = np.zeros(ngroups)
            np.add.at(pred_g, group, np.where(active, pred.cpu().numpy(), 0.0))
            pred_o = pred_g[group]
        else:
            pred_o = pred.cpu().numpy()
        accept = accept_g[group] & active
        pars = torch.where(torch.from_numpy(accept).to(dev)[:, None], trial, pars)
        lam = np.where(accept, np.maximum(lam / 10.0, LAMBDA_FLOOR),
                       np.where(active, lam * 10.0, lam))
        conv = conv | (accept & (pred_o <= float(tol)))
    ne = problem.normal(pars)
    cov = _covariance(ne, max_group)
    group = ne["_group"]
    ngroups = int(group.max()) + 1 if n else 0
    g_conv = np.ones(ngroups, dtype=bool)
    np.logical_and.at(g_conv, group, conv)
    conv = g_conv[group] if n else conv
    flags = cov["flags"].cpu().numpy().astype(np.int32)
    flags = np.where((flags == 0) & ~conv, MAXITER, flags).astype(np.int32)
    pars_cov = cov["pars_cov"].cpu().numpy()
    with np.errstate(invalid="ignore"):
        pars_err = np.sqrt(np.einsum("nii->ni", pars_cov))
    return {"pars": pars.cpu().numpy(), "pars_cov": pars_cov, "pars_err": pars_err,
            "flags": flags, "group": group.copy(), "niter": niter, "converged": conv,
            "joint_status": cov["joint_status"].cpu().numpy() * (2 if cg else 1),
            "chi2": problem.chi2(ne), "lambda": lam, "cg_iter": cg_iter}


# ------------------------------------- normal equations of many frames (3.18)
# (and, with F = 1, of the one frame of the section above)

FRAMES_KMAX = 16         # csrc/scene_normal_frames.hip: SNF_KMAX


def _frames_pairs(pairs, n):
    """the union of the frames' pair lists [(P_f, 2) int64 tensor, ...] (one
    device): (P, 2) int64, every pair once, sorted by (a, b).  One list is its
    own union: _scene_pairs gives it unique and sorted"""
    torch = _torch()
    if len(pairs) == 1:
        return pairs[0]
    allp = torch.cat([p.reshape(-1, 2) for p in pairs]) if len(pairs) else \
        torch.zeros((0, 2), dtype=torch.int64)
    if int(allp.shape[0]) == 0:
        return allp.to(torch.int64)
    key = torch.unique(allp[:, 0].to(torch.int64) * int(n) + allp[:, 1].to(torch.int64))
    a = torch.div(key, int(n), rounding_mode="floor")
    return torch.stack([a, key - a * int(n)], dim=1)


def _frames_arguments(frames, weights, jacobians, pars, model, psf, frame_band, who):
    """the arguments every call over a list of frames shares, checked on the
    host before a device is asked for.  Returns (pars tensor (N, K) float64 on
    the frames' device, model name, frame_band (F,) int64 host array, the
    weights as a list of F entries)"""
    from . import autodiff
    torch = _torch()
    if not isinstance(frames, (list, tuple)) or len(frames) == 0:
        raise ValueError("%s: frames must be a non-empty sequence of 2-d device tensors" % who)
    F = len(frames)
    for f, fr in enumerate(frames):
        if not isinstance(fr, torch.Tensor) or fr.ndim != 2:
            raise ValueError("%s: frame %d must be a 2-d device tensor" % (who, f))
        if fr.dtype != torch.float64:
            raise ValueError("%s: frame %d must be float64, got %s" % (who, f, fr.dtype))
        if fr.shape[0] < 1 or fr.shape[1] < 1:
            raise ValueError("%s: frame %d needs nrow * ncol > 0, got %r"
                             % (who, f, tuple(fr.shape)))
        if fr.device != frames[0].device:
            raise ValueError("%s: frame %d is on %s, frame 0 on %s"
                             % (who, f, fr.device, frames[0].device))
    dev = frames[0].device
    if isinstance(weights, (list, tuple)):
        if len(weights) != F:
            raise ValueError("%s: %d weights for %d frames" % (who, len(weights), F))
        weights = list(weights)
    elif isinstance(weights, torch.Tensor) and weights.ndim != 0:
        raise ValueError("%s: weights must be None, a scalar, or one entry per frame" % who)
    else:
        weights = [weights] * F
    for f, w in enumerate(weights):
        if isinstance(w, torch.Tensor) and w.ndim != 0:
            if tuple(w.shape) != tuple(frames[f].shape):
                raise ValueError("%s: weight %d must be None, a scalar or have the shape of "
                                 "frame %d, %r" % (who, f, f, tuple(frames[f].shape)))
            if w.device != dev:
                raise ValueError("%s: weight %d must be on the frames' device (%s)"
                                 % (who, f, dev))
    if isinstance(pars, torch.Tensor):
        if pars.device != dev:
            raise ValueError("%s: pars must be on the frames' device (%s)" % (who, dev))
        p = pars.detach().to(torch.float64)
    else:
        p = torch.from_numpy(np.array(pars, dtype=np.float64))
    if p.ndim != 2:
        raise ValueError("%s: pars must be (nobj, npars)" % who)
    n, K = int(p.shape[0]), int(p.shape[1])
    name = autodiff._model_name(model)
    if name == "coellip" or name not in autodiff._NLOC:
        raise ValueError("%s: model '%s' has no [shape, one flux per band] layout: not built"
                         % (who, name))
    nshape = autodiff._NLOC[name] - 1
    if K > FRAMES_KMAX:
        raise ValueError("%s: at most %d parameters per object, got K = %d"
                         % (who, FRAMES_KMAX, K))
    nband = K - nshape
    if nband < 1:
        raise ValueError("%s: model '%s' needs %d shape parameters and one flux per band, got "
                         "K = %d" % (who, name, nshape, K))
    try:
        njac = len(jacobians)
    except TypeError:
        raise ValueError("%s: jacobians must be a sequence with one entry per frame" % who)
    if njac != F:
        raise ValueError("%s: %d jacobian sets for %d frames" % (who, njac, F))
    for f in range(F):
        _check_jacobians(jacobians[f], n, "%s: frame %d" % (who, f))
    if frame_band is None:
        if F != nband:
            raise ValueError("%s: frame_band is required when the %d frames are not one per "
                             "band (nband = %d)" % (who, F, nband))
        band = np.arange(F, dtype=np.int64)
    else:
        if isinstance(frame_band, torch.Tensor):
            frame_band = frame_band.detach().cpu().numpy()
        band = np.asarray(frame_band)
        if band.shape != (F,) or band.dtype.kind not in "iu":
            raise ValueError("%s: frame_band must be (%d,) integers" % (who, F))
        band = band.astype(np.int64)
        for f in range(F):
            if band[f] < 0 or band[f] >= nband:
                raise ValueError("%s: frame_band[%d] = %d is outside [0, %d)"
                                 % (who, f, band[f], nband))
    if psf is not None:
        if not isinstance(psf, (list, tuple)) or len(psf) != F:
            raise ValueError("%s: psf must be None or a sequence with one entry per frame (%d)"
                             % (who, F))
        P = None
        for f, q in enumerate(psf):
            if isinstance(q, GMixBatch):
                nq, Pq, qdev = q.n, q.ngauss, q.device
            elif isinstance(q, torch.Tensor) and q.ndim == 3 and q.shape[2] == 6:
                nq, Pq, qdev = int(q.shape[0]), int(q.shape[1]), q.device
            else:
                raise ValueError("%s: psf[%d]: (nobj, ngauss_psf, 6) tensor or a GMixBatch"
                                 % (who, f))
            if nq != n:
                raise ValueError("%s: psf[%d] must hold one mixture per object (%d), got %d"
                                 % (who, f, n, nq))
            if torch.device(qdev) != dev:
                raise ValueError("%s: psf[%d] must be on the frames' device (%s)"
                                 % (who, f, dev))
            if P is not None and Pq != P:
                raise ValueError("%s: psf[%d] has %d gaussians, psf[0] has %d: P must be the "
                                 "same in all frames" % (who, f, Pq, P))
            P = Pq if P is None else P
    return p, name, band, weights


class _Frames(object):
    """the checked arguments of a joint call, on the device, and what _fit_loop
    asks of its problem: normal(pars), trial(ne, trial, ngroups) and chi2(ne).
    The one-frame API (normal_equations, joint_covariance, fit_joint) comes in
    through one(): it is the case F = 1, band [0], no prior"""

    def __init__(self, frames, weights, jacobians, pars, model, psf, frame_band, prior, who):
        from .prior_batch import as_batch_prior
        pars, name, band, weights = _frames_arguments(frames, weights, jacobians, pars, model, psf,
                                                      frame_band, who)
        self._fill(frames, weights, jacobians, pars, name, psf, band, as_batch_prior(prior))

    @classmethod
    def one(cls, frame, weight, jacobians, pars, model, psf, who):
        """the one-frame API's arguments, checked by _joint_arguments (its
        messages, K <= NORMAL_KMAX and the one-flux rule are that API's)"""
        pars, name = _joint_arguments(frame, weight, jacobians, pars, model, psf, who)
        self = cls.__new__(cls)
        self._fill([frame], [weight], [jacobians], pars, name, None if psf is None else [psf],
                   np.zeros(1, dtype=np.int64), None)
        return self

    def _fill(self, frames, weights, jacobians, pars, name, psf, band, prior):
        from . import autodiff
        torch = _torch()
        self.name, self.band, self.prior = name, band, prior
        dev = _require_cuda(frames[0].device)
        self.dev = dev
        self.pars = pars.to(dev)
        self.n, self.K = int(pars.shape[0]), int(pars.shape[1])
        self.F = len(frames)
        self.nshape = autodiff._NLOC[self.name] - 1
        self.frames = [fr.detach().contiguous() for fr in frames]
        self.shapes = [(int(fr.shape[0]), int(fr.shape[1])) for fr in frames]
        ww = [_weight_frame(fr, w) for fr, w in zip(self.frames, weights)]
        self.wframes = [w[0] for w in ww]
        self.wpos = [w[1] for w in ww]
        self.jacs = [_jacobian_tensor(jacobians[f], self.n, dev) for f in range(self.F)]
        # the "stamps" of autodiff's layout: object-major, stamp o * F + f
        self.stamp_obj = np.repeat(np.arange(self.n, dtype=np.int64), self.F)
        self.stamp_band = np.tile(self.band, self.n)
        self.psf = None
        if psf is not None and self.n:
            per = [autodiff._psf_tensor(q.detach() if isinstance(q, torch.Tensor) else q,
                                        self.n, dev) for q in psf]
            # (one frame: its tensor as it is, no copy)
            self.psf = per[0] if self.F == 1 else \
                torch.stack(per, dim=1).reshape(self.n * self.F, -1, 6).contiguous()

    def normal(self, pars):
        return _normal_frames(self, pars, None, None)

    def trial(self, ne, trial, ngroups):
        fm = _frames_model(self, trial, None, None, False)
        resids = [fr - m for fr, m in zip(self.frames, fm["models"])]
        new = _frames_chi2_group(self, resids, ne["_tile_group"], ne["_group"], ngroups,
                                 _prior_ff(self, trial, fm["flag"]))[0]
        return new, fm["flag"]

    def chi2(self, ne):
        tot = 0.0
        for fr, m, w in zip(self.frames, ne["_models"], self.wpos):
            r = fr - m
            tot = tot + float((r * r * w).sum())
        return tot + float(ne["_prior_ff"].sum())


def _prior_ff(fs, pars, flag):
    """the prior's r.r per object at pars (host (N,); 0 without a prior and for
    a refused object; inf where the prior is out of range)"""
    if fs.prior is None or fs.n == 0:
        return np.zeros(fs.n)
    r0, bad0 = fs.prior.fill_fdiff_batch(pars)
    ff = (r0 * r0).sum(dim=1)
    ff = _torch().where(bad0, _torch().full_like(ff, float("inf")), ff)
    return np.where(flag.cpu().numpy() != 0, 0.0, ff.cpu().numpy())


def _frames_chi2_group(fs, resids, tile_group, group, ngroups, prior_ff):
    """(chi2 per group: the fixed-order sum over the frames of the group's
    per-tile sum w r^2, r = resids[f] = frame f - its model, plus its members'
    prior r.r in ascending index; the frames' per-tile sums)"""
    chi2 = np.zeros(ngroups)
    tile_chi2 = []
    for f in range(fs.F):
        r = resids[f]
        t = _tile_sums(r * r * fs.wpos[f]).cpu().numpy()
        tile_chi2.append(t)
        chi2 = chi2 + _segment_sums(t, tile_group[f], ngroups)
    if fs.prior is not None:
        chi2 = chi2 + _segment_sums(prior_ff, group, ngroups)
    return chi2, tile_chi2


def _frames_model(fs, pars, ngauss, max_pairs, tangents):
    """the objects at pars in every frame: per frame the gaussian records, the
    scene lists and the model frame (render_scene's bits); with tangents: and
    d mixture / d (the frame's Kloc local parameters).  An object refused in
    any frame is left out of every frame: flag is its first refusal's code, in
    frame order"""
    from . import autodiff
    torch = _torch()
    dev, n, F = fs.dev, fs.n, fs.F
    geom = autodiff._SceneGeometry(n * F, dev)
    if tangents:
        (_, _, mix, code, _), dmix = autodiff._mixture_tangents(
            geom, pars, fs.name, fs.psf, fs.stamp_obj, fs.stamp_band, ngauss)
    else:
        _, _, mix, code, _ = autodiff._stamp_mixtures(geom, pars, fs.name, fs.psf, fs.stamp_obj,
                                                      fs.stamp_band, ngauss)
        dmix = None
    G = int(mix.shape[1])
    mix = mix.reshape(n, F, G, 6)
    code = code.reshape(n, F)

    def lists(f, rec):
        return _scene_lists(fs.shapes[f][0], fs.shapes[f][1], rec, G, n, fs.jacs[f], max_pairs,
                            boxes_to_host=True)

    def without(rec, out):
        # all-zero records, which the norms refuse (as autodiff.scene_render)
        return torch.where(out.repeat_interleave(G)[:, None], torch.zeros_like(rec), rec)

    recs, sl, flags = [], [], []
    for f in range(F):
        rec = without(autodiff._gauss_records(mix[:, f].contiguous(), True), code[:, f] != 0)
        recs.append(rec)
        sl.append(lists(f, rec))
        flags.append(torch.where(code[:, f] == 0, sl[f][1], code[:, f]))
    flag = flags[0]
    for f in range(1, F):
        flag = torch.where((flag == 0) & (flags[f] != 0), flags[f], flag)
    # an object refused in another frame is taken out of this one's lists; with
    # one frame there is no other, and nothing to read back
    if F > 1:
        dead = flag != 0
        if bool(dead.any()):
            for f in range(F):
                if bool((dead & (flags[f] == 0)).any()):
                    recs[f] = without(recs[f], dead)
                    sl[f] = lists(f, recs[f])
    models = [_render_fresh(fs.shapes[f][0], fs.shapes[f][1], sl[f][0], G, fs.jacs[f], sl[f][3],
                            sl[f][4]) for f in range(F)]
    A = None
    if tangents:
        d5 = dmix.reshape(n, F, G, 6, fs.K)
        if fs.K == fs.nshape + 1:
            # one band: every column is local in every frame (F = 1: a view)
            A = d5.permute(1, 0, 2, 3, 4).contiguous()
        else:
            # the Kloc = nshape + 1 columns that are not zero in frame f
            cols = np.concatenate([np.tile(np.arange(fs.nshape), (F, 1)),
                                   (fs.nshape + fs.band)[:, None]], axis=1)
            A = torch.stack([d5[:, f][..., torch.from_numpy(cols[f]).to(dev)]
                             for f in range(F)]).contiguous()
    return dict(G=G, recs=recs, A=A, flag=flag, boxes=[s[2] for s in sl],
                pair_obj=[s[3] for s in sl], tile_start=[s[4] for s in sl], models=models)


def _scene_normal(fs, fm, resids, items_host, one_frame=None):
    """
    The blocks (nitems, K, K) and vectors (nitems, K) of the (nitems, 2) int32
    host item table, from fm = _frames_model(fs, ..., tangents=True) and the
    frames' residuals: the one place that launches the normal-equation kernels.

    One frame of one band (K == Kloc) goes through ngmix_scene_normal, anything
    else through ngmix_scene_normal_frames.  There the two give the same bits
    (scene_normal_frames_kernel adds the one frame's block once into +0, under
    the identity column map), so the choice is speed only: the one-frame kernel
    was measured about 6 % faster over the same blocks, at 104 against 136
    VGPRs.  one_frame: True / False force an entry (the
    tests hold the two together through it).
    """
    torch = _torch()
    dev, n, K, F, G = fs.dev, fs.n, fs.K, fs.F, fm["G"]
    Kloc = fs.nshape + 1
    if one_frame is None:
        one_frame = F == 1 and K == Kloc
    elif one_frame and not (F == 1 and K == Kloc):
        raise ValueError("scene: ngmix_scene_normal takes one frame of one band")
    nitems = int(items_host.shape[0])
    mat = torch.empty((nitems, K, K), dtype=torch.float64, device=dev)
    vec = torch.empty((nitems, K), dtype=torch.float64, device=dev)
    items_host = np.ascontiguousarray(items_host, dtype=np.int32)
    items = torch.from_numpy(items_host).to(dev)
    boxes = torch.from_numpy(np.ascontiguousarray(np.stack(fm["boxes"]), dtype=np.int32)).to(dev)
    L = _lib.lib()
    if one_frame:
        w = fs.wframes[0]
        with _on_device(dev):
            st = L.ngmix_scene_normal(
                _dptr(fm["recs"][0]), G, _dptr(fs.jacs[0]), n, _dptr(fm["A"]), K,
                _dptr(w) if w is not None else None, _dptr(resids[0]), fs.shapes[0][0],
                fs.shapes[0][1], _dptr(boxes), _dptr(items), _lib.ptr(items_host), nitems,
                _dptr(mat), _dptr(vec), _stream())
        _lib.check(st, "ngmix_scene_normal")
        return mat, vec
    rec = torch.cat(fm["recs"]).contiguous()
    jac = torch.cat(fs.jacs).contiguous()
    table = np.zeros(F, dtype=_lib.SCENE_FRAME_DTYPE)
    for f in range(F):
        table[f] = (resids[f].data_ptr(),
                    fs.wframes[f].data_ptr() if fs.wframes[f] is not None else 0,
                    fs.shapes[f][0], fs.shapes[f][1], int(fs.band[f]), 0)
    d_table = torch.from_numpy(table.view(np.uint8)).to(dev)
    with _on_device(dev):
        st = L.ngmix_scene_normal_frames(
            _dptr(rec), G, _dptr(jac), n, _dptr(fm["A"]), Kloc, K, _dptr(d_table),
            _lib.ptr(table), F, _dptr(boxes), _dptr(items), _lib.ptr(items_host), nitems,
            _dptr(mat), _dptr(vec), _stream())
    _lib.check(st, "ngmix_scene_normal_frames")
    return mat, vec


def _normal_frames(fs, pars, ngauss, max_pairs):
    """normal_equations and normal_equations_frames on checked arguments (fs);
    their dict plus what _fit_loop and _Frames read: _tile_chi2, _tile_group
    (per frame, host), _group, _models, _prior_ff"""
    from .prior_batch import prior_normal_sums
    torch = _torch()
    dev, n, K, F = fs.dev, fs.n, fs.K, fs.F
    f64 = dict(dtype=torch.float64, device=dev)
    if n == 0:
        models = [torch.zeros_like(fr) for fr in fs.frames]
        ntiles = [((s[0] + TILE_H - 1) // TILE_H) * ((s[1] + TILE_W - 1) // TILE_W)
                  for s in fs.shapes]
        tile_group = [np.full(t, -1, dtype=np.int64) for t in ntiles]
        # (no model: the residuals are the frames)
        _, tile_chi2 = _frames_chi2_group(fs, fs.frames, tile_group,
                                          np.zeros(0, dtype=np.int64), 0, np.zeros(0))
        return dict(F_self=torch.zeros((0, K, K), **f64), grad=torch.zeros((0, K), **f64),
                    pairs=torch.zeros((0, 2), dtype=torch.int64, device=dev),
                    F_cross=torch.zeros((0, K, K), **f64),
                    group=torch.zeros(0, dtype=torch.int64, device=dev),
                    chi2_group=torch.zeros(0, **f64),
                    status=torch.zeros(0, dtype=torch.int32, device=dev),
                    _tile_chi2=tile_chi2, _tile_group=tile_group,
                    _group=np.zeros(0, dtype=np.int64), _models=models, _prior_ff=np.zeros(0))
    fm = _frames_model(fs, pars, ngauss, max_pairs, True)
    resids = [(fs.frames[f] - fm["models"][f]).contiguous() for f in range(F)]
    pairs = _frames_pairs(
        [_scene_pairs(fm["pair_obj"][f], fm["tile_start"][f],
                      torch.from_numpy(fm["boxes"][f].astype(np.int64)), n, max_pairs)
         for f in range(F)], n)
    P = int(pairs.shape[0])
    group, tile_group = _scene_groups_frames(
        [(fm["pair_obj"][f].cpu().numpy(), fm["tile_start"][f].cpu().numpy()) for f in range(F)],
        n)
    ngroups = int(group.max()) + 1
    prior_ff = _prior_ff(fs, pars, fm["flag"])
    chi2_group, tile_chi2 = _frames_chi2_group(fs, resids, tile_group, group, ngroups, prior_ff)
    items = np.empty((n + P, 2), dtype=np.int32)
    items[:n, 0] = np.arange(n)
    items[:n, 1] = -1
    items[n:] = pairs.cpu().numpy()
    mat, vec = _scene_normal(fs, fm, resids, items)
    F_self, grad = mat[:n], vec[:n]
    if fs.prior is not None:
        sums, _ = prior_normal_sums(fs.prior, pars)
        iu = torch.triu_indices(K, K, device=dev)
        ntri = int(iu.shape[1])
        tri = sums[:, :ntri]
        Pm = pars.new_zeros((n, K, K))
        Pm[:, iu[0], iu[1]] = tri
        Pm[:, iu[1], iu[0]] = tri
        F_self = F_self + Pm
        grad = grad - sums[:, ntri:ntri + K]
    bad = fm["flag"] != 0
    nan = float("nan")
    F_self = torch.where(bad[:, None, None], torch.full_like(F_self, nan), F_self)
    grad = torch.where(bad[:, None], torch.full_like(grad, nan), grad)
    return dict(F_self=F_self, grad=grad, pairs=pairs, F_cross=mat[n:],
                group=torch.from_numpy(group).to(dev),
                chi2_group=torch.from_numpy(chi2_group).to(dev), status=fm["flag"],
                _tile_chi2=tile_chi2, _tile_group=tile_group, _group=group,
                _models=fm["models"], _prior_ff=prior_ff)


def normal_equations_frames(frames, weights, jacobians, pars, model, psf=None, frame_band=None,
                            prior=None, ngauss=None, max_pairs=None):
    """
    normal_equations over a LIST of frames -- several bands, several epochs per
    band, each image with its own shape, jacobians (WCS, dither) and psf -- and
    with a prior (csrc/scene_normal_frames.hip).  With
    r_f = frames[f] - render_scene(objects at pars in frame f) and J_a,f =
    d model_a,f / d pars_a,
        F_self[a]  = sum_f sum w J_a,f J_a,f^T     symmetric to the bit
        grad[a]    = sum_f sum w r_f J_a,f
        F_cross[p] = sum_f sum w J_a,f J_b,f^T     (a, b) = pairs[p]
    summed over the frames in ascending index by the one wave that owns the
    block.  An object whose box misses a frame adds nothing there.

    frames: a sequence of F 2-d float64 device tensors; their shapes may differ
    weights: None, a scalar, or a sequence of F entries, each None, a scalar or
        a tensor of that frame's shape
    jacobians: a sequence of F jacobian sets, each as normal_equations' (one
        jacobian per object, in that frame's pixel coordinates)
    pars: (N, nshape + nband) in LMBatchFitter.go's layout: the model's shape
        parameters, then one flux per band; K = nshape + nband <= 16.
        'coellip' is refused
    psf: None, or a sequence of F entries, each a GMixBatch or an (N, P, 6)
        tensor with one mixture per object; P the same in all frames
    frame_band: (F,) ints, the band of every frame; default arange(F) when
        F == nband, otherwise required
    prior: what autodiff.fisher takes (prior_batch.as_batch_prior): the
        triangle of its rows' J^T J is added to F_self as autodiff.fisher adds
        it, J^T r is subtracted from grad (grad is minus half the gradient of
        chi2 + r_p . r_p), and every member's r_p . r_p is added to its group's
        chi2_group

    Returns normal_equations' keys with K = nshape + nband: pairs is the union
    of the frames' pairs, group the connected components of the union of the
    frames' tile-sharing graphs, chi2_group the fixed-order sum over the frames
    of the group's per-tile sum w r^2 (plus the prior's).  An object refused in
    any frame is left out of every frame's model: its status is the code of its
    first refusal in frame order, its rows are NaN, it is in no pair, and all
    other objects' bits are those of the catalogue without it.  No atomics: two
    calls give the same bits.
    """
    fs = _Frames(frames, weights, jacobians, pars, model, psf, frame_band, prior,
                 "normal_equations_frames")
    return _public(_normal_frames(fs, fs.pars, ngauss, max_pairs))


def joint_covariance_frames(frames, weights, jacobians, pars, model, psf=None, frame_band=None,
                            prior=None, ngauss=None, max_pairs=None, max_group=16):
    """
    joint_covariance over a list of frames and with a prior: the blocks of
    normal_equations_frames, inverted per group by the same bucketed Cholesky.
    For an isolated object this is autodiff.covariance over one stamp per
    frame, with the same prior.  Arguments as normal_equations_frames and
    joint_covariance; returns joint_covariance's keys.
    """
    _GroupLayout(np.zeros(0, dtype=np.int64), max_group)
    fs = _Frames(frames, weights, jacobians, pars, model, psf, frame_band, prior,
                 "joint_covariance_frames")
    return _covariance(_normal_frames(fs, fs.pars, ngauss, max_pairs), max_group)


def fit_joint_frames(frames, weights, jacobians, guess, model, psf=None, frame_band=None,
                     prior=None, maxiter=50, tol=1e-6, lambda0=1e-3, max_group=16,
                     large_groups="jacobi", cg_tol=1e-8, cg_maxiter=200):
    """
    fit_joint over a list of frames (bands, epochs) and with a prior: the same
    Levenberg-Marquardt loop, one lambda per group, over
    normal_equations_frames.  Per iteration one trial is rendered per frame; a
    group accepts its step when its chi2 decreases, taken over its current
    tiles in ALL frames plus its members' prior r . r; a trial where the prior
    is out of range (r . r = inf) is rejected.

    frames, weights, jacobians, psf, frame_band, prior: as
        normal_equations_frames; guess: (N, nshape + nband)
    the other keywords: fit_joint's.  large_groups="cg" goes through
        solve_normal unchanged, whose blocks hold at most 8 parameters per
        object: with K > 8 it is refused (ValueError naming K); a wider
        csrc/scene_solve.hip is not built

    Returns fit_joint's keys; chi2 includes the prior's r . r, and pars_cov is
    joint_covariance_frames at pars, bit for bit.
    """
    kw = _fit_keywords("fit_joint_frames", maxiter, tol, lambda0, max_group, large_groups,
                       cg_tol, cg_maxiter)
    K = int(np.shape(guess)[-1]) if np.ndim(guess) == 2 else 0
    if kw["cg"] and K > NORMAL_KMAX:
        raise ValueError("fit_joint_frames: large_groups='cg' solves blocks of at most %d "
                         "parameters per object (scene.solve_normal), got K = %d"
                         % (NORMAL_KMAX, K))
    fs = _Frames(frames, weights, jacobians, guess, model, psf, frame_band, prior,
                 "fit_joint_frames")
    return _fit_loop(fs, fs.pars, **kw)
