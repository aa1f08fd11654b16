"""
Differentiable log-likelihoods and model images of batched fits, for torch
autograd.

The pixel pass is one HIP kernel (csrc/loglike_grad.hip,
ngmix_loglike_grad_batch): for every stamp it returns get_loglike's value and
the gradient of that value with respect to the six parameters
(p, row, col, irr, irc, icc) of every gaussian of the stamp's convolved
mixture, in the convention of the reference's deriv_images
(ngmix/fitting/derivs_nb.py:41-127): the derivative of the apodised
exp5_smooth model the fits minimise.  Everything between the fit parameters
and those gaussians -- the model mixture (gmix_nb.py:307-558) and the psf
convolution (gmix_nb.py:609-649) -- is written here in torch ops, so autograd
carries the chain rule to the parameters and to the psf.

    from ngmix_amd import autodiff
    pars.requires_grad_(True)
    lnp = autodiff.lnprob(stamps, pars, "exp", psf=psf, prior=prior)
    lnp.sum().backward()          # pars.grad: d lnprob / d pars, per object

Objects the reference would refuse (|g| >= 1, a zero Tfactor, a psf of zero
flux, a convolved gaussian whose determinant or T is not positive) get a NaN
value, a NaN gradient (with respect to pars and to the psf rows of their
stamps) and a nonzero flag (return_flags=True); the other objects' values and
gradients do not depend on them.  First derivatives only: differentiating the
gradient again (create_graph=True) raises.

For objectives of your own, render() returns every stamp's model image (flat,
in StampBatch.render's layout), differentiable with respect to pars and the
psf.  Its backward is one HIP kernel (csrc/render_grad.hip,
ngmix_render_vjp_batch): the vector-Jacobian product over the pixels, with no
(nstamps, G, npix) intermediate.  stamp_render() does the same for raw
(nstamps, G, 6) mixtures.  A Poisson loss, and a blend of two objects drawn
into the same stamps by concatenating their mixtures along G:

    img = autodiff.render(stamps, pars, "exp", psf=psf)
    loss = (img - counts * torch.log(img)).sum()     # -ln L up to a constant
    loss.backward()

    ma, _ = autodiff.convolve(autodiff.mixture_from_pars(pars_a, "exp")[0], psf)
    mb, _ = autodiff.convolve(autodiff.mixture_from_pars(pars_b, "dev")[0], psf)
    img, status = autodiff.stamp_render(stamps, torch.cat([ma, mb], dim=1))
    ((img - stamps.val) ** 2 * stamps.ierr ** 2).sum().backward()

Error bars at any parameters -- after an LBFGS fit over lnprob, a Fisher
forecast at the truth, a blend -- come from fisher() and covariance(): the
Gauss-Newton matrix sum_pix w J J^T of every object (and its inverse), from
one HIP kernel (csrc/fisher.hip, ngmix_fisher_batch) that contracts the same
first derivatives with d theta / d pars and forms the outer products without
writing J to memory.  stamp_fisher() is the raw form over (nstamps, G, 6)
mixtures with a caller's tangents (nstamps, G, 6, K).

A whole frame: scene_render() draws a catalogue into ONE image (every object
with a jacobian of its own, in frame coordinates; csrc/scene.hip), so any torch
loss on the frame gets gradients with respect to every object's parameters:

    frame = autodiff.scene_render((4096, 4096), jacobians, pars, "exp", psf=psf)
    ((frame - data) ** 2 * weight).sum().backward()
"""
import ctypes
import math

import numpy as np

from . import _lib
from .batch import GMixBatch, _dptr, _on_device, _stream, _torch
from .gmix import get_model_num, get_model_name

__all__ = ["mixture_from_pars", "convolve", "stamp_loglike_grad", "loglike", "lnprob",
           "stamp_render", "render", "stamp_fisher", "fisher", "covariance", "scene_render"]

# the model tables of csrc/common.hpp (gmix_nb.py:243-304): 0-5 exp,
# 6-15 dev, 16-18 turb, 19 gauss
_PVALS = (0.00061601229677880041, 0.0079461395724623237, 0.053280454055540001,
          0.21797364640726541, 0.45496740582554868, 0.26521634184240478,
          6.5288960012625658e-05, 0.00044199216814302695, 0.0020859587871659754,
          0.0075913681418996841, 0.02260266219257237, 0.056532254390212859,
          0.11939049233042602, 0.20969545753234975, 0.29254151133139222,
          0.28905301416582552, 0.596510042804182, 0.4034898268889178,
          1.303069003078001e-07, 1.0)
_FVALS = (0.002467115141477932, 0.018147435573256168, 0.07944063151366336,
          0.27137669897479122, 0.79782256866993773, 2.1623306025075739,
          2.9934935706271918e-07, 3.4651596338231207e-06, 2.4807910570562753e-05,
          1.4307404300535354e-04, 7.2753169298239500e-04, 3.4582464394427260e-03,
          1.6086645440719100e-02, 7.7006776775654429e-02, 4.1012562102501476e-01,
          2.9812509778548648e00, 0.5793612389470884, 1.621860687127999,
          7.019347162356363, 1.0)
_SIMPLE = {"exp": (0, 6), "dev": (6, 10), "turb": (16, 3), "gauss": (19, 1)}
_NLOC = {"gauss": 6, "turb": 6, "exp": 6, "dev": 6, "bdf": 7, "bd": 8}


def _model_name(model):
    name = get_model_name(get_model_num(model))
    if name not in _NLOC and name != "coellip":
        raise ValueError("autodiff supports %s and 'coellip', got %r"
                         % (tuple(_NLOC), model))
    return name


def _e1e2(g1, g2):
    """g1g2_to_e1e2 (gmix_nb.py:652-678) in torch ops; bad marks g >= 1.  At
    g = 0 the value is the reference's 0 and the slope its limit, 2."""
    torch = _torch()
    gsq = g1 * g1 + g2 * g2
    nz = gsq > 0.0
    # (sqrt at 0 has an infinite slope: keep it out of the graph)
    g = torch.sqrt(torch.where(nz, gsq, torch.ones_like(gsq)))
    bad = nz & (g >= 1)
    pos = nz & ~bad
    gs = torch.where(pos, g, torch.full_like(g, 0.5))
    e = torch.tanh(2 * torch.atanh(gs))
    e = torch.where(e >= 1.0, torch.full_like(e, 0.99999999), e)
    fac = torch.where(pos, e / gs, torch.full_like(e, 2.0))
    return fac * g1, fac * g2, bad


def _tfactor(ifracdev, fracdev, TdByTe):
    """get_cm_Tfactor's sum (gmix_nb.py:561-593), in its order"""
    tf = 0.0
    for i in range(6):
        tf = tf + (_PVALS[i] * ifracdev) * _FVALS[i]
    for i in range(10):
        tf = tf + (_PVALS[6 + i] * fracdev) * (_FVALS[6 + i] * TdByTe)
    return tf


def _safe_row(name, npars):
    """a parameter row every model accepts: what refused rows are evaluated
    at (their results are then replaced by NaN)"""
    row = [0.0, 0.0, 0.0, 0.0] + [1.0] * (npars - 4)
    if name == "bdf":
        row[5] = 0.5
    elif name == "bd":
        row[5], row[6] = 0.0, 0.5
    return row


def _mixture(pars, name, ngauss):
    """(mixture (n, ngauss, 6), bad (n,)): refused rows are evaluated at a
    safe row, so that nothing non-finite enters the graph"""
    torch = _torch()
    n, npars = pars.shape
    c1, c2, g1, g2 = pars[:, 0], pars[:, 1], pars[:, 2], pars[:, 3]
    _, _, bad = _e1e2(g1.detach(), g2.detach())
    if name in ("bdf", "bd"):
        fd = pars[:, 5] if name == "bdf" else pars[:, 6]
        tdbyte = 1.0 if name == "bdf" else torch.pow(10.0, pars[:, 5].detach())
        bad = bad | (_tfactor(1.0 - fd.detach(), fd.detach(), tdbyte) == 0.0)
    if bool(bad.any()):
        safe = torch.tensor(_safe_row(name, npars), dtype=pars.dtype, device=pars.device)
        pars = torch.where(bad[:, None], safe[None, :], pars)
        c1, c2, g1, g2 = pars[:, 0], pars[:, 1], pars[:, 2], pars[:, 3]
    e1, e2, _ = _e1e2(g1, g2)
    dt = dict(dtype=pars.dtype, device=pars.device)
    if name == "coellip":
        T_i_2 = 0.5 * pars[:, 4:4 + ngauss]
        flux_i = pars[:, 4 + ngauss:4 + 2 * ngauss]
    elif name in ("bdf", "bd"):
        if name == "bdf":
            fracdev, flux, TdByTe = pars[:, 5], pars[:, 6], 1.0
        else:
            fracdev, flux = pars[:, 6], pars[:, 7]
            TdByTe = torch.pow(10.0, pars[:, 5])
        ifracdev = 1.0 - fracdev
        T = pars[:, 4] * (1.0 / _tfactor(ifracdev, fracdev, TdByTe))
        pv = torch.tensor(_PVALS[:16], **dt)
        fv = torch.tensor(_FVALS[:16], **dt)
        isdev = torch.arange(16, device=pars.device) >= 6
        p = torch.where(isdev[None, :], pv[None, :] * fracdev[:, None],
                        pv[None, :] * ifracdev[:, None])
        if name == "bdf":
            f = fv[None, :].expand(n, 16)
        else:
            f = torch.where(isdev[None, :], fv[None, :] * TdByTe[:, None],
                            fv[None, :].expand(n, 16))
        T_i_2 = (0.5 * T)[:, None] * f
        flux_i = flux[:, None] * p
    else:
        off, ng = _SIMPLE[name]
        fv = torch.tensor(_FVALS[off:off + ng], **dt)
        pv = torch.tensor(_PVALS[off:off + ng], **dt)
        T_i_2 = (0.5 * pars[:, 4])[:, None] * fv[None, :]
        flux_i = pars[:, 5][:, None] * pv[None, :]
    ng = T_i_2.shape[1]
    irr = T_i_2 * (1 - e1)[:, None]
    irc = T_i_2 * e2[:, None]
    icc = T_i_2 * (1 + e1)[:, None]
    mix = torch.stack([flux_i, c1[:, None].expand(n, ng), c2[:, None].expand(n, ng),
                       irr, irc, icc], dim=2)
    return mix, bad


def _ngauss_of(name, npars, ngauss):
    if name == "coellip":
        ng = (npars - 4) // 2 if ngauss is None else int(ngauss)
        if ng < 1 or npars != 4 + 2 * ng:
            raise ValueError("coellip needs 4 + 2 * ngauss parameters, got %d" % npars)
        return ng
    if npars != _NLOC[name]:
        raise ValueError("model '%s' needs %d parameters, got %d" % (name, _NLOC[name], npars))
    return {"gauss": 1, "turb": 3, "exp": 6, "dev": 10, "bdf": 16, "bd": 16}[name]


def mixture_from_pars(pars, model, ngauss=None):
    """
    The model mixtures of GMixBatch.from_pars / GMixModel (gmix_nb.py:307-558)
    in differentiable torch ops, on pars' device.  pars: (n, npars) float64
    tensor of one band's parameters (coellip: [cen1, cen2, g1, g2, T_1..,
    F_1..] with ngauss pairs).  Returns (mix, bad): mix (n, ngauss, 6) as
    (p, row, col, irr, irc, icc), bad (n,) bool where the reference refuses
    the row (|g| >= 1, or a zero Tfactor for bdf / bd); those rows are NaN.
    """
    torch = _torch()
    name = _model_name(model)
    if pars.ndim == 1:
        pars = pars[None, :]
    ng = _ngauss_of(name, pars.shape[1], ngauss)
    mix, bad = _mixture(pars, name, ng)
    return torch.where(bad[:, None, None], torch.full_like(mix, math.nan), mix), bad


def _psf_tensor(psf, nstamps, device):
    torch = _torch()
    if isinstance(psf, GMixBatch):
        assert psf.n == nstamps, "one psf mixture per stamp"
        return psf.data[:, :6].reshape(psf.n, psf.ngauss, 6).to(device)
    psf = torch.as_tensor(psf, dtype=torch.float64, device=device)
    if psf.ndim != 3 or psf.shape[0] != nstamps or psf.shape[2] != 6:
        raise ValueError("psf: (nstamps, ngauss_psf, 6) tensor or a GMixBatch")
    return psf


def _convolve(mix, psf):
    """gmix_convolve_fill per row, in its order of operations; bad marks a
    psf of zero total flux (evaluated at psum = 1, then replaced)"""
    torch = _torch()
    psum = 0.0
    rsum = 0.0
    csum = 0.0
    for j in range(psf.shape[1]):
        q = psf[:, j]
        rsum = rsum + q[:, 0] * q[:, 1]
        csum = csum + q[:, 0] * q[:, 2]
        psum = psum + q[:, 0]
    bad = psum == 0.0
    psum = torch.where(bad, torch.ones_like(psum), psum)
    rowcen = rsum / psum
    colcen = csum / psum
    ipsum = 1.0 / psum
    o = mix[:, :, None, :]
    q = psf[:, None, :, :]
    p = o[..., 0] * q[..., 0] * ipsum[:, None, None]
    row = o[..., 1] + (q[..., 1] - rowcen[:, None, None])
    col = o[..., 2] + (q[..., 2] - colcen[:, None, None])
    cov = o[..., 3:6] + q[..., 3:6]
    out = torch.cat([torch.stack([p, row, col], dim=3), cov], dim=3)
    return out.reshape(mix.shape[0], -1, 6), bad


def convolve(mix, psf):
    """
    GMixBatch.convolve / GMix.convolve (gmix_nb.py:609-649) in differentiable
    torch ops: mix (n, G, 6), psf (n, P, 6) or a GMixBatch.  Returns
    (conv (n, G*P, 6), bad (n,)) with bad where the psf's flux sums to zero
    (the reference's ZeroDivisionError); those rows are NaN.
    """
    torch = _torch()
    psf = _psf_tensor(psf, mix.shape[0], mix.device)
    out, bad = _convolve(mix, psf)
    return torch.where(bad[:, None, None], torch.full_like(out, math.nan), out), bad


def _gauss_records(gpars, with_det):
    """the kernels' (n * G, 13) gaussian records of gpars (n, G, 6): the six
    parameters, (with_det) det as the kernels form it, the rest zero"""
    torch = _torch()
    g = gpars.detach().reshape(-1, 6)
    rec = torch.zeros((g.shape[0], 13), dtype=torch.float64, device=g.device)
    rec[:, :6] = g
    if with_det:
        rec[:, 6] = g[:, 3] * g[:, 5] - g[:, 4] * g[:, 4]
    return rec


def _pix_extent(stamps):
    """the length of a flat pixel array that holds every frame of the batch"""
    extent = int(stamps.total_pix)
    if stamps.n:
        extent = max(extent, int((stamps.pix_off + stamps.npix).max()))
    return extent


def _first_order_only(name):
    """called by the backward passes.  First derivatives only.  Grad mode is on
    there exactly when the caller asked for a graph of the gradient
    (create_graph=True, e.g. a Hessian-vector product): the kernel's
    second-order terms do not exist, and the rest of the chain would still be
    differentiable, so the result would be silently wrong -- refuse instead."""
    if _torch().is_grad_enabled():
        raise RuntimeError(
            "autodiff.%s gives first derivatives only: create_graph=True "
            "(second derivatives through the pixel kernel) is not supported" % name)


def _make_functions():
    torch = _torch()

    class _LoglikeGrad(torch.autograd.Function):
        """forward: ngmix_loglike_grad_batch over the stamps, (nstamps,)
        loglikes (NaN where the stamp's status is not 0); backward:
        grad_output times the per-gaussian gradients the kernel left"""

        @staticmethod
        def forward(ctx, gpars, stamps):
            n, G, _ = gpars.shape
            dev = stamps.device
            # (stamp_loglike_grad does not check gpars' device: copied, as ever)
            rec = _gauss_records(gpars.to(dev), False)
            out = torch.empty((n, 4), dtype=torch.float64, device=dev)
            grad = torch.empty((n * G, 6), dtype=torch.float64, device=dev)
            status = torch.empty(n, dtype=torch.int32, device=dev)
            b = stamps._batch(G)
            with _on_device(dev):
                st = _lib.lib().ngmix_loglike_grad_batch(
                    ctypes.byref(b), _dptr(rec), _dptr(out), _dptr(grad), _dptr(status),
                    _stream())
            _lib.check(st, "ngmix_loglike_grad_batch")
            ctx.save_for_backward(grad.reshape(n, G, 6), status)
            ctx.mark_non_differentiable(out, status)
            return out[:, 0].clone(), out, status

        @staticmethod
        def backward(ctx, g_ll, g_out, g_status):
            _first_order_only("loglike")
            grad, status = ctx.saved_tensors
            ok = (status == 0)[:, None, None]
            grad = torch.where(ok, grad, torch.zeros_like(grad))
            return g_ll[:, None, None] * grad, None

    class _RenderVJP(torch.autograd.Function):
        """forward: ngmix_render_batch over the stamps (as StampBatch.render
        with image=None); backward: one ngmix_render_vjp_batch call, the
        upstream image contracted with the derivative of every pixel"""

        @staticmethod
        def forward(ctx, gpars, stamps, fast_exp, exact):
            n, G, _ = gpars.shape
            dev = stamps.device
            rec = _gauss_records(gpars, True)
            extent = _pix_extent(stamps)
            packed = stamps._packed()
            if packed:
                image = torch.empty(extent, dtype=torch.float64, device=dev)
            else:
                image = torch.zeros(extent, dtype=torch.float64, device=dev)
            status = torch.empty(n, dtype=torch.int32, device=dev)
            b = stamps._batch(G, False, exact)
            if packed:
                b.flags |= _lib.BATCH_RENDER_OVERWRITE
            with _on_device(dev):
                st = _lib.lib().ngmix_render_batch(
                    ctypes.byref(b), _dptr(rec), _dptr(image), int(bool(fast_exp)),
                    _dptr(status), _stream())
            _lib.check(st, "ngmix_render_batch")
            ctx.stamps = stamps
            ctx.fast_exp = bool(fast_exp)
            ctx.shape = (n, G)
            ctx.save_for_backward(rec, status)
            ctx.mark_non_differentiable(status)
            return image, status

        @staticmethod
        def backward(ctx, g_image, g_status):
            _first_order_only("render")
            rec, status = ctx.saved_tensors
            n, G = ctx.shape
            stamps = ctx.stamps
            dev = stamps.device
            # (image.sum() hands back a stride-0 expanded tensor)
            gimg = g_image.to(torch.float64).contiguous()
            grad = torch.empty((n * G, 6), dtype=torch.float64, device=dev)
            vstatus = torch.empty(n, dtype=torch.int32, device=dev)
            b = stamps._batch(G)
            with _on_device(dev):
                st = _lib.lib().ngmix_render_vjp_batch(
                    ctypes.byref(b), _dptr(rec), _dptr(gimg), int(ctx.fast_exp),
                    _dptr(grad), _dptr(vstatus), _stream())
            _lib.check(st, "ngmix_render_vjp_batch")
            grad = grad.reshape(n, G, 6)
            ok = (status == 0)[:, None, None]
            return torch.where(ok, grad, torch.zeros_like(grad)), None, None, None

    return _LoglikeGrad, _RenderVJP


_FUNCS = None


def _functions():
    """(_LoglikeGrad, _RenderVJP), made at first use: torch is imported lazily"""
    global _FUNCS
    if _FUNCS is None:
        _FUNCS = _make_functions()
    return _FUNCS


def stamp_loglike_grad(stamps, gpars):
    """
    The raw kernel call: gpars (nstamps, G, 6) device tensor of each stamp's
    convolved gaussians (p, row, col, irr, irc, icc).  Returns (loglike
    (nstamps,), record (nstamps, 4) = loglike, s2n_numer, s2n_denom, npix,
    status (nstamps,) int32); loglike is differentiable with respect to gpars.
    """
    if gpars.shape[0] != stamps.n:
        raise ValueError("one mixture per stamp: %d != %d" % (gpars.shape[0], stamps.n))
    return _functions()[0].apply(gpars, stamps)


def stamp_render(stamps, gpars, fast_exp=True, exact=False):
    """
    The raw render: gpars (nstamps, G, 6) device tensor of each stamp's
    gaussians (p, row, col, irr, irc, icc).  Returns (image, status
    (nstamps,) int32): the image is StampBatch.render's (flat, the stamps'
    layout, bit for bit for the same fast_exp / exact) and differentiable with
    respect to gpars; its backward is one ngmix_render_vjp_batch call
    (fast_exp: deriv_images' convention, else the true derivative).  A stamp
    whose status is not 0 renders zeros and gets a zero gradient.
    """
    if gpars.ndim != 3 or gpars.shape[2] != 6:
        raise ValueError("gpars: (nstamps, G, 6) tensor of (p, row, col, irr, irc, icc)")
    if gpars.shape[0] != stamps.n:
        raise ValueError("one mixture per stamp: %d != %d" % (gpars.shape[0], stamps.n))
    if gpars.shape[1] < 1:
        raise ValueError("gpars: at least one gaussian per stamp")
    if gpars.device != stamps.device:
        raise ValueError("gpars must live on the stamps' device (%s)" % stamps.device)
    return _functions()[1].apply(gpars, stamps, fast_exp, exact)


def _stamp_layout(nstamps, nobj, stamp_obj, stamp_band):
    """(stamp_obj, stamp_band) as int64 numpy arrays, checked as LMBatchFitter
    checks them"""
    if stamp_obj is None:
        if nstamps != nobj:
            raise ValueError("stamp_obj is needed when objects have several stamps")
        sobj = np.arange(nstamps, dtype=np.int64)
    else:
        sobj = np.asarray(stamp_obj, dtype=np.int64).reshape(-1)
        if sobj.shape != (nstamps,):
            raise ValueError("stamp_obj: one entry per stamp")
        if nstamps and (np.any(np.diff(sobj) < 0) or sobj[0] < 0 or sobj[-1] >= nobj):
            raise ValueError("stamp_obj must be non-decreasing object indices")
        if np.any(np.bincount(sobj, minlength=nobj) == 0):
            raise ValueError("every object needs at least one stamp")
    if stamp_band is None:
        sband = np.zeros(nstamps, dtype=np.int64)
    else:
        sband = np.asarray(stamp_band, dtype=np.int64).reshape(-1)
        if sband.shape != (nstamps,) or np.any(sband < 0):
            raise ValueError("stamp_band: one non-negative band per stamp")
    return sobj, sband


def _stamp_mixtures(stamps, pars, model, psf, stamp_obj, stamp_band, ngauss):
    """what loglike and render share: the layout checks, every stamp's
    (convolved) mixture and its code (0, or why the reference refuses it).
    Returns (pars (nobj, npars), sobj, mix (nstamps, G, 6), code (nstamps,)
    int32, psf tensor or None)"""
    torch = _torch()
    name = _model_name(model)
    if pars.ndim == 1:
        pars = pars[None, :]
    nobj, npars = pars.shape
    dev = stamps.device
    if pars.device != dev:
        raise ValueError("pars must live on the stamps' device (%s)" % dev)
    sobj, sband = _stamp_layout(stamps.n, nobj, stamp_obj, stamp_band)
    nst = stamps.n
    if name == "coellip":
        if np.any(sband != 0):
            raise ValueError("coellip fits one band")
        bpars = pars[torch.from_numpy(sobj).to(dev)]
    else:
        nshape = _NLOC[name] - 1
        nband = npars - nshape
        if nband < 1 or (nst and sband.max() >= nband):
            raise ValueError("pars needs %d shape columns and one flux per band" % nshape)
        d_obj = torch.from_numpy(sobj).to(dev)
        d_band = torch.from_numpy(nshape + sband).to(dev)
        bpars = torch.cat([pars[d_obj, :nshape], pars[d_obj, d_band][:, None]], dim=1)
    ng = _ngauss_of(name, bpars.shape[1], ngauss)
    mix, bad = _mixture(bpars, name, ng)
    code = torch.where(bad, torch.full_like(bad, _lib.ERR_G_RANGE, dtype=torch.int32),
                       torch.zeros_like(bad, dtype=torch.int32))
    psf_t = None
    if psf is not None:
        psf_t = _psf_tensor(psf, nst, dev)
        mix, pbad = _convolve(mix, psf_t)
        code = torch.where((code == 0) & pbad, torch.full_like(code, _lib.ERR_ZERO_DIV), code)
    return pars, sobj, mix, code, psf_t


def _object_rows(sobj, nobj, dev):
    """the j-th stamp of every object, j = 0 .. (most stamps) - 1, as device
    indices into a per-stamp array padded with one entry (index nstamps) that
    objects with fewer stamps read"""
    torch = _torch()
    counts = np.bincount(sobj, minlength=nobj)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    L = int(counts.max()) if nobj else 0
    return [torch.from_numpy(np.where(j < counts, start + j, len(sobj))).to(dev)
            for j in range(L)]


def _first_flag(code, rows, nobj):
    """each object's flag: the code of its first refused stamp, in stamp order"""
    torch = _torch()
    flag = torch.zeros(nobj, dtype=torch.int32, device=code.device)
    code_pad = torch.cat([code, code.new_zeros(1)])
    for d_idx in rows:
        cj = code_pad[d_idx]
        flag = torch.where((flag == 0) & (cj != 0), cj, flag)
    return flag


def _sum_over_stamps(values, rows, tot=None):
    """tot plus every object's sum of the per-stamp values, added in stamp
    order (a fixed order: the same bits every time); tot None starts from the
    first stamp's term, and stays None when there is no stamp at all"""
    torch = _torch()
    pad = torch.cat([values, values.new_zeros((1,) + tuple(values.shape[1:]))])
    for d_idx in rows:
        tot = pad[d_idx] if tot is None else tot + pad[d_idx]
    return tot


def _poison_term(pars, psf_t, flag, sobj):
    """what makes a flagged object's gradients NaN: per object (nobj,) NaN *
    its pars, and per stamp (nstamps,) NaN * its psf rows (None unless the psf
    requires grad); both are 0 * x for the objects that are not flagged.
    sobj: device indices"""
    torch = _torch()
    zero = pars.new_zeros(pars.shape[0])
    poison = torch.where(flag != 0, torch.full_like(zero, math.nan), zero)
    obj_term = (pars * poison[:, None]).sum(dim=1)
    psf_term = None
    if psf_t is not None and psf_t.requires_grad:
        psf_term = (psf_t.reshape(sobj.shape[0], -1) * poison[sobj][:, None]).sum(dim=1)
    return obj_term, psf_term


def loglike(stamps, pars, model, psf=None, stamp_obj=None, stamp_band=None,
            ngauss=None, return_flags=False):
    """
    Log-likelihood of every object, summed over its stamps as
    FitModel.calc_lnprob sums its observations, differentiable with respect
    to pars and to psf (when a tensor that requires grad).

    stamps: StampBatch of every stamp of every object
    pars: (nobj, nshape + nband) float64 device tensor, LMBatchFitter.go's
        layout: the model's shape parameters then one flux per band
        (coellip: one band, [cen1, cen2, g1, g2, T_1.., F_1..])
    psf: None, a GMixBatch (one mixture per stamp) or a (nstamps, P, 6)
        tensor of (p, row, col, irr, irc, icc)
    stamp_obj / stamp_band: as in LMBatchFitter.go

    Returns (nobj,) loglikes; with return_flags, also (nobj,) int32 flags:
    0, or the code of the object's first refused stamp (_lib.ERR_*), whose
    value and gradient (pars, and the psf rows of its stamps) are NaN.
    """
    torch = _torch()
    pars, sobj, mix, code, psf_t = _stamp_mixtures(stamps, pars, model, psf, stamp_obj,
                                                   stamp_band, ngauss)
    nobj = pars.shape[0]
    dev = stamps.device
    ll, _, status = stamp_loglike_grad(stamps, mix)
    code = torch.where(code == 0, status, code)
    ll = torch.where(code == 0, ll, torch.zeros_like(ll))

    # fixed-order sum over each object's stamps (stamp order), and its flag
    rows = _object_rows(sobj, nobj, dev)
    tot = _sum_over_stamps(ll, rows)
    flag = _first_flag(code, rows, nobj)
    if tot is None:
        tot = pars.new_zeros(nobj)
    # a flagged object's value, and its gradient with respect to pars and to
    # the psf rows of its stamps, are NaN: a term that is 0 * x elsewhere
    nan_term, psf_term = _poison_term(pars, psf_t, flag, torch.from_numpy(sobj).to(dev))
    if psf_term is not None:
        nan_term = _sum_over_stamps(psf_term, rows, nan_term)
    out = torch.where(flag != 0, nan_term, tot)
    if return_flags:
        return out, flag
    return out


def render(stamps, pars, model, psf=None, stamp_obj=None, stamp_band=None, ngauss=None,
           fast_exp=True, exact=False, return_flags=False):
    """
    The model image of every stamp of every object (render_nb.py:9-36, as
    GMix.make_image draws it), flat in the stamps' layout (StampBatch.render's
    image), differentiable with respect to pars and to psf (when a tensor that
    requires grad).  Arguments as loglike(); fast_exp / exact as
    StampBatch.render.  Every pixel of the frame is drawn: weights play no
    part (masking is the loss's business).

    Returns the image; with return_flags, also (nobj,) int32 flags as
    loglike's.  Every pixel of a flagged object's stamps is NaN, and so are its
    gradient with respect to pars and the psf rows of its stamps; the other
    objects' pixels and gradients do not depend on it.
    """
    torch = _torch()
    pars, sobj, mix, code, psf_t = _stamp_mixtures(stamps, pars, model, psf, stamp_obj,
                                                   stamp_band, ngauss)
    nobj = pars.shape[0]
    nst = stamps.n
    dev = stamps.device
    image, status = stamp_render(stamps, mix, fast_exp=fast_exp, exact=exact)
    code = torch.where(code == 0, status, code)
    flag = _first_flag(code, _object_rows(sobj, nobj, dev), nobj)
    if nst and bool((flag != 0).any()):
        # the NaN term of each stamp (its object's pars, its own psf rows),
        # put on every pixel of the stamps of flagged objects
        d_sobj = torch.from_numpy(sobj).to(dev)
        obj_term, psf_term = _poison_term(pars, psf_t, flag, d_sobj)
        term = obj_term[d_sobj]
        if psf_term is not None:
            term = term + psf_term
        npix = torch.from_numpy(stamps.npix).to(dev)
        start = torch.cumsum(npix, 0) - npix
        pos = torch.repeat_interleave(torch.from_numpy(stamps.pix_off).to(dev) - start, npix) + \
            torch.arange(int(stamps.total_pix), device=dev)
        pix_stamp = torch.full((image.shape[0],), nst, dtype=torch.int64, device=dev)
        pix_stamp[pos] = torch.repeat_interleave(torch.arange(nst, device=dev), npix)
        bad_pad = torch.cat([flag[d_sobj] != 0, torch.zeros(1, dtype=torch.bool, device=dev)])
        term_pad = torch.cat([term, term.new_zeros(1)])
        image = torch.where(bad_pad[pix_stamp], term_pad[pix_stamp], image)
    if return_flags:
        return image, flag
    return image


def lnprob(stamps, pars, model, psf=None, stamp_obj=None, stamp_band=None,
           ngauss=None, prior=None, return_flags=False):
    """
    loglike() plus the prior's ln p of every object (prior.get_lnprob_batch:
    PriorSepBatch / PriorSimpleSepBatch, or a reference joint prior that
    prior_batch.as_batch_prior turns into one), the objective LMBatchFitter
    maximises.  A prior that as_batch_prior can only evaluate on the host
    (PriorBatchAdapter) has no gradient: asking for one is a TypeError.
    """
    from .prior_batch import as_batch_prior, PriorBatchAdapter
    torch = _torch()
    bp = as_batch_prior(prior)
    # (refused before any launch)
    if isinstance(bp, PriorBatchAdapter) and torch.is_grad_enabled() and pars.requires_grad:
        raise TypeError(
            "prior %r is evaluated object by object on the host (PriorBatchAdapter) and "
            "has no gradient: use a PriorSepBatch / PriorSimpleSepBatch, or evaluate "
            "under torch.no_grad()" % (type(prior).__name__,))
    res = loglike(stamps, pars, model, psf=psf, stamp_obj=stamp_obj,
                  stamp_band=stamp_band, ngauss=ngauss, return_flags=return_flags)
    if bp is None:
        return res
    lp = bp.get_lnprob_batch(pars if pars.ndim == 2 else pars[None, :])
    if return_flags:
        return res[0] + lp, res[1]
    return res + lp


# ------------------------------------------------------------------ Fisher

FISHER_KMAX = 16   # parameters per stamp: one 16 x 16 MFMA accumulator


def stamp_fisher(stamps, gpars, dgpars, weight=None, fast_exp=True):
    """
    The raw Fisher kernel (ngmix_fisher_batch): for every stamp,
        F[k, l] = sum_pix w J_k J_l,
        J_k = sum_g sum_a d model / d theta_a(g) dgpars[s, g, a, k],
    theta = (p, row, col, irr, irc, icc).

    gpars: (nstamps, G, 6) device tensor of each stamp's gaussians (for a
        blend, the objects' mixtures concatenated along G, as stamp_render)
    dgpars: (nstamps, G, 6, K) d theta / d q, 1 <= K <= 16 (e.g. from
        torch.func.jacfwd)
    weight: None for w = ierr^2 of the stamps (loglike's weighting: zero-weight
        pixels drop out), or a flat float64 device tensor in StampBatch.render's
        layout (every frame pixel, at pix_off).  Weights must be >= 0: the
        kernel takes sqrt(w).
    fast_exp: True for deriv_images' convention (the fits' jacobian, their
        pars_cov), False for the true derivative of the exp render.

    Returns (F (nstamps, K, K) float64, symmetric to the bit, status
    (nstamps,) int32).  A stamp whose status is not 0 gets a NaN matrix.  No
    autograd graph.
    """
    torch = _torch()
    if gpars.ndim != 3 or gpars.shape[2] != 6:
        raise ValueError("gpars: (nstamps, G, 6) tensor of (p, row, col, irr, irc, icc)")
    n, G, _ = gpars.shape
    if n != stamps.n:
        raise ValueError("one mixture per stamp: %d != %d" % (n, stamps.n))
    if G < 1:
        raise ValueError("gpars: at least one gaussian per stamp")
    if dgpars.ndim != 4 or tuple(dgpars.shape[:3]) != (n, G, 6):
        raise ValueError("dgpars: (nstamps, G, 6, K) tensor, got %s" % (tuple(dgpars.shape),))
    K = int(dgpars.shape[3])
    if K < 1 or K > FISHER_KMAX:
        raise ValueError("dgpars: K must be 1..%d parameters per stamp, got %d"
                         % (FISHER_KMAX, K))
    dev = stamps.device
    if gpars.device != dev or dgpars.device != dev:
        raise ValueError("gpars and dgpars must live on the stamps' device (%s)" % dev)
    wt = None
    if weight is not None:
        if weight.ndim != 1 or weight.device != dev:
            raise ValueError("weight: a flat tensor on the stamps' device, in "
                             "StampBatch.render's layout")
        extent = _pix_extent(stamps)
        if weight.shape[0] < extent:
            raise ValueError("weight: %d pixels, the stamps span %d"
                             % (weight.shape[0], extent))
        wt = weight.detach().to(torch.float64).contiguous()
    rec = _gauss_records(gpars, False)
    dg = dgpars.detach().to(torch.float64).contiguous()
    out = torch.empty((n, K, K), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    b = stamps._batch(G)
    with _on_device(dev):
        st = _lib.lib().ngmix_fisher_batch(
            ctypes.byref(b), _dptr(rec), _dptr(dg), K,
            _dptr(wt) if wt is not None else None, int(bool(fast_exp)), _dptr(out),
            _dptr(status), _stream())
    _lib.check(st, "ngmix_fisher_batch")
    return out, status


def _mixture_tangents(stamps, pars, model, psf, stamp_obj, stamp_band, ngauss):
    """_stamp_mixtures at pars, and d mix / d pars (nstamps, G, 6, npars) by
    forward-mode AD in ONE dual pass: the objects repeated npars times, copy k
    with tangent e_k (every stamp's mixture depends on its own object only)"""
    import torch.autograd.forward_ad as fwAD
    torch = _torch()
    pars = pars.detach()
    if pars.ndim == 1:
        pars = pars[None, :]
    if isinstance(psf, torch.Tensor):
        psf = psf.detach()
    base = _stamp_mixtures(stamps, pars, model, psf, stamp_obj, stamp_band, ngauss)
    _, sobj, mix, _, psf_t = base
    nobj, npars = pars.shape
    nst = stamps.n
    sband = _stamp_layout(nst, nobj, stamp_obj, stamp_band)[1]

    class _Rows(object):
        n = npars * nst
        device = stamps.device

    rep = pars.repeat(npars, 1)
    tan = torch.eye(npars, dtype=pars.dtype, device=pars.device).repeat_interleave(nobj, 0)
    sobj_rep = (sobj[None, :] + nobj * np.arange(npars)[:, None]).reshape(-1)
    psf_rep = psf_t.repeat(npars, 1, 1) if psf_t is not None else None
    with fwAD.dual_level():
        m = _stamp_mixtures(_Rows(), fwAD.make_dual(rep, tan), model, psf_rep, sobj_rep,
                            np.tile(sband, npars), ngauss)[2]
        dm = fwAD.unpack_dual(m).tangent
    if dm is None:
        dm = torch.zeros((npars,) + tuple(mix.shape), dtype=torch.float64, device=mix.device)
    dmix = dm.reshape((npars,) + tuple(mix.shape)).permute(1, 2, 3, 0).contiguous()
    return base, dmix


def fisher(stamps, pars, model, psf=None, stamp_obj=None, stamp_band=None, ngauss=None,
           prior=None, weight=None, fast_exp=True, return_flags=False):
    """
    The Fisher (Gauss-Newton) matrix sum_pix w J J^T of every object at pars,
    J = d model / d pars, summed over the object's stamps in stamp order:
    what LMBatchFitter inverts for pars_cov0, at any parameters (a torch fit,
    a forecast at the truth).  Arguments as loglike(); prior: a batch prior or
    a reference joint prior (as lnprob), whose rows' J^T J by the reference's
    differences (prior_batch.prior_normal_sums) is added, as the fitter adds
    it; weight / fast_exp as stamp_fisher (a caller weight, e.g. 1 / model
    for a Poisson fit, must be >= 0).

    Returns (nobj, npars, npars) float64; with return_flags, also (nobj,)
    int32 flags as loglike's: a flagged object's matrix is NaN, and the others
    do not depend on it.  No autograd graph: the result is a value, not
    differentiable with respect to pars or the psf.
    """
    from .prior_batch import as_batch_prior, prior_normal_sums
    torch = _torch()
    if pars.shape[-1] > FISHER_KMAX:
        raise ValueError("fisher: at most %d parameters per object, got %d"
                         % (FISHER_KMAX, pars.shape[-1]))
    bp = as_batch_prior(prior)
    (pars, sobj, mix, code, _), dmix = _mixture_tangents(
        stamps, pars, model, psf, stamp_obj, stamp_band, ngauss)
    nobj, npars = pars.shape
    dev = stamps.device
    F, status = stamp_fisher(stamps, mix, dmix, weight=weight, fast_exp=fast_exp)
    code = torch.where(code == 0, status, code)
    rows = _object_rows(sobj, nobj, dev)
    tot = _sum_over_stamps(F, rows, pars.new_zeros((nobj, npars, npars)))
    if bp is not None:
        sums, _ = prior_normal_sums(bp, pars)
        iu = torch.triu_indices(npars, npars, device=dev)
        tri = sums[:, :iu.shape[1]]
        P = pars.new_zeros((nobj, npars, npars))
        P[:, iu[0], iu[1]] = tri
        P[:, iu[1], iu[0]] = tri
        tot = tot + P
    flag = _first_flag(code, rows, nobj)
    tot = torch.where((flag != 0)[:, None, None], torch.full_like(tot, math.nan), tot)
    if return_flags:
        return tot, flag
    return tot


def covariance(stamps, pars, model, psf=None, stamp_obj=None, stamp_band=None,
               ngauss=None, prior=None, weight=None, fast_exp=True, return_flags=False):
    """
    The inverse of fisher() per object, by a batched Cholesky
    (torch.linalg.cholesky_ex): LMBatchFitter's pars_cov0 convention, NOT
    rescaled by chi2 / dof.  Arguments and flags as fisher(); a matrix that is
    not positive definite gives NaN and flags.LM_SINGULAR_MATRIX.  No autograd
    graph.
    """
    from .flags import LM_SINGULAR_MATRIX
    torch = _torch()
    F, flag = fisher(stamps, pars, model, psf=psf, stamp_obj=stamp_obj,
                     stamp_band=stamp_band, ngauss=ngauss, prior=prior, weight=weight,
                     fast_exp=fast_exp, return_flags=True)
    n = F.shape[1]
    bad = flag != 0
    eye = torch.eye(n, dtype=F.dtype, device=F.device).expand_as(F)
    L, info = torch.linalg.cholesky_ex(torch.where(bad[:, None, None], eye, F))
    sing = (info != 0) & ~bad
    cov = torch.cholesky_inverse(L)
    cov = torch.where((bad | sing)[:, None, None], torch.full_like(cov, math.nan), cov)
    flag = torch.where(sing, torch.full_like(flag, LM_SINGULAR_MATRIX), flag)
    if return_flags:
        return cov, flag
    return cov


class _SceneGeometry(object):
    """what _stamp_mixtures asks of its stamps: one "stamp" per object"""

    def __init__(self, n, device):
        self.n = int(n)
        self.device = device


def _make_scene_functions():
    torch = _torch()
    from . import scene as _scene
    from .batch import StampBatch

    class _PoisonRows(torch.autograd.Function):
        """forward: x itself; backward: the gradient with NaN in the rows of
        the objects that holder["flag"] marks by then (the flags come out of
        the forward pass that follows)"""

        @staticmethod
        def forward(ctx, x, holder):
            ctx.holder = holder
            return x.view_as(x)

        @staticmethod
        def backward(ctx, g):
            flag = ctx.holder.get("flag")
            if flag is None:
                return g, None
            bad = (flag != 0).reshape((-1,) + (1,) * (g.ndim - 1))
            return torch.where(bad, torch.full_like(g, math.nan), g), None

    class _SceneRender(torch.autograd.Function):
        """forward: the scene kernels (scene.render_scene's bits); backward:
        every object's clipped union box cut out of the upstream frame
        (ngmix_frame_gather), then one ngmix_render_vjp_batch call (fast) on
        those ragged windows"""

        @staticmethod
        def forward(ctx, gpars, image, jac, shape, code):
            n, G, _ = gpars.shape
            nrow, ncol = shape
            rec = _gauss_records(gpars, True)
            # an object refused before the kernels (|g| >= 1, a zero-flux psf)
            # is left out: all-zero records, which the norms refuse
            rec = torch.where((code != 0).repeat_interleave(G)[:, None],
                              torch.zeros_like(rec), rec)
            frame = None if image is None else image.detach().clone().contiguous()
            frame, status, boxes = _scene._render_records(nrow, ncol, rec, G, n, jac, frame,
                                                          None, boxes_to_host=True)
            ctx.boxes = boxes
            ctx.shape = (n, G, nrow, ncol)
            ctx.has_image = image is not None
            ctx.save_for_backward(rec, status, jac)
            ctx.mark_non_differentiable(status)
            return frame, status

        @staticmethod
        def backward(ctx, g_frame, g_status):
            _first_order_only("scene_render")
            rec, status, jac = ctx.saved_tensors
            n, G, nrow, ncol = ctx.shape
            dev = rec.device
            U = g_frame.to(torch.float64).contiguous()
            g_image = U if ctx.has_image else None
            if n == 0:
                return rec.new_zeros((0, G, 6)), g_image, None, None, None
            hb = ctx.boxes.astype(np.int64)
            hit = hb[:, 1] >= hb[:, 0]
            # (an object that misses the frame: a 1 x 1 window, gradient zeroed)
            r_lo = np.where(hit, hb[:, 0], 0)
            c_lo = np.where(hit, hb[:, 2], 0)
            wr = np.where(hit, hb[:, 1] - hb[:, 0] + 1, 1)
            wc = np.where(hit, hb[:, 3] - hb[:, 2] + 1, 1)
            npix = wr * wc
            off = np.concatenate([[0], np.cumsum(npix)[:-1]]).astype(np.int64)
            gimg = _scene._gather(U, np.stack([r_lo, c_lo, wr, wc], axis=1), off,
                                  int(npix.sum()), 0)
            wjac = jac.clone()
            wjac[:, 0] -= torch.from_numpy(r_lo.astype(np.float64)).to(dev)
            wjac[:, 1] -= torch.from_numpy(c_lo.astype(np.float64)).to(dev)
            stamps = StampBatch(None, None, wjac, wr, wc, off, False)
            grad = torch.empty((n * G, 6), dtype=torch.float64, device=dev)
            vstatus = torch.empty(n, dtype=torch.int32, device=dev)
            b = stamps._batch(G)
            with _on_device(dev):
                st = _lib.lib().ngmix_render_vjp_batch(
                    ctypes.byref(b), _dptr(rec), _dptr(gimg), 1, _dptr(grad), _dptr(vstatus),
                    _stream())
            _lib.check(st, "ngmix_render_vjp_batch")
            grad = grad.reshape(n, G, 6)
            ok = ((status == 0) & torch.from_numpy(hit).to(dev))[:, None, None]
            return torch.where(ok, grad, torch.zeros_like(grad)), g_image, None, None, None

    return _PoisonRows, _SceneRender


_SCENE_FUNCS = None


def scene_render(shape, jacobians, pars, model, psf=None, ngauss=None, image=None,
                 return_flags=False, fast_exp=True):
    """
    A catalogue drawn into ONE frame: the (nrow, ncol) image of the nobj
    objects pars (nobj, npars: the model's parameters with one flux), object i
    with jacobians[i] (row0 / col0 in FRAME pixel coordinates; centres may lie
    outside the frame) and, with psf, its own psf mixture (a GMixBatch or a
    (nobj, P, 6) tensor).  Differentiable with respect to pars, to a psf tensor
    and to image (an (nrow, ncol) tensor the objects are added to; it is not
    modified).  The values are scene.render_scene's, bit for bit: objects
    added in ascending index (fast exp; fast_exp=False is refused).

    Backward: each object's chi2 < 25 box, clipped to the frame, is cut out of
    the upstream gradient frame and one ngmix_render_vjp_batch call (deriv_
    images' convention, as render(fast_exp=True)) runs over those windows; a
    gaussian contributes nothing outside its box, so the window loses nothing.
    An object that misses the frame gets a zero gradient.  The gradient with
    respect to image is the upstream frame.  First derivatives only.

    With return_flags, also (nobj,) int32 flags (_lib.ERR_*).  An object the
    reference would refuse (|g| >= 1, a zero-flux psf, a refused gaussian) is
    LEFT OUT of the frame and reported in flags; its gradient rows, and its psf
    rows' gradient rows, are NaN, and every other object's pixels and gradients
    are bit-identical with or without it.  Deliberately not render()'s
    NaN-on-every-pixel of a flagged object's stamps: here the objects share
    their pixels, and one bad catalogue row must not erase a frame.
    """
    global _SCENE_FUNCS
    torch = _torch()
    from . import scene as _scene
    nrow, ncol = _scene._frame_shape(shape)
    if not fast_exp:
        raise ValueError("scene_render: only fast_exp=True is built: the chi2 < 25 gate of "
                         "the fast exp is what makes the tile binning exact")
    if not isinstance(pars, torch.Tensor) or pars.ndim != 2:
        raise ValueError("scene_render: pars must be an (nobj, npars) tensor")
    nobj = int(pars.shape[0])
    _scene._check_jacobians(jacobians, nobj, "scene_render")
    _scene._check_image(image, nrow, ncol, "scene_render")
    from .batch import _require_cuda
    dev = _require_cuda(pars.device)
    if image is not None and image.device != dev:
        raise ValueError("scene_render: image must live on pars' device (%s)" % dev)
    if _SCENE_FUNCS is None:
        _SCENE_FUNCS = _make_scene_functions()
    poison, render_fn = _SCENE_FUNCS
    holder = {}
    pars_in = poison.apply(pars, holder) if pars.requires_grad else pars
    psf_in = psf
    if psf is not None and not isinstance(psf, GMixBatch):
        psf_in = _psf_tensor(psf, nobj, dev)
        if psf_in.requires_grad:
            psf_in = poison.apply(psf_in, holder)
    _, _, mix, code, _ = _stamp_mixtures(_SceneGeometry(nobj, dev), pars_in, model, psf_in,
                                         None, None, ngauss)
    jac = _scene._jacobian_tensor(jacobians, nobj, dev)
    frame, status = render_fn.apply(mix, image, jac, (nrow, ncol), code)
    flag = torch.where(code == 0, status, code)
    holder["flag"] = flag
    if return_flags:
        return frame, flag
    return frame
