"""
Fourier-space profile fits: 'gauss', 'exp',
'spergel', 'moffat' and the gaussian mixtures 'dev10' and 'bdf' fitted to the
transform of a stamp's own samples, and the linear flux of a fixed profile or
of the psf in the same definition.

The reference's GalsimFitter / GalsimSpergelFitter / GalsimMoffatFitter fit the
exact profile to a k-space observation that galsim draws, and its
GalsimPSFFluxFitter the flux of the psf there.  Here the observation is the rfft2 half
plane of the stamp itself times the centre phase, the psf enters as the
transform of its own stamp (no psf model is fitted), and the lock-step LM
driver of ngmix_amd/lm_batch.py runs with kfit_eval_kernel in place of the
pixel pass:

    KStampBatch              the transforms D^, P^n, the Parseval weight
    KSpaceBatchFitter        N fits in lock step, a dict of arrays back
    KSpaceFitter             Observation / ObsList / MultiBandObsList in, one
                             batch per call
    kmodel_images            the model's real-space image, for residuals
    KSpaceFluxBatch          the linear flux of a fixed unit-flux template (a
                             model at given parameters, or the psf itself) per
                             object: kfit_flux_kernel, no LM
    KSpaceFluxFitter         the same for Observation / ObsList

What this is NOT: the pixel values of a KStampBatch are not galsim's (no
interpolant, no stepk / getGoodImageSize grid), the weight is the Parseval
weight (twice the reference's), aliases of the profile are not summed (galsim's
k-space fit does not sum them either), the Moffat profile is not truncated,
and 'dev', the exact de Vaucouleurs profile, is not offered (it has no
closed-form transform).  'dev10' is the transform of ngmix's ten-gaussian
approximation of it, the mixture GMixModel(pars, 'dev') builds, and 'bdf' that
of GMixModel(pars, 'bdf') (bulge + disk, TdByTe = 1): the pixel-space models
themselves, fitted in Fourier space with the pixel-space fitters' parameters.

Parameters: [cen1, cen2, g1, g2, r50, F_band...]; 'spergel':
[cen1, cen2, g1, g2, r50, nu, F_band...]; 'moffat': [cen1, cen2, g1, g2, size,
beta, F_band...], the size r50 (size_type 'r50', the default, or its aliases
'hlr' / 'half_light_radius') or the fwhm (size_type 'fwhm'); 'dev10':
[cen1, cen2, g1, g2, T, F_band...]; 'bdf': [cen1, cen2, g1, g2, T, fracdev,
F_band...] -- the size of these two is ngmix's T, not r50, and they take no
size_type.
"""
import ctypes
import math

import numpy as np

from . import _lib
from .batch import StampBatch, _dptr, _stream, _torch, _on_device, _as_device_f64
from .defaults import PDEF, CDEF, DEFAULT_LM_PARS
from .fitting import STEP_PRIOR
from .prior_batch import as_batch_prior, bounds_arrays

__all__ = ["KStampBatch", "KSpaceBatchFitter", "KSpaceFitter", "kmodel_images",
           "KSpaceFluxBatch", "KSpaceFluxFitter", "metacal_mode_weights"]

MODELS = {"gauss": _lib.KFIT_GAUSS, "exp": _lib.KFIT_EXP, "spergel": _lib.KFIT_SPERGEL,
          "moffat": _lib.KFIT_MOFFAT, "dev10": _lib.KFIT_DEV10, "bdf": _lib.KFIT_BDF}
MODEL_NLOC = {"gauss": 6, "exp": 6, "spergel": 7, "moffat": 7, "dev10": 6, "bdf": 7}
MIX_MODELS = ("dev10", "bdf")     # the size parameter is T
SIZE_TYPES = ("r50", "hlr", "half_light_radius", "fwhm")
HLR_GAUSS = math.sqrt(2.0 * math.log(2.0))
HLR_EXP = 1.6783469900166605
ROUNDS_FIRST = 12      # rounds queued blind before the first look at the counts


def _model_id(model, size_type=None):
    if model not in MODELS:
        raise ValueError("k-space fits offer %s, got %r ('dev', the exact profile, has no "
                         "closed-form transform; 'dev10' is its ten-gaussian mixture)"
                         % (tuple(MODELS), model))
    if size_type is not None:
        if model in MIX_MODELS:
            raise ValueError("'%s' takes T and no size_type, got %r" % (model, size_type))
        if size_type not in SIZE_TYPES:
            raise ValueError("size_type must be one of %s, got %r" % (SIZE_TYPES, size_type))
        if model != "moffat" and size_type == "fwhm":
            raise ValueError("size_type 'fwhm' is the Moffat fit's; '%s' takes r50" % model)
        if model == "moffat" and size_type == "fwhm":
            return _lib.KFIT_MOFFAT_FWHM
    return MODELS[model]


def _moffat_phi(nu, x):
    """Phi of the Moffat transform at the pairs (nu, x), device tensors of one
    shape, by ngmix_moffat_phi_batch"""
    torch = _torch()
    nu, x = nu.contiguous(), x.contiguous()
    out = torch.empty(x.shape + (3,), dtype=torch.float64, device=x.device)
    with _on_device(x.device):
        _lib.check(_lib.lib().ngmix_moffat_phi_batch(_dptr(nu), _dptr(x), x.numel(), _dptr(out),
                                                     _stream()), "ngmix_moffat_phi_batch")
    return out[..., 0]


def _mode_grid(R, C, dev):
    """q_r (R, 1) and q_c (1, C//2+1) of the stored modes"""
    torch = _torch()
    qr = 2.0 * math.pi * torch.fft.fftfreq(R, dtype=torch.float64, device=dev)
    qc = 2.0 * math.pi * torch.arange(C // 2 + 1, dtype=torch.float64, device=dev) / C
    return qr[:, None], qc[None, :]


def _centred_transform(img, cen, R, C):
    """rfft2 of (n, r, c) stamps zero-padded to R x C, times the phase that puts
    the origin at cen (n, 2): sum I exp(-i (q_r (r - r0) + q_c (c - c0)))"""
    torch = _torch()
    qr, qc = _mode_grid(R, C, img.device)
    F = torch.fft.rfft2(img, s=(R, C))
    ang = qr[None] * cen[:, 0, None, None] + qc[None] * cen[:, 1, None, None]
    return F * torch.polar(torch.ones_like(ang), ang)


class KStampBatch(object):
    """
    N stamps of ONE shape in Fourier space, resident on the device:

      dhat      (N, R, C//2+1, 2) float64, interleaved complex: the transform of
                each stamp about its jacobian centre
      phat      the same for the psf stamp about its own centre, zero-padded to
                R x C and divided by its sum; None without a psf
      wbar      (N,) the largest weight of each stamp (a weight map does not
                transfer to k-space; the reference takes the maximum too)
      jac       (N, 8) the jacobian records
      npix_eff  the residual components of a stamp that enter dof:
                (R - [R even]) (C - [C even]), the Nyquist row and column dropped
      mode_weight  None, or (N, R, C//2+1) float64 u >= 0: the
                weight of a mode is its Parseval weight times u, a mode with
                u = 0 is not read, and dof counts the components with a
                positive weight in place of npix_eff.  None: the kernels
                without the plane, untouched
    """

    def __init__(self, dhat, phat, wbar, jac, nrow, ncol, mode_weight=None):
        self.dhat, self.phat, self.wbar, self.jac = dhat, phat, wbar, jac
        self.nrow, self.ncol = int(nrow), int(ncol)
        self.n = int(dhat.shape[0])
        self.device = dhat.device
        self.npix_eff = (self.nrow - (self.nrow % 2 == 0)) * (self.ncol - (self.ncol % 2 == 0))
        if mode_weight is not None:
            if tuple(mode_weight.shape) != (self.n, self.nrow, self.ncol // 2 + 1) or \
                    mode_weight.dtype != dhat.dtype or mode_weight.device != dhat.device:
                raise ValueError("mode_weight must be (%d, %d, %d) float64 on the batch's device"
                                 % (self.n, self.nrow, self.ncol // 2 + 1))
            mode_weight = mode_weight.contiguous()
        self.mode_weight = mode_weight
        self.mcal_flags = None

    @staticmethod
    def _planes(sb, what):
        if sb.n == 0:
            raise ValueError("%s: no stamps" % what)
        if not (np.all(sb.nrow == sb.nrow[0]) and np.all(sb.ncol == sb.ncol[0])):
            raise ValueError("%s: a k-space batch holds stamps of one shape" % what)
        R, C = int(sb.nrow[0]), int(sb.ncol[0])
        if not np.array_equal(sb.pix_off, np.arange(sb.n, dtype=np.int64) * R * C):
            raise ValueError("%s: the stamps must be packed back to back" % what)
        return sb.val.view(sb.n, R, C), sb.ierr.view(sb.n, R, C), R, C

    @classmethod
    def from_stamps(cls, sb, psf_sb=None):
        torch = _torch()
        val, ierr, R, C = cls._planes(sb, "KStampBatch")
        with _on_device(sb.device):
            dhat = torch.view_as_real(_centred_transform(val, sb.jac[:, 0:2], R, C)).contiguous()
            wbar = (ierr * ierr).reshape(sb.n, -1).max(dim=1).values.contiguous()
            phat = None
            if psf_sb is not None:
                pval, _, Rp, Cp = cls._planes(psf_sb, "KStampBatch psf")
                if psf_sb.n != sb.n:
                    raise ValueError("KStampBatch: one psf stamp per stamp")
                if Rp > R or Cp > C:
                    raise ValueError("KStampBatch: the psf stamp (%d x %d) is larger than "
                                     "the image (%d x %d)" % (Rp, Cp, R, C))
                if not torch.equal(psf_sb.jac[:, 2:6], sb.jac[:, 2:6]):
                    raise ValueError("KStampBatch: the psf stamps must share their images' "
                                     "jacobian derivatives")
                P = _centred_transform(pval, psf_sb.jac[:, 0:2], R, C)
                P = P / pval.reshape(sb.n, -1).sum(dim=1)[:, None, None]
                phat = torch.view_as_real(P).contiguous()
        return cls(dhat, phat, wbar, sb.jac.contiguous(), R, C)

    @classmethod
    def from_images(cls, images, weights=None, jacobians=None, psf_images=None,
                    psf_jacobians=None, device=None):
        sb = StampBatch.from_images(images, weights, jacobians, device=device)
        psf_sb = None
        if psf_images is not None:
            psf_sb = StampBatch.from_images(psf_images, None, psf_jacobians, device=device)
        return cls.from_stamps(sb, psf_sb)

    @classmethod
    def from_metacal(cls, stamps, psf_stamps, types=None, step=0.01, psf="fitgauss",
                     target_sigma=None, weight="flat", fixnoise=False, rng=None):
        """
        The metacal types of a stamp batch as ONE k-space batch of ntypes * N
        stamps, type-major as MetacalBatch.get_all orders them, without leaving
        Fourier space: D^ is the sheared, reconvolved spectrum
        about the jacobian centre, P^n the target psf over the psf stamp's sum,
        both from the KFIT form of metacal_spectrum_kernel.  stamps, psf_stamps,
        psf, target_sigma, types, step: as MetacalBatch and get_all take them.

        mode_weight: a mode's u is zero unless EVERY requested type of the
        object keeps the mode, so an object's types are fitted on the same
        modes.  weight='flat': u is that 0/1 mask.  weight='noise': u = mask
        rho_min^2 / rho^2(q) with rho = |T^(q)| / |P^(q')|, the factor by which
        the operation scales white pixel noise at the mode -- the
        maximum-likelihood weight of stationary noise; rho_min over the type's
        masked-in modes of the object; modes with rho^2 < 1e-24 rho_max^2 in any
        type are masked out.

        mcal_flags (ntypes, N) int32 stays on the batch; a flagged stamp's D^ is
        NaN, so its fit is refused.  fixnoise is not served here.
        """
        if fixnoise:
            raise NotImplementedError("from_metacal: fixnoise is not served in Fourier space; "
                                      "MetacalBatch.get_all(fixnoise=True) serves it")
        if weight not in ("flat", "noise"):
            raise ValueError("weight must be 'flat' or 'noise', got %r" % (weight,))
        from . import metacal as mc
        torch = _torch()
        mb = mc.MetacalBatch(stamps, psf_stamps, psf=psf, target_sigma=target_sigma, rng=rng)
        types = mc._check_types(types, mc.DILATE_EXACT if mb.dilate else "fitgauss")
        g = mc._type_shears(types, float(step))
        dil = kind = None
        if mb.dilate:
            dil = np.full(len(types), 1.0 + 2.0 * abs(float(step)))
            kind = mc._type_kinds(types)
        dhat, phat, aux, flags = mb.kfit_spectra(g, False, dil, kind)
        nt, n = len(types), mb.n
        R, C = mb.shape
        with _on_device(mb.device):
            u = metacal_mode_weights(aux.view(nt, n, R, C // 2 + 1, 2), flags, weight)
            nan = torch.full((), float("nan"), dtype=torch.float64, device=mb.device)
            dhat = torch.where(flags.reshape(-1)[:, None, None, None] != 0, nan, dhat)
            ierr = stamps.ierr.reshape(n, -1)
            wbar = (ierr * ierr).max(dim=1).values.repeat(nt).contiguous()
            jac = stamps.jac.repeat(nt, 1).contiguous()
        kb = cls(dhat, phat, wbar, jac, R, C, mode_weight=u.view(nt * n, R, C // 2 + 1))
        kb.mcal_flags = flags.cpu().numpy()
        kb.types = types
        return kb


RHO2_FLOOR = 1.0e-24    # below this of rho_max^2 a mode is under double round-off of the DC mode


def metacal_mode_weights(aux, flags, weight):
    """
    The mode weights (T, N, R, C//2+1) of from_metacal from the kernel's aux
    planes (T, N, R, C//2+1, 2) = keep, rho^2 and the flags (T, N): the common
    mask of an object's types and, weight='noise', rho_min^2 / rho^2 on it.  A
    flagged (type, object) takes no part in the others' mask.
    """
    torch = _torch()
    bad = (flags != 0)[:, :, None, None]
    keep = torch.where(bad, torch.ones_like(aux[..., 0]), aux[..., 0])
    mask = keep.amin(dim=0, keepdim=True) > 0
    if weight == "flat":
        return mask.expand_as(keep).to(torch.float64).contiguous()
    rho2 = torch.where(bad, torch.ones_like(keep), aux[..., 1])
    zero = torch.zeros_like(rho2)
    rmax = torch.where(mask, rho2, zero).amax(dim=(2, 3), keepdim=True)
    mask = mask & (rho2 >= RHO2_FLOOR * rmax).all(dim=0, keepdim=True)
    inf = torch.full_like(rho2, float("inf"))
    rmin = torch.where(mask, rho2, inf).amin(dim=(2, 3), keepdim=True)
    return torch.where(mask, rmin / rho2, zero).contiguous()


def _mix_table(model, fracdev):
    """amplitudes a_i (N, ncomp) and T_i / T = f_i tau (N, ncomp) of the
    mixture of 'dev10' (fracdev None) or 'bdf' at fracdev (N, 1, 1), from
    autodiff's copy of the model tables and its T factor"""
    torch = _torch()
    from .autodiff import _PVALS, _FVALS, _tfactor
    lo = 6 if model == "dev10" else 0
    dt = dict(dtype=torch.float64, device=fracdev.device)
    pv, fv = torch.tensor(_PVALS[lo:16], **dt), torch.tensor(_FVALS[lo:16], **dt)
    if model == "dev10":
        return pv.expand(fracdev.shape[0], -1), fv.expand(fracdev.shape[0], -1)
    fd = fracdev.reshape(-1, 1)
    amp = torch.cat([(1.0 - fd) * pv[:6], fd * pv[6:]], dim=1)
    return amp, fv[None, :] / _tfactor(1.0 - fd, fd, 1.0)


def _spergel_hlr(nu):
    c, dc = ctypes.c_double(), ctypes.c_double()
    _lib.check(_lib.lib().ngmix_spergel_hlr(float(nu), ctypes.byref(c), ctypes.byref(dc)),
               "ngmix_spergel_hlr")
    return c.value


def kmodel_images(kb, pars, model, size_type=None):
    """
    The real-space images (N, R, C) of the band-limited, periodic model at
    pars (N, nloc) -- each stamp's LOCAL parameters, one flux -- by irfft2 of
    M^ about the stamp's centre: what the fit's residuals are residuals of (the
    Nyquist modes included here, dropped there).  torch ops; not a hot path.
    """
    torch = _torch()
    model_id = _model_id(model, size_type)
    nloc = MODEL_NLOC[model]
    p = _as_device_f64(np.asarray(pars) if not hasattr(pars, "device") else pars, kb.device)
    if p.shape != (kb.n, nloc):
        raise ValueError("pars must be (%d, %d)" % (kb.n, nloc))
    R, C = kb.nrow, kb.ncol
    qr, qc = _mode_grid(R, C, kb.device)
    j = kb.jac
    det = (j[:, 2] * j[:, 5] - j[:, 3] * j[:, 4])[:, None, None]
    col = lambda t: t[:, None, None]
    kv = (col(j[:, 5]) * qr[None] - col(j[:, 4]) * qc[None]) / det
    ku = (-col(j[:, 3]) * qr[None] + col(j[:, 2]) * qc[None]) / det
    g1, g2, r50, F = col(p[:, 2]), col(p[:, 3]), col(p[:, 4]), col(p[:, nloc - 1])
    a = (1.0 + g1) * ku + g2 * kv
    b = g2 * ku + (1.0 - g1) * kv
    theta = kv * col(p[:, 0]) + ku * col(p[:, 1])
    if model in MIX_MODELS:
        # (parameter 4 is T: a gaussian of trace T_i at shear g has k^T C_i k =
        # T_i (a^2 + b^2) / (2 (1 + g^2)))
        amp, frac = _mix_table(model, p[:, 5] if model == "bdf" else p[:, 4])
        s = r50 * (a * a + b * b) / (2.0 * (1.0 + g1 * g1 + g2 * g2))
        phi = torch.zeros_like(s)
        for i in range(amp.shape[1]):
            phi = phi + col(amp[:, i]) * torch.exp(-0.5 * col(frac[:, i]) * s)
        return _model_image(kb, F * phi, theta)
    if model == "spergel":
        c = torch.tensor([_spergel_hlr(v) for v in p[:, 5].cpu().numpy()],
                         dtype=torch.float64, device=kb.device)
    elif model_id == _lib.KFIT_MOFFAT:
        c = torch.sqrt(torch.expm1(math.log(2.0) / (p[:, 5] - 1.0)))
    elif model_id == _lib.KFIT_MOFFAT_FWHM:
        c = 2.0 * torch.sqrt(torch.expm1(math.log(2.0) / p[:, 5]))
    else:
        c = torch.full((kb.n,), HLR_GAUSS if model == "gauss" else HLR_EXP,
                       dtype=torch.float64, device=kb.device)
    r0 = r50 / col(c)
    s = r0 * r0 * (a * a + b * b) / (1.0 - g1 * g1 - g2 * g2)
    if model == "gauss":
        phi = torch.exp(-0.5 * s)
    elif model == "exp":
        phi = (1.0 + s) ** -1.5
    elif model == "moffat":
        phi = _moffat_phi((col(p[:, 5]) - 1.0).expand_as(s), torch.sqrt(s))
    else:
        phi = torch.exp(-(1.0 + col(p[:, 5])) * torch.log1p(s))
    return _model_image(kb, F * phi, theta)


def _model_image(kb, amp, theta):
    """irfft2 of M^ = amp exp(-i theta) P^n with the phase that takes the origin
    back from the centre to pixel (0, 0)"""
    torch = _torch()
    R, C = kb.nrow, kb.ncol
    qr, qc = _mode_grid(R, C, kb.device)
    col = lambda t: t[:, None, None]
    ang = -theta - (qr[None] * col(kb.jac[:, 0]) + qc[None] * col(kb.jac[:, 1]))
    M = torch.polar(amp, ang)
    if kb.phat is not None:
        M = M * torch.view_as_complex(kb.phat)
    return torch.fft.irfft2(M, s=(R, C))


class KSpaceBatchFitter(object):
    """
    N Fourier-space fits in lock step on the device.

        fitter = KSpaceBatchFitter("spergel", prior=PriorSpergelSepBatch(...))
        res = fitter.go(kb, guess)          # guess (nobj, nloc - 1 + nband)

    prior: a batch prior whose descriptor() the device prior kernel serves
    (PriorSimpleSepBatch for 'gauss' / 'exp' / 'dev10', whose size term is then
    a T prior, PriorSpergelSepBatch for 'spergel' and for 'moffat', whose beta it
    serves as the one middle term, for 'bdf' a joint_prior.PriorBDFSep or the
    PriorSepBatch of one middle term as_batch_prior makes of it, or any
    joint_prior object as_batch_prior converts), up to
    NGMIX_PRIOR_MAXBAND bands; bounds: [(lo, hi)] * npars (None: the prior's),
    run through leastsqbound's transform by ngmix_lm_init_batch.  size_type
    ('moffat'): what parameter 4 is, 'r50' (or 'hlr', 'half_light_radius') or
    'fwhm'; 'dev10' and 'bdf' take T there and no size_type.  round_s2n: one more evaluation at the fitted parameters with g = 0
    adds 's2n_r' = sqrt(sum over stamps of sum w |M^|^2) to the result.
    """

    def __init__(self, model, prior=None, fit_pars=None, bounds=None, size_type=None,
                 round_s2n=False):
        self.model_id = _model_id(model, size_type)
        self.size_type = size_type
        self.round_s2n = bool(round_s2n)
        self.model = model
        self.nloc = MODEL_NLOC[model]
        self.prior = as_batch_prior(prior)
        self.fit_pars = dict(DEFAULT_LM_PARS if fit_pars is None else fit_pars)
        self.bounds = bounds
        self.rounds_launched = 0

    def _prior_record(self, npars, nband):
        if self.prior is None:
            return None
        desc = self.prior.descriptor() if hasattr(self.prior, "descriptor") else None
        if desc is None:
            raise ValueError("the k-space fit takes a prior the device prior kernel evaluates "
                             "(GaussianCen, GPriorBA, the 1-d terms of prior_batch, at most %d "
                             "bands)" % _lib.PRIOR_MAXBAND)
        if self.nloc - 1 != 5 + int(desc["nmid"][0]):
            raise ValueError("the prior is laid out for %d parameters before the fluxes, model "
                             "'%s' has %d" % (5 + int(desc["nmid"][0]), self.model,
                                              self.nloc - 1))
        if int(desc["nband"][0]) != nband:
            raise ValueError("the prior has %d flux terms, the guess %d bands"
                             % (int(desc["nband"][0]), nband))
        return desc

    @staticmethod
    def _stamp_maps(ns, nobj, stamp_obj, stamp_band, nband):
        sobj = np.arange(ns, dtype=np.int32) if stamp_obj is None else \
            np.ascontiguousarray(stamp_obj, dtype=np.int32)
        sband = np.zeros(ns, dtype=np.int32) if stamp_band is None else \
            np.ascontiguousarray(stamp_band, dtype=np.int32)
        if sobj.shape != (ns,) or sband.shape != (ns,):
            raise ValueError("stamp_obj and stamp_band have one entry per stamp")
        if ns and (np.any(np.diff(sobj) < 0) or sobj[0] < 0 or sobj[-1] >= nobj):
            raise ValueError("stamp_obj must be sorted and within the guesses")
        if np.any(sband < 0) or np.any(sband >= nband):
            raise ValueError("stamp_band must be within the guess's %d bands" % nband)
        start = np.searchsorted(sobj, np.arange(nobj + 1)).astype(np.int64)
        if np.any(np.diff(start) == 0):
            raise ValueError("every object needs a stamp")
        return sobj, sband, start

    def go(self, kb, guess, stamp_obj=None, stamp_band=None):
        torch = _torch()
        L = _lib.lib()
        dev = kb.device
        d_guess = _as_device_f64(np.asarray(guess) if not hasattr(guess, "device") else guess, dev)
        if d_guess.ndim != 2:
            raise ValueError("guess must be (nobj, npars)")
        nobj, n = d_guess.shape
        nband = n - (self.nloc - 1)
        if nband < 1 or n > _lib.LM_NPMAX:
            raise ValueError("'%s' takes %d + nband parameters, at most %d; got %d"
                             % (self.model, self.nloc - 1, _lib.LM_NPMAX, n))
        sobj, sband, start = self._stamp_maps(kb.n, nobj, stamp_obj, stamp_band, nband)
        desc = self._prior_record(n, nband)
        bounds = self.bounds
        if bounds is None and self.prior is not None:
            bounds = getattr(self.prior, "bounds", None)
        lo = hi = None
        if bounds is not None:
            lo, hi = bounds_arrays(bounds, n)
        fp = self.fit_pars
        maxfev = int(fp.get("maxfev", 4000))
        nsum, nosum = _lib.LM_NSUM if self.nloc == 6 else 36, n * (n + 1) // 2 + n + 1
        up = lambda a: torch.from_numpy(a).to(dev)
        with _on_device(dev):
            stream = _stream()
            d_states = torch.empty(nobj * _lib.LM_STATE_DTYPE.itemsize, dtype=torch.uint8,
                                   device=dev)
            d_sobj, d_sband, d_start = up(sobj), up(sband), up(start)
            d_npix = up(np.diff(start) * np.int64(kb.npix_eff))
            # with mode weights the kernel counts the components that enter dof
            d_mw = kb.mode_weight
            d_ncomp = torch.zeros(kb.n, dtype=torch.int32, device=dev) if d_mw is not None \
                else None
            d_sums = torch.zeros((kb.n, nsum), dtype=torch.float64, device=dev)
            d_status = torch.zeros(kb.n, dtype=torch.int32, device=dev)
            d_sstats = torch.zeros((kb.n, 2), dtype=torch.float64, device=dev)
            d_ostats = torch.zeros((nobj, 2), dtype=torch.float64, device=dev)
            d_osums = torch.zeros((nobj, nosum), dtype=torch.float64, device=dev) \
                if desc is not None else None
            _lib.check(L.ngmix_lm_init_batch(
                _dptr(d_states), nobj, n, _dptr(d_guess), float(fp.get("ftol", 1.49012e-8)),
                float(fp.get("xtol", 1.49012e-8)), float(fp.get("gtol", 0.0)), maxfev,
                float(fp.get("factor", 100.0)), _lib.LM_MODE_ANALYTIC,
                _lib.ptr(lo) if lo is not None else None,
                _lib.ptr(hi) if hi is not None else None, stream), "ngmix_lm_init_batch")
            P = _lib.KFitProblem()
            P.dhat, P.wbar, P.jac = kb.dhat.data_ptr(), kb.wbar.data_ptr(), kb.jac.data_ptr()
            P.phat = kb.phat.data_ptr() if kb.phat is not None else None
            P.nstamps, P.nobj, P.states = kb.n, nobj, d_states.data_ptr()
            P.stamp_obj, P.stamp_band = d_sobj.data_ptr(), d_sband.data_ptr()
            P.obj_start = d_start.data_ptr()
            P.sums, P.status = d_sums.data_ptr(), d_status.data_ptr()
            P.stamp_stats, P.obj_stats = d_sstats.data_ptr(), d_ostats.data_ptr()
            if desc is not None:
                P.prior, P.obj_sums = desc.ctypes.data, d_osums.data_ptr()
            P.prior_step = STEP_PRIOR
            P.nrow, P.ncol, P.model = kb.nrow, kb.ncol, self.model_id
            P.nloc_npars = self.nloc + 256 * n

            # rounds queued blind; the pinned count of running fits says when to stop
            total, grow, chunks = 0, ROUNDS_FIRST, []
            while True:
                nr = min(grow, 2 * maxfev + 5 - total)
                d_counts = torch.empty(nr, dtype=torch.int32, device=dev)
                h_counts = torch.empty(nr, dtype=torch.int32, pin_memory=True)
                if d_mw is None:
                    _lib.check(L.ngmix_kfit_rounds_batch(
                        ctypes.byref(P), nr, _dptr(d_counts),
                        ctypes.c_void_p(h_counts.data_ptr()), None, stream),
                        "ngmix_kfit_rounds_batch")
                else:
                    _lib.check(L.ngmix_kfit_rounds_w_batch(
                        ctypes.byref(P), _dptr(d_mw), _dptr(d_ncomp), nr, _dptr(d_counts),
                        ctypes.c_void_p(h_counts.data_ptr()), None, stream),
                        "ngmix_kfit_rounds_w_batch")
                torch.cuda.current_stream(dev).synchronize()
                chunks.append((d_counts, h_counts))
                total += nr
                if int(h_counts[-1]) == 0:
                    break
                if total >= 2 * maxfev + 5:
                    raise RuntimeError("batched LM did not terminate")
                grow = min(2 * grow, 64)
            self.rounds_launched = total
            if d_mw is not None:
                d_npix = torch.zeros(nobj, dtype=torch.int64, device=dev)
                d_npix.index_add_(0, d_sobj.long(), d_ncomp.long())

            d_ffx = None
            if desc is not None:
                d_ffx = torch.empty(nobj, dtype=torch.float64, device=dev)
                d_lnp = torch.empty(nobj, dtype=torch.float64, device=dev)
                _lib.check(L.ngmix_lm_prior_finish_batch(
                    _dptr(d_states), nobj, _lib.ptr(desc), _dptr(d_ffx), _dptr(d_lnp), stream),
                    "ngmix_lm_prior_finish_batch")
            d_rec = torch.empty((nobj, 4 + 2 * n + 2 * n * n), dtype=torch.float64, device=dev)
            _lib.check(L.ngmix_lm_finalize_batch(
                _dptr(d_states), nobj, _dptr(d_npix), _dptr(d_ffx), float(PDEF), float(CDEF),
                _dptr(d_rec), stream), "ngmix_lm_finalize_batch")
            d_flat = torch.empty(nobj * (2 * n + _lib.LM_NCOLS), dtype=torch.float64, device=dev)
            d_tri = torch.empty((nobj, n * (n + 1) // 2), dtype=torch.float64, device=dev)
            _lib.check(L.ngmix_lm_pack_batch(
                _dptr(d_states), nobj, n, _dptr(d_rec), _dptr(d_ostats), None, _dptr(d_npix),
                _dptr(d_flat), ctypes.c_void_p(d_flat.data_ptr() + 8 * nobj * 2 * n),
                _dptr(d_tri), stream), "ngmix_lm_pack_batch")
            flat = d_flat.cpu().numpy()
            tri = d_tri.cpu().numpy()
            self.stamp_status = d_status.cpu().numpy()
            s2n_r = self._round_s2n(kb, P, d_states, d_sobj, nobj, n) if self.round_s2n else None
        self._d_states = d_states
        res = self._package(flat, tri, nobj, n)
        if s2n_r is not None:
            res["s2n_r"] = s2n_r
        return res

    def _round_s2n(self, kb, P, d_states, d_sobj, nobj, n):
        """sqrt(sum w |M^|^2) over each object's stamps at its fitted parameters
        with g = 0: one evaluation on a copy of the states (xt = x, g zeroed,
        every fit running again), read from the stamp_stats column"""
        torch = _torch()
        L = _lib.lib()
        dev = kb.device
        rec = _lib.LM_STATE_DTYPE
        states = np.frombuffer(d_states.cpu().numpy().tobytes(), dtype=rec).copy()
        states["xt"] = states["x"]
        states["xt"][:, 2:4] = 0.0
        states["phase"] = 0
        d_copy = torch.from_numpy(states.view(np.uint8)).to(dev)
        d_sums = torch.empty((kb.n, _lib.LM_NSUM if self.nloc == 6 else 36), dtype=torch.float64,
                             device=dev)
        d_stats = torch.zeros((kb.n, 2), dtype=torch.float64, device=dev)
        if kb.mode_weight is None:
            _lib.check(L.ngmix_kfit_eval_batch(
                P.dhat, P.phat, P.wbar, P.jac, kb.nrow, kb.ncol, kb.n, self.model_id,
                _dptr(d_copy), P.stamp_obj, P.stamp_band, _dptr(d_sums), None, _dptr(d_stats),
                _stream()), "ngmix_kfit_eval_batch")
        else:
            _lib.check(L.ngmix_kfit_eval_w_batch(
                P.dhat, P.phat, _dptr(kb.mode_weight), P.wbar, P.jac, kb.nrow, kb.ncol, kb.n,
                self.model_id, _dptr(d_copy), P.stamp_obj, P.stamp_band, _dptr(d_sums), None,
                _dptr(d_stats), None, _stream()), "ngmix_kfit_eval_w_batch")
        mm = torch.zeros(nobj, dtype=torch.float64, device=dev)
        mm.index_add_(0, d_sobj.long(), d_stats[:, 1])
        return torch.sqrt(mm).cpu().numpy()

    def states(self):
        """the raw ngmix_lm_state records of the last go() (debugging, tests)"""
        return np.frombuffer(self._d_states.cpu().numpy().tobytes(), dtype=_lib.LM_STATE_DTYPE)

    def _package(self, flat, tri, nobj, n):
        rec = flat[:nobj * 2 * n].reshape(nobj, 2 * n)
        cols = flat[nobj * 2 * n:].reshape(_lib.LM_NCOLS, nobj)
        pars = rec[:, :n].copy()
        cov = np.empty((nobj, n, n))
        iu = np.triu_indices(n)
        cov[:, iu[0], iu[1]] = tri
        cov[:, iu[1], iu[0]] = tri
        res = {
            "model": self.model,
            "pars": pars, "pars_err": rec[:, n:2 * n].copy(), "pars_cov": cov,
            "flags": cols[0].astype(np.int64), "nfev": cols[1].astype(np.int64),
            "ier": cols[2].astype(np.int64), "njev": cols[4].astype(np.int64),
            "dof": cols[9].astype(np.int64), "lnprob": cols[5].copy(),
            "chi2per": cols[10].copy(), "s2n": cols[11].copy(),
            "g": pars[:, 2:4].copy(), "g_cov": cov[:, 2:4, 2:4].copy(),
            "flux": pars[:, self.nloc - 1:].copy(),
        }
        size = "T" if self.model in MIX_MODELS else "r50"
        res[size] = pars[:, 4].copy()
        if size == "T":
            res["T_err"] = res["pars_err"][:, 4].copy()
        if self.model == "bdf":
            res["fracdev"] = pars[:, 5].copy()
            res["fracdev_err"] = res["pars_err"][:, 5].copy()
        if self.model == "spergel":
            res["nu"] = pars[:, 5].copy()
        if self.model == "moffat":
            res["beta"] = pars[:, 5].copy()
        return res


def _flatten_to_kbatch(list_of_obs):
    """the stamps of a list of Observation / ObsList / MultiBandObsList as one
    KStampBatch, with the object and the band of each stamp"""
    from .observation import get_mb_obs
    images, weights, jacs, pimages, pjacs, sobj, sband = [], [], [], [], [], [], []
    for i, obs in enumerate(list_of_obs):
        for band, olist in enumerate(get_mb_obs(obs)):
            for o in olist:
                images.append(o.image)
                weights.append(o.weight)
                jacs.append(o.jacobian._data)
                if o.has_psf():
                    pimages.append(o.psf.image)
                    pjacs.append(o.psf.jacobian._data)
                sobj.append(i)
                sband.append(band)
    if pimages and len(pimages) != len(images):
        raise ValueError("either every observation carries a psf or none does")
    shapes = {im.shape for im in images} | {("psf",) + im.shape for im in pimages}
    if len({s for s in shapes if s[0] != "psf"}) != 1 or \
            len({s for s in shapes if s[0] == "psf"}) > 1:
        raise ValueError("a k-space batch holds stamps of one shape")
    kb = KStampBatch.from_images(
        np.stack(images), np.stack(weights), np.concatenate(jacs).view(np.float64).reshape(-1, 8),
        psf_images=np.stack(pimages) if pimages else None,
        psf_jacobians=np.concatenate(pjacs).view(np.float64).reshape(-1, 8)
        if pimages else None)
    return kb, sobj, sband


class KSpaceFitter(object):
    """
    The per-object entry point: Observation / ObsList / MultiBandObsList in,
    one dict per object out.  go_many fits all its objects as ONE batch; go is
    go_many of one object.  Every observation of a call has one shape, and
    either all of them carry a psf observation or none does.
    """

    def __init__(self, model, prior=None, fit_pars=None, size_type=None, round_s2n=False):
        self._batch = KSpaceBatchFitter(model, prior=prior, fit_pars=fit_pars,
                                        size_type=size_type, round_s2n=round_s2n)
        self.model = model

    def go(self, obs, guess):
        return self.go_many([obs], [guess])[0]

    def go_many(self, list_of_obs, guesses):
        kb, sobj, sband = _flatten_to_kbatch(list_of_obs)
        res = self._batch.go(kb, np.atleast_2d(np.asarray(guesses, dtype=np.float64)),
                             stamp_obj=sobj, stamp_band=sband)
        out = []
        for i in range(len(list_of_obs)):
            out.append({k: (v if isinstance(v, str) else v[i]) for k, v in res.items()})
        return out


class KSpaceFluxBatch(object):
    """
    The linear flux of a FIXED unit-flux template in the k-space definition of
    the fits, per object over its stamps of one band (kfit_flux_kernel: three
    sums per stamp, no LM):

        res = KSpaceFluxBatch().go(kb)                       # the psf's flux
        res = KSpaceFluxBatch("exp", pars).go(kb)            # a profile's

    model None: a point source at the stamp's centre, so the template is the
    psf itself (the reference's GalsimPSFFluxFitter); pars is then None, or
    (nstamps, 2) centres.  Otherwise pars (nstamps, nloc - 1): each stamp's
    [cen1, cen2, g1, g2, size, (nu | beta | fracdev)], the size T for 'dev10'
    and 'bdf'.  res: (nobj,) arrays flags, flux,
    flux_err, chi2per, dof, as PSFFluxBatch gives them: where the template's
    sum is not positive or a sum is not finite, DIV_ZERO with flux = PDEF,
    flux_err = CDEF and chi2per = 0.
    """

    def __init__(self, model=None, pars=None, size_type=None):
        self.model = model
        self.model_id = _lib.KFIT_POINT if model is None else _model_id(model, size_type)
        self.npars = 5 if model is None else MODEL_NLOC[model] - 1
        self.pars = pars

    def sums(self, kb):
        """the per-stamp sums (nstamps, 3) and status, device tensors"""
        torch = _torch()
        dev = kb.device
        if self.pars is None:
            if self.model is not None:
                raise ValueError("a '%s' template needs its parameters" % self.model)
            p = np.zeros((kb.n, 5))
        else:
            p = self.pars
        d_p = _as_device_f64(np.asarray(p) if not hasattr(p, "device") else p, dev)
        if self.model is None and d_p.shape == (kb.n, 2):
            d_p = torch.cat([d_p, torch.zeros((kb.n, 3), dtype=torch.float64, device=dev)], dim=1)
        if d_p.shape != (kb.n, self.npars):
            raise ValueError("pars must be (%d, %d)" % (kb.n, self.npars))
        d_p = d_p.contiguous()
        with _on_device(dev):
            d_out = torch.empty((kb.n, 3), dtype=torch.float64, device=dev)
            d_status = torch.zeros(kb.n, dtype=torch.int32, device=dev)
            self._ncomp = None
            if kb.mode_weight is None:
                _lib.check(_lib.lib().ngmix_kfit_flux_batch(
                    _dptr(kb.dhat), _dptr(kb.phat) if kb.phat is not None else None,
                    _dptr(kb.wbar), ctypes.c_void_p(kb.jac.data_ptr()), kb.nrow, kb.ncol, kb.n,
                    self.model_id, _dptr(d_p), _dptr(d_out), _dptr(d_status), _stream()),
                    "ngmix_kfit_flux_batch")
            else:
                d_ncomp = torch.zeros(kb.n, dtype=torch.int32, device=dev)
                _lib.check(_lib.lib().ngmix_kfit_flux_w_batch(
                    _dptr(kb.dhat), _dptr(kb.phat) if kb.phat is not None else None,
                    _dptr(kb.mode_weight), _dptr(kb.wbar), ctypes.c_void_p(kb.jac.data_ptr()),
                    kb.nrow, kb.ncol, kb.n, self.model_id, _dptr(d_p), _dptr(d_out),
                    _dptr(d_status), _dptr(d_ncomp), _stream()), "ngmix_kfit_flux_w_batch")
                self._ncomp = d_ncomp.cpu().numpy()
        return d_out, d_status

    def go(self, kb, stamp_obj=None, stamp_band=None):
        from .flags import DIV_ZERO
        ns = kb.n
        sobj = np.arange(ns, dtype=np.int64) if stamp_obj is None else \
            np.ascontiguousarray(stamp_obj, dtype=np.int64)
        if sobj.shape != (ns,) or (ns and sobj.min() < 0):
            raise ValueError("stamp_obj must be (nstamps,) object indices")
        if stamp_band is not None:
            sband = np.asarray(stamp_band)
            if sband.shape != (ns,):
                raise ValueError("stamp_band has one entry per stamp")
            for o in np.unique(sobj):
                if np.unique(sband[sobj == o]).size != 1:
                    raise ValueError("the stamps of an object must be of one band")
        d_out, d_status = self.sums(kb)
        out = d_out.cpu().numpy()
        self.stamp_status = d_status.cpu().numpy()
        nobj = int(sobj.max()) + 1 if ns else 0
        A, B, E = (np.bincount(sobj, weights=out[:, k], minlength=nobj) for k in range(3))
        nstamp = np.bincount(sobj, minlength=nobj)
        bad_stamp = np.bincount(sobj, weights=self.stamp_status != 0, minlength=nobj) > 0
        with np.errstate(all="ignore"):
            bad = ~(B > 0) | ~np.isfinite(A + B + E) | bad_stamp
            Bs = np.where(bad, 1.0, B)
            flux = np.where(bad, PDEF, A / Bs)
            flux_err = np.where(bad, CDEF, 1.0 / np.sqrt(Bs))
            chi2 = np.where(bad, 0.0, E - A * A / Bs)
        if self._ncomp is None:
            dof = (nstamp * kb.npix_eff - 1).astype("f8")
        else:
            # (mode weights: the components with a positive weight)
            dof = np.bincount(sobj, weights=self._ncomp, minlength=nobj) - 1.0
        dof = np.where(dof <= 0, 1.0e-6, dof)
        flags = np.where(bad, DIV_ZERO, 0).astype(np.int64)
        return {"flags": flags, "flux": flux, "flux_err": flux_err, "chi2per": chi2 / dof,
                "dof": dof}


class KSpaceFluxFitter(object):
    """
    KSpaceFluxBatch for Observation / ObsList, the two the reference's
    GalsimPSFFluxFitter takes: go(obs) one dict, go_many(list) a dict of
    (nobj,) arrays.  model None: the psf's flux (every observation carries a
    psf); a model name with pars [cen1, cen2, g1, g2, size, (nu | beta |
    fracdev)] per object: that profile's.
    """

    def __init__(self, model=None, size_type=None):
        self.model = model
        self.size_type = size_type

    def go(self, obs, pars=None):
        res = self.go_many([obs], None if pars is None else [pars])
        return {k: v[0] for k, v in res.items()}

    def go_many(self, list_of_obs, pars=None):
        from .observation import Observation, ObsList
        for obs in list_of_obs:
            if not isinstance(obs, (Observation, ObsList)):
                raise ValueError("obs should be Observation or ObsList")
        kb, sobj, _ = _flatten_to_kbatch(list_of_obs)
        if self.model is None and kb.phat is None:
            raise ValueError("the psf flux needs the observations' psf images")
        if pars is not None:
            pars = np.atleast_2d(np.asarray(pars, dtype=np.float64))[np.asarray(sobj)]
        return KSpaceFluxBatch(self.model, pars, size_type=self.size_type).go(kb, stamp_obj=sobj)
