"""
Fourier-space profile fits: 'gauss', 'exp' and 'spergel'
fitted to the transform of a stamp's own samples.

The reference's GalsimFitter / GalsimSpergelFitter fit the exact profile to a
k-space observation that galsim draws.  Here the observation is the rfft2 half
plane of the stamp itself times the centre phase, the psf enters as the
transform of its own stamp (no psf model is fitted), and the lock-step LM
driver of ngmix_amd/lm_batch.py runs with kfit_eval_kernel in place of the
pixel pass:

    KStampBatch              the transforms D^, P^n, the Parseval weight
    KSpaceBatchFitter        N fits in lock step, a dict of arrays back
    KSpaceFitter             Observation / ObsList / MultiBandObsList in, one
                             batch per call
    kmodel_images            the model's real-space image, for residuals

What this is NOT: the pixel values of a KStampBatch are not galsim's (no
interpolant, no stepk / getGoodImageSize grid), the weight is the Parseval
weight (twice the reference's), aliases of the profile are not summed (galsim's
k-space fit does not sum them either), and 'dev' and Moffat are not offered.

Parameters: [cen1, cen2, g1, g2, r50, F_band...]; 'spergel':
[cen1, cen2, g1, g2, r50, nu, F_band...].
"""
import ctypes
import math

import numpy as np

from . import _lib
from .batch import StampBatch, _dptr, _stream, _torch, _on_device, _as_device_f64
from .defaults import PDEF, CDEF, DEFAULT_LM_PARS
from .fitting import STEP_PRIOR
from .prior_batch import as_batch_prior, bounds_arrays

__all__ = ["KStampBatch", "KSpaceBatchFitter", "KSpaceFitter", "kmodel_images"]

MODELS = {"gauss": _lib.KFIT_GAUSS, "exp": _lib.KFIT_EXP, "spergel": _lib.KFIT_SPERGEL}
MODEL_NLOC = {"gauss": 6, "exp": 6, "spergel": 7}
HLR_GAUSS = math.sqrt(2.0 * math.log(2.0))
HLR_EXP = 1.6783469900166605
ROUNDS_FIRST = 12      # rounds queued blind before the first look at the counts


def _model_id(model):
    if model not in MODELS:
        raise ValueError("k-space fits offer %s, got %r ('dev' has no closed-form transform)"
                         % (tuple(MODELS), model))
    return MODELS[model]


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
    """

    def __init__(self, dhat, phat, wbar, jac, nrow, ncol):
        self.dhat, self.phat, self.wbar, self.jac = dhat, phat, wbar, jac
        self.nrow, self.ncol = int(nrow), int(ncol)
        self.n = int(dhat.shape[0])
        self.device = dhat.device
        self.npix_eff = (self.nrow - (self.nrow % 2 == 0)) * (self.ncol - (self.ncol % 2 == 0))

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


def _spergel_hlr(nu):
    c, dc = ctypes.c_double(), ctypes.c_double()
    _lib.check(_lib.lib().ngmix_spergel_hlr(float(nu), ctypes.byref(c), ctypes.byref(dc)),
               "ngmix_spergel_hlr")
    return c.value


def kmodel_images(kb, pars, model):
    """
    The real-space images (N, R, C) of the band-limited, periodic model at
    pars (N, nloc) -- each stamp's LOCAL parameters, one flux -- by irfft2 of
    M^ about the stamp's centre: what the fit's residuals are residuals of (the
    Nyquist modes included here, dropped there).  torch ops; not a hot path.
    """
    torch = _torch()
    _model_id(model)
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
    if model == "spergel":
        c = torch.tensor([_spergel_hlr(v) for v in p[:, 5].cpu().numpy()],
                         dtype=torch.float64, device=kb.device)
    else:
        c = torch.full((kb.n,), HLR_GAUSS if model == "gauss" else HLR_EXP,
                       dtype=torch.float64, device=kb.device)
    r0 = r50 / col(c)
    a = (1.0 + g1) * ku + g2 * kv
    b = g2 * ku + (1.0 - g1) * kv
    s = r0 * r0 * (a * a + b * b) / (1.0 - g1 * g1 - g2 * g2)
    if model == "gauss":
        phi = torch.exp(-0.5 * s)
    elif model == "exp":
        phi = (1.0 + s) ** -1.5
    else:
        phi = torch.exp(-(1.0 + col(p[:, 5])) * torch.log1p(s))
    theta = kv * col(p[:, 0]) + ku * col(p[:, 1])
    # M^ and the phase that takes the origin back from the centre to pixel (0, 0)
    ang = -theta - (qr[None] * col(j[:, 0]) + qc[None] * col(j[:, 1]))
    M = torch.polar(F * phi, ang)
    if kb.phat is not None:
        M = M * torch.view_as_complex(kb.phat)
    return torch.fft.irfft2(M, s=(R, C))


class KSpaceBatchFitter(object):
    """
    N Fourier-space fits in lock step on the device.

        fitter = KSpaceBatchFitter("spergel", prior=PriorSpergelSepBatch(...))
        res = fitter.go(kb, guess)          # guess (nobj, nloc - 1 + nband)

    prior: a batch prior whose descriptor() the device prior kernel serves
    (PriorSimpleSepBatch for 'gauss' / 'exp', PriorSpergelSepBatch for
    'spergel', or a joint_prior object as_batch_prior converts), up to
    NGMIX_PRIOR_MAXBAND bands; bounds: [(lo, hi)] * npars (None: the prior's),
    run through leastsqbound's transform by ngmix_lm_init_batch.
    """

    def __init__(self, model, prior=None, fit_pars=None, bounds=None):
        self.model_id = _model_id(model)
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
                _lib.check(L.ngmix_kfit_rounds_batch(
                    ctypes.byref(P), nr, _dptr(d_counts), ctypes.c_void_p(h_counts.data_ptr()),
                    None, stream), "ngmix_kfit_rounds_batch")
                torch.cuda.current_stream(dev).synchronize()
                chunks.append((d_counts, h_counts))
                total += nr
                if int(h_counts[-1]) == 0:
                    break
                if total >= 2 * maxfev + 5:
                    raise RuntimeError("batched LM did not terminate")
                grow = min(2 * grow, 64)
            self.rounds_launched = total

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
        self._d_states = d_states
        return self._package(flat, tri, nobj, n)

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
            "r50": pars[:, 4].copy(), "flux": pars[:, self.nloc - 1:].copy(),
        }
        if self.model == "spergel":
            res["nu"] = pars[:, 5].copy()
        return res


class KSpaceFitter(object):
    """
    The per-object entry point: Observation / ObsList / MultiBandObsList in,
    one dict per object out.  go_many fits all its objects as ONE batch; go is
    go_many of one object.  Every observation of a call has one shape, and
    either all of them carry a psf observation or none does.
    """

    def __init__(self, model, prior=None, fit_pars=None):
        self._batch = KSpaceBatchFitter(model, prior=prior, fit_pars=fit_pars)
        self.model = model

    def go(self, obs, guess):
        return self.go_many([obs], [guess])[0]

    def go_many(self, list_of_obs, guesses):
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
        res = self._batch.go(kb, np.atleast_2d(np.asarray(guesses, dtype=np.float64)),
                             stamp_obj=sobj, stamp_band=sband)
        out = []
        for i in range(len(list_of_obs)):
            out.append({k: (v if isinstance(v, str) else v[i]) for k, v in res.items()})
        return out
