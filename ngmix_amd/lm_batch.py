"""
Batched Levenberg-Marquardt fitting: N independent objects advance in lock
step, two kernel launches per LM step for all of them.

Reference (per object): Fitter.go -> run_leastsq -> scipy leastsq / MINPACK
lmder, calling back into FitModel.calc_fdiff / calc_jacobian once per
evaluation (ngmix/fitting/fitters.py:64-112, leastsqbound.py:33-155,
results.py:439-570).  Here the same iteration (csrc/lm_core.hpp: lmder's
decision logic, tested against MINPACK in tests/test_lm_core.py) runs on the
device for every object at once:

    ngmix_lm_eval_batch     residuals + analytic jacobian at each object's
                            trial point, reduced on chip to J^T J, J^T f, |f|^2
    ngmix_lm_advance_batch  one lmder step per object

    ngmix_lm_finalize_batch run_leastsq's packaging per object (cov_x from
                            R / ipvt, chi2/dof scaling, flags)

and the results are packaged exactly as run_leastsq / FitModel.set_fit_result
package one fit: flags, nfev, ier, pars, pars_err, pars_cov0, pars_cov, and for
flags == 0 lnprob, s2n_numer, s2n_denom, npix, chi2per, dof, s2n_w, s2n, g,
g_cov, g_err, T, T_err, flux, flux_err (flux_cov when nband > 1).

Scope: gauss / exp / dev with the analytic jacobian (lmder, as the reference's
Fitter: results.py SIMPLE_ANALYTIC_MODELS) and gauss / turb / exp / dev / bdf /
bd with MINPACK's forward differences evaluated inside the pixel pass (lmdif,
what the reference runs for the models without analytic derivatives).  A
batch prior (ngmix_amd/prior_batch.py) adds the reference's prior rows to every
object's residual vector and its bounds run leastsqbound's parameter transform
inside the iteration; prior=None is legal as in the reference (zero prior rows,
no bounds, results.py:354-357).
"""
import collections
import ctypes
import os
import time

import numpy as np

from . import _lib
from .batch import GMixBatch, _dptr, _stream, _torch, _on_device
from .defaults import PDEF, CDEF, DEFAULT_LM_PARS
from .gmix import get_model_num
from .fitting import get_lm_n_prior_pars, STEP_PRIOR
from .prior_batch import as_batch_prior, bounds_arrays, prior_normal_sums

__all__ = ["LMBatchFitter"]


SIMPLE_ANALYTIC_MODELS = ("gauss", "exp", "dev")
# local (per band) parameter count of the models the device kernels fill
MODEL_NLOC = {"gauss": 6, "turb": 6, "exp": 6, "dev": 6, "bdf": 7, "bd": 8}


class LMBatchResult(dict):
    """the dict of per-object arrays LMBatchFitter.go returns (run_leastsq's
    and set_fit_result's keys); entries registered with set_lazy stay on the
    device and are downloaded when first read"""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self._lazy = {}

    def set_lazy(self, key, fetch):
        """fetch(result) -> value, called once when `key` is first read (it is
        handed the result instead of closing over it: a closure would make a
        reference cycle, and the pinned download buffers behind the arrays
        would wait for the cyclic collector instead of going back to the
        allocator when the result is dropped)"""
        self._lazy[key] = fetch

    def __missing__(self, key):
        if key in self._lazy:
            value = self._lazy.pop(key)(self)
            self[key] = value
            return value
        raise KeyError(key)

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self._lazy

    def get(self, key, default=None):
        return self[key] if key in self else default

    def keys(self):
        return list(dict.keys(self)) + list(self._lazy)

    def __setitem__(self, key, value):
        self._lazy.pop(key, None)
        dict.__setitem__(self, key, value)

    def __delitem__(self, key):
        if self._lazy.pop(key, None) is None:
            dict.__delitem__(self, key)

    # every whole-mapping view counts the lazy keys and reads through them, so
    # that items() / dict(res) / {**res} / copy / pickle see one ordinary dict
    def materialize(self):
        for key in list(self._lazy):
            self[key]
        return self

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return dict.__len__(self) + len(self._lazy)

    def values(self):
        return [self[k] for k in self.keys()]

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def pop(self, key, *default):
        if key in self:
            value = self[key]
            dict.__delitem__(self, key)
            return value
        if default:
            return default[0]
        raise KeyError(key)

    def copy(self):
        return LMBatchResult(self.items())

    __copy__ = copy

    def __eq__(self, other):
        return dict.__eq__(self.materialize(), other)

    __hash__ = None

    def __repr__(self):
        return dict.__repr__(self.materialize())

    def __reduce__(self):
        # the fetchers are closures over device tensors: pickle the values
        return (LMBatchResult, (dict(self.items()),))


class _Job(object):
    """one batch on its way through LMBatchFitter: what the stages of _enqueue_on
    leave for each other and for _collect (an undeclared field cannot be set)"""
    __slots__ = (
        # the call: device, raw stream handle, arguments, host timing
        "dev", "stream", "streaming", "check_every", "phases", "tmark", "host_enqueue_ms",
        # the batch and its layout (_stamp_maps, _psf_records)
        "stamps", "batch", "psf", "npsf", "nobj", "npars", "nband", "ns", "nsum", "sobj",
        "sband", "obj_start", "trivial_map", "npix_obj", "maxfev", "modnum",
        # device buffers (_alloc_buffers): views of the arena or separate tensors
        "arena", "out_shapes", "d_states", "d_sums", "d_status", "d_sstats", "d_ostats",
        "d_flat", "d_tri", "d_rec",
        # the one pinned upload and its views (_upload)
        "h_all", "d_all", "d_guess", "d_npix", "d_sobj", "d_sband", "d_start",
        # the prior record and the precise-covariance buffers
        "prior_desc", "d_osums", "d_prior_lnp", "d_jacpt", "d_psums",
        # the lock-step loop: its form, the library's problem record, what ran
        "loop_stats", "nsplit", "host_loop", "problem", "chunks", "useful_rounds",
        "loop_ms_host", "legacy_ev", "ev_init", "ev_post",
        # the results (_queue_results): device views, pinned downloads, events
        "d_cov0", "fit_ctx", "h_flat", "h_tri", "h_cov0", "copied", "cov_copied")

    def __init__(self):   # the fields that are read before their stage has run
        self.problem = self.d_psums = self.d_prior_lnp = self.useful_rounds = None
        self.ev_post = self.legacy_ev = None
        self.chunks, self.loop_ms_host = [], 0.0


# one call of ngmix_lm_rounds_batch: rounds queued, their counts of running fits (device,
# pinned host), the per-launch timing events or None, the _HipEvents pair around the call
_Chunk = collections.namedtuple("_Chunk", "nrounds d_counts h_counts events span")


class _Piece(object):
    """a run of whole objects in the host-driven loop: objects [o_lo, o_hi),
    stamps [s_lo, s_hi), its ngmix_batch record, side stream, device counter of
    running fits, the pinned ring it comes back through, reads pending, rounds"""
    __slots__ = ("o_lo", "o_hi", "s_lo", "s_hi", "batch", "stream", "nact", "live", "active",
                 "ring", "pend", "launched", "ev_idx")


class _HipEvents(object):
    """n hipEvent_t of the library (ngmix_events_create), destroyed with it"""

    def __init__(self, n):
        self.n = n
        self.handles = (ctypes.c_void_p * n)()
        _lib.check(_lib.lib().ngmix_events_create(n, self.handles), "ngmix_events_create")

    def __del__(self):
        try:
            _lib.lib().ngmix_events_destroy(self.n, self.handles)
        except Exception:
            pass


def _record(events, i, stream):
    """record event i of an array of hipEvent_t on a stream (None: no timing)"""
    if events is not None:
        _lib.check(_lib.lib().ngmix_event_record(events[i], stream), "ngmix_event_record")


def _elapsed_ms(a, b, context="ngmix_event_elapsed_ms"):
    ms = ctypes.c_float()
    _lib.check(_lib.lib().ngmix_event_elapsed_ms(a, b, ctypes.byref(ms)), context)
    return float(ms.value)


class _EventPool(object):
    """timing events handed out as ctypes arrays and taken back (bench.py's
    time_kernels mode records ~25 events per fit: no create / destroy per fit)"""

    def __init__(self):
        self.free = []
        self.owned = []

    def take(self, n):
        arr = (ctypes.c_void_p * n)()
        need = n - min(n, len(self.free))
        if need:
            fresh = _HipEvents(need)
            self.owned.append(fresh)
            self.free.extend(fresh.handles[i] for i in range(need))
        for i in range(n):
            arr[i] = self.free.pop()
        return arr

    def give(self, arr):
        if arr is not None:
            self.free.extend(arr[i] for i in range(len(arr)))


# A small batch (the per-object interface's one-object fits above all) is host
# bound: ~0.4 ms of Python per fit against 0.26 ms of kernels, and every
# torch.empty / copy_ / event is 2-8 us of it.  Its device buffers are therefore
# views of ONE allocation, its outputs (packed block | covariance triangle |
# finalize records) contiguous at the end of it so that they come back in ONE
# download, and the zeros of the statistics accumulator ride in the upload.
SMALL_BATCH = 64
# the most lock-step rounds queued blind from the last batch's count (a round
# that finds every fit finished costs two empty launches, ~20 us; co-elliptical
# psf fits run 60-70 rounds, their tails hundreds: a cap below the rounds a
# workload needs makes every call take the miss path)
ROUNDS_HINT_CAP = 256


def _carve(torch, dev, pieces):
    """one uint8 allocation cut into named views: pieces = [(name, shape,
    torch dtype)], each 16-byte aligned; returns (buffer, views, offsets)"""
    offs, at = {}, 0
    for name, shape, dt in pieces:
        nbytes = int(np.prod(shape)) * dt.itemsize
        offs[name] = (at, nbytes)
        at += (nbytes + 15) // 16 * 16
    buf = torch.empty(at, dtype=torch.uint8, device=dev)
    views = {}
    for name, shape, dt in pieces:
        a, nb = offs[name]
        views[name] = buf[a:a + nb].view(dt).reshape(shape)
    return buf, views, offs


def _stamp_maps(ns, npix_kept, guess, stamp_obj, stamp_band, nloc):
    """the layout of a batch, checked, in host arrays (numpy alone): ns stamps of
    npix_kept pixels, guess (nobj, nloc - 1 + nband) or one row, the stamps'
    object and band indices or None.  Returns guess (2-d float64), sobj, sband
    (int32), obj_start (nobj + 1 stamp offsets), trivial_map (no map given: stamp
    i is object i in band 0), npix_obj (pixels per object) and nband."""
    guess = np.ascontiguousarray(np.atleast_2d(guess), dtype="f8")
    nobj, npars = guess.shape
    nshape = nloc - 1
    nband = npars - nshape
    if nband < 1 or npars > _lib.LM_NPMAX:
        raise ValueError("guess must have %d + nband (1..%d) columns"
                         % (nshape, _lib.LM_NPMAX - nshape))
    if stamp_obj is None:
        if ns != nobj:
            raise ValueError("stamp_obj is needed when objects have several stamps")
        sobj = np.arange(ns, dtype=np.int32)
    else:
        sobj = np.ascontiguousarray(stamp_obj, dtype=np.int32)
        if sobj.shape != (ns,):
            raise ValueError("stamp_obj must be (nstamps,) and non-decreasing")
        if nobj == 1:
            # (a one-object fit: the per-object interface's batches)
            if sobj.any():
                raise ValueError("stamp_obj out of range")
        else:
            if np.any(np.diff(sobj) < 0):
                raise ValueError("stamp_obj must be (nstamps,) and non-decreasing")
            if sobj.min() < 0 or sobj.max() >= nobj:
                raise ValueError("stamp_obj out of range")
    if stamp_band is None:
        sband = np.zeros(ns, dtype=np.int32)
    else:
        sband = np.ascontiguousarray(stamp_band, dtype=np.int32)
        if sband.shape != (ns,) or sband.min() < 0 or sband.max() >= nband:
            raise ValueError("stamp_band out of range")
    trivial_map = stamp_obj is None and stamp_band is None
    npix_obj = np.asarray(npix_kept).astype(np.int64)
    if trivial_map:
        obj_start = np.arange(nobj + 1, dtype=np.int64)
    else:
        obj_start = np.array([0, ns], dtype=np.int64) if nobj == 1 else \
            np.searchsorted(sobj, np.arange(nobj + 1)).astype(np.int64)
    if ns < nobj or (nobj > 1 and np.any(np.diff(obj_start) == 0)) or ns == 0:
        raise ValueError("every object needs at least one stamp")
    if not trivial_map:
        npix_obj = np.add.reduceat(npix_obj, obj_start[:-1])
    return guess, sobj, sband, obj_start, trivial_map, npix_obj, nband


def _psf_records(psf, ns):
    """the psf argument of a fit -> (npsf, psf_host): gaussians per stamp, and
    host gauss2d records (nstamps, npsf) as the array that rides in the upload
    (Fitter.go's one-object batches); None for a GMixBatch and for no psf"""
    if psf is None:
        return 0, None
    if isinstance(psf, np.ndarray):
        psf_host = np.ascontiguousarray(psf, dtype=_lib.GAUSS2D_DTYPE).reshape(ns, -1)
        return psf_host.shape[1], psf_host
    assert psf.n == ns, "one psf mixture per stamp"
    return psf.ngauss, None


def _state_cols(d_states, name, n):
    """the first n entries of the per-parameter array `name` of every state
    record, as a float64 view (nobj, n) of the records on the device"""
    a = _lib.LM_STATE_DTYPE.fields[name][1] // 8
    return d_states.view(_torch().float64)[:, a:a + n]


def _off(t, nbytes):
    """the address nbytes into a device tensor (None for None)"""
    return ctypes.c_void_p(t.data_ptr() + int(nbytes)) if t is not None else None


class LMBatchFitter(object):
    """
    fitter = LMBatchFitter(model='exp')
    res = fitter.go(stamps, guess, psf=psf_gmixes)

    model: 'gauss' | 'exp' | 'dev' (analytic jacobian, MINPACK lmder, as the
        reference's Fitter) or 'turb' | 'bdf' | 'bd' (forward differences,
        MINPACK lmdif, as the reference runs the models without analytic
        derivatives), or 'coellip' with ngauss = 1..3 (CoellipFitter, lmdif)
    fit_pars: dict with maxfev / ftol / xtol as for Fitter (defaults
        DEFAULT_LM_PARS, ngmix/defaults.py:17)
    analytic_jacobian: False forces forward differences for gauss/exp/dev
        too (Fitter's switch of the same name)
    prior: a joint prior as the reference's callers build it
        (joint_prior.PriorSimpleSep ... of priors.py terms: put in its batch
        form by prior_batch.as_batch_prior), or a batch prior
        (prior_batch.PriorSimpleSepBatch, PriorBatchAdapter, or anything with
        their three members)
    use_noise_image: every fit that ends with flags == 0 gets the noise-power
        sandwich covariance (Fitter(use_noise_image=True), fitters.py:108-109)
        from the noise images given to go(noise=...), computed on the device
        from the batch's own pars_cov0 (noise_cov.apply_noise_cov_device); not
        for coellip, as the reference's CoellipFitter has no such switch
    """

    def __init__(self, model, fit_pars=None, analytic_jacobian=True, prior=None,
                 device_prior=True, ngauss=None, use_noise_image=False):
        # host joint priors (joint_prior.py) are put in their batch form
        self.prior = as_batch_prior(prior)
        # evaluate a PriorSimpleSepBatch inside one kernel (False: torch ops)
        self.device_prior = device_prior
        self.ngauss = None
        if model == "coellip":
            # CoellipFitter (fitters.py:120-141): ngauss co-elliptical gaussians,
            # parameters cen1, cen2, g1, g2, T_1.., F_1.., one band, lmdif
            if ngauss is None or not 1 <= int(ngauss) <= (_lib.LM_NPMAX - 4) // 2:
                raise ValueError("coellip needs ngauss = 1..%d" % ((_lib.LM_NPMAX - 4) // 2))
            self.ngauss = int(ngauss)
            self.model = model
            self.nloc = 4 + 2 * self.ngauss
        elif model not in MODEL_NLOC:
            raise ValueError("LMBatchFitter supports %s and 'coellip'" % (tuple(MODEL_NLOC),))
        else:
            self.model = model
            self.nloc = MODEL_NLOC[model]
        self.fd = not (analytic_jacobian and model in SIMPLE_ANALYTIC_MODELS)
        self.fit_pars = dict(DEFAULT_LM_PARS if fit_pars is None else fit_pars)
        if use_noise_image and model == "coellip":
            raise ValueError("use_noise_image is not available for coellip")
        self.use_noise_image = bool(use_noise_image)
        self._event_pool = _EventPool()   # the timing events of time_kernels
        self._side_streams = {}           # (device, which) -> torch stream

    def go(self, stamps, guess, psf=None, stamp_obj=None, stamp_band=None,
           check_every=1, noise=None):
        """
        one batch, start to finish

        stamps: StampBatch -- every observation (epoch / band) of every object
        guess: (nobj, nshape + nband) starting parameters: the model's shape
            parameters ([cen1, cen2, g1, g2, T] for gauss/turb/exp/dev, plus
            fracdev for bdf, plus logTratio and fracdev for bd) followed by
            one flux per band
        psf: GMixBatch with one mixture per stamp, or None
        stamp_obj: (nstamps,) object index of each stamp, non-decreasing;
            None: stamp i is object i
        stamp_band: (nstamps,) band of each stamp; None: band 0
        check_every: (host-driven loop only) read the count of running fits
            every so many rounds
        noise: with use_noise_image, the stamps' noise images: a flat float64
            device tensor laid out like stamps.val, or one host array per stamp

        returns a dict of arrays indexed by object
        """
        d_noise = self._noise_images(stamps, noise)
        job = self._enqueue(stamps, guess, psf, stamp_obj, stamp_band, check_every, False)
        return self._apply_noise_cov(job, self._collect(job), d_noise)

    def _noise_images(self, stamps, noise):
        """the checked noise images of a batch (ValueError before any launch)"""
        if not self.use_noise_image:
            return None
        from .noise_cov import noise_flat
        return noise_flat(stamps, noise)

    def _apply_noise_cov(self, job, res, d_noise):
        """the sandwich covariance of the fits with flags == 0, from the
        solutions and pars_cov0 where the finalize kernel left them"""
        if d_noise is None:
            return res
        from .noise_cov import apply_noise_cov_device
        stamps, psf, sobj, sband, d_rec, _, n = job.fit_ctx
        c0 = 4 + 2 * n
        return apply_noise_cov_device(res, stamps, d_noise, self.model, psf=psf,
                                      stamp_obj=sobj, stamp_band=sband,
                                      pars=d_rec[:, 4:4 + n],
                                      pars_cov0=d_rec[:, c0:c0 + n * n])

    # host time of the last batch, by what the host was doing (milliseconds):
    # "enqueue" (set-up and queueing, _enqueue), "wait" (blocked on the batch's
    # downloads: the GPU is the bottleneck while this is > 0), "package"
    # (_collect after the wait) -- a pipeline keeps up as long as enqueue +
    # package stays below the GPU's time per batch
    host_ms = None
    # switches of the driver (tests, tools/, bench.py): the fit is the same to the bit
    time_phases = False     # wall clock per phase into phase_ms (True: synced; "nosync")
    time_kernels = False    # HIP events around every launch: kernel_ms, eval_launches
    stats_pass = False      # True: statistics by a loglike pass, not by the loop's sums
    precise_cov = True      # double-double covariance for fd fits of nloc >= 10
    host_loop = False       # True: the host-driven loop where the blind one would serve
    lazy_jacobian = True    # lmder without the jacobian in trials predicted to end a fit
    advance_hint = True     # False: the generic one-thread form of lm_advance
    keep_job = False        # True: the collected job stays in fitter.last_job
    round_hook = None       # hook(job, round) after every round of the host-driven loop
    nsplit = None           # pieces on separate streams (None: NGMIX_LM_NSPLIT, else 1)
    _rounds_hint = None     # rounds the next fit queues blind (the last fit's + 1)

    def go_stream(self, batches, check_every=1):
        """
        Fit a SEQUENCE of batches as a software pipeline: a generator of result
        dicts, one per batch, in order.  batches: an iterable of (stamps,
        guess, kwargs) with kwargs the keyword arguments of go() (psf=...,
        stamp_obj=..., stamp_band=..., noise=...).

        Everything a batch needs on the device -- set-up, the lock-step rounds,
        finalize, pack, the downloads -- is queued without the host waiting for
        anything (_enqueue), and batch i + 1 is queued before the host turns to
        batch i's arrays: the GPU always has a whole batch of work in front of
        it, whatever the host's pace.  That matters twice: the host phases of a
        call disappear behind kernels, and the GPU stays in the clock state it
        only reaches under uninterrupted load (the same lm_eval launch takes
        1.30 ms then, 1.42-1.45 ms when the GPU idles a millisecond between
        launches: tools/lm_eval_warm.py).  Every result is what go() returns
        for that batch, bit for bit.
        """
        prev = None
        for stamps, guess, kw in batches:
            d_noise = self._noise_images(stamps, kw.get("noise"))
            job = self._enqueue(stamps, guess, kw.get("psf"), kw.get("stamp_obj"),
                                kw.get("stamp_band"), check_every, True)
            if prev is not None:
                yield self._apply_noise_cov(prev[0], self._collect(prev[0]), prev[1])
            prev = (job, d_noise)
        if prev is not None:
            yield self._apply_noise_cov(prev[0], self._collect(prev[0]), prev[1])

    # the two halves of a fit: all the device needs, queued; then the host's half

    def _mark(self, job, name):
        # time_phases: wall clock per phase of this call, each phase closed by a
        # device synchronisation (which removes the overlap between phases)
        if job.phases is None:
            return
        if self.time_phases != "nosync":
            _torch().cuda.synchronize(job.dev)
        now = time.perf_counter()
        job.phases[name] = job.phases.get(name, 0.0) + (now - job.tmark) * 1e3
        job.tmark = now

    def _enqueue(self, stamps, guess, psf, stamp_obj, stamp_band, check_every, streaming):
        """set a batch up and queue its whole fit on the current stream; returns
        the job _collect() turns into the result dict"""
        job = _Job()
        job.dev = stamps.device
        # (the device context and the stream handle are looked up once per fit:
        # ~10 us each, a tenth of a one-object fit when done per launch)
        t0 = time.perf_counter()
        with _on_device(job.dev):
            job.stream = _stream()
            self._enqueue_on(job, stamps, guess, psf, stamp_obj, stamp_band,
                             check_every, streaming)
        job.host_enqueue_ms = (time.perf_counter() - t0) * 1e3
        return job

    def _enqueue_on(self, job, stamps, guess, psf, stamp_obj, stamp_band, check_every,
                    streaming):
        """the stages of a fit's set-up, each leaving its fields on the job,
        then the lock-step rounds and the results queued behind them"""
        torch = _torch()
        job.phases = {} if self.time_phases else None
        job.tmark = time.perf_counter()
        self.phase_ms = job.phases
        job.stamps, job.ns = stamps, stamps.n
        job.streaming, job.check_every = streaming, check_every
        (guess, job.sobj, job.sband, job.obj_start, job.trivial_map, job.npix_obj,
         job.nband) = _stamp_maps(stamps.n, stamps.npix_kept, guess, stamp_obj, stamp_band,
                                  self.nloc)
        job.nobj, job.npars = guess.shape
        job.psf = psf
        job.npsf, psf_host = _psf_records(psf, job.ns)
        # leastsq's convention: maxfev = 0 (or absent) means 100 (n + 1) function
        # calls with an analytic jacobian, 200 (n + 1) in forward-difference mode
        job.maxfev = int(self.fit_pars.get("maxfev", 0)) or \
            (200 if self.fd else 100) * (job.npars + 1)
        job.ev_init = self._timing_events(2)
        nsplit = int(self.nsplit if self.nsplit is not None
                     else (os.environ.get("NGMIX_LM_NSPLIT") or 1))   # (an A/B knob)
        job.nsum = self.nloc * (self.nloc + 1) // 2 + self.nloc + 1
        # the loglike statistics of set_fit_result ride with the analytic
        # kernel's sums (lnprob = -fnorm^2 / 2 has no prior term to add)
        job.loop_stats = not self.fd and self.prior is None and not self.stats_pass and \
            not os.environ.get("NGMIX_LM_JBASIS")
        self._alloc_buffers(job, nsplit)
        self._upload(job, guess, psf_host, nsplit)
        self._lm_init(job)
        if job.loop_stats and job.arena is None:
            job.d_ostats = torch.zeros((job.nobj, 2), dtype=torch.float64, device=job.dev)
        self._prior_record(job)
        # Forward-difference fits of ten and more local parameters (co-elliptical
        # psf fits with 3+ gaussians: cond(J) ~ 1e8 at the solution) take their
        # covariance from a double-double factorisation of the last jacobian's
        # normal equations (ngmix_lm_precise_cov_batch), at the point in d_jacpt
        job.d_jacpt = None
        if self.fd and self.nloc >= _lib.LM_PRECISE_MIN_NLOC and self.precise_cov and \
                not os.environ.get("NGMIX_LM_NO_PRECISE_COV") and self.prior is None:
            job.d_jacpt = torch.zeros((job.nobj, 3, _lib.LM_NPMAX), dtype=torch.float64,
                                      device=job.dev)
        torch_prior = self.prior is not None and job.prior_desc is None
        job.nsplit = 1 if torch_prior else max(1, min(int(nsplit), job.nobj))
        # the host-free loop serves one piece with no prior or the kernel prior; a
        # torch-evaluated prior sits between the two launches of a round, pieces on
        # several streams are interleaved by the host: the host-driven loop
        job.host_loop = (job.nsplit > 1 or torch_prior
                         or bool(os.environ.get("NGMIX_LM_HOST_LOOP"))
                         or bool(self.host_loop))
        job.batch = stamps._batch(1)
        self._mark(job, "setup")
        if job.host_loop:
            self._rounds_host_loop(job)
            self._queue_results(job)
            return
        # the whole fit, queued blind: rounds sized by the last batch's count, then
        # the results; _collect() finds out whether they were enough (the rare miss)
        hint = self._rounds_hint
        first = 4 if hint is None else max(1, min(int(hint), ROUNDS_HINT_CAP))
        self._queue_rounds(job, first)
        self._mark(job, "loop")
        self._queue_results(job)

    def _alloc_buffers(self, job, nsplit):
        """the buffer stage.  Reads nobj, ns, npars, nsum, loop_stats; leaves
        d_states, d_sums, d_status, d_sstats, d_flat, d_tri, d_rec: for a small
        batch (SMALL_BATCH) views of one allocation, job.arena holding the bytes of
        the outputs and their offsets; else separate tensors, arena None and the
        outputs (out_shapes) left to _finalize_and_pack.  d_ostats comes later."""
        torch = _torch()
        dev, nobj, ns, npars = job.dev, job.nobj, job.ns, job.npars
        shapes = [
            ("states", (nobj, _lib.LM_STATE_DTYPE.itemsize), torch.uint8),
            ("sums", (ns, job.nsum), torch.float64),
            ("status", (ns,), torch.int32),
            ("sstats", (ns, 2), torch.float64),
            # the three outputs, contiguous: one download
            ("flat", (nobj * (2 * npars + _lib.LM_NCOLS),), torch.float64),
            ("tri", (nobj, npars * (npars + 1) // 2), torch.float64),
            ("rec", (nobj, 4 + 2 * npars + 2 * npars * npars), torch.float64)]
        job.arena = job.d_ostats = job.d_flat = job.d_tri = job.d_rec = None
        job.out_shapes = [shape for _, shape, _ in shapes[4:]]
        if nobj <= SMALL_BATCH and ns <= 16 * SMALL_BATCH and nsplit <= 1 and \
                not os.environ.get("NGMIX_LM_NO_ARENA"):
            abuf, v, off = _carve(torch, dev, shapes)
            job.arena = {"out": abuf[off["flat"][0]:off["rec"][0] + off["rec"][1]],
                         "out_off": {k: off[k][0] - off["flat"][0]
                                     for k in ("flat", "tri", "rec")}}
            job.d_flat, job.d_tri, job.d_rec = v["flat"], v["tri"], v["rec"]
        else:
            # (every row is written by the first round's launch)
            v = {name: torch.empty(shape, dtype=dt, device=dev)
                 for name, shape, dt in (shapes[:4] if job.loop_stats else shapes[:3])}
        job.d_states, job.d_sums, job.d_status = v["states"], v["sums"], v["status"]
        job.d_sstats = v["sstats"] if job.loop_stats else None

    def _upload(self, job, guess, psf_host, nsplit):
        """the upload stage: ONE host-to-device copy (~30 us whatever its size)
        of the guess, the pixel counts, the arena form's zeroed d_ostats, host psf
        records and, unless stamp i is object i, the maps.  Leaves h_all, d_all and
        its views d_guess, d_npix, d_ostats, psf, d_sobj, d_sband, d_start."""
        torch = _torch()
        nobj, ns = job.nobj, job.ns
        # 8-byte aligned pieces of one buffer, viewed in their own types
        u8 = lambda a: a.view(np.uint8).reshape(-1)
        pieces = [("guess", u8(guess)), ("npix", u8(job.npix_obj))]
        if job.arena is not None and job.loop_stats:
            pieces.append(("ostats", np.zeros(16 * nobj, dtype=np.uint8)))
        if psf_host is not None:
            pieces.append(("psf", u8(psf_host)))
        if not job.trivial_map:
            pad = np.zeros((ns + 1) // 2 * 2 - ns, dtype=np.int32)
            pieces += [("start", u8(job.obj_start)),
                       ("sobj", u8(np.concatenate([job.sobj, pad]))),
                       ("sband", u8(np.concatenate([job.sband, pad])))]
        # (through pinned memory: a copy from pageable memory makes torch
        # synchronise the stream, i.e. wait for the previous batch of a pipeline)
        nbytes = sum(a.size for _, a in pieces)
        job.h_all = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        np.concatenate([a for _, a in pieces], out=job.h_all.numpy())
        job.d_all = job.h_all.to(job.dev, non_blocking=True)
        view, at = {}, 0
        for name, a in pieces:
            view[name] = job.d_all[at:at + a.size]
            at += a.size
        job.d_guess = view["guess"].view(torch.float64).reshape(nobj, job.npars)
        job.d_npix = view["npix"].view(torch.int64)
        if "ostats" in view:
            job.d_ostats = view["ostats"].view(torch.float64).reshape(nobj, 2)
        if psf_host is not None:
            job.psf = GMixBatch(view["psf"].view(torch.float64).reshape(-1, 13), ns, job.npsf)
        job.d_sobj = job.d_sband = job.d_start = None
        if not job.trivial_map:
            job.d_start = view["start"].view(torch.int64)
            job.d_sobj = view["sobj"].view(torch.int32)[:ns]
            job.d_sband = view["sband"].view(torch.int32)[:ns]
        elif nsplit > 1:
            # stamp i is object i in band 0: the kernels take NULL for the three
            # maps (as pieces on several streams they need the absolute indices)
            job.d_sobj = torch.arange(ns, dtype=torch.int32, device=job.dev)
            job.d_sband = torch.zeros(ns, dtype=torch.int32, device=job.dev)
            job.d_start = torch.arange(nobj + 1, dtype=torch.int64, device=job.dev)

    def _lm_init(self, job):
        """the state records at the guess (ngmix_lm_init_batch), with the
        prior's bounds.  Reads d_states, d_guess, maxfev, ev_init; leaves modnum."""
        fp, lo, hi = self.fit_pars, None, None
        if self.prior is not None and getattr(self.prior, "bounds", None) is not None:
            lo, hi = bounds_arrays(self.prior.bounds, job.npars)
        _record(job.ev_init, 0, job.stream)
        _lib.check(_lib.lib().ngmix_lm_init_batch(
            _dptr(job.d_states), job.nobj, job.npars, _dptr(job.d_guess),
            float(fp.get("ftol", 1.49012e-8)), float(fp.get("xtol", 1.49012e-8)),
            float(fp.get("gtol", 0.0)), job.maxfev, float(fp.get("factor", 100.0)),
            self._lm_mode(),
            _lib.ptr(lo) if lo is not None else None,
            _lib.ptr(hi) if hi is not None else None, job.stream),
            "ngmix_lm_init_batch")
        _record(job.ev_init, 1, job.stream)
        job.modnum = get_model_num(self.model)
        if self.ngauss is not None:
            job.modnum += 256 * self.ngauss   # the count rides with the model id
            if job.nband != 1:
                raise ValueError("coellip fits one band: guess needs %d columns" % self.nloc)

    def _prior_record(self, job):
        """the prior stage: the record ngmix_lm_prior_sums_batch evaluates,
        checked against the fit's layout.  Reads npars, nband; leaves prior_desc,
        d_osums (None for a torch-evaluated prior or none), fitter.prior_path."""
        nshape = self.nloc - 1
        desc = None
        if self.prior is not None and self.device_prior and hasattr(self.prior, "descriptor"):
            desc = self.prior.descriptor()
            if desc is not None and nshape != 5 + int(desc["nmid"][0]):
                raise ValueError("the prior is laid out for %d parameters before the fluxes, "
                                 "model '%s' has %d" % (5 + int(desc["nmid"][0]),
                                                        self.model, nshape))
            if desc is not None and int(desc["nband"][0]) != job.nband:
                raise ValueError("the prior has %d flux terms, the guess %d bands"
                                 % (int(desc["nband"][0]), job.nband))
        job.prior_desc, job.d_osums = desc, None
        if desc is not None:
            n = job.npars
            job.d_osums = _torch().zeros((job.nobj, n * (n + 1) // 2 + n + 1),
                                         dtype=_torch().float64, device=job.dev)
        self.prior_path = ("kernel" if desc is not None else
                           "torch" if self.prior is not None else None)

    @staticmethod
    def _job_stream(job):
        """the stream a job was queued on (job.stream, a raw handle) as a torch
        stream, for the rare paths that queue torch work behind it again"""
        torch = _torch()
        handle = job.stream.value or 0
        if handle == 0:
            return torch.cuda.default_stream(job.dev)
        return torch.cuda.ExternalStream(handle, device=job.dev)

    def _lm_mode(self):
        """ngmix_lm_state.mode of this fitter's fits: lmdif, or lmder with the
        jacobian left out of the trials predicted to end the fit (lazy_jacobian
        off: with every evaluation; the same iterates to the bit either way)"""
        if self.fd:
            return _lib.LM_MODE_FD
        lazy = self.lazy_jacobian and \
            not os.environ.get("NGMIX_LM_EAGER_JAC") and \
            not os.environ.get("NGMIX_LM_JBASIS")
        return _lib.LM_MODE_ANALYTIC_LAZY if lazy else _lib.LM_MODE_ANALYTIC

    def _problem(self, job):
        """the ngmix_lm_problem record of a job, made once and kept alive with it"""
        if job.problem is not None:
            return job.problem
        P = job.problem = _lib.LMProblem()
        P.batch = ctypes.pointer(job.batch)
        P.states = job.d_states.data_ptr()
        P.nobj = job.nobj
        opt = lambda t: t.data_ptr() if t is not None else None
        P.stamp_obj = opt(job.d_sobj)
        P.stamp_band = opt(job.d_sband)
        P.obj_start = opt(job.d_start)
        P.psf = job.psf.data.data_ptr() if job.psf is not None else None
        P.sums = job.d_sums.data_ptr()
        P.status = job.d_status.data_ptr()
        P.stamp_stats = opt(job.d_sstats)
        P.obj_stats = opt(job.d_ostats)
        if job.prior_desc is not None:
            P.prior = job.prior_desc.ctypes.data
            P.obj_sums = job.d_osums.data_ptr()
        P.prior_step = STEP_PRIOR
        P.model = job.modnum
        P.fd = int(self.fd)
        P.npsf = job.npsf
        P.nloc_npars = self._nloc_npars(job.npars)
        P.jac_point = opt(job.d_jacpt)
        return P

    def _nloc_npars(self, npars):
        """the nloc argument of ngmix_lm_advance_batch carrying the fits'
        parameter count (nloc + 256 npars), which selects the step's kernel: the
        register form for 6-8 parameters, the team form for 9-14, the generic
        one-thread form (what the tests compare the two with) without the hint"""
        hint = npars if self.advance_hint else _lib.LM_NPARS_GENERIC
        return self.nloc + 256 * hint

    def _timing_events(self, n):
        """n hipEvent_t handles of the fitter's pool under time_kernels, else None"""
        return self._event_pool.take(n) if self.time_kernels else None

    def _queue_rounds(self, job, nrounds):
        """nrounds lock-step rounds by one call into the library
        (ngmix_lm_rounds_batch): no host between the launches"""
        torch = _torch()
        d_counts = torch.empty(nrounds, dtype=torch.int32, device=job.dev)
        h_counts = torch.empty(nrounds, dtype=torch.int32, pin_memory=True)
        ev = self._timing_events(3 * nrounds)
        span = _HipEvents(2)
        # (the caller holds the device context; the copy of the counts is
        # queued by the library on the same stream)
        _record(span.handles, 0, job.stream)
        _lib.check(_lib.lib().ngmix_lm_rounds_batch(
            ctypes.byref(self._problem(job)), nrounds, _dptr(d_counts),
            ctypes.c_void_p(h_counts.data_ptr()), ev, job.stream),
            "ngmix_lm_rounds_batch")
        _record(span.handles, 1, job.stream)
        job.chunks.append(_Chunk(nrounds, d_counts, h_counts, ev, span))

    def _rounds_done(self, job):
        """after the last queued chunk has run: the count of fits still running"""
        return int(job.chunks[-1].h_counts[-1])

    def _collect(self, job):
        """the host's half: wait for the downloads, make sure the rounds queued
        blind were enough (else run more and re-make the results), package"""
        t0 = time.perf_counter()
        job.copied.synchronize()
        t1 = time.perf_counter()
        if not job.host_loop:
            torch, grow, redo = _torch(), 2, False
            total = sum(c.nrounds for c in job.chunks)
            while self._rounds_done(job) != 0:
                if total > 2 * job.maxfev + 5:
                    raise RuntimeError("batched LM did not terminate")
                redo = True
                # (on the fit's OWN stream, whatever stream the consumer of
                # go_stream() iterates under, and waited for through the event the
                # chunk records there: the counts read next are this chunk's)
                with torch.cuda.device(job.dev), torch.cuda.stream(self._job_stream(job)):
                    self._queue_rounds(job, grow)
                _lib.check(_lib.lib().ngmix_event_synchronize(job.chunks[-1].span.handles[1]),
                           "ngmix_event_synchronize")
                total += grow
                grow = min(2 * grow, ROUNDS_HINT_CAP)
            if redo:
                with torch.cuda.device(job.dev), torch.cuda.stream(self._job_stream(job)):
                    self._queue_results(job)
                job.copied.synchronize()
            # counts after each round -> the rounds that had fits to advance
            counts = np.concatenate([c.h_counts.numpy() for c in job.chunks])
            before = np.concatenate([[job.nobj], counts[:-1]])
            job.useful_rounds = int((before > 0).sum())
            self.rounds_launched = int(counts.size)
            self._rounds_hint = job.useful_rounds + 1
            # the device time of the rounds (events around every chunk)
            self.loop_seconds = sum(_elapsed_ms(*c.span.handles) for c in job.chunks) * 1e-3
            if job.chunks[0].events is not None:
                self._kernel_times(job, before)
        else:
            self.loop_seconds = job.loop_ms_host * 1e-3
            self.rounds_launched = job.useful_rounds
            if job.legacy_ev is not None:
                self._kernel_times_host_loop(job)
        self.rounds = job.useful_rounds
        self.nsplit_used = job.nsplit
        self._d_states = job.d_states
        if self.keep_job:
            self.last_job = job   # (tests: the device buffers of the batch)
        # (fitter.gmix belongs to the batch whose result is being returned)
        self._fit_ctx = job.fit_ctx
        self._gmix = None
        self._mark(job, "download")
        res = self._package(job)
        self._mark(job, "package")
        self.host_ms = {"enqueue": job.host_enqueue_ms, "wait": (t1 - t0) * 1e3,
                        "package": (time.perf_counter() - t1) * 1e3}
        return res

    def _kernel_times(self, job, before):
        """HIP-event times of every launch of the rounds (time_kernels)"""
        elapsed = lambda a, b: _elapsed_ms(a, b, "elapsed")
        rounds = [(c.events, 3 * r) for c in job.chunks for r in range(c.nrounds)]
        ev_ms = [elapsed(e[i], e[i + 1]) for e, i in rounds]
        adv_ms = [elapsed(e[i + 1], e[i + 2]) for e, i in rounds]
        w = before.astype("f8") * (job.ns / float(job.nobj))
        # (the launches that found every fit finished are left out of the mean)
        self._eval_times(ev_ms, w, before > 0)
        self.advance_ms_total = float(np.sum(adv_ms))
        self.kernel_ms = {
            "lm_eval": float(np.sum(ev_ms)), "lm_advance": float(np.sum(adv_ms)),
            "lm_init": elapsed(job.ev_init[0], job.ev_init[1]),
            "lm_finalize": elapsed(job.ev_post[0], job.ev_post[1]),
            "lm_pack": elapsed(job.ev_post[1], job.ev_post[2]),
        }
        self._event_pool.give(job.ev_init)
        self._event_pool.give(job.ev_post)
        for c in job.chunks:
            self._event_pool.give(c.events)

    def _kernel_times_host_loop(self, job):
        ev = job.legacy_ev
        # (a launch whose count was never read -- check_every > 1 -- keeps the
        # last count known before it)
        last = 0.0
        for rec_ in ev:
            if rec_[2] is None:
                rec_[2] = last
            last = rec_[2]
        self._eval_times([a.elapsed_time(b) for a, b, _ in ev], [w for _, _, w in ev],
                         np.ones(len(ev), dtype=bool))

    def _eval_times(self, ms, w, live):
        """per-launch mean over the live launches, and the whole fit: stamps
        evaluated / time spent"""
        self.eval_ms = float(np.mean(np.asarray(ms)[live]))
        self.eval_ms_total = float(np.sum(ms))
        self.eval_stamps_total = float(np.sum(w))
        self.eval_launches = [(float(t), float(x)) for t, x in zip(ms, w)]
        self.eval_launch_count = int(live.sum())

    def _pieces(self, job):
        """the batch cut into job.nsplit runs of whole objects, each with its own
        ngmix_batch record, counter and side stream (no gain measured: DESIGN 3.7)"""
        torch = _torch()
        b, nobj, nsplit = job.batch, job.nobj, job.nsplit
        pieces = []
        for k in range(nsplit):
            p = _Piece()
            p.o_lo, p.o_hi = nobj * k // nsplit, nobj * (k + 1) // nsplit
            p.s_lo, p.s_hi = int(job.obj_start[p.o_lo]), int(job.obj_start[p.o_hi])
            p.batch = _lib.Batch()
            ctypes.memmove(ctypes.byref(p.batch), ctypes.byref(b), ctypes.sizeof(p.batch))
            p.batch.nstamps = p.s_hi - p.s_lo
            p.batch.stamps = b.stamps + p.s_lo * _lib.STAMP_DTYPE.itemsize
            p.batch.jac = b.jac + p.s_lo * _lib.JACOBIAN_DTYPE.itemsize
            # (val, ierr and the mixtures keep their bases: pix_off and gm_off of a
            # piece's table are not i * npix, i * ngauss -- the piece is not regular)
            p.batch.flags &= ~(_lib.BATCH_REGULAR | _lib.BATCH_REGULAR_STAMP_FLAGS)
            p.stream = self._side_stream(job.dev, 1 + k) if nsplit > 1 else None
            p.nact = torch.zeros(1, dtype=torch.int32, device=job.dev)
            p.live, p.active = True, p.o_hi - p.o_lo
            p.ring = [torch.zeros(1, dtype=torch.int32, pin_memory=True) for _ in range(3)]
            p.pend, p.launched, p.ev_idx = [], 0, []
            pieces.append(p)
        return pieces

    def _rounds_host_loop(self, job):
        """the lock-step loop driven from the host, one round at a time (a prior
        evaluated by torch ops between the two launches of a round; pieces of
        the batch on several streams, fitter.nsplit)"""
        torch = _torch()
        dev = job.dev
        pieces = self._pieces(job)
        rounds = 0
        if not job.streaming:
            torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        # time_kernels: HIP events around every pixel-pass launch (bench.py),
        # with the number of stamps each launch still had to evaluate
        ev = job.legacy_ev = [] if self.time_kernels else None
        nstamp_obj = job.ns / float(job.nobj)
        with torch.cuda.device(dev):
            main = torch.cuda.current_stream(dev)
            if job.nsplit > 1:
                start = torch.cuda.Event()
                start.record(main)
                for p in pieces:
                    p.stream.wait_event(start)
            # One round is kept in flight AHEAD of the count being read (a 4-byte
            # pinned copy behind each round): the GPU never waits for the host, and
            # the last round finds every fit finished and returns at once (~30 us)
            depth = 1 if job.check_every == 1 else 0
            while any(p.live for p in pieces):
                for p in pieces:
                    if not p.live:
                        continue
                    with torch.cuda.stream(p.stream or main):
                        if len(p.pend) > depth and (
                                p.launched % job.check_every == 0 or
                                p.launched > 2 * job.maxfev):
                            while len(p.pend) > depth:
                                done, h = p.pend.pop(0)
                            done.synchronize()
                            p.active = int(h[0])
                            # (that count is what the launch after it evaluates)
                            k = p.launched - len(p.pend)
                            if ev is not None and k < len(p.ev_idx):
                                ev[p.ev_idx[k]][2] = p.active * nstamp_obj
                            if p.active == 0:
                                p.live = False
                                continue
                        self._enqueue_round(job, p)
                rounds += 1
                if rounds > 2 * job.maxfev + 5:
                    raise RuntimeError("batched LM did not terminate")
            # rounds that had fits to advance (not the one in flight at the end)
            rounds = max(p.launched - len(p.pend) for p in pieces)
            if job.nsplit > 1:
                for p in pieces:
                    main.wait_stream(p.stream)
        if not job.streaming:
            torch.cuda.synchronize(dev)
        # seconds in the lock-step loop (kernels + one 4-byte readback per round)
        job.loop_ms_host = (time.perf_counter() - t0) * 1e3
        job.useful_rounds = rounds
        self._mark(job, "loop")

    def _enqueue_round(self, job, p):
        """one round of piece p on the current stream: pixel pass, prior rows,
        step, and the count of running fits on its way to the host behind them"""
        torch = _torch()
        L = _lib.lib()
        n, psf, ev = job.npars, job.psf, job.legacy_ev
        d_states = job.d_states
        isz = _lib.LM_STATE_DTYPE.itemsize
        wosum = n * (n + 1) // 2 + n + 1
        if ev is not None:
            # (the stamps this launch still has to evaluate are known when
            # the previous round's counter is read: filled in then)
            ev.append([torch.cuda.Event(enable_timing=True),
                       torch.cuda.Event(enable_timing=True),
                       p.active * (job.ns / float(job.nobj)) if not p.launched else None])
            p.ev_idx.append(len(ev) - 1)
            ev[-1][0].record()
        _lib.check(L.ngmix_lm_eval_batch(
            ctypes.byref(p.batch), job.modnum, int(self.fd), _dptr(d_states),
            _off(job.d_sobj, 4 * p.s_lo), _off(job.d_sband, 4 * p.s_lo),
            _off(psf.data, 104 * job.npsf * p.s_lo) if psf is not None else None,
            job.npsf, _off(job.d_sums, 8 * job.nsum * p.s_lo), _off(job.d_status, 4 * p.s_lo),
            _off(job.d_sstats, 16 * p.s_lo), _stream()),
            "ngmix_lm_eval_batch")
        if ev is not None:
            ev[-1][1].record()
        osums = None
        if job.prior_desc is not None:
            # the prior rows at the same trial points (results.py:454)
            _lib.check(L.ngmix_lm_prior_sums_batch(
                _off(d_states, isz * p.o_lo), p.o_hi - p.o_lo, _lib.ptr(job.prior_desc),
                STEP_PRIOR, _off(job.d_osums, 8 * wosum * p.o_lo), _stream()),
                "ngmix_lm_prior_sums_batch")
            osums = job.d_osums
        elif self.prior is not None:
            steps = [_state_cols(d_states, c, n) for c in ("xstep", "hstep")] if self.fd else []
            osums = prior_normal_sums(self.prior, _state_cols(d_states, "xt", n), *steps)[0]
        # obj_start holds absolute stamp indices: sums / stamp_band stay whole
        _lib.check(L.ngmix_lm_advance_batch(
            _off(d_states, isz * p.o_lo), p.o_hi - p.o_lo, _off(job.d_start, 8 * p.o_lo),
            _dptr(job.d_sband), _dptr(job.d_sums), self._nloc_npars(n),
            _off(osums, 8 * wosum * p.o_lo), _dptr(p.nact),
            _dptr(job.d_sstats) if job.loop_stats else None,
            _off(job.d_ostats, 16 * p.o_lo), _stream()),
            "ngmix_lm_advance_batch")
        if self.round_hook is not None:
            # (tests: the state records after every round of the host loop)
            self.round_hook(job, p.launched)
        # the count of fits still running follows the round that made it
        h = p.ring[p.launched % len(p.ring)]
        h.copy_(p.nact, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        p.pend.append((done, h))
        p.launched += 1

    def _queue_results(self, job):
        """run_leastsq's packaging, one thread per fit (ngmix_lm_finalize_batch),
        the statistics / packing kernel and the downloads, all queued.  Leaves
        h_flat, h_tri, h_cov0 (pinned) and the events copied, cov_copied."""
        d_ffx = self._prior_ffx(job) if self.prior is not None else None
        ev_post = self._finalize_and_pack(job, d_ffx)
        side = self._side_stream(job.dev)   # (made with a fitter's first fit of any size)
        job.h_flat, job.h_tri, job.h_cov0, job.copied, job.cov_copied = \
            self._download_arena(job) if job.arena is not None else self._download_side(job, side)
        self._event_pool.give(job.ev_post)   # (results re-made after a miss)
        job.ev_post = ev_post
        self._mark(job, "enqueue_copy")

    def _prior_ffx(self, job):
        """the part of |f|^2 at the solutions that chi2/dof leaves out, per object
        (leaves d_prior_lnp when the kernel prior ran): the prior rows
        (leastsqbound.py:97) and, the reference reserving more slots than
        PriorSimpleSep fills (results.py:1050-1078, 454-461), the first pixels"""
        torch = _torch()
        nobj, dev = job.nobj, job.dev
        x = _state_cols(job.d_states, "x", job.npars)
        if job.prior_desc is not None:
            # one launch at the fits' points (the record the prior kernel
            # evaluated during the rounds)
            d_ffx = torch.empty(nobj, dtype=torch.float64, device=dev)
            job.d_prior_lnp = torch.empty(nobj, dtype=torch.float64, device=dev)
            _lib.check(_lib.lib().ngmix_lm_prior_finish_batch(
                _dptr(job.d_states), nobj, _lib.ptr(job.prior_desc), _dptr(d_ffx),
                _dptr(job.d_prior_lnp), job.stream), "ngmix_lm_prior_finish_batch")
            nrows = 4 + int(job.prior_desc["nmid"][0]) + int(job.prior_desc["nband"][0])
        else:
            rows, bad = self.prior.fill_fdiff_batch(x)
            d_ffx = torch.where(bad, torch.zeros_like(rows[:, 0]), (rows * rows).sum(dim=1))
            d_ffx = torch.where(torch.isfinite(d_ffx), d_ffx, torch.zeros_like(d_ffx))
            nrows = rows.shape[1]
        nskip = get_lm_n_prior_pars(self.model, job.nband) - nrows
        if nskip > 0:
            d_ffx = d_ffx + self._first_pixels_fdiff2(
                job.stamps, job.psf, x, job.obj_start, job.sband, nskip)
        return d_ffx.contiguous()

    def _finalize_and_pack(self, job, d_ffx):
        """the precise covariance where it applies, ngmix_lm_finalize_batch, the
        statistics where the loop did not carry them, ngmix_lm_pack_batch.
        Leaves d_cov0, fit_ctx (d_psums); returns the timing events."""
        torch = _torch()
        L = _lib.lib()
        dev, nobj, n = job.dev, job.nobj, job.npars
        d_states, d_npix = job.d_states, job.d_npix
        if job.arena is None:
            # (here, not in _alloc_buffers: a miss re-makes the results into fresh
            # buffers while the side stream may still be reading the first ones)
            job.d_flat, job.d_tri, job.d_rec = (
                torch.empty(shape, dtype=torch.float64, device=dev) for shape in job.out_shapes)
        d_rec, d_flat = job.d_rec, job.d_flat
        ev_post = self._timing_events(3)
        if job.d_jacpt is not None and not job.host_loop:
            # R / ipvt of the fits that ended, re-made from double-double normal
            # equations at the point of their last jacobian
            job.d_psums = torch.empty((job.ns, 2, job.nsum), dtype=torch.float64, device=dev)
            _lib.check(L.ngmix_lm_precise_cov_batch(
                ctypes.byref(self._problem(job)), _dptr(job.d_psums), job.stream),
                "ngmix_lm_precise_cov_batch")
        _record(ev_post, 0, job.stream)
        _lib.check(L.ngmix_lm_finalize_batch(
            _dptr(d_states), nobj, _dptr(d_npix), _dptr(d_ffx), float(PDEF), float(CDEF),
            _dptr(d_rec), job.stream), "ngmix_lm_finalize_batch")
        _record(ev_post, 1, job.stream)
        self._mark(job, "finalize")
        # pars_cov0 stays on the device until it is asked for
        job.d_cov0 = d_rec[:, 4 + 2 * n:4 + 2 * n + n * n]
        d_ok = d_rec[:, 0] == 0.0
        job.fit_ctx = self._fit_ctx = (job.stamps, job.psf, job.sobj, job.sband, d_rec, d_ok, n)
        self._gmix = None
        tot = None
        if not job.loop_stats:
            tot = self._loglike_at_solutions(
                job.stamps, job.psf, job.sobj, job.sband, job.obj_start,
                prior_lnp=job.d_prior_lnp).contiguous()
        # pars | pars_err rows, then twelve contiguous columns (integers and
        # statistics): one kernel, one download, contiguous host views
        _lib.check(L.ngmix_lm_pack_batch(
            _dptr(d_states), nobj, n, _dptr(d_rec),
            _dptr(job.d_ostats) if job.loop_stats else None,
            _dptr(tot), _dptr(d_npix), _dptr(d_flat),
            ctypes.c_void_p(d_flat.data_ptr() + 8 * nobj * 2 * n), _dptr(job.d_tri),
            job.stream),
            "ngmix_lm_pack_batch")
        _record(ev_post, 2, job.stream)
        self._mark(job, "pack")
        return ev_post

    def _download_arena(self, job):
        """one download of the arena's three outputs on the fit's own stream (the
        host waits for all of it); h_flat, h_tri, h_cov0, copied, cov_copied"""
        torch = _torch()
        n = job.npars
        d_out, oo = job.arena["out"], job.arena["out_off"]
        h_out = torch.empty(d_out.shape, dtype=torch.uint8, pin_memory=True)
        h_out.copy_(d_out, non_blocking=True)
        copied = torch.cuda.Event()
        copied.record()

        def hview(name, like):
            nb = like.numel() * 8
            return h_out[oo[name]:oo[name] + nb].view(torch.float64).reshape(like.shape)
        h_cov0 = hview("rec", job.d_rec)[:, 4 + 2 * n:4 + 2 * n + n * n]
        return hview("flat", job.d_flat), hview("tri", job.d_tri), h_cov0, copied, copied

    def _download_side(self, job, side):
        """two downloads through pinned memory on the side stream: the head (pars,
        pars_err, twelve columns), which go() waits for (copied), and the triangle
        of pars_cov, waited for -- and mirrored -- when pars_cov is first read
        (cov_copied); returns h_flat, h_tri, h_cov0, copied, cov_copied"""
        torch = _torch()
        nobj, n = job.nobj, job.npars
        d_flat, d_tri = job.d_flat, job.d_tri
        h_flat = torch.empty(d_flat.shape, dtype=torch.float64, pin_memory=True)
        h_tri = torch.empty(d_tri.shape, dtype=torch.float64, pin_memory=True)
        self._mark(job, "pinned_alloc")
        ready = torch.cuda.Event()
        ready.record()
        with torch.cuda.stream(side):
            side.wait_event(ready)
            h_flat.copy_(d_flat, non_blocking=True)
            copied = torch.cuda.Event()
            copied.record()
            h_tri.copy_(d_tri, non_blocking=True)
            h_cov0 = None
            if nobj <= 4096:
                # (a small batch: pars_cov0 rides along instead of costing its
                # first reader a synchronous download of its own)
                h_cov0 = torch.empty((nobj, n * n), dtype=torch.float64, pin_memory=True)
                h_cov0.copy_(job.d_cov0, non_blocking=True)
            cov_copied = torch.cuda.Event()
            cov_copied.record()
        d_flat.record_stream(side)
        d_tri.record_stream(side)
        return h_flat, h_tri, h_cov0, copied, cov_copied

    def _package(self, job):
        """the result dict over the downloaded block (views, no copies)"""
        nobj, n = job.nobj, job.npars
        ncols = _lib.LM_NCOLS
        flat = job.h_flat.numpy()
        rec = flat[:nobj * 2 * n].reshape(nobj, 2 * n)
        cols = flat[nobj * 2 * n:].reshape(ncols, nobj)
        res = LMBatchResult({
            "model": self.model,
            "flags": cols[0].astype(np.int64),
            "nfev": cols[1].astype(np.int64),
            "njev": cols[4].astype(np.int64),
            "ier": cols[2].astype(np.int64),
            # views of the downloaded block (no copies)
            "pars": rec[:, 0:n],
            "pars_err": rec[:, n:2 * n],
            "npix": job.npix_obj,
            "dof": cols[3].astype(np.int64),
        })
        h_tri, cov_copied, d_cov0 = job.h_tri, job.cov_copied, job.d_cov0

        def fetch_cov(_):
            cov_copied.synchronize()
            iu = np.triu_indices(n)
            a = np.empty((nobj, n, n))
            tri = h_tri.numpy()
            a[:, iu[0], iu[1]] = tri
            a[:, iu[1], iu[0]] = tri
            a.flags.writeable = False
            return a
        res.set_lazy("pars_cov", fetch_cov)
        h_cov0 = job.h_cov0

        def fetch_cov0(_):
            if h_cov0 is None:
                return d_cov0.cpu().numpy().reshape(nobj, n, n)
            cov_copied.synchronize()
            return h_cov0.numpy().reshape(nobj, n, n)
        res.set_lazy("pars_cov0", fetch_cov0)
        self._add_stats(res, cols[5:], job.nband)
        return res

    @property
    def gmix(self):
        """the fitted (pre-psf) mixtures of the last go(), one per stamp"""
        if self._gmix is None:
            self._fitted_mixtures()
        return self._gmix

    def _side_stream(self, dev, which=0):
        torch = _torch()
        cache = self._side_streams
        key = (dev.type, dev.index, which)
        if key not in cache:
            cache[key] = torch.cuda.Stream(device=dev)
        return cache[key]

    def _first_pixels_fdiff2(self, stamps, psf, x, obj_start, sband, nskip):
        """sum of fdiff^2 over the first nskip listed pixels of each object's
        first stamp at the parameters x (device tensor (nobj, npars)): the rows
        the reference's chi2/dof leaves out next to the prior's (see go())"""
        torch = _torch()
        dev = stamps.device
        nobj = x.shape[0]
        nshape = self.nloc - 1
        s0 = obj_start[:-1]
        band_pars = torch.empty((nobj, self.nloc), dtype=torch.float64, device=dev)
        band_pars[:, :nshape] = x[:, :nshape]
        idx = torch.from_numpy(nshape + sband[s0].astype(np.int64)).to(dev)
        band_pars[:, nshape] = x.gather(1, idx[:, None])[:, 0]
        gm, _ = GMixBatch.from_pars(band_pars, self.model, device=dev, ngauss=self.ngauss)
        d_s0 = torch.from_numpy(s0).to(dev)
        if psf is not None:
            pdata = psf.data.reshape(stamps.n, psf.ngauss, 13)[d_s0]
            gm, _ = gm.convolve(GMixBatch(pdata.reshape(-1, 13).contiguous(), nobj,
                                          psf.ngauss))
        gm.set_norms()
        # one launch: the first nskip listed pixels of each object's first
        # stamp through fill_fdiff's own arithmetic
        out = torch.empty(nobj, dtype=torch.float64, device=dev)
        b = stamps._batch(1)
        with _on_device(dev):
            st = _lib.lib().ngmix_first_pixels_fdiff2_batch(
                ctypes.byref(b), _dptr(d_s0), _dptr(gm.data), gm.ngauss, nobj, int(nskip),
                _dptr(out), _stream())
        _lib.check(st, "ngmix_first_pixels_fdiff2_batch")
        return out

    def states(self):
        """the raw ngmix_lm_state records of the last go() (debugging)"""
        return self._d_states.cpu().numpy().reshape(-1).view(_lib.LM_STATE_DTYPE)

    def _fitted_mixtures(self):
        """the mixtures at the solutions of the last go(): (pre-psf, convolved),
        one per stamp; a harmless model stands in for failed fits (their
        statistics are not reported)"""
        torch = _torch()
        stamps, psf, sobj, sband, d_rec, d_ok, n = self._fit_ctx
        dev = stamps.device
        nobj = d_rec.shape[0]
        nshape = self.nloc - 1
        default = np.zeros(n)
        default[4] = 1.0
        if self.model == "bdf":
            default[5] = 0.5
        if self.model == "bd":
            default[6] = 0.5
        default[nshape:] = 1.0
        if self.model == "coellip":
            default[4:] = 1.0
        usable = torch.where(d_ok[:, None], d_rec[:, 4:4 + n],
                             torch.from_numpy(default).to(dev)[None, :])
        if stamps.n == nobj and np.all(sband == 0):
            band_pars = usable[:, :self.nloc].contiguous()
        else:
            d_sobj = torch.from_numpy(sobj.astype(np.int64)).to(dev)
            d_sband = torch.from_numpy(sband.astype(np.int64)).to(dev)
            band_pars = torch.empty((stamps.n, self.nloc), dtype=torch.float64,
                                    device=dev)
            per_stamp = usable[d_sobj]
            band_pars[:, :nshape] = per_stamp[:, :nshape]
            band_pars[:, nshape] = per_stamp.gather(1, (nshape + d_sband)[:, None])[:, 0]
        gm0, st0 = GMixBatch.from_pars(band_pars, self.model, device=dev,
                                       ngauss=self.ngauss)
        gm = gm0
        if psf is not None:
            gm, _ = gm0.convolve(psf)
        self._gmix = gm0
        return gm, usable

    def _loglike_at_solutions(self, stamps, psf, sobj, sband, obj_start, prior_lnp=None):
        """the device half of FitModel.set_fit_result (results.py:45-72,
        398-408) when the lock-step loop did not carry the statistics
        (forward-difference fits, fits with a prior): one batched get_loglike
        at the solutions, folded per object on the device; (nobj, 4) lnprob,
        s2n_numer, s2n_denom, npix"""
        torch = _torch()
        dev = stamps.device
        gm, usable = self._fitted_mixtures()
        nobj = usable.shape[0]
        out, st1 = stamps.loglike(gm)
        if stamps.n == nobj:
            tot = out
        else:
            # (stamps of an object are contiguous: a fixed-order segmented sum)
            lengths = torch.from_numpy(np.diff(obj_start)).to(dev)
            tot = torch.segment_reduce(out, "sum", lengths=lengths, axis=0)
        if self.prior is not None:
            # calc_lnprob adds the joint prior (results.py:410-437)
            tot = tot.clone()
            if prior_lnp is not None:
                tot[:, 0] += prior_lnp
            else:
                tot[:, 0] += self.prior.get_lnprob_batch(usable.contiguous())
        return tot

    def _add_stats(self, res, out, nband):
        """the host half: the keys FitModel.set_fit_result adds for fits with
        flags == 0 (NaN elsewhere); out: the seven statistics columns of
        ngmix_lm_pack_batch (contiguous rows); g / T / flux blocks are VIEWS
        of the downloaded arrays"""
        pars = res["pars"]
        nshape = self.nloc - 1
        res["lnprob"] = out[0]
        res["s2n_numer"] = out[1]
        res["s2n_denom"] = out[2]
        res["npix"] = out[3].astype(np.int64)
        res["dof"] = out[4].astype(np.int64)
        res["chi2per"] = out[5]
        res["s2n_w"] = out[6]
        res["s2n"] = res["s2n_w"]
        perr = res["pars_err"]
        res["g"] = pars[:, 2:4]
        res["g_err"] = perr[:, 2:4]
        # (blocks of pars_cov: read when asked for, like pars_cov itself)
        res.set_lazy("g_cov", lambda r: r["pars_cov"][:, 2:4, 2:4])
        # pars_err is sqrt(diag(pars_cov)) (fitters.py:333-339), made by the
        # finalize kernel with the same IEEE square root
        res["T"] = pars[:, 4]
        res["T_err"] = perr[:, 4]
        if self.model == "coellip":
            # CoellipFitModel._set_flux is a no-op (results.py:648-652); _set_T
            # is not overridden: T is pars[4], the first component's
            return
        if nband == 1:
            res["flux"] = pars[:, nshape]
            res["flux_err"] = perr[:, nshape]
        else:
            res["flux"] = pars[:, nshape:]
            res.set_lazy("flux_cov", lambda r: r["pars_cov"][:, nshape:, nshape:])
            res["flux_err"] = perr[:, nshape:]
