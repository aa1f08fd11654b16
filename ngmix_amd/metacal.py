"""
Metacalibration images (reference: ngmix/metacal/): for every stamp the five
images `noshear, 1p, 1m, 2p, 2m` -- the object deconvolved from its psf,
sheared, and reconvolved with a slightly larger round gaussian -- as batches
on the device.

THE INTERPOLANT DIFFERS FROM THE REFERENCE'S.  The reference shears through
galsim: it interpolates a padded FFT of the stamp (Lanczos-15 in x, quintic in
k).  Here the discrete-time Fourier transform of the stamp's own samples is
evaluated exactly at the sheared frequency of every output mode -- the
band-limited interpolant, with no interpolation error (csrc/metacal.hip;
DESIGN.md, "metacalibration images", has the definition).  Pixel values and
random streams are therefore NOT the reference's; signatures, container
shapes, the target psf of 'fitgauss', the fixnoise recipe and the use made of
`rng` are.

    MetacalBatch(stamps, psf_stamps, psf='fitgauss', target_sigma=None, rng=None)
        .get_all(step=0.01, types=None, fixnoise=False, noise=None)
        .get_obs_galshear(g1, g2)
        .get_obs_psfshear(g1, g2)              (psf='dilate-exact')
        .device_noise(seed, ids=None, rotated=False)
    get_all_metacal(obs, psf='fitgauss', step=0.01, types=None, fixnoise=True,
                    rng=None, use_noise_image=False)

and, from the images to a shear catalogue ("metacal shear
catalogues"):

    metacal_bootstrap_batch(stamps, psf_stamps, model='gauss', step=0.01, ...,
                            noise_seed=None, ids=None, ...) -> (resdict, batchdict)
    shear_response(resdict, step=0.01, key='g') -> {'g', 'R', 'flags'[, 'Rpsf']}
    mean_shear(resp, select=None, psf_g=None) -> (2,)
    metacal_bootstrap(obs, runner, psf_runner=None, ...), MetacalBootstrapper
    metacal_bootstrap_many(list_of_obs, model='gauss', ...)
    (psf= and types= go through all of them to MetacalBatch / get_all_metacal)

and the pre-psf moments of the five types straight from the stamps, without
the images ("metacal pre-psf moments"; csrc/prepsf_shear.hip):

    metacal_moments_batch(stamps, psf_stamps, measure, step=0.01, types=None,
                          fixnoise=False, noise=None, noise_seed=None, ids=None) -> resdict
    metacal_moments_many(list_of_obs, measure, step=0.01, types=None, fixnoise=False,
                         noise_seed=None, ids=None, use_noise_image=False) -> [resdict_i]

and the fit of an exact profile in Fourier space to every type, without the
images either ("metacal shear from Fourier-space fits"):

    metacal_kfit_batch(stamps, psf_stamps, model='gauss', step=0.01, types=None,
                       psf='fitgauss', target_sigma=None, weight='flat', ...) -> resdict
    MetacalBatch.kfit_spectra(g, per_stamp=False, dil=None, kind=None)

Moments of noisy stamps carry the noise response; fixnoise=True with noise_seed
(or noise) sums the cancelling term of the turned, deconvolved, sheared noise
field with them ("fixnoise for the pre-psf moments").

With noise_seed the fixnoise field is drawn on the device as a pure function
of (seed, object id, pixel) (csrc/metacal_noise.hip): the same object gets the
same field however the catalogue is cut into batches.

psf='fitgauss' and an explicit target_sigma are served: a round gaussian
target, the five types.  psf='dilate-exact' is the reference's Metacal base
class (its psf='dilate') under this module's interpolant: the target is the psf
stamp's own image, deconvolved from the pixel, dilated by 1 + 2|g| and
reconvolved with the pixel -- the psf stamp's transform at one more frequency
per mode, nothing fitted, no METACAL_PSF_FIT_FAILURE ("the psf's own
dilated, sheared image as target").  Under it, and under it alone, get_all
takes all nine METACAL_TYPES: for `1p_psf, 1m_psf, 2p_psf, 2m_psf` the image is
left alone and the target psf is dilated and sheared (get_obs_psfshear), and

    shear_response(resdict) -> {..., 'Rpsf'}   with the four `*_psf` types
    mean_shear(resp, psf_g=(N, 2))             <R> gamma = <g> - <Rpsf psf_g>

psf='gauss', 'azgauss', 'dilate' and galsim-object psfs are defined through
galsim's stepk and interpolated images and raise NotImplementedError; so does
shearing the psf (the `*_psf` types) under every psf but 'dilate-exact', and in
the pre-psf moments, which have no target psf to shear.
"""
import numpy as np

from . import _lib
from .flags import METACAL_BAND_LIMIT   # a sheared mode of the pre-psf moments left the band
from .jacobian import Jacobian
from .observation import Observation, ObsList, MultiBandObsList

__all__ = ["MetacalBatch", "get_all_metacal", "METACAL_TYPES", "METACAL_MINIMAL_TYPES",
           "METACAL_PSF_FIT_FAILURE", "METACAL_NONFINITE", "DeviceNoise",
           "metacal_bootstrap_batch", "shear_response", "mean_shear", "metacal_bootstrap",
           "MetacalBootstrapper", "metacal_bootstrap_many", "METACAL_BAND_LIMIT",
           "metacal_moments_batch", "metacal_moments_many", "metacal_kfit_batch"]

METACAL_MINIMAL_TYPES = ["noshear", "1p", "1m", "2p", "2m"]
METACAL_PSF_TYPES = ["1p_psf", "1m_psf", "2p_psf", "2m_psf"]
METACAL_TYPES = METACAL_MINIMAL_TYPES + METACAL_PSF_TYPES     # all served by psf='dilate-exact'
DEFAULT_STEP = 0.01
DILATE_EXACT = "dilate-exact"

# per-stamp flags of the outputs
METACAL_PSF_FIT_FAILURE = 1     # the adaptive moments of the psf stamp failed
METACAL_NONFINITE = 2           # a kept mode of the spectrum was not finite
# (METACAL_BAND_LIMIT = 1 << 16 lives in flags.py: it is also ORed into the fit flags)

_PSF_FIT_NTRY = 4


def _torch():
    import torch
    return torch


def _check_psf_kind(psf):
    if isinstance(psf, str):
        if psf in ("fitgauss", DILATE_EXACT):
            return
        if psf in ("gauss", "azgauss", "dilate"):
            raise NotImplementedError(
                "metacal psf='%s' is defined through galsim's stepk and interpolated images; "
                "use psf='fitgauss', psf='dilate-exact' or an explicit target_sigma" % psf)
        raise ValueError("bad metacal psf: '%s'" % psf)
    raise NotImplementedError(
        "a galsim object as the metacal psf needs galsim's interpolants; use psf='fitgauss', "
        "psf='dilate-exact' or an explicit target_sigma")


def _check_types(types, psf="fitgauss"):
    """the list of types; the `*_psf` types only under psf='dilate-exact' (psf
    None: the pre-psf moments, which have no target psf)"""
    if types is None:
        return list(METACAL_MINIMAL_TYPES)
    types = list(types)
    dilate = isinstance(psf, str) and psf == DILATE_EXACT
    for t in types:
        if isinstance(t, str) and t in METACAL_PSF_TYPES:
            if dilate:
                continue
            if psf is None:
                raise NotImplementedError(
                    "metacal type '%s': shearing the psf is not served by the pre-psf moments, "
                    "which have no target psf to shear; the images of psf='dilate-exact' "
                    "serve it" % t)
            raise NotImplementedError(
                "metacal type '%s': shearing the psf is not served under this psf; "
                "psf='dilate-exact' serves it" % t)
        if t not in METACAL_MINIMAL_TYPES:
            raise ValueError("bad metacal type: %s" % (t,))
    return types


def _type_shears(types, step):
    table = {"noshear": (0.0, 0.0), "1p": (step, 0.0), "1m": (-step, 0.0),
             "2p": (0.0, step), "2m": (0.0, -step)}
    return np.array([table[t[:-4] if t.endswith("_psf") else t] for t in types],
                    dtype=np.float64).reshape(len(types), 2)


def _type_kinds(types):
    """1 where the type shears the psf, 0 where it shears the image"""
    return np.array([1 if t in METACAL_PSF_TYPES else 0 for t in types], dtype=np.int32)


def _check_shears(g):
    if not np.all(g[..., 0] ** 2 + g[..., 1] ** 2 < 1.0):
        raise ValueError("shears must lie inside the unit circle")


def _one_shape(stamps, what):
    if stamps.n == 0:
        raise ValueError("%s: an empty batch" % what)
    nrow, ncol = int(stamps.nrow[0]), int(stamps.ncol[0])
    if np.any(stamps.nrow != nrow) or np.any(stamps.ncol != ncol) or \
            np.any(stamps.pix_off != np.arange(stamps.n, dtype=np.int64) * (nrow * ncol)):
        raise ValueError("%s: all stamps of a batch share one shape" % what)
    return nrow, ncol


def fitgauss_sigma(irr, irc, icc):
    """
    The width of the reference's fitgauss target psf (fitgauss_target_psf.py)
    from the gaussian fitted to the psf: T = irr + icc dilated by
    _get_ellip_dilation -- the largest eigenvalue of the covariance over T/2,
    square root, doubled excess, at most 1.1 -- and sigma = sqrt(T dilation / 2).
    """
    T = irr + icc
    with np.errstate(invalid="ignore", divide="ignore"):
        eig = 0.5 * T + np.sqrt((0.5 * (icc - irr)) ** 2 + irc ** 2)
        dilation = np.minimum(1.0 + 2.0 * (np.sqrt(eig / (T / 2.0)) - 1.0), 1.1)
        return np.sqrt(T * dilation / 2.0)


class DeviceNoise(object):
    """
    Stands for MetacalBatch.device_noise(seed, ids) as the `noise` of get_all:
    the planes are drawn straight into the turned layout the spectrum kernel
    reads, without the copy torch.rot90 makes.  The images are those of the
    two-step route to the bit.
    """

    def __init__(self, seed, ids=None):
        self.seed, self.ids = seed, ids


class MetacalBatch(object):
    """
    stamps, psf_stamps: StampBatch of the images and of their psf images (stamp
        i of one belongs to stamp i of the other).  All stamps share one shape,
        the psf stamps share one, possibly another; every stamp has its own
        jacobian, whose derivatives its psf stamp shares.
    psf: 'fitgauss' -- the target is the round gaussian of the reference's
        MetacalFitGaussPSF: adaptive moments of every psf stamp, as one batch
        (StampBatch.admom, up to four starts), T and e of the fit, the
        ellipticity dilation, sigma_T = sqrt(T dilation / 2).  A stamp whose
        moments fail is flagged METACAL_PSF_FIT_FAILURE and its outputs are
        NaN.  (The reference falls back to an LM fit of a gaussian, then to a
        stored gmix; that fallback is not made here.)
        'dilate-exact' -- the target is the psf stamp's own image, deconvolved
        from the pixel, dilated (and, in the `*_psf` types and
        get_obs_psfshear, sheared) and reconvolved with the pixel: the
        reference's Metacal base class.  Nothing is fitted: fit_flags stay
        zero and target_sigma is None.  get_all gives every type, noshear
        included, the dilation 1 + 2 step; the per-stamp calls 1 + 2|g|.  The
        output psf stamps keep the input psf stamps' jacobians and centres.
    target_sigma: (N,) widths used instead of the fit (a ValueError with
        psf='dilate-exact').
    rng: np.random.RandomState for the fit's starting points and for the noise
        fields of fixnoise.

    Every output is resident on the device, ready for bootstrap_batch,
    LMBatchFitter and the other batch consumers.
    """

    def __init__(self, stamps, psf_stamps, psf="fitgauss", target_sigma=None, rng=None):
        self.dilate = isinstance(psf, str) and psf == DILATE_EXACT
        if self.dilate and target_sigma is not None:
            raise ValueError("psf='dilate-exact' has no gaussian target: do not send target_sigma")
        if target_sigma is None:
            _check_psf_kind(psf)
        from .batch import StampBatch
        if not isinstance(stamps, StampBatch) or not isinstance(psf_stamps, StampBatch):
            raise ValueError("stamps and psf_stamps must be StampBatch objects")
        if stamps.n != psf_stamps.n:
            raise ValueError("one psf stamp per stamp: %d stamps, %d psf stamps"
                             % (stamps.n, psf_stamps.n))
        if stamps.val is None or psf_stamps.val is None:
            raise ValueError("stamps and psf_stamps must hold pixel data")
        self.shape = _one_shape(stamps, "stamps")
        self.psf_shape = _one_shape(psf_stamps, "psf_stamps")
        self.stamps, self.psf_stamps = stamps, psf_stamps
        self.n = stamps.n
        self.device = stamps.device
        self.rng = rng if rng is not None else np.random.RandomState()
        torch = _torch()
        self._psf_cen = psf_stamps.jac[:, 0:2].contiguous()
        self._psf_flux = psf_stamps.val.reshape(self.n, -1).sum(dim=1).contiguous()
        self.fit_flags = np.zeros(self.n, dtype=np.int32)
        if self.dilate:
            self.target_sigma = self._sigma = None
            return
        if target_sigma is not None:
            sigma = np.ascontiguousarray(target_sigma, dtype=np.float64)
            if sigma.shape != (self.n,):
                raise ValueError("target_sigma must have shape (%d,)" % self.n)
            if not np.all(sigma > 0):
                raise ValueError("target_sigma must be positive")
        else:
            sigma = self._fit_target_sigma()
        self.target_sigma = sigma
        self._sigma = torch.from_numpy(sigma).to(self.device)

    # ------------------------------------------------------------ the psf fit
    def _fit_target_sigma(self):
        """adaptive moments of the psf stamps -> sigma_T; fit_flags where they fail"""
        from .batch import GMixBatch
        psf = self.psf_stamps
        scale = psf.jac[:, 7].cpu().numpy()
        sigma = np.full(self.n, np.nan)
        todo = np.arange(self.n)
        for itry in range(_PSF_FIT_NTRY):
            batch = psf if todo.size == self.n else psf.select(todo)
            m = todo.size
            # round starts of two pixels' T, scattered by ten per cent, within
            # a tenth of a pixel of the jacobian's centre
            guess = np.zeros((m, 6))
            guess[:, 0:2] = self.rng.uniform(-0.1, 0.1, size=(m, 2)) * scale[todo, None]
            guess[:, 4] = 4.0 * scale[todo] ** 2 * (1.0 + self.rng.uniform(-0.1, 0.1, size=m)) \
                * (1.0 + 0.5 * itry)
            guess[:, 5] = 1.0
            wt, _ = GMixBatch.from_pars(guess, "gauss", device=self.device)
            res, status = batch.admom(wt, no_cov=True)
            torch = _torch()
            cols = wt.data[:, 3:6].cpu().numpy()        # irr, irc, icc of the weight
            # (the int32 flags head the 584-byte records)
            flags = res[:, 0:1].clone().view(torch.int32)[:, 0].cpu().numpy()
            status = status.cpu().numpy()
            s = fitgauss_sigma(cols[:, 0], cols[:, 1], cols[:, 2])
            ok = (flags == 0) & (status == 0) & np.isfinite(s) & (s > 0)
            sigma[todo[ok]] = s[ok]
            todo = todo[~ok]
            if todo.size == 0:
                break
        self.fit_flags[todo] = METACAL_PSF_FIT_FAILURE
        return sigma

    # ------------------------------------------------------------ the operation
    def _noise_planes(self, noise):
        """the (N, R, C) noise stamps on the device: given, or drawn as
        N(0, 1/sqrt(w)), zero where w = 0 (simobs.simulate_obs with no model)"""
        torch = _torch()
        nrow, ncol = self.shape
        if isinstance(noise, DeviceNoise):
            return noise
        if noise is None:
            ierr = self.stamps.ierr.reshape(self.n, nrow, ncol).cpu().numpy()
            with np.errstate(divide="ignore"):
                sd = np.where(ierr > 0, 1.0 / ierr, 0.0)
            noise = self.rng.normal(size=sd.shape) * sd
        if isinstance(noise, torch.Tensor):
            d = noise.to(device=self.device, dtype=torch.float64)
        else:
            d = torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float64)).to(self.device)
        if d.numel() != self.n * nrow * ncol:
            raise ValueError("noise must hold one %d x %d plane per stamp" % (nrow, ncol))
        return d.reshape(self.n, nrow, ncol)

    def device_noise(self, seed, ids=None, rotated=False):
        """
        The noise planes of fixnoise drawn on the device, (N, R, C) float64:
        unit normals of Philox4x32-10 under the key `seed` (0 <= seed < 2^64)
        and the counter (object id, pixel pair), over the stamps' ierr, +0.0
        where ierr is not positive (csrc/metacal_noise.hpp).  ids: (N,) int64
        object ids, default the positions 0 .. N-1.  A stamp's plane depends on
        (seed, id, ierr) alone, not on the batch it is drawn in.  rotated: the
        planes as torch.rot90(., 1, dims=(1, 2)) has them (square stamps).
        """
        torch = _torch()
        from .batch import _dptr, _stream, _on_device
        nrow, ncol = self.shape
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("the noise seed must be in [0, 2^64)")
        d_ids = None
        if ids is not None:
            if isinstance(ids, torch.Tensor):
                d_ids = ids.to(device=self.device, dtype=torch.int64).contiguous()
            else:
                d_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(self.device)
            if tuple(d_ids.shape) != (self.n,):
                raise ValueError("ids must have shape (%d,)" % self.n)
        if rotated and nrow != ncol:
            raise ValueError("the rotated noise planes need square stamps, got %d x %d"
                             % (nrow, ncol))
        ierr = self.stamps.ierr
        if ierr is None or ierr.numel() != self.n * nrow * ncol:
            raise ValueError("the stamps hold no per-pixel ierr to draw the noise over")
        ierr = ierr.reshape(-1).contiguous()
        out = torch.empty((self.n, nrow, ncol), dtype=torch.float64, device=self.device)
        with _on_device(self.device):
            st = _lib.lib().ngmix_metacal_noise_batch(
                _dptr(ierr), _dptr(d_ids), seed, self.n, nrow, ncol, 1 if rotated else 0,
                _dptr(out), _stream())
        _lib.check(st, "ngmix_metacal_noise_batch")
        return out

    def _run(self, g, per_stamp, noise, dil=None, kind=None):
        """
        g: (T, 2), or (N, T, 2) with per_stamp; noise: (N, R, C) device tensor,
        a DeviceNoise (drawn here, already turned) or None.  With
        psf='dilate-exact', dil (float64) and kind (int32: 1 where the psf is
        sheared), both (T,) or (N, T).  Returns the images (T, N, R, C), the
        target psf images (T, N, Rp, Cp) and the flags (T, N), all on the device.
        """
        torch = _torch()
        from .batch import _dptr, _stream, _on_device
        n, (nrow, ncol), (prow, pcol) = self.n, self.shape, self.psf_shape
        ntypes = g.shape[-2]
        g = np.ascontiguousarray(g, dtype=np.float64)
        _check_shears(g)
        d_g = torch.from_numpy(g).to(self.device)
        if self.dilate:
            dil = np.ascontiguousarray(dil, dtype=np.float64)
            kind = np.ascontiguousarray(kind, dtype=np.int32)
            if dil.shape != g.shape[:-1] or kind.shape != g.shape[:-1]:
                raise ValueError("one dilation and one kind per shear")
            d_dil, d_kind = torch.from_numpy(dil).to(self.device), \
                torch.from_numpy(kind).to(self.device)
        planes = 1 if noise is None else 2
        d_noise = None
        if noise is not None:
            if nrow != ncol:
                raise ValueError("fixnoise turns the noise stamp by 90 degrees: the stamps "
                                 "must be square, got %d x %d" % (nrow, ncol))
            if isinstance(noise, DeviceNoise):
                d_noise = self.device_noise(noise.seed, noise.ids, rotated=True)
            else:
                d_noise = torch.rot90(noise, 1, dims=(1, 2)).contiguous()
        spec = torch.empty((n, ntypes, planes, nrow, ncol // 2 + 1, 2), dtype=torch.float64,
                           device=self.device)
        kflags = torch.empty((n, ntypes), dtype=torch.int32, device=self.device)
        images = self.stamps.val.reshape(n, nrow, ncol)
        if not images.is_contiguous():
            images = images.contiguous()
        if self.dilate:
            pspec = torch.empty((n, ntypes, prow, pcol // 2 + 1, 2), dtype=torch.float64,
                                device=self.device)
            pflags = torch.empty((n, ntypes), dtype=torch.int32, device=self.device)
            with _on_device(self.device):
                L = _lib.lib()
                st = L.ngmix_metacal_dilate_spectrum_batch(
                    _dptr(images), _dptr(d_noise), _dptr(self.psf_stamps.val),
                    _dptr(self.stamps.jac), _dptr(self._psf_cen), _dptr(d_g), _dptr(d_dil),
                    _dptr(d_kind), _lib.ptr(g), _lib.ptr(dil), _lib.ptr(kind), int(per_stamp), n,
                    ntypes, nrow, ncol, prow, pcol, _dptr(spec), _dptr(kflags), _stream())
                _lib.check(st, "ngmix_metacal_dilate_spectrum_batch")
                st = L.ngmix_metacal_dilate_psf_spectrum_batch(
                    _dptr(self.psf_stamps.val), _dptr(self.psf_stamps.jac), _dptr(self._psf_cen),
                    _dptr(d_g), _dptr(d_dil), _dptr(d_kind), _lib.ptr(g), _lib.ptr(dil),
                    _lib.ptr(kind), int(per_stamp), n, ntypes, prow, pcol, _dptr(pspec),
                    _dptr(pflags), _stream())
                _lib.check(st, "ngmix_metacal_dilate_psf_spectrum_batch")
            kflags = kflags | pflags
        else:
            with _on_device(self.device):
                st = _lib.lib().ngmix_metacal_spectrum_batch(
                    _dptr(images), _dptr(d_noise), _dptr(self.psf_stamps.val),
                    _dptr(self.stamps.jac), _dptr(self._psf_cen), _dptr(self._psf_flux),
                    _dptr(self._sigma), _dptr(d_g), _lib.ptr(g), int(per_stamp), n, ntypes, nrow,
                    ncol, prow, pcol, _dptr(spec), _dptr(kflags), _stream())
            _lib.check(st, "ngmix_metacal_spectrum_batch")
        # the regular-grid inverse transform (rocFFT); the spectrum is
        # hermitian on its Nyquist row and column, where a complex-to-real
        # transform would otherwise drop what does not fit
        out = torch.fft.irfft2(torch.view_as_complex(spec), s=(nrow, ncol))
        if noise is not None:
            out = out[:, :, 0] + torch.rot90(out[:, :, 1], 3, dims=(2, 3))
        else:
            out = out[:, :, 0]
        flags = torch.where(kflags != 0, METACAL_NONFINITE, 0).to(torch.int32) | \
            torch.from_numpy(self.fit_flags).to(self.device)[:, None]
        nan = torch.full((), float("nan"), dtype=torch.float64, device=self.device)
        out = torch.where(flags[:, :, None, None] != 0, nan, out)
        out = out.permute(1, 0, 2, 3).contiguous()
        flags = flags.t().contiguous()
        if self.dilate:
            # (the same inverse transform on the psf stamps' own grid)
            psf_images = torch.fft.irfft2(torch.view_as_complex(pspec), s=(prow, pcol))
            psf_images = psf_images.permute(1, 0, 2, 3).contiguous()
        else:
            psf_images = self._target_psf_images(g, per_stamp)
        psf_images = torch.where(flags[:, :, None, None] != 0, nan, psf_images)
        return out, psf_images, flags

    def kfit_spectra(self, g, per_stamp=False, dil=None, kind=None):
        """
        The operation of _run without a noise plane, written for the
        Fourier-space fits (the KFIT form of
        metacal_spectrum_kernel): g, dil, kind as _run takes them.  Returns
        dhat, phat, aux, all (T N, R, C//2+1, 2) and type-major -- O^ about the
        jacobian centre, the target psf over the psf stamp's sum, and (keep,
        rho^2) per mode -- and the flags (T, N) int32 as _run's, on the device.
        """
        torch = _torch()
        from .batch import _dptr, _stream, _on_device
        n, (nrow, ncol), (prow, pcol) = self.n, self.shape, self.psf_shape
        g = np.ascontiguousarray(g, dtype=np.float64)
        ntypes = g.shape[-2]
        if g.shape != ((n, ntypes, 2) if per_stamp else (ntypes, 2)):
            raise ValueError("g must be (T, 2), or (N, T, 2) with per_stamp")
        _check_shears(g)
        d_g = torch.from_numpy(g).to(self.device)
        d_dil = d_kind = None
        if self.dilate:
            dil = np.ascontiguousarray(dil, dtype=np.float64)
            kind = np.ascontiguousarray(kind, dtype=np.int32)
            if dil.shape != g.shape[:-1] or kind.shape != g.shape[:-1]:
                raise ValueError("one dilation and one kind per shear")
            d_dil, d_kind = torch.from_numpy(dil).to(self.device), \
                torch.from_numpy(kind).to(self.device)
        shape = (ntypes * n, nrow, ncol // 2 + 1, 2)
        dhat, phat, aux = (torch.empty(shape, dtype=torch.float64, device=self.device)
                           for _ in range(3))
        kflags = torch.empty((ntypes, n), dtype=torch.int32, device=self.device)
        images = self.stamps.val.reshape(n, nrow, ncol).contiguous()
        with _on_device(self.device):
            st = _lib.lib().ngmix_metacal_kfit_spectrum_batch(
                _dptr(images), _dptr(self.psf_stamps.val), _dptr(self.stamps.jac),
                _dptr(self._psf_cen), _dptr(self._psf_flux),
                None if self.dilate else _dptr(self._sigma), _dptr(d_g), _dptr(d_dil),
                _dptr(d_kind), _lib.ptr(g), _lib.ptr(dil) if self.dilate else None,
                _lib.ptr(kind) if self.dilate else None, int(per_stamp), n, ntypes, nrow, ncol,
                prow, pcol, _dptr(dhat), _dptr(phat), _dptr(aux), _dptr(kflags), _stream())
        _lib.check(st, "ngmix_metacal_kfit_spectrum_batch")
        flags = torch.where(kflags != 0, METACAL_NONFINITE, 0).to(torch.int32) | \
            torch.from_numpy(self.fit_flags).to(self.device)[None, :]
        return dhat, phat, aux, flags

    def _psf_jacobians(self):
        """the psf stamps' jacobians with the centre at the stamp's exact centre"""
        jac = self.psf_stamps.jac.clone()
        jac[:, 0] = (self.psf_shape[0] - 1.0) / 2.0
        jac[:, 1] = (self.psf_shape[1] - 1.0) / 2.0
        return jac

    def _target_psf_images(self, g, per_stamp):
        """the round gaussians of width sigma_T (1 + 2|g|) carrying the psf
        images' flux, on the psf stamps' grid about its centre: (T, N, Rp, Cp)"""
        torch = _torch()
        from .batch import StampBatch, GMixBatch
        n, (prow, pcol) = self.n, self.psf_shape
        ntypes = g.shape[-2]
        gabs = np.sqrt(g[..., 0] ** 2 + g[..., 1] ** 2)          # (T,) or (N, T)
        gabs = np.broadcast_to(gabs.T if per_stamp else gabs[:, None], (ntypes, n))
        sig = self._sigma[None, :] * torch.from_numpy(1.0 + 2.0 * gabs).to(self.device)
        bad = ~torch.isfinite(sig)
        pars = torch.zeros((ntypes * n, 6), dtype=torch.float64, device=self.device)
        pars[:, 4] = torch.where(bad, torch.ones_like(sig), 2.0 * sig * sig).reshape(-1)
        pars[:, 5] = self._psf_flux[None, :].expand(ntypes, n).reshape(-1)
        gm, _ = GMixBatch.from_pars(pars, "gauss", device=self.device)
        m = ntypes * n
        geom = StampBatch(None, None, self._psf_jacobians().repeat(ntypes, 1), np.full(m, prow),
                          np.full(m, pcol), np.arange(m, dtype=np.int64) * (prow * pcol), False)
        image, _ = geom.render(gm, fast_exp=False, no_skip=True)
        return image.reshape(ntypes, n, prow, pcol)

    def _stamp_batches(self, images, psf_images, fixnoise):
        """the StampBatch pair of one type: the input's jacobians and weights
        (halved by fixnoise), the target psf about its stamp's centre"""
        from .batch import StampBatch
        s, p = self.stamps, self.psf_stamps
        ierr = s.ierr * np.sqrt(0.5) if fixnoise else s.ierr
        izw = (s.flags & _lib.STAMP_IGNORE_ZERO_WEIGHT) != 0
        out = StampBatch(images.reshape(-1), ierr, s.jac, s.nrow, s.ncol, s.pix_off, izw,
                         npix_kept=s.npix_kept,
                         uniform_ierr=(s.flags & _lib.STAMP_UNIFORM_IERR) != 0)
        pizw = (p.flags & _lib.STAMP_IGNORE_ZERO_WEIGHT) != 0
        # (the dilated psf stays where the psf stamp has it: the base class's _make_psf_obs)
        pjac = p.jac if self.dilate else self._psf_jacobians()
        pout = StampBatch(psf_images.reshape(-1), p.ierr, pjac, p.nrow, p.ncol,
                          p.pix_off, pizw, npix_kept=p.npix_kept,
                          uniform_ierr=(p.flags & _lib.STAMP_UNIFORM_IERR) != 0)
        return out, pout

    def get_all(self, step=DEFAULT_STEP, types=None, fixnoise=False, noise=None):
        """
        {type: {'stamps': StampBatch, 'psf_stamps': StampBatch, 'flags': (N,)
        int32 array}} for types of METACAL_MINIMAL_TYPES (default: all five),
        all in one launch; noshear is the same path at g = 0.  With
        psf='dilate-exact' the types of METACAL_TYPES, the four `*_psf` too (the
        default stays the five); every type, noshear included, has the target
        psf dilated by 1 + 2 step, as the reference draws noshear with 1p's psf.

        fixnoise: a noise stamp per image -- `noise` ((N, R, C) array or device
        tensor), or drawn from the weights with the batch's rng -- is turned by
        rot90(k=1), put through the same operation with the same shear, turned
        back by k=3 and added; the weight becomes 1 / (1/w + 1/w) where w > 0.
        Square stamps only.
        """
        types = _check_types(types, DILATE_EXACT if self.dilate else "fitgauss")
        g = _type_shears(types, float(step))
        _check_shears(g)
        if fixnoise and self.shape[0] != self.shape[1]:
            raise ValueError("fixnoise turns the noise stamp by 90 degrees: the stamps must be "
                             "square, got %d x %d" % self.shape)
        planes = self._noise_planes(noise) if fixnoise else None
        if self.dilate:
            dil = np.full(len(types), 1.0 + 2.0 * abs(float(step)))
            images, psf_images, flags = self._run(g, False, planes, dil, _type_kinds(types))
        else:
            images, psf_images, flags = self._run(g, False, planes)
        flags = flags.cpu().numpy()
        out = {}
        for i, t in enumerate(types):
            sb, psb = self._stamp_batches(images[i], psf_images[i], fixnoise)
            out[t] = {"stamps": sb, "psf_stamps": psb, "flags": flags[i]}
        return out

    def get_obs_galshear(self, g1, g2):
        """the images sheared by (g1[i], g2[i]), one shear per stamp: a dict
        as one entry of get_all's"""
        return self._per_stamp_shear(g1, g2, 0)

    def get_obs_psfshear(self, g1, g2):
        """psf='dilate-exact': the images left unsheared and reconvolved with
        the psf dilated by 1 + 2|g| and sheared by (g1[i], g2[i]), one shear
        per stamp (the reference's Metacal.get_obs_psfshear): a dict as one
        entry of get_all's"""
        if not self.dilate:
            raise NotImplementedError("get_obs_psfshear: shearing the psf is not served under "
                                      "this psf; psf='dilate-exact' serves it")
        return self._per_stamp_shear(g1, g2, 1)

    def _per_stamp_shear(self, g1, g2, kind):
        g = np.stack([np.broadcast_to(np.asarray(g1, dtype=np.float64), (self.n,)),
                      np.broadcast_to(np.asarray(g2, dtype=np.float64), (self.n,))], axis=1)
        g = g.reshape(self.n, 1, 2)
        if self.dilate:
            dil = 1.0 + 2.0 * np.sqrt(g[..., 0] ** 2 + g[..., 1] ** 2)
            images, psf_images, flags = self._run(g, True, None, dil,
                                                  np.full((self.n, 1), kind, dtype=np.int32))
        else:
            images, psf_images, flags = self._run(g, True, None)
        sb, psb = self._stamp_batches(images[0], psf_images[0], False)
        return {"stamps": sb, "psf_stamps": psb, "flags": flags[0].cpu().numpy()}


# ---------------------------------------------------------------------------
# the reference's entry point

def _flatten(obs):
    """(list of Observations, rebuild(list of new Observations) -> container)"""
    if isinstance(obs, Observation):
        return [obs], lambda new: new[0]
    if isinstance(obs, MultiBandObsList):
        flat = [o for ol in obs for o in ol]
        sizes = [len(ol) for ol in obs]

        def rebuild(new):
            out, at = MultiBandObsList(), 0
            for m in sizes:
                ol = ObsList()
                for o in new[at:at + m]:
                    ol.append(o)
                out.append(ol)
                at += m
            return out
        return flat, rebuild
    if isinstance(obs, ObsList):
        def rebuild(new):
            out = ObsList()
            for o in new:
                out.append(o)
            return out
        return list(obs), rebuild
    raise ValueError("obs must be Observation, ObsList, or MultiBandObsList")


def get_all_metacal(obs, psf="fitgauss", step=DEFAULT_STEP, types=None, fixnoise=True,
                    rng=None, use_noise_image=False):
    """
    The reference's get_all_metacal (ngmix/metacal/convenience.py): a dict
    {type: container like obs} of metacal Observations.

    obs: Observation, ObsList or MultiBandObsList; every Observation has a psf
        Observation with the same jacobian derivatives
    psf: 'fitgauss' (the default here), or 'dilate-exact': the psf's own
        dilated image as the target (MetacalBatch), which also serves the
        `*_psf` types; its psf observations get the new image and keep their
        jacobian and weight, no psf noise is added, and rng is needed only to
        draw a fixnoise field.  ('gauss', 'azgauss', 'dilate' and galsim
        objects raise NotImplementedError: they rest on galsim)
    fixnoise: add the sheared, rotated noise field and halve the weights
        (_get_all_metacal_fixnoise); the noise field is obs.noise with
        use_noise_image, else drawn from the weights with rng
    rng: required; it also draws the small noise (max / 50000) added to the
        target psf images, whose weights become (50000 / max)^2
        (_setup_psf_noise)

    Observations are grouped by image and psf shape; each group runs as one
    batch on the device.  Pixel values are not the reference's: the interpolant
    differs (see the top of this module).
    """
    _check_psf_kind(psf)
    types = _check_types(types, psf)
    flat, rebuild = _flatten(obs)
    dilate = psf == DILATE_EXACT
    if rng is None and dilate and fixnoise and not use_noise_image:
        raise ValueError("send an rng to get_all_metacal: psf='dilate-exact' draws the "
                         "fixnoise field with it")
    if rng is None and not dilate:
        raise ValueError("send an rng to get_all_metacal (psf='fitgauss')")
    for o in flat:
        if not o.has_psf():
            raise ValueError("observation must have a psf observation set")
        if use_noise_image and fixnoise and not o.has_noise():
            raise ValueError("obs.noise must be set when use_noise_image=True")
        if fixnoise and o.image.shape[0] != o.image.shape[1]:
            raise ValueError("fixnoise needs square images, got %s" % (o.image.shape,))
        a, b = o.jacobian, o.psf.jacobian
        if any(getattr(a, k) != getattr(b, k) for k in ("dvdrow", "dvdcol", "dudrow", "dudcol")):
            raise ValueError("the psf and the observation must have the same jacobian "
                             "derivatives")
    from .batch import StampBatch
    groups = {}
    for i, o in enumerate(flat):
        groups.setdefault((o.image.shape, o.psf.image.shape), []).append(i)
    new = {t: [None] * len(flat) for t in types}
    for idx in groups.values():
        sub = [flat[i] for i in idx]
        mc = MetacalBatch(StampBatch.from_observations(sub),
                          StampBatch.from_observations([o.psf for o in sub]), psf=psf, rng=rng)
        noise = None
        if fixnoise and use_noise_image:
            noise = np.stack([o.noise for o in sub])
        res = mc.get_all(step=step, types=types, fixnoise=fixnoise, noise=noise)
        for t in types:
            shape, pshape = sub[0].image.shape, sub[0].psf.image.shape
            ims = res[t]["stamps"].val.reshape((len(sub),) + shape).cpu().numpy()
            pims = res[t]["psf_stamps"].val.reshape((len(sub),) + pshape).cpu().numpy()
            for k, i in enumerate(idx):
                new[t][i] = _make_obs(sub[k], ims[k], pims[k], int(res[t]["flags"][k]),
                                      fixnoise, rng, dilate)
    return {t: rebuild(new[t]) for t in types}


def _make_obs(obs, image, psf_image, flags, fixnoise, rng, dilate=False):
    """a copy of obs with the metacal image and the target psf (_make_obs,
    _make_psf_obs and, with fixnoise, _doadd_single_obs of the reference);
    dilate: the base class's psf observation -- the new image, the psf's own
    jacobian and weight, no noise added"""
    pim = obs.psf.image
    new_psf = obs.psf.copy()
    if dilate:
        with new_psf.writeable():
            new_psf.image[:, :] = psf_image
    else:
        psf_noise = pim.max() / 50000.0
        psf_image = psf_image + rng.normal(size=pim.shape, scale=psf_noise)
        with new_psf.writeable():
            new_psf.image[:, :] = psf_image
            new_psf.weight[:, :] = pim * 0 + 1.0 / psf_noise ** 2
        # the centre goes where the target psf was drawn: the stamp's exact centre
        jac = new_psf.jacobian
        new_psf.jacobian = Jacobian(row=(pim.shape[0] - 1.0) / 2.0,
                                    col=(pim.shape[1] - 1.0) / 2.0,
                                    dvdrow=jac.dvdrow, dvdcol=jac.dvdcol, dudrow=jac.dudrow,
                                    dudcol=jac.dudcol)
    new = obs.copy()
    if fixnoise:
        # (the image before the noise field was added stays on the device: only
        # the weight's original is kept, as _doadd_single_obs keeps it)
        new.weight_orig = obs.weight.copy()
    new.image = image
    if fixnoise:
        w = obs.weight
        halved = np.zeros_like(w)
        pos = w > 0
        halved[pos] = 1.0 / (1.0 / w[pos] + 1.0 / w[pos])
        new.weight = halved
    new.psf = new_psf
    new.meta["metacal_flags"] = flags
    return new


# ---------------------------------------------------------------------------
# from the images to a shear catalogue

def metacal_bootstrap_batch(stamps, psf_stamps, model="gauss", step=DEFAULT_STEP, types=None,
                            fixnoise=True, noise_seed=None, ids=None, psf="fitgauss",
                            target_sigma=None, rng=None, **bootstrap_kws):
    """
    The metacal images of a stamp batch and a bootstrap fit on every type, all
    on the device: MetacalBatch(stamps, psf_stamps, psf, target_sigma,
    rng).get_all(step, types, fixnoise, noise), then
    pipeline.bootstrap_batch(stamps, psf_stamps, model=model, rng=rng,
    **bootstrap_kws) on each type's pair, in the order of `types`.

    noise_seed: with fixnoise, the noise field is drawn on the device from
        (noise_seed, ids, pixel) (MetacalBatch.device_noise; ids default to
        the positions in the batch); None: drawn on the host from rng, as
        get_all does
    rng: np.random.RandomState of the psf fits' and the guesses' starting
        points (and of the host noise draw)
    psf, types: as MetacalBatch and get_all take them; psf='dilate-exact' with
        types=METACAL_TYPES gives the nine fits shear_response makes 'Rpsf' of

    Returns (resdict, batchdict): resdict[type] is bootstrap_batch's dict with
    'mcal_flags', the type's metacal flags (N,), added; batchdict is get_all's
    dict.  A stamp flagged by metacal has NaN images: its psf fit fails, its
    row comes back with flags = BOOT_PSF_FAILURE and NaN parameters.
    """
    from .pipeline import bootstrap_batch
    for k in ("stamp_obj", "stamp_band"):
        if bootstrap_kws.get(k) is not None:
            raise ValueError("metacal_bootstrap_batch fits one stamp per object: no %s" % k)
    if ids is not None and noise_seed is None:
        raise ValueError("ids belong to the device noise: send noise_seed too")
    mc = MetacalBatch(stamps, psf_stamps, psf=psf, target_sigma=target_sigma, rng=rng)
    noise = None
    if fixnoise and noise_seed is not None:
        noise = DeviceNoise(noise_seed, ids)
    batchdict = mc.get_all(step=step, types=types, fixnoise=fixnoise, noise=noise)
    resdict = {}
    for t, d in batchdict.items():
        res = bootstrap_batch(d["stamps"], d["psf_stamps"], model=model, rng=rng, **bootstrap_kws)
        res["mcal_flags"] = d["flags"]
        resdict[t] = res
    return resdict, batchdict


def _flat_moment_T(stamps, psf_stamps):
    """a starting T per stamp from the flat-weight second moments about the
    jacobian centres: T = sum I (v^2 + u^2) / sum I of the image less the psf
    stamp's; where that is not positive, half the image's own T, and at least
    that of a round gaussian of half a pixel's sigma"""
    torch = _torch()

    def flat_T(sb):
        nrow, ncol = _one_shape(sb, "stamps")
        val = sb.val.reshape(sb.n, nrow, ncol)
        r = torch.arange(nrow, dtype=torch.float64, device=sb.device)[None, :, None] \
            - sb.jac[:, 0, None, None]
        c = torch.arange(ncol, dtype=torch.float64, device=sb.device)[None, None, :] \
            - sb.jac[:, 1, None, None]
        col = lambda k: sb.jac[:, k, None, None]
        v, u = col(2) * r + col(3) * c, col(4) * r + col(5) * c
        return (val * (v * v + u * u)).sum(dim=(1, 2)) / val.sum(dim=(1, 2))

    T, Tp = flat_T(stamps), flat_T(psf_stamps)
    floor = (0.5 * stamps.jac[:, 7]) ** 2
    Tobj = torch.where(T - Tp > 0, T - Tp, 0.5 * T)
    return torch.where(torch.isfinite(Tobj) & (Tobj > 2.0 * floor), Tobj, 2.0 * floor)


def _flat_moment_r50(stamps, psf_stamps):
    """_flat_moment_T as a round gaussian's r50 = sqrt(2 ln 2) sqrt(T / 2)"""
    torch = _torch()
    return np.sqrt(2.0 * np.log(2.0)) * torch.sqrt(0.5 * _flat_moment_T(stamps, psf_stamps))


def metacal_kfit_batch(stamps, psf_stamps, model="gauss", step=DEFAULT_STEP, types=None,
                       psf="fitgauss", target_sigma=None, weight="flat", prior=None, guess=None,
                       size_type=None, fit_pars=None, fixnoise=False, rng=None):
    """
    Metacal shear from Fourier-space fits of an exact profile:
    KStampBatch.from_metacal(stamps, psf_stamps, types, step, psf, target_sigma,
    weight) -- the types' spectra straight in the fit's layout, the target psf
    analytic, a weight per mode -- then ONE KSpaceBatchFitter(model, prior,
    fit_pars, size_type=size_type).go over all types' stamps.

    guess: (N, npars) used for every type, or (ntypes N, npars) type-major;
        None: centre 0, g = 0, r50 from the stamp's flat-weight second moments
        (less the psf stamp's) -- for 'dev10' and 'bdf' that T itself --,
        nu = 0.5 | beta = 2.5 | fracdev = 0.5, flux D^(0)
    weight: 'flat' or 'noise', as from_metacal
    psf='dilate-exact' serves the `*_psf` types too; fixnoise is not served.

    Returns {type: KSpaceBatchFitter.go's dict of the type's N objects, with
    'mcal_flags' (N,) added}: what shear_response and mean_shear take.
    """
    from .kfit import KStampBatch, KSpaceBatchFitter, MODEL_NLOC, MIX_MODELS
    torch = _torch()
    kb = KStampBatch.from_metacal(stamps, psf_stamps, types=types, step=step, psf=psf,
                                  target_sigma=target_sigma, weight=weight, fixnoise=fixnoise,
                                  rng=rng)
    ntypes, n = len(kb.types), stamps.n
    fitter = KSpaceBatchFitter(model, prior=prior, fit_pars=fit_pars, size_type=size_type)
    npars = MODEL_NLOC[model]
    if guess is None:
        d_guess = torch.zeros((ntypes * n, npars), dtype=torch.float64, device=kb.device)
        size = _flat_moment_T if model in MIX_MODELS else _flat_moment_r50
        d_guess[:, 4] = size(stamps, psf_stamps).repeat(ntypes)
        if npars == 7:
            d_guess[:, 5] = 2.5 if model == "moffat" else 0.5
        flux = kb.dhat[:, 0, 0, 0]
        d_guess[:, npars - 1] = torch.where(torch.isfinite(flux), flux, torch.ones_like(flux))
        guess = d_guess
    else:
        guess = np.asarray(guess, dtype=np.float64)
        if guess.shape == (n, npars):
            guess = np.tile(guess, (ntypes, 1))
        if guess.shape != (ntypes * n, npars):
            raise ValueError("guess must be (%d, %d) or (%d, %d)" % (n, npars, ntypes * n, npars))
    res = fitter.go(kb, guess)
    out = {}
    for i, t in enumerate(kb.types):
        sl = slice(i * n, (i + 1) * n)
        out[t] = {k: (v if isinstance(v, str) else v[sl]) for k, v in res.items()}
        out[t]["mcal_flags"] = kb.mcal_flags[i]
    return out


def _response_column(res, key):
    if key in res:
        v = res[key]
    elif key == "g":
        v = res["pars"][:, 2:4]
    else:
        raise ValueError("the fit results have no '%s'" % key)
    v = np.asarray(v, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 2:
        raise ValueError("'%s' must be (N, 2), got %s" % (key, v.shape))
    return v


def shear_response(resdict, step=DEFAULT_STEP, key="g"):
    """
    The finite-difference shear response of every object from the five fits
    of metacal_bootstrap_batch (or any dict {type: {key: (N, 2), 'flags': (N,)
    [, 'mcal_flags': (N,)]}}).

    Returns {'g': (N, 2) noshear's `key`, 'R': (N, 2, 2) with R[:, i, j] =
    (res[jp][key][:, i] - res[jm][key][:, i]) / (2 step), 'flags': (N,) the OR
    of the five types' fit flags and metacal flags}; the rows of flagged
    objects are NaN.

    When resdict also holds all four of `1p_psf, 1m_psf, 2p_psf, 2m_psf`
    (psf='dilate-exact'), the dict has 'Rpsf' too, the psf response (N, 2, 2)
    with Rpsf[:, i, j] = (res[jp_psf][key][:, i] - res[jm_psf][key][:, i]) /
    (2 step), and their flags are ORed in.  With fewer of them the dict is the
    one above.
    """
    step = float(step)
    if not step > 0:
        raise ValueError("step must be positive")
    missing = [t for t in METACAL_MINIMAL_TYPES if t not in resdict]
    if missing:
        raise ValueError("shear_response needs all five types; missing: %s" % (missing,))
    g0 = _response_column(resdict["noshear"], key)
    n = g0.shape[0]
    flags = np.zeros(n, dtype=np.int64)

    def _or_flags(t):
        res = resdict[t]
        for k in ("flags", "mcal_flags"):
            if k in res:
                f = np.asarray(res[k])
                if f.shape != (n,):
                    raise ValueError("type '%s': '%s' must be (%d,)" % (t, k, n))
                flags[:] |= f.astype(np.int64)
    for t in METACAL_MINIMAL_TYPES:
        _or_flags(t)
    R = np.empty((n, 2, 2))
    for j in (0, 1):
        p = _response_column(resdict["%dp" % (j + 1)], key)
        m = _response_column(resdict["%dm" % (j + 1)], key)
        if p.shape != g0.shape or m.shape != g0.shape:
            raise ValueError("the five types must hold the same objects")
        R[:, :, j] = (p - m) / (2.0 * step)
    Rpsf = None
    if all(t in resdict for t in METACAL_PSF_TYPES):
        for t in METACAL_PSF_TYPES:
            _or_flags(t)
        Rpsf = np.empty((n, 2, 2))
        for j in (0, 1):
            p = _response_column(resdict["%dp_psf" % (j + 1)], key)
            m = _response_column(resdict["%dm_psf" % (j + 1)], key)
            if p.shape != g0.shape or m.shape != g0.shape:
                raise ValueError("the psf-sheared types must hold the same objects")
            Rpsf[:, :, j] = (p - m) / (2.0 * step)
    g = g0.copy()
    bad = flags != 0
    g[bad] = np.nan
    R[bad] = np.nan
    out = {"g": g, "R": R, "flags": flags}
    if Rpsf is not None:
        Rpsf[bad] = np.nan
        out["Rpsf"] = Rpsf
    return out


def mean_shear(resp, select=None, psf_g=None):
    """
    <g> <R>^-1 over the unflagged objects of shear_response's dict -- the
    solution of <R> gamma = <g> with the 2 x 2 mean response -- and, with
    `select` (a boolean mask or an index array), over the selected ones of
    them.  No selection response is applied.

    psf_g: (N, 2) psf shapes; with the psf response 'Rpsf' of the dict (the
    four `*_psf` types, psf='dilate-exact') the psf leakage is taken out first:
    <R> gamma = <g> - <Rpsf psf_g> over the same objects.  A ValueError
    without 'Rpsf'.
    """
    if psf_g is not None:
        if "Rpsf" not in resp:
            raise ValueError("mean_shear: psf_g needs the psf response 'Rpsf' of the four "
                             "`*_psf` types (psf='dilate-exact')")
        psf_g = np.asarray(psf_g, dtype=np.float64)
        if psf_g.shape != np.asarray(resp["g"]).shape:
            raise ValueError("psf_g must be (N, 2), got %s" % (psf_g.shape,))
    flags = np.asarray(resp["flags"])
    use = flags == 0
    if select is not None:
        sel = np.asarray(select)
        mask = np.zeros(flags.shape[0], dtype=bool)
        if sel.dtype == bool:
            if sel.shape != flags.shape:
                raise ValueError("select: a mask must have one entry per object")
            mask = sel
        else:
            mask[sel] = True
        use = use & mask
    if not use.any():
        raise ValueError("mean_shear: no unflagged object is selected")
    rhs = resp["g"][use].mean(axis=0)
    if psf_g is not None:
        rhs = rhs - np.einsum("nij,nj->ni", resp["Rpsf"][use], psf_g[use]).mean(axis=0)
    return np.linalg.solve(resp["R"][use].mean(axis=0), rhs)


def _moments_measure(measure):
    from .prepsfmom import PrePSFMom
    if not isinstance(measure, PrePSFMom):
        raise ValueError("measure must be a PGaussMom, KSigmaMom or PrePSFMom instance")
    return measure


def metacal_moments_batch(stamps, psf_stamps, measure, step=DEFAULT_STEP, types=None,
                          fixnoise=False, noise=None, noise_seed=None, ids=None):
    """
    The pre-psf moments (`measure`: a PGaussMom / KSigmaMom / PrePSFMom) of the
    metacal types of a stamp batch WITHOUT the metacal images: the moment sums
    are taken in Fourier space at the sheared frequency of every mode the
    weight kernel keeps (PrePSFMom.go_metacal_batch; the target psf of the
    image route cancels exactly).

    stamps, psf_stamps: the StampBatch pair of metacal_bootstrap_batch -- one
    square shape each, one psf stamp per stamp, the same jacobian derivatives
    for every stamp and its psf stamp.  The weight of a pixel is its ierr^2.

    Returns resdict: {type: make_mom_result_batch dict with 'mcal_flags' (N,)},
    what shear_response(resdict, step, key='e') and mean_shear take.  The
    `*_psf` types are not served.

    fixnoise: sum the term of metacalibration's noise field -- turned by 90
        degrees, deconvolved by the un-turned psf, sheared, turned back -- with
        the moments, and the variance it brings with the covariance (DESIGN.md
        3.22).  The field comes from one of
    noise_seed: drawn on the device from (noise_seed, ids, pixel) over the
        batch's ierr, straight into the turned layout (ids (N,) object ids,
        default the positions in the batch): a stamp's field does not depend on
        how the catalogue is cut into batches;
    noise: (N, dim, dim) un-turned planes, numpy or device tensor, or a
        DeviceNoise.
    fixnoise=True with neither raises NotImplementedError (the host draw from
    an rng is not served); a noise source with fixnoise=False, or both, is a
    ValueError.

    A `measure` made with use_noise_image=True needs the stamps' noise images
    (DESIGN.md 3.28), which a StampBatch does not hold and this function has
    no argument for: it raises the reference's ValueError for a missing
    obs.noise.  Send them to measure.go_metacal_batch(..., noise_images=) with
    the batch's arrays, or measure observations with metacal_moments_many.
    """
    from .batch import StampBatch
    from .prepsfmom import _fixnoise_source
    noise = _fixnoise_source(fixnoise, noise, noise_seed, ids)
    _moments_measure(measure)
    types = _check_types(types, None)
    if not isinstance(stamps, StampBatch) or not isinstance(psf_stamps, StampBatch):
        raise ValueError("stamps and psf_stamps must be StampBatch objects")
    if stamps.n != psf_stamps.n:
        raise ValueError("one psf stamp per stamp: %d stamps, %d psf stamps"
                         % (stamps.n, psf_stamps.n))
    if stamps.val is None or psf_stamps.val is None or stamps.ierr is None:
        raise ValueError("stamps and psf_stamps must hold pixel data")
    shape, pshape = _one_shape(stamps, "stamps"), _one_shape(psf_stamps, "psf_stamps")
    if shape[0] != shape[1] or pshape[0] != pshape[1]:
        raise ValueError("pre-psf moments require square stamps, got %s and %s" % (shape, pshape))
    n = stamps.n
    derivs = stamps.jac[:, 2:6].cpu().numpy()
    if np.any(derivs != derivs[0]) or np.any(psf_stamps.jac[:, 2:6].cpu().numpy() != derivs[0]):
        raise ValueError("the stamps and their psf stamps must share one set of jacobian "
                         "derivatives")
    ierr = stamps.ierr.reshape(n, shape[0], shape[1])
    return measure.go_metacal_batch(
        stamps.val.reshape(n, shape[0], shape[1]), ierr * ierr, stamps.jac[:, 0:2],
        tuple(float(d) for d in derivs[0]), psf_stamps.val.reshape(n, pshape[0], pshape[1]),
        psf_stamps.jac[:, 0:2], step=step, types=types, fixnoise=fixnoise, noise=noise,
        noise_ierr=ierr if isinstance(noise, DeviceNoise) else None)


def metacal_moments_many(list_of_obs, measure, step=DEFAULT_STEP, types=None, fixnoise=False,
                         noise_seed=None, ids=None, use_noise_image=False):
    """
    metacal_moments_batch for a catalogue of Observations (each with a psf
    Observation of the same jacobian derivatives): grouped by (image size, psf
    size, derivatives) as PrePSFMom.go_many groups, each group one batch on the
    device.  Returns a list: element i is object i's {type:
    moments.make_mom_result dict with 'mcal_flags'}, its 'flags' carrying the
    metacal flag too.

    fixnoise, as in metacal_moments_batch, with the field of every object from
    noise_seed: drawn on the device from (noise_seed, ids, pixel) over
        sqrt(weight) where weight > 0 (ids: one per observation, default the
        positions in the list), or
    use_noise_image: each observation's own ob.noise, as get_all_metacal takes it.

    A `measure` made with use_noise_image=True takes the noise power of every
    mode of every object from that object's ob.noise (ValueError if one has
    none), whatever this function's own use_noise_image= says: the keyword
    chooses the fixnoise FIELD, the measure's switch the power ESTIMATE of the
    covariance.  Both may name ob.noise; then the one plane serves as field
    (turned, tapered) and as power estimate (neither), as in the reference's
    metacal, where the noise image that is sheared and added is the one the
    moments' errors are then taken from.
    """
    from .moments import make_mom_result
    from .prepsfmom import _check_obs_and_get_psf_obs, _fixnoise_source
    seeded = _fixnoise_source(fixnoise, None, noise_seed, ids, use_noise_image)
    _moments_measure(measure)
    types = _check_types(types, None)
    list_of_obs = list(list_of_obs)
    if ids is not None:
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        if ids.shape != (len(list_of_obs),):
            raise ValueError("ids must have shape (%d,)" % len(list_of_obs))
    if use_noise_image:
        for o in list_of_obs:
            if not o.has_noise():
                raise ValueError("use_noise_image=True: every observation needs a noise image")
    if measure.use_noise_image and not all(o.has_noise() for o in list_of_obs):
        raise ValueError('obs.noise must be set when use_noise_image=True')
    psfs = [_check_obs_and_get_psf_obs(o, False) for o in list_of_obs]
    groups = {}
    for i, (o, p) in enumerate(zip(list_of_obs, psfs)):
        j = o.jacobian
        key = (o.image.shape[0], p.image.shape[0], j.dvdrow, j.dvdcol, j.dudrow, j.dudcol)
        groups.setdefault(key, []).append(i)
    g = _type_shears(types, float(step))
    out = [None] * len(list_of_obs)
    for key, idx in groups.items():
        sub, psub = [list_of_obs[i] for i in idx], [psfs[i] for i in idx]
        noise = None
        if use_noise_image:
            noise = np.stack([o.noise for o in sub])
        elif seeded is not None:
            noise = DeviceNoise(seeded.seed, np.asarray(idx, dtype=np.int64) if ids is None
                                else ids[idx])
        mom, cov, flags, kernels, _ = measure.measure_arrays_sheared(
            np.stack([o.image for o in sub]), np.stack([o.weight for o in sub]),
            np.array([[o.jacobian.row0, o.jacobian.col0] for o in sub]), key[2:],
            np.stack([p.image for p in psub]),
            np.array([[p.jacobian.row0, p.jacobian.col0] for p in psub]), g, noise=noise,
            noise_images=np.stack([o.noise for o in sub]) if measure.use_noise_image else None)
        for k, i in enumerate(idx):
            out[i] = {}
            for it, t in enumerate(types):
                res = make_mom_result(mom[k, it], cov[k, it], sums_norm=kernels["fk00"])
                res["mcal_flags"] = int(flags[k, it])
                res["flags"] |= int(flags[k, it])
                out[i][t] = res
    return out


def metacal_bootstrap(obs, runner, psf_runner=None, ignore_failed_psf=True, rng=None,
                      **metacal_kws):
    """
    The reference's metacal_bootstrap (ngmix/metacal/bootstrap.py): the metacal
    observations of get_all_metacal(obs, rng=rng, **metacal_kws), then
    bootstrap(obs, runner, psf_runner, ignore_failed_psf) on each type.

    Returns (resdict, obsdict), both keyed by the metacal type.  As in the
    reference, obs.psf.meta['result'] and obs.psf.gmix of the metacal
    observations may be set by the psf runner.
    """
    from .bootstrap import bootstrap
    obsdict = get_all_metacal(obs=obs, rng=rng, **metacal_kws)
    resdict = {}
    for key, tobs in obsdict.items():
        resdict[key] = bootstrap(obs=tobs, runner=runner, psf_runner=psf_runner,
                                 ignore_failed_psf=ignore_failed_psf)
    return resdict, obsdict


class MetacalBootstrapper(object):
    """
    The reference's MetacalBootstrapper: runner / psf_runner have go(obs=obs);
    **metacal_kws go to get_all_metacal.
    """

    def __init__(self, runner, psf_runner, ignore_failed_psf=True, rng=None, **metacal_kws):
        self.runner = runner
        self.psf_runner = psf_runner
        self.ignore_failed_psf = ignore_failed_psf
        self.metacal_kws = metacal_kws
        self.rng = rng

    def go(self, obs):
        return metacal_bootstrap(obs=obs, runner=self.runner, psf_runner=self.psf_runner,
                                 ignore_failed_psf=self.ignore_failed_psf, rng=self.rng,
                                 **self.metacal_kws)

    @property
    def fitter(self):
        return self.runner.fitter


def metacal_bootstrap_many(list_of_obs, model="gauss", rng=None, metacal_kws=None,
                           **bootstrap_kws):
    """
    metacal_bootstrap for a catalogue: list_of_obs is a sequence of Observation
    / ObsList / MultiBandObsList with psf observations.  The metacal images of
    all of them are made together (get_all_metacal: one batch per stamp shape)
    and every type is fitted as one batch (pipeline.bootstrap_many(., model,
    rng=rng, **bootstrap_kws)).

    Returns a list: element i is the pair (resdict, obsdict) of object i, as
    metacal_bootstrap returns it -- resdict[type] the object's result dict
    (flags != 0 and NaN parameters where the reference raises BootPSFFailure),
    obsdict[type] its metacal observation(s).
    """
    from .pipeline import bootstrap_many
    list_of_obs = list(list_of_obs)
    if not list_of_obs:
        return []
    parts = [_flatten(o) for o in list_of_obs]
    everything = ObsList()
    for flat, _ in parts:
        for o in flat:
            everything.append(o)
    obsdict = get_all_metacal(everything, rng=rng, **(metacal_kws or {}))
    out = [({}, {}) for _ in list_of_obs]
    for t, tobs in obsdict.items():
        objs, at = [], 0
        for flat, rebuild in parts:
            objs.append(rebuild(list(tobs[at:at + len(flat)])))
            at += len(flat)
        many = bootstrap_many(objs, model=model, rng=rng, **bootstrap_kws)
        for i, o in enumerate(objs):
            out[i][0][t] = many[i]
            out[i][1][t] = o
    return out
