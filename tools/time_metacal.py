"""
Time ngmix_amd.metacal on the device: N stamps of 32 x 32 and of 48 x 48, the
five metacal types, with and without fixnoise (a given noise plane).

Device events around whole get_all calls and around the spectrum kernel alone
(the C entry, same arguments), after warm-up runs; the median of the repeats.
Prints one JSON line per configuration: stamps/s of the whole call, the time
of the spectrum kernel and of the rest (inverse FFT, psf images, assembly), the
kernel's FMA rate and its fraction of the derived ceiling.

--noise times the fixnoise noise field instead: the noise kernel alone
(csrc/metacal_noise.hip), get_all(fixnoise=True) with the noise drawn on the
device, and the same with the host draw (numpy normals, scaled and uploaded).

--moments times the pre-psf moments of the five types, PGaussMom(fwhm=2.0):
the sheared-mode kernel alone (csrc/prepsf_shear.hip), metacal_moments_batch
end to end, and the two-step route for the same quantities -- get_all(
fixnoise=False), then measure_arrays on each type's images and target psf
images.  Prints nmodes, the kept modes of the kernel's plan, and the smallest
and largest of the repeats beside every median.  With --fixnoise also the
fixnoise form: its kernel alone on a turned noise plane, and
metacal_moments_batch(fixnoise=True, noise_seed=...) end to end.

--psf dilate-exact adds, after every row of the gaussian target and in the same
run, the rows of psf='dilate-exact'  with the five and with the
nine types: whole get_all calls, the two spectrum kernels alone (the images',
and the target psf's on the psf stamp's grid), and the image kernel's FMA rate
by the count of 3.19 plus (4 + 2) Rp Cp per work item for the psf's second
transform.

usage: python tools/time_metacal.py [--n 100000] [--repeats 7] [--warmup 2]
                                    [--noise | --moments [--fixnoise] |
                                     --psf dilate-exact]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_VECTOR_FMA_PER_S = 78.6e12 / 2      # MI355X vector fp64 peak, FMA = 2 flop


def fma_count(dim, planes):
    """FMAs of the spectrum kernel per stamp and type: every work item (the
    half plane plus the partners of the Nyquist row and column) walks every
    pixel: 4 for the phase recurrence, 2 per plane (image, psf, noise)"""
    items = dim * (dim // 2 + 1) + (dim // 2 + 1) + dim - 1
    return items * dim * dim * (4 + 2 * planes)


def dilate_fma_count(dim, pdim, planes):
    """fma_count plus the psf plane's transform at the target frequency, with a
    recurrence of its own: (4 + 2) Rp Cp per work item"""
    items = dim * (dim // 2 + 1) + (dim // 2 + 1) + dim - 1
    return fma_count(dim, planes) + items * pdim * pdim * (4 + 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--noise", action="store_true",
                    help="time the fixnoise noise field instead: the noise kernel alone, "
                         "get_all(fixnoise=True) with device noise, and with the host draw "
                         "and its upload")
    ap.add_argument("--moments", action="store_true",
                    help="time the pre-psf moments of the five types instead: the sheared-mode "
                         "kernel alone, metacal_moments_batch, and get_all + measure_arrays")
    ap.add_argument("--fixnoise", action="store_true",
                    help="with --moments: also the fixnoise kernel alone and "
                         "metacal_moments_batch(fixnoise=True, noise_seed=...)")
    ap.add_argument("--psf", choices=["fitgauss", "dilate-exact"], default="fitgauss",
                    help="dilate-exact: after each row of the gaussian target, the same "
                         "configuration with the psf's own dilated image as the target, five "
                         "and nine types")
    args = ap.parse_args()
    import torch
    from ngmix_amd import metacal
    from ngmix_amd.batch import StampBatch
    assert torch.cuda.is_available(), "time_metacal needs the device"
    dev = torch.device("cuda", 0)
    n = args.n

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        times = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e-3)
        timed.spread = (float(min(times)), float(max(times)))
        return float(np.median(times))

    for dim in (32, 48):
        gen = torch.Generator(device=dev)
        gen.manual_seed(dim)
        scale = 0.263
        r = torch.arange(dim, dtype=torch.float64, device=dev) - (dim - 1) / 2.0
        cen = torch.rand((n, 2), generator=gen, dtype=torch.float64, device=dev) - 0.5
        rr = (r[None, :, None] - cen[:, 0, None, None]) * scale
        cc = (r[None, None, :] - cen[:, 1, None, None]) * scale
        images = 100.0 * torch.exp(-0.5 * (rr * rr + cc * cc) / 0.35) + \
            torch.randn((n, dim, dim), generator=gen, dtype=torch.float64, device=dev)
        rr, cc = r[None, :, None] * scale, r[None, None, :] * scale
        psfs = torch.exp(-0.5 * (rr * rr + cc * cc) / 0.35 ** 2).expand(n, dim, dim).contiguous()
        noise = torch.randn((n, dim, dim), generator=gen, dtype=torch.float64, device=dev)
        jac = np.tile([0.0, 0.0, scale, 0.0, 0.0, scale, scale ** 2, scale], (n, 1))
        jac[:, 0:2] = (dim - 1) / 2.0 + cen.cpu().numpy()
        pjac = jac.copy()
        pjac[:, 0:2] = (dim - 1) / 2.0
        sb = StampBatch.from_images(images, torch.ones_like(images), jac)
        psb = StampBatch.from_images(psfs, None, pjac)
        mc = metacal.MetacalBatch(sb, psb, target_sigma=np.full(n, 0.4),
                                  rng=np.random.RandomState(dim))
        if args.noise:
            # (the kernel reads 8 B and writes 8 B per pixel)
            kernel = timed(lambda: mc.device_noise(12345))
            turned = timed(lambda: mc.device_noise(12345, rotated=True))
            fused = timed(lambda: mc.get_all(fixnoise=True, noise=metacal.DeviceNoise(12345)))
            two_step = timed(lambda: mc.get_all(fixnoise=True, noise=mc.device_noise(12345)))
            host = timed(lambda: mc.get_all(fixnoise=True))
            given = timed(lambda: mc.get_all(fixnoise=True, noise=noise))
            nbytes = 16.0 * n * dim * dim
            print(json.dumps({
                "stamp": dim, "n": n, "noise_kernel_ms": kernel * 1e3,
                "noise_kernel_rotated_ms": turned * 1e3,
                "noise_kernel_GB_per_s": nbytes / kernel * 1e-9,
                "get_all_device_noise_ms": fused * 1e3,
                "get_all_device_noise_two_step_ms": two_step * 1e3,
                "get_all_host_draw_ms": host * 1e3, "get_all_given_noise_ms": given * 1e3,
            }), flush=True)
            continue
        if args.moments:
            print(json.dumps(_moments(mc, sb, psb, dim, scale, timed, args.fixnoise)), flush=True)
            continue
        for fixnoise in (False, True):
            planes = 3 if fixnoise else 2
            total = timed(lambda: mc.get_all(fixnoise=fixnoise, noise=noise if fixnoise else None))
            # the kernel alone: _run's launch with the transforms after it stubbed out
            g = metacal._type_shears(metacal.METACAL_MINIMAL_TYPES, 0.01)
            kernel = timed(lambda: _spectrum_only(mc, g, noise if fixnoise else None))
            fma = fma_count(dim, planes) * 5 * n
            print(json.dumps({
                "stamp": dim, "n": n, "fixnoise": fixnoise, "types": 5,
                "stamps_per_s": n / total, "total_ms": total * 1e3,
                "spectrum_kernel_ms": kernel * 1e3, "rest_ms": (total - kernel) * 1e3,
                "kernel_fma_per_s": fma / kernel,
                "fraction_of_fp64_vector_fma_peak": fma / kernel / FP64_VECTOR_FMA_PER_S,
            }), flush=True)
            if args.psf != "dilate-exact":
                continue
            md = metacal.MetacalBatch(sb, psb, psf="dilate-exact", rng=np.random.RandomState(dim))
            for types in (metacal.METACAL_MINIMAL_TYPES, metacal.METACAL_TYPES):
                nt = len(types)
                total = timed(lambda: md.get_all(types=types, fixnoise=fixnoise,
                                                 noise=noise if fixnoise else None))
                kernel = timed(lambda: _dilate_spectrum_only(md, types, noise if fixnoise else None,
                                                             False))
                pkernel = timed(lambda: _dilate_spectrum_only(md, types, None, True))
                fma = dilate_fma_count(dim, dim, planes) * nt * n
                print(json.dumps({
                    "psf": "dilate-exact", "stamp": dim, "n": n, "fixnoise": fixnoise,
                    "types": nt, "stamps_per_s": n / total, "total_ms": total * 1e3,
                    "spectrum_kernel_ms": kernel * 1e3, "psf_spectrum_kernel_ms": pkernel * 1e3,
                    "rest_ms": (total - kernel - pkernel) * 1e3, "kernel_fma_per_s": fma / kernel,
                    "fraction_of_fp64_vector_fma_peak": fma / kernel / FP64_VECTOR_FMA_PER_S,
                }), flush=True)


def _moments(mc, sb, psb, dim, scale, timed, fixnoise=False):
    """the three timings of --moments for one stamp size, and with fixnoise the
    two of the fixnoise form"""
    import torch
    from ngmix_amd import _lib, metacal, prepsfmom
    from ngmix_amd.batch import _dptr, _stream
    n, dev = mc.n, mc.device
    m = prepsfmom.PGaussMom(fwhm=2.0)
    deriv = (scale, 0.0, 0.0, scale)
    D = int(dim * m.pad_factor)
    kernels = prepsfmom._kernels(m.kind, D, float(m.fwhm), deriv, float(m.fwhm_smooth))
    plan = [torch.from_numpy(a).to(dev) for a in prepsfmom._shear_plan(kernels, D)]
    nmodes = int(plan[0].numel())
    g = metacal._type_shears(metacal.METACAL_MINIMAL_TYPES, 0.01)
    d_g = torch.from_numpy(g).to(dev)
    edge = torch.from_numpy(prepsfmom._apodization_edge(dim, m.ap_rad)).to(dev)
    images = sb.val.reshape(n, dim, dim)
    weights = (sb.ierr * sb.ierr).reshape(n, dim, dim)
    cen, pcen = sb.jac[:, 0:2].contiguous(), psb.jac[:, 0:2].contiguous()
    sums = torch.empty((n, 5, 14), dtype=torch.float64, device=dev)
    flags = torch.empty((n, 5), dtype=torch.int32, device=dev)

    def kernel_only():
        st = _lib.lib().ngmix_prepsf_shear_sums_batch(
            _dptr(images), _dptr(weights), _dptr(psb.val), _dptr(cen), _dptr(pcen), _dptr(edge),
            _dptr(d_g), _lib.ptr(g), 0, _dptr(plan[0]), _dptr(plan[1]), _dptr(plan[2]),
            _dptr(plan[3]), n, 5, nmodes, dim, dim, D, deriv[0], deriv[1], deriv[2], deriv[3],
            _dptr(sums), _dptr(flags), _stream())
        _lib.check(st, "ngmix_prepsf_shear_sums_batch")

    def two_step():
        both = mc.get_all(fixnoise=False)
        for t in metacal.METACAL_MINIMAL_TYPES:
            d = both[t]
            m.measure_arrays(d["stamps"].val.reshape(n, dim, dim), weights, cen.cpu().numpy(), deriv,
                             d["psf_stamps"].val.reshape(n, dim, dim),
                             d["psf_stamps"].jac[:, 0:2].cpu().numpy())
    def spread_ms():
        return [t * 1e3 for t in timed.spread]
    kernel = timed(kernel_only)
    kernel_spread = spread_ms()
    total = timed(lambda: metacal.metacal_moments_batch(sb, psb, m))
    total_spread = spread_ms()
    parent = timed(two_step)
    # per (stamp, type): every kept mode walks every pixel of the image and the psf
    fma = float(nmodes) * dim * dim * (4 + 2 * 2) * 5 * n
    out = {"stamp": dim, "n": n, "types": 5, "fft_dim": D, "nmodes": nmodes,
           "modes_of_the_spectrum_kernel": dim * (dim // 2 + 1) + (dim // 2 + 1) + dim - 1,
           "shear_sums_kernel_ms": kernel * 1e3, "shear_sums_kernel_min_max_ms": kernel_spread,
           "metacal_moments_batch_ms": total * 1e3,
           "metacal_moments_batch_min_max_ms": total_spread,
           "get_all_then_measure_arrays_ms": parent * 1e3,
           "kernel_fma_per_s": fma / kernel,
           "fraction_of_fp64_vector_fma_peak": fma / kernel / FP64_VECTOR_FMA_PER_S}
    if not fixnoise:
        return out
    turned = mc.device_noise(12345, rotated=True)

    def fixnoise_kernel_only():
        st = _lib.lib().ngmix_prepsf_shear_fixnoise_sums_batch(
            _dptr(images), _dptr(weights), _dptr(psb.val), _dptr(turned), _dptr(cen), _dptr(pcen),
            _dptr(edge), _dptr(d_g), _lib.ptr(g), 0, _dptr(plan[0]), _dptr(plan[1]),
            _dptr(plan[2]), _dptr(plan[3]), n, 5, nmodes, dim, dim, D, deriv[0], deriv[1],
            deriv[2], deriv[3], _dptr(sums), _dptr(flags), _stream())
        _lib.check(st, "ngmix_prepsf_shear_fixnoise_sums_batch")
    fkernel = timed(fixnoise_kernel_only)
    fkernel_spread = spread_ms()
    ftotal = timed(lambda: metacal.metacal_moments_batch(sb, psb, m, fixnoise=True,
                                                         noise_seed=12345))
    # a second pass of the phase recurrence, over the noise plane and the psf
    out.update({"fixnoise_sums_kernel_ms": fkernel * 1e3,
                "fixnoise_sums_kernel_min_max_ms": fkernel_spread,
                "fixnoise_kernel_over_plain_kernel": fkernel / kernel,
                "metacal_moments_batch_fixnoise_ms": ftotal * 1e3,
                "metacal_moments_batch_fixnoise_min_max_ms": spread_ms(),
                "fixnoise_kernel_fma_per_s": 2 * fma / fkernel,
                "fixnoise_fraction_of_fp64_vector_fma_peak":
                    2 * fma / fkernel / FP64_VECTOR_FMA_PER_S})
    return out


def _spectrum_only(mc, g, noise):
    import torch
    from ngmix_amd import _lib
    from ngmix_amd.batch import _dptr, _stream
    n, (nrow, ncol), (prow, pcol) = mc.n, mc.shape, mc.psf_shape
    planes = 1 if noise is None else 2
    key = ("bufs", planes)
    if not hasattr(mc, "_time_bufs") or mc._time_bufs[0] != key:
        mc._time_bufs = (key, torch.empty((n, 5, planes, nrow, ncol // 2 + 1, 2),
                                          dtype=torch.float64, device=mc.device),
                         torch.empty((n, 5), dtype=torch.int32, device=mc.device),
                         torch.from_numpy(g).to(mc.device))
    _, spec, flags, d_g = mc._time_bufs
    st = _lib.lib().ngmix_metacal_spectrum_batch(
        _dptr(mc.stamps.val), _dptr(noise), _dptr(mc.psf_stamps.val), _dptr(mc.stamps.jac),
        _dptr(mc._psf_cen), _dptr(mc._psf_flux), _dptr(mc._sigma), _dptr(d_g), _lib.ptr(g), 0, n,
        5, nrow, ncol, prow, pcol, _dptr(spec), _dptr(flags), _stream())
    _lib.check(st, "ngmix_metacal_spectrum_batch")


def _dilate_spectrum_only(mc, types, noise, psf_only):
    """the launch of MetacalBatch._run for psf='dilate-exact': the images' spectra,
    or with psf_only the target psf's on the psf stamp's grid"""
    import torch
    from ngmix_amd import _lib, metacal
    from ngmix_amd.batch import _dptr, _stream
    n, (nrow, ncol), (prow, pcol) = mc.n, mc.shape, mc.psf_shape
    nt = len(types)
    planes = 1 if noise is None else 2
    key = ("dilate", nt, planes, psf_only)
    if not hasattr(mc, "_time_bufs") or mc._time_bufs[0] != key:
        g = metacal._type_shears(types, 0.01)
        dil = np.full(nt, 1.02)
        kind = metacal._type_kinds(types)
        shape = (n, nt, prow, pcol // 2 + 1, 2) if psf_only else \
            (n, nt, planes, nrow, ncol // 2 + 1, 2)
        mc._time_bufs = (key, torch.empty(shape, dtype=torch.float64, device=mc.device),
                         torch.empty((n, nt), dtype=torch.int32, device=mc.device), (g, dil, kind),
                         [torch.from_numpy(a).to(mc.device) for a in (g, dil, kind)])
    _, spec, flags, (g, dil, kind), (d_g, d_dil, d_kind) = mc._time_bufs
    L = _lib.lib()
    if psf_only:
        st = L.ngmix_metacal_dilate_psf_spectrum_batch(
            _dptr(mc.psf_stamps.val), _dptr(mc.psf_stamps.jac), _dptr(mc._psf_cen), _dptr(d_g),
            _dptr(d_dil), _dptr(d_kind), _lib.ptr(g), _lib.ptr(dil), _lib.ptr(kind), 0, n, nt, prow,
            pcol, _dptr(spec), _dptr(flags), _stream())
    else:
        st = L.ngmix_metacal_dilate_spectrum_batch(
            _dptr(mc.stamps.val), _dptr(noise), _dptr(mc.psf_stamps.val), _dptr(mc.stamps.jac),
            _dptr(mc._psf_cen), _dptr(d_g), _dptr(d_dil), _dptr(d_kind), _lib.ptr(g), _lib.ptr(dil),
            _lib.ptr(kind), 0, n, nt, nrow, ncol, prow, pcol, _dptr(spec), _dptr(flags), _stream())
    _lib.check(st, "ngmix_metacal_dilate_spectrum_batch")


if __name__ == "__main__":
    main()
