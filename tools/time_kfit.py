#!/usr/bin/env python3
"""
Timing of the Fourier-space fits on one GPU:
kfit_eval_kernel per launch (device events, the median of 7 after 2 warm-ups)
and whole fits per second through KSpaceBatchFitter, for N 32x32 and 48x48
stamps, 'exp' and 'spergel', each stamp with a psf transform.

    python tools/time_kfit.py [--n 100000] [--json out.json] [--model moffat] [--flux]
    python tools/time_kfit.py --metacal [--n 100000] [--json out.json]

--model moffat times 'spergel' and 'moffat' side by side (the ratio says
whether K_nu or the sums dominate); --flux adds kfit_flux_kernel per launch for
the point source and for each timed model.

--metacal times the metacal shear from Fourier-space fits
instead: the five types of N stamps, 'gauss', an explicit target width, by
KStampBatch.from_metacal + one fit (metacal_kfit_batch) against
MetacalBatch.get_all + KStampBatch.from_stamps + a fit per type on the same
stamps, both in the same run, each the median of 7 after 2 warm-ups between
device events, with the parts of either route beside the totals.

The real-space LMBatchFitter is a different model (a gaussian mixture against
a fitted psf mixture) and is not timed here; nothing gates on these figures.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ngmix_amd import _lib  # noqa: E402
from ngmix_amd.batch import _stream  # noqa: E402
from ngmix_amd.kfit import (KSpaceBatchFitter, KStampBatch, kmodel_images, MODEL_NLOC,  # noqa: E402
                            MODELS)


def make_batch(n, dim, model, seed):
    """n noisy stamps of the model itself with a gaussian psf stamp"""
    rng = np.random.RandomState(seed)
    scale = 0.263
    jac = np.zeros((n, 8))
    jac[:, 0] = (dim - 1) / 2 + rng.uniform(-0.4, 0.4, n)
    jac[:, 1] = (dim - 1) / 2 + rng.uniform(-0.4, 0.4, n)
    jac[:, 2] = jac[:, 5] = scale
    jac[:, 6], jac[:, 7] = scale * scale, scale
    r = np.arange(dim) - (dim - 1) / 2
    psf = np.exp(-0.5 * (r[:, None] ** 2 + r[None, :] ** 2) / 1.3 ** 2)
    psfs = np.broadcast_to(psf, (n, dim, dim)).copy()
    pjac = jac.copy()
    pjac[:, 0] = pjac[:, 1] = (dim - 1) / 2
    cols = [scale * rng.uniform(-0.5, 0.5, n), scale * rng.uniform(-0.5, 0.5, n),
            rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), scale * rng.uniform(1.5, 2.5, n)]
    if model == "spergel":
        cols.append(rng.uniform(0.0, 1.5, n))
    if model == "moffat":
        cols.append(rng.uniform(2.0, 4.5, n))
    cols.append(rng.uniform(50.0, 150.0, n))
    truth = np.stack(cols, axis=1)
    # the data: the model's own image plus noise
    kb0 = KStampBatch.from_images(np.zeros((n, dim, dim)), None, jac, psf_images=psfs,
                                  psf_jacobians=pjac)
    imgs = kmodel_images(kb0, truth, model) + 0.01 * torch.randn(
        (n, dim, dim), dtype=torch.float64, device="cuda",
        generator=torch.Generator(device="cuda").manual_seed(seed))
    kb = KStampBatch.from_images(imgs, torch.full_like(imgs, 1e4), jac, psf_images=psfs,
                                 psf_jacobians=pjac)
    guess = truth * (1.0 + 0.03 * rng.uniform(-1, 1, truth.shape))
    return kb, guess


def time_eval(kb, guess, model):
    L = _lib.lib()
    n, npars = guess.shape
    nsum = 28 if MODEL_NLOC[model] == 6 else 36
    d_guess = torch.from_numpy(guess).cuda()
    d_states = torch.empty(n * _lib.LM_STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(L.ngmix_lm_init_batch(p(d_states), n, npars, p(d_guess), 1e-8, 1e-8, 0.0, 100,
                                     100.0, _lib.LM_MODE_ANALYTIC, None, None, _stream()),
               "ngmix_lm_init_batch")
    sums = torch.empty((n, nsum), dtype=torch.float64, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    stats = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    ms = []
    for it in range(9):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(L.ngmix_kfit_eval_batch(p(kb.dhat), p(kb.phat), p(kb.wbar), p(kb.jac), kb.nrow,
                                           kb.ncol, n, MODELS[model], p(d_states), None, None,
                                           p(sums), p(status), p(stats), _stream()),
                   "ngmix_kfit_eval_batch")
        b.record()
        b.synchronize()
        if it >= 2:
            ms.append(a.elapsed_time(b))
    assert int((status != 0).sum()) == 0
    return float(np.median(ms))


def time_flux(kb, guess, model):
    """kfit_flux_kernel per launch; model None: the point source"""
    L = _lib.lib()
    n = guess.shape[0]
    npars = 5 if model is None else MODEL_NLOC[model] - 1
    d_pars = torch.from_numpy(np.ascontiguousarray(guess[:, :npars])).cuda()
    out = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ms = []
    for it in range(9):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(L.ngmix_kfit_flux_batch(p(kb.dhat), p(kb.phat), p(kb.wbar), p(kb.jac), kb.nrow,
                                           kb.ncol, n, _lib.KFIT_POINT if model is None
                                           else MODELS[model], p(d_pars), p(out), p(status),
                                           _stream()), "ngmix_kfit_flux_batch")
        b.record()
        b.synchronize()
        if it >= 2:
            ms.append(a.elapsed_time(b))
    assert int((status != 0).sum()) == 0
    return float(np.median(ms))


def time_fit(kb, guess, model):
    fitter = KSpaceBatchFitter(model)
    secs = []
    for it in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fitter.go(kb, guess)
        torch.cuda.synchronize()
        if it >= 1:
            secs.append(time.perf_counter() - t0)
    return float(np.median(secs)), int((res["flags"] == 0).sum()), fitter.rounds_launched


def _events_ms(fn, reps=9, warm=2):
    """fn() between two device events: the median of reps - warm after warm"""
    ms, out = [], None
    for it in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        if it >= warm:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


def time_metacal(n, dim, seed=5):
    """one row: the direct route against the route through the images"""
    from ngmix_amd import metacal
    from ngmix_amd.batch import StampBatch
    rng = np.random.RandomState(seed)
    scale = 0.263
    jac = np.zeros((n, 8))
    jac[:, 0] = (dim - 1) / 2 + rng.uniform(-0.4, 0.4, n)
    jac[:, 1] = (dim - 1) / 2 + rng.uniform(-0.4, 0.4, n)
    jac[:, 2] = jac[:, 5] = scale
    jac[:, 6], jac[:, 7] = scale * scale, scale
    pjac = jac.copy()
    pjac[:, 0] = pjac[:, 1] = (dim - 1) / 2
    r = torch.arange(dim, dtype=torch.float64, device="cuda")
    d_jac = torch.from_numpy(jac).cuda()

    def gauss(cen, sig2, flux):
        dr = r[None, :, None] - cen[:, 0, None, None]
        dc = r[None, None, :] - cen[:, 1, None, None]
        return flux[:, None, None] * torch.exp(-0.5 * (dr * dr + dc * dc) / sig2[:, None, None]) \
            / (2 * np.pi * sig2[:, None, None])
    one = torch.ones(n, dtype=torch.float64, device="cuda")
    sig_psf = 1.3
    sig2 = torch.from_numpy(sig_psf ** 2 + rng.uniform(1.5, 2.5, n) ** 2).cuda()
    flux = torch.from_numpy(rng.uniform(50.0, 150.0, n)).cuda()
    imgs = gauss(d_jac[:, 0:2], sig2, flux) + 0.01 * torch.randn(
        (n, dim, dim), dtype=torch.float64, device="cuda",
        generator=torch.Generator(device="cuda").manual_seed(seed))
    psfs = gauss(torch.from_numpy(pjac[:, 0:2]).cuda(), sig_psf ** 2 * one, one)
    sb = StampBatch.from_images(imgs, torch.full_like(imgs, 1e4), jac)
    psb = StampBatch.from_images(psfs, None, pjac)
    sigma = np.full(n, 1.1 * sig_psf * scale)
    guess = np.zeros((n, 6))
    guess[:, 4] = 2.0 * scale * 1.1774
    guess[:, 5] = flux.cpu().numpy()
    types = metacal.METACAL_MINIMAL_TYPES
    fit_pars = {"maxfev": 200}

    def direct():
        return metacal.metacal_kfit_batch(sb, psb, model="gauss", target_sigma=sigma,
                                          guess=guess, fit_pars=fit_pars)

    def spectra_only():
        return KStampBatch.from_metacal(sb, psb, target_sigma=sigma)

    def images_only():
        return metacal.MetacalBatch(sb, psb, target_sigma=sigma).get_all()

    def through_images():
        res = {}
        for t, d in images_only().items():
            kb = KStampBatch.from_stamps(d["stamps"], d["psf_stamps"])
            res[t] = KSpaceBatchFitter("gauss", fit_pars=fit_pars).go(kb, guess)
        return res

    direct_ms, a = _events_ms(direct)
    images_ms, b = _events_ms(through_images)
    from_metacal_ms, _ = _events_ms(spectra_only)
    get_all_ms, _ = _events_ms(images_only)
    ok = lambda res: int(sum((res[t]["flags"] == 0).sum() for t in types))
    dg = float(np.nanmax(np.abs(a["1p"]["g"] - b["1p"]["g"])))
    return {"metacal": True, "dim": dim, "n": n, "types": len(types),
            "direct_ms": direct_ms, "through_images_ms": images_ms,
            "from_metacal_ms": from_metacal_ms, "get_all_ms": get_all_ms,
            "direct_flags_ok": ok(a), "through_images_flags_ok": ok(b),
            "max_abs_dg_1p_between_routes": dg}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--json", default=None)
    ap.add_argument("--model", default=None, choices=["moffat"])
    ap.add_argument("--flux", action="store_true")
    ap.add_argument("--metacal", action="store_true")
    args = ap.parse_args()
    out = []
    if args.metacal:
        for dim in (32, 48):
            row = time_metacal(args.n, dim)
            print(json.dumps(row), flush=True)
            out.append(row)
            torch.cuda.empty_cache()
        if args.json:
            with open(args.json, "w") as f:
                json.dump(out, f, indent=1)
        return
    for dim in (32, 48):
        for model in ("spergel", "moffat") if args.model == "moffat" else ("exp", "spergel"):
            kb, guess = make_batch(args.n, dim, model, 5)
            ev = time_eval(kb, guess, model)
            sec, ok, rounds = time_fit(kb, guess, model)
            row = {"model": model, "dim": dim, "n": args.n, "eval_ms": ev,
                   "modes_per_stamp": dim * (dim // 2 + 1), "fit_s": sec,
                   "fits_per_s": args.n / sec, "flags_ok": ok, "rounds": rounds}
            if args.flux:
                row["flux_ms"] = time_flux(kb, guess, model)
                row["flux_point_ms"] = time_flux(kb, guess, None)
            print(json.dumps(row), flush=True)
            out.append(row)
            del kb
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
