#!/usr/bin/env python3
"""
Timing of the Fourier-space fits on one GPU:
kfit_eval_kernel per launch (device events, the median of 7 after 2 warm-ups)
and whole fits per second through KSpaceBatchFitter, for N 32x32 and 48x48
stamps, 'exp' and 'spergel', each stamp with a psf transform.

    python tools/time_kfit.py [--n 100000] [--json out.json] [--model moffat] [--flux]

--model moffat times 'spergel' and 'moffat' side by side (the ratio says
whether K_nu or the sums dominate); --flux adds kfit_flux_kernel per launch for
the point source and for each timed model.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--json", default=None)
    ap.add_argument("--model", default=None, choices=["moffat"])
    ap.add_argument("--flux", action="store_true")
    args = ap.parse_args()
    out = []
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
