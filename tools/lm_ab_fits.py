"""Final pars / nfev / ier of seeded LM fits, for comparing two builds of the
library: 'exp' over 1, 2, 3, 4, 5 and 9 bands (6, 7, 8, 9, 10, 14 parameters),
65 objects, 4 seeds, lmder and lmdif, the form the launcher picks and the
run-time form, a quarter of the guesses poor.
usage: NGMIX_HIP_LIB=<library A> python tools/lm_ab_fits.py dump a.npz
       NGMIX_HIP_LIB=<library B> python tools/lm_ab_fits.py dump b.npz
       python tools/lm_ab_fits.py compare a.npz b.npz     (exit status 1 if any byte differs)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

if sys.argv[1] == "compare":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    assert sorted(a.files) == sorted(b.files)
    bad = [k for k in a.files if a[k].tobytes() != b[k].tobytes()]
    print("lm_ab_fits: %d arrays compared as bytes, %d differ %s" % (len(a.files), len(bad), bad[:5]))
    sys.exit(1 if bad else 0)

from test_gpu_lm_team import _multiband  # noqa: E402
from ngmix_amd.lm_batch import LMBatchFitter  # noqa: E402

out = {}
for seed in range(4):
    for nband in (1, 2, 3, 4, 5, 9):
        for fd in (False, True):
            rng = np.random.RandomState(1000 * seed + nband)
            sb, psf, guess, sobj, sband = _multiband(65, nband, "exp", rng)
            guess[::4, 4:] *= 1.6
            guess[::6, 2:4] = 0.4, -0.3
            for hint in (True, False):
                f = LMBatchFitter("exp", analytic_jacobian=not fd)
                f.advance_hint = hint
                r = f.go(sb, guess, psf=psf, stamp_obj=sobj, stamp_band=sband)
                for k in ("pars", "nfev", "ier"):
                    out["s%d_b%d_fd%d_h%d_%s" % (seed, nband, fd, hint, k)] = np.asarray(r[k])
np.savez(sys.argv[2], **out)
print("lm_ab_fits: %d arrays -> %s" % (len(out), sys.argv[2]))
