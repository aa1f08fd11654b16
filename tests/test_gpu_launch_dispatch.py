"""
The launchers' dispatch (csrc/launch_util.hpp: a table row or a template list
picks the instantiation and its census name): every branch of the pixel-pass,
lmder-step, lm_eval and fused-EM dispatch is walked once at the smallest shapes
that reach it, and after each call the launch census must hold exactly the
expected name.  The names are what the census has always called these kernels.
(The NGMIX_LM_JBASIS forms of lm_eval_kernel are not walked: the knob is read
once per process.)
"""
import numpy as np
import pytest
import torch

import ngmix_amd as ngmix
from ngmix_amd import _lib
from ngmix_amd.batch import StampBatch, GMixBatch
from ngmix_amd.lm_batch import LMBatchFitter

from test_gpu_lm_team import _rounds, _assert_same_rounds, _multiband

pytestmark = pytest.mark.gpu


def _stamps(dim, masked, rng, n=3):
    pars = np.zeros((n, 6))
    pars[:, 0:2] = rng.uniform(-0.1, 0.1, size=(n, 2))
    pars[:, 2:4] = rng.normal(scale=0.1, size=(n, 2))
    pars[:, 4] = rng.uniform(0.3, 1.0, size=n)
    pars[:, 5] = rng.uniform(50, 500, size=n)
    gm0, _ = GMixBatch.from_pars(pars, "exp")
    psf, _ = GMixBatch.from_pars(np.tile([0.0, 0.0, 0.0, 0.0, 0.27, 1.0], (n, 1)), "gauss")
    gm, _ = gm0.convolve(psf)
    images = rng.normal(size=(n, dim, dim))
    weights = rng.uniform(0.5, 2.0, size=(n, dim, dim))
    if masked:
        weights[:, dim // 3, dim // 4:dim // 2] = 0.0
    c = (dim - 1) / 2.0
    jac = np.array([c, c, 0.263, 0.0, 0.0, 0.263, 0.263 ** 2, 0.263])
    return StampBatch.from_images(images, weights, jac), gm


def _one(call):
    """the census of one call: exactly one kernel variant, launched once"""
    _lib.launch_census(reset=True)
    res = call()
    torch.cuda.synchronize()
    seen = _lib.launch_census(reset=True)
    assert len(seen) == 1 and list(seen.values()) == [1], seen
    return list(seen)[0], res


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("dim", [8, 33])
def test_pixpass_dispatch(dim, masked):
    """loglike, fdiff, s2n and render: the fused kernels with and without
    stream_ierr (bitwise equal), the overwriting render, and the exact kernels
    (K = 4 tiles per wave up to 1024 pixels, 9 beyond: 8 x 8 and 33 x 33)"""
    rng = np.random.RandomState(dim + masked)
    sb, gm = _stamps(dim, masked, rng)
    passes = {
        "loglike": (lambda **kw: sb.loglike(gm, **kw), "pixpass_wave_kernel7<loglike>"),
        "fdiff": (lambda **kw: sb.fill_fdiff(gm, **kw), "pixpass_wave_kernel<fdiff>"),
        "s2n": (lambda **kw: sb.model_s2n_sum(gm, **kw), "pixpass_wave_kernel<s2n>"),
    }
    for op, (run, fused_name) in passes.items():
        sb.stream_ierr = False
        name, (a, st) = _one(run)
        assert name == fused_name, (op, name)
        assert int(st.abs().sum()) == 0
        sb.stream_ierr = True
        name, (b, st) = _one(run)
        assert name == fused_name, (op, name)
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), op
        sb.stream_ierr = False
        name, (x, st) = _one(lambda: run(exact=True))
        assert name == "pixpass_grid_kernel<%s>" % op, (op, name)
        assert int(st.abs().sum()) == 0
    # the render: adding into an image, overwriting a fresh one, no_skip, exact
    base = torch.zeros(sb.total_pix, dtype=torch.float64, device="cuda")
    name, (added, st) = _one(lambda: sb.render(gm, image=base))
    assert name == "pixpass_wave_kernel<render>"
    name, (fresh, st) = _one(lambda: sb.render(gm))
    assert name == "pixpass_wave_kernel<render>"
    name, (full, st) = _one(lambda: sb.render(gm, no_skip=True))
    assert name == "pixpass_wave_kernel<render>"
    assert added.cpu().numpy().tobytes() == fresh.cpu().numpy().tobytes()
    assert fresh.cpu().numpy().tobytes() == full.cpu().numpy().tobytes()
    for fast in (True, False):
        name, _ = _one(lambda: sb.render(gm, fast_exp=fast, exact=True))
        assert name == "pixpass_grid_kernel<render>"
    name, _ = _one(lambda: sb.render(gm, fast_exp=False))      # true exp: no fused form
    assert name == "pixpass_grid_kernel<render>"


def _advance_names(seen):
    return sorted(k for k in seen if k.startswith("lm_advance"))


@pytest.fixture(scope="module")
def band_fits():
    """'exp' over 1, 2, 3, 4, 5, 7 and 9 bands: 6, 7, 8, 9, 10, 12 and 14
    parameters; the generic form's rounds of each, computed once"""
    fits = {}
    for nband in (1, 2, 3, 4, 5, 7, 9):
        rng = np.random.RandomState(40 + nband)
        sb, psf, guess, sobj, sband = _multiband(4, nband, "exp", rng)

        def go(f, sb=sb, psf=psf, guess=guess, sobj=sobj, sband=sband):
            return f.go(sb, guess, psf=psf, stamp_obj=sobj, stamp_band=sband)
        _, generic = _rounds(LMBatchFitter("exp"), go, False)
        fits[5 + nband] = (go, generic)
    return fits


def _step_names(go, hint=True):
    _lib.launch_census(reset=True)
    _, snaps = _rounds(LMBatchFitter("exp"), go, hint)
    return _advance_names(_lib.launch_census(reset=True)), snaps


@pytest.mark.parametrize("npars", [6, 7, 8])
def test_lm_advance_register_form(npars, band_fits, monkeypatch):
    monkeypatch.delenv("NGMIX_LM_TEAM_MIN", raising=False)
    go, generic = band_fits[npars]
    names, snaps = _step_names(go)
    assert names == ["lm_advance_kernel<%d, true>" % npars], names
    _assert_same_rounds(snaps, generic)


@pytest.mark.parametrize("teams", [1, 2, 4])
@pytest.mark.parametrize("npars, built", [(9, 10), (10, 10), (12, 12), (14, 14)])
def test_lm_advance_team_form(npars, built, teams, band_fits, monkeypatch):
    monkeypatch.delenv("NGMIX_LM_TEAM_MIN", raising=False)
    monkeypatch.setenv("NGMIX_LM_TEAMS", str(teams))
    go, generic = band_fits[npars]
    names, snaps = _step_names(go)
    assert names == ["lm_advance_team_kernel<%d, %d>" % (teams, built)], names
    _assert_same_rounds(snaps, generic)


@pytest.mark.parametrize("npars", [9, 10])
def test_lm_advance_team_min_sends_9_and_10_to_the_register_form(npars, band_fits, monkeypatch):
    monkeypatch.setenv("NGMIX_LM_TEAM_MIN", "11")
    go, generic = band_fits[npars]
    names, snaps = _step_names(go)
    assert names == ["lm_advance_kernel<%d, true>" % npars], names
    _assert_same_rounds(snaps, generic)


def test_lm_advance_generic_form_and_count_not_said(band_fits, monkeypatch):
    monkeypatch.delenv("NGMIX_LM_TEAM_MIN", raising=False)
    monkeypatch.delenv("NGMIX_LM_TEAMS", raising=False)
    go, generic = band_fits[8]
    names, snaps = _step_names(go, hint=False)
    assert names == ["lm_advance_kernel<14, false>"], names
    _assert_same_rounds(snaps, generic)
    # the count not said (hint 0): the team form built for 14 parameters
    f = LMBatchFitter("exp")
    f._nloc_npars = lambda npars: f.nloc
    _lib.launch_census(reset=True)
    f.host_loop = True
    snaps = []
    from test_gpu_lm_team import _live

    def hook(job, r):
        torch.cuda.synchronize()
        rec = job.d_states.cpu().numpy().view(_lib.LM_STATE_DTYPE).reshape(-1)
        snaps.append(_live(rec))
    f.round_hook = hook
    go(f)
    names = _advance_names(_lib.launch_census(reset=True))
    assert names == ["lm_advance_team_kernel<4, 14>"], names
    _assert_same_rounds(snaps, generic)


# ---------------------------------------------------------------- lm_eval

def _eval_names(seen):
    return sorted(k for k in seen if k.startswith("lm_eval"))


def _small_fit(model, rng, dim=9, n=3, analytic=True):
    """(fitter, go) of n fits on dim x dim stamps: 'gauss' (6 local parameters),
    'bdf' (7) or ('coellip', ngauss) (4 + 2 ngauss)"""
    scale = 0.263
    c = (dim - 1) / 2.0
    jac = ngmix.DiagonalJacobian(row=c, col=c, scale=scale)
    fp = {"maxfev": 30, "ftol": 1e-5, "xtol": 1e-5}
    if isinstance(model, tuple):
        ngauss = model[1]
        gm = ngmix.GMixModel([0.0, 0.0, 0.02, -0.01, 0.3, 1.0], "turb")
        im0 = gm.make_image((dim, dim), jacobian=jac)
        images = im0[None] + 2.0e-4 * rng.normal(size=(n, dim, dim))
        sb = StampBatch.from_images(images, np.full((n, dim, dim), 1.0 / 2.0e-4 ** 2), jac)
        T = 0.3 * np.array([0.3, 0.7, 1.5, 3.0, 6.0])[:ngauss]
        F = np.array([0.25, 0.35, 0.25, 0.1, 0.05])[:ngauss]
        g0 = np.concatenate([[0.0, 0.0, 0.02, -0.01], T, F / F.sum()])
        guess = g0[None] * rng.uniform(0.9, 1.1, size=(n, g0.size))

        def make():
            return LMBatchFitter("coellip", ngauss=ngauss, fit_pars=fp)
        return make, lambda f: f.go(sb, guess)
    gm = ngmix.GMixModel([0.0, 0.0, 0.05, -0.03, 0.4, 100.0], "gauss")
    im0 = gm.make_image((dim, dim), jacobian=jac)
    images = im0[None] + 0.01 * rng.normal(size=(n, dim, dim))
    sb = StampBatch.from_images(images, np.full((n, dim, dim), 1.0e4), jac)
    guess = np.tile([0.0, 0.0, 0.05, -0.03, 0.15, 100.0], (n, 1)) * rng.uniform(0.95, 1.05, (n, 6))
    psf, _ = GMixBatch.from_pars(np.tile([0.0, 0.0, 0.0, 0.0, 0.25, 1.0], (n, 1)), "gauss")
    if model == "bdf":
        guess = np.concatenate([guess[:, :5], np.full((n, 1), 0.5), guess[:, 5:]], axis=1)
    return ((lambda: LMBatchFitter(model, fit_pars=fp, analytic_jacobian=analytic)),
            (lambda f: f.go(sb, guess, psf=psf)))


@pytest.mark.parametrize("tiles, tail", [("2d", ""), ("linear", ", linear")])
@pytest.mark.parametrize("model, nloc", [("gauss", 6), (("coellip", 1), 6), ("bdf", 7),
                                         (("coellip", 2), 8), (("coellip", 3), 10),
                                         (("coellip", 4), 12), (("coellip", 5), 14)])
def test_lm_eval_fd_dispatch(model, nloc, tiles, tail, monkeypatch):
    """the forward-difference pixel pass on 9 x 9 stamps, both tile forms; from
    ten local parameters on the fit ends with the precise pass"""
    monkeypatch.setenv("NGMIX_LM_FD_TILES", tiles)
    monkeypatch.delenv("NGMIX_LM_NO_PRECISE_COV", raising=False)
    make, go = _small_fit(model, np.random.RandomState(nloc), analytic=False)
    _lib.launch_census(reset=True)
    go(make())
    torch.cuda.synchronize()
    names = _eval_names(_lib.launch_census(reset=True))
    want = ["lm_eval_fd_kernel<%d%s>" % (nloc, tail)]
    if nloc >= 10:
        want.append("lm_eval_fd_kernel<%d%s, precise>" % (nloc, tail))
    assert names == sorted(want), names


@pytest.mark.parametrize("dim, name", [(9, "lm_eval_kernel<true, true>"),
                                       (264, "lm_eval_kernel<false, true>")])
def test_lm_eval_analytic_dispatch(dim, name):
    """the analytic pass with its tile records in LDS, and on a stamp of more
    tiles (264 x 264: 1089) than records fit"""
    make, go = _small_fit("gauss", np.random.RandomState(dim), dim=dim, n=2)
    _lib.launch_census(reset=True)
    go(make())
    torch.cuda.synchronize()
    assert _eval_names(_lib.launch_census(reset=True)) == [name]


# ---------------------------------------------------------------- fused EM

def _em_stamps(dim, rng, nst=2, sky=0.01):
    scale = 0.263
    obs, Ts = [], []
    for k in range(nst):
        jac = ngmix.DiagonalJacobian(row=(dim - 1) / 2.0 + rng.uniform(-0.4, 0.4),
                                     col=(dim - 1) / 2.0 + rng.uniform(-0.4, 0.4), scale=scale)
        T = 0.3 + 0.01 * dim * rng.uniform(0.8, 1.2)
        gm = ngmix.GMixModel([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05),
                              rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), T, 30.0], "dev")
        im = gm.make_image((dim, dim), jacobian=jac) + sky
        im += 0.001 * rng.normal(size=im.shape)
        wt = np.full(im.shape, 1.0 / 0.001 ** 2)
        if k % 2:
            wt[dim // 4, dim // 3] = 0.0
        obs.append(ngmix.Observation(im, weight=wt, jacobian=jac))
        Ts.append(T)
    return StampBatch.from_observations(obs), np.array(Ts)


def _em_run(sb, Ts, ngauss, npsf, kind, rng_seed, monkeypatch, nt):
    rng = np.random.RandomState(rng_seed)
    nst, scale = len(Ts), 0.263
    full = np.zeros((nst, ngauss, 6))
    for i in range(ngauss):
        full[:, i, 0] = 30.0 * scale ** 2 / ngauss * rng.uniform(0.9, 1.1, size=nst)
        full[:, i, 1:3] = rng.uniform(-0.03, 0.03, size=(nst, 2))
        full[:, i, 3] = 0.5 * Ts * (0.3 + 0.5 * i)
        full[:, i, 5] = 0.5 * Ts * (0.3 + 0.5 * i)
    gm0, _ = GMixBatch.from_pars(full.reshape(nst, -1), "full", ngauss=ngauss)
    if npsf == 1:
        psf, _ = GMixBatch.from_pars(np.tile([0.0, 0.0, 0.0, 0.0, 0.05, 1.0], (nst, 1)), "gauss")
    else:
        psf, _ = GMixBatch.from_pars(np.tile([0.0, 0.0, 0.01, -0.02, 0.06, 1.0], (nst, 1)), "turb")
    if nt is None:
        monkeypatch.delenv("NGMIX_EM_NT", raising=False)
    else:
        monkeypatch.setenv("NGMIX_EM_NT", nt)
    _lib.launch_census(reset=True)
    out, status, conv = sb.em(gm0, psf, sky=0.01, kind=kind, miniter=6, maxiter=6, tol=1e-6)
    torch.cuda.synchronize()
    seen = _lib.launch_census(reset=True)
    assert int(status.abs().sum()) == 0
    return list(seen), out.cpu().numpy(), gm0.to_numpy()


# (stamp size, psf gaussians, kinds, gaussian counts, threads, pixels per lane)
EM_CASES = [
    (16, 1, (0, 1, 2, 3), range(1, 9), 64, 16),        # one wave
    (16, 3, (0,), range(1, 9), 64, 16),                # the psf count compile-time for <= 3
    (40, 1, (0, 1, 2, 3), range(1, 9), 128, 16),       # two waves
    (48, 1, (0,), range(1, 9), 128, 18),               # the full run: 18 slots per lane
    (64, 1, (0, 1, 2, 3), range(1, 7), 256, 16),       # four waves, <= 6 gaussians
]


@pytest.mark.parametrize("dim, npsf, kinds, counts, nt, ppt", EM_CASES,
                         ids=["16", "16-turb", "40", "48-full", "64"])
def test_em_wave_dispatch(dim, npsf, kinds, counts, nt, ppt, monkeypatch):
    """every (kind, ngauss) of the fused EM kernels at each thread count, named
    exactly, against em.hip's generic kernel (NGMIX_EM_NT=256): the same
    iteration count, mixtures to the 1e-9 of test_gpu_iter.py's comparison"""
    sb, Ts = _em_stamps(dim, np.random.RandomState(dim))
    for kind in kinds:
        for ngauss in counts:
            cpsf = 1 if npsf == 1 else (3 if ngauss <= 3 and nt == 64 else 0)
            seed = 1000 * dim + 10 * ngauss + kind
            seen, o1, g1 = _em_run(sb, Ts, ngauss, npsf, kind, seed, monkeypatch, None)
            assert seen == ["em_wave_kernel<%d, %d, %d, %d, %d>" % (nt, ppt, kind, ngauss, cpsf)]
            seen, o2, g2 = _em_run(sb, Ts, ngauss, npsf, kind, seed, monkeypatch, "256")
            assert len(seen) == 1 and seen[0].startswith("em_grid_kernel<256, "), seen
            np.testing.assert_array_equal(o1[:, 0], o2[:, 0])
            np.testing.assert_allclose(o1[:, 2], o2[:, 2], rtol=1e-9)
            for f in ("p", "row", "col", "irr", "irc", "icc"):
                np.testing.assert_allclose(g1[f], g2[f], rtol=1e-9, atol=1e-11,
                                           err_msg="%s kind %d ngauss %d" % (f, kind, ngauss))
