"""
The host twins of the Fourier-space 'dev10' and 'bdf' fits:
ngmix_kfit_eval_host, ngmix_kfit_flux_host and their mode-weight forms against
the dense longdouble reference built from the pixel-space mixtures' covariance
matrices (tests/helpers/kfit_mix_reference.py), the special parameter points,
the refusals, and the agreement with the rendered pixel-space model.  No GPU.
"""
import numpy as np
import pytest

from ngmix_amd import _lib

from helpers import kfit_cases as KC
from helpers import kfit_mix_cases as MC
from helpers import kfit_mix_reference as MR
from helpers import kfit_reference as K

KEYS = sorted(MC.sums_cases())
MODEL_DEV, MODEL_BDF = 4, 6         # NGMIX_MODEL_DEV, NGMIX_MODEL_BDF


def test_the_helpers_tables_are_the_librarys():
    """ngmix_fill_model's 'dev' and 'bdf' mixtures at g = 0: amplitudes and
    traces of the helper's components, to two roundings"""
    L = _lib.lib()
    for model, pars, mid in ((MODEL_DEV, [0.0, 0.0, 0.0, 0.0, 3.0, 1.0], MR.DEV10),
                             (MODEL_BDF, [0.0, 0.0, 0.0, 0.0, 3.0, 0.3, 1.0], MR.BDF)):
        pars = np.array(pars)
        gm = np.zeros(10 if mid == MR.DEV10 else 16, dtype=_lib.GAUSS2D_DTYPE)
        assert L.ngmix_fill_model(_lib.ptr(gm), gm.size, model, _lib.ptr(pars), pars.size) == 0
        comps = MR.components(mid, K.LD(0), K.LD(0), K.LD(3), K.LD(0.3))
        np.testing.assert_allclose(gm["p"], [float(c[0]) for c in comps], rtol=4e-16)
        np.testing.assert_allclose(gm["irr"] + gm["icc"], [float(c[1] + c[3]) for c in comps],
                                   rtol=1e-15)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "modew"])
@pytest.mark.parametrize("key", KEYS, ids=str)
def test_sums_against_the_dense_reference(key, weighted):
    """every stamp of the group within C_ROUND * 2^-52 * sum |terms|, the
    statistics too; with mode weights, the counted components"""
    sts = MC.sums_cases()[key]
    refs = MC.references(weighted)[key]
    sums, status, stats, ncomp = MC.eval_host(sts, KC.host_states(MC.trial_points(sts)), weighted)
    assert np.all(status == 0)
    ws, wt = MC.worst_of_group(sums, stats, refs)
    print("kfit mix host %s %s worst %.2f (stats %.2f) of 2^-52 sum|terms|"
          % (key, "modew" if weighted else "plain", ws, wt))
    assert ws <= MC.C_ROUND and wt <= MC.C_ROUND
    if weighted:
        assert list(ncomp) == [r["ncomp"] for r in refs]


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "modew"])
@pytest.mark.parametrize("key", KEYS, ids=str)
def test_flux_sums_against_the_dense_reference(key, weighted):
    sts = MC.sums_cases()[key]
    refs = MC.flux_references(weighted)[key]
    out, status = MC.flux_host(sts, MC.trial_points(sts)[:, :MR.NLOC[key[0]] - 1], weighted)
    assert np.all(status == 0)
    worst = max(KC.worst_ratio(out[i], r[0], r[1]) for i, r in enumerate(refs))
    print("kfit mix flux host %s worst %.2f of 2^-52 sum|terms|" % (key, worst))
    assert worst <= MC.C_FLUX


def _dev_twin(st, tau):
    tw = dict(st)
    tw["model"] = MR.DEV10
    tw["p"] = np.concatenate([st["p"][:4], [st["p"][4] * tau], st["p"][6:]])
    return tw


def test_bdf_at_fracdev_one_is_dev10_at_T_tau():
    """every entry that does not involve fracdev; the T column carries tau, the
    factor between the two models' T"""
    worst = 0.0
    tau = float(1 / MR.tau_denominator(K.LD(1)))
    for key in [k for k in KEYS if k[0] == MR.BDF]:
        st = MC.sums_cases()[key][MC.FRACDEVS.index(1.0)]
        assert st["p"][5] == 1.0
        tw = _dev_twin(st, tau)
        sb, _, tb, _ = MC.eval_host([st], KC.host_states(st["p"][None]))
        sd, _, td, _ = MC.eval_host([tw], KC.host_states(tw["p"][None]))
        ref = MR.stamp_sums(MR.DEV10, tw["p"], tw["md"], K.from_interleaved(tw["dhat"]),
                            MC.phat_of(tw), tw["wbar"])
        # dev10's entries out of bdf's: drop parameter 5, scale parameter 4's by tau
        idx7 = [(i, j) for i in range(7) for j in range(i, 7)]
        pick = [k for k, (i, j) in enumerate(idx7) if 5 not in (i, j)]
        scale = [tau ** ((i == 4) + (j == 4)) for (i, j) in idx7 if 5 not in (i, j)]
        pick += [28 + i for i in range(7) if i != 5] + [35]
        scale += [tau if i == 4 else 1.0 for i in range(7) if i != 5] + [1.0]
        got = sb[0][pick] / np.array(scale)
        worst = max(worst, KC.worst_ratio(got, sd[0].astype(K.LD), ref["abs"]),
                    KC.worst_ratio(tb[0], td[0].astype(K.LD), ref["stats_abs"]))
    print("bdf(fracdev=1) against dev10(T tau): worst %.2f" % worst)
    assert worst <= MC.C_ROUND


def test_bdf_at_fracdev_zero_is_the_six_exp_components():
    worst = 0.0
    for key in [k for k in KEYS if k[0] == MR.BDF]:
        st = MC.sums_cases()[key][MC.FRACDEVS.index(0.0)]
        assert st["p"][5] == 0.0
        md, D = st["md"], K.from_interleaved(st["dhat"])
        T = MR.unit_model(MR.BDF, st["p"][:6], md, MC.phat_of(st), only="exp")
        keep = md["mult"] > 0
        w = (K.LD(st["wbar"]) / (md["R"] * md["C"])) * md["mult"][keep]
        rr, ii = (T.real * D.real)[keep], (T.imag * D.imag)[keep]
        B = np.sum(w * np.abs(T[keep]) ** 2)
        E = np.sum(w * np.abs(D[keep]) ** 2)
        ref = np.array([np.sum(w * (rr + ii)), B, E])
        absum = np.array([np.sum(w * (np.abs(rr) + np.abs(ii))), B, E])
        out, status = MC.flux_host([st], st["p"][None, :6])
        assert status[0] == 0
        worst = max(worst, KC.worst_ratio(out[0], ref, absum))
    print("bdf(fracdev=0) against the exp components: worst %.2f" % worst)
    assert worst <= MC.C_FLUX


@pytest.mark.parametrize("model", [MR.DEV10, MR.BDF], ids=["dev10", "bdf"])
def test_out_of_range_points_are_refused(model):
    nloc = MR.NLOC[model]
    base = MC.sums_cases()[(model, (9, 12), True)][1 if model == MR.BDF else 0]
    bad = []
    for T in (0.0, -1.0, np.nan, np.inf):
        p = base["p"].copy()
        p[4] = T
        bad.append(p)
    for g in ((0.8, 0.6), (0.8, 0.7), (np.nan, 0.0)):
        p = base["p"].copy()
        p[2:4] = g
        bad.append(p)
    for k in (0, 1, nloc - 2, nloc - 1):
        p = base["p"].copy()
        p[k] = np.nan
        bad.append(p)
    x0 = np.stack([base["p"]] + bad)
    stamps = [base] * len(x0)
    sums, status, stats, _ = MC.eval_host(stamps, KC.host_states(x0))
    assert list(status) == [0] + [_lib.ERR_G_RANGE] * len(bad)
    assert np.all(np.isfinite(sums[0]))
    for i in range(1, len(x0)):
        assert np.isposinf(sums[i, -1]) and np.all(sums[i, :-1] == 0) and np.all(stats[i] == 0)
        ref = MR.stamp_sums(model, x0[i], base["md"], None, None, 1.0)
        assert ref["status"] == _lib.ERR_G_RANGE
    out, status = MC.flux_host(stamps[:-1], x0[:-1, :nloc - 1])
    assert list(status) == [0] + [_lib.ERR_G_RANGE] * (len(bad) - 1)
    assert np.all(out[1:] == 0.0) and np.all(out[0] != 0.0)
    # fracdev itself is unrestricted
    if model == MR.BDF:
        x1 = np.stack([base["p"]] * 2)
        x1[:, 5] = -3.0, 7.5
        _, status, _, _ = MC.eval_host([base] * 2, KC.host_states(x1))
        assert list(status) == [0, 0]


def test_unknown_ids_between_the_models_stay_refused():
    sts = MC.sums_cases()[(MR.DEV10, (8, 8), False)][:1]
    states = KC.host_states(MC.trial_points(sts))
    dhat, _, wbar, jac = KC.pack_stamps(sts)
    sums = np.zeros((1, 28))
    for bad in (5, 6, 7, 10):
        assert _lib.lib().ngmix_kfit_eval_host(
            _lib.ptr(dhat), None, _lib.ptr(wbar), _lib.ptr(jac), 8, 8, 1, bad, _lib.ptr(states),
            None, None, _lib.ptr(sums), None, None) == _lib.ERR_BAD_ARG
        assert "_DEV10 or _BDF" in _lib.last_error()


# ---- agreement with the pixel-space model ----------------------------------------------
# A 32 x 32 stamp of unit pixels, GMixModel(pars, 'bdf').convolve(psf) with a round
# gaussian psf of sigma = 2 pixels and T = 4 pixel^2, rendered by the CPU oracle.
# ALIAS_MEASURED is sum w |D^ - Phi P^|^2 / sum w |D^|^2 with the helper's analytic
# Phi P^ alone (aliases of the sampled model and what the stamp's edge cuts off),
# measured once with the reference; the host twin's f.f at the truth is gated at
# ten times it.
PIX_PARS = np.array([0.2, -0.1, 0.1, -0.05, 4.0, 0.4, 100.0])
PSF_SIGMA = 2.0
ALIAS_MEASURED = 8.64e-14


def test_agreement_with_the_rendered_pixel_space_model():
    from ngmix_amd.gmix import GMixModel
    from oracle import oracle as ora
    shape = (32, 32)
    deriv = (1.0, 0.0, 0.0, 1.0)
    cen = (15.5, 15.5)
    psf = GMixModel([0.0, 0.0, 0.0, 0.0, 2.0 * PSF_SIGMA ** 2, 1.0], "gauss")
    gm = GMixModel(PIX_PARS, "bdf").convolve(psf)
    gm.set_norms_if_needed()
    data = gm.get_data()
    g = np.zeros(data.size, dtype=ora.GAUSS2D_DTYPE)
    for name in ora.GAUSS2D_DTYPE.names:
        g[name] = data[name]
    j = np.zeros(1, dtype=ora.JACOBIAN_DTYPE)
    j[0] = (cen[0], cen[1]) + deriv + (1.0, 1.0)
    img = np.zeros(shape[0] * shape[1])
    ora.render(g, ora.make_coords(shape, j), img, 0)
    md = K.modes(shape[0], shape[1], deriv)
    D = K.dense_transform(img.reshape(shape), cen, md)
    ksq = md["kv"] ** 2 + md["ku"] ** 2
    P = np.exp(-K.LD(PSF_SIGMA) ** 2 * ksq / 2).astype(K.CLD)
    M = K.LD(PIX_PARS[-1]) * MR.unit_model(MR.BDF, PIX_PARS[:-1], md, P)
    keep = md["mult"] > 0
    w = md["mult"][keep] / K.LD(shape[0] * shape[1])
    E = np.sum(w * np.abs(D[keep]) ** 2)
    alias = float(np.sum(w * np.abs((M - D)[keep]) ** 2) / E)
    st = {"shape": shape, "model": MR.BDF, "dhat": K.interleaved(D), "phat": K.interleaved(P),
          "wbar": 1.0, "jac": KC.jac_record(cen, deriv), "p": PIX_PARS}
    sums, status, _, _ = MC.eval_host([st], KC.host_states(PIX_PARS[None]))
    assert status[0] == 0
    ff = float(sums[0, -1] / E)
    print("pixel-space 'bdf' against Phi P^: alias + truncation %.3e, host f.f / E %.3e"
          % (alias, ff))
    assert alias <= 1.01 * ALIAS_MEASURED
    assert ff <= 10.0 * ALIAS_MEASURED
