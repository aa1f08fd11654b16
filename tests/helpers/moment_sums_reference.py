"""
Dense reference of the moment-sum kernels (CPU only; TEST INFRASTRUCTURE).

What get_weighted_sums / get_higher_order_weighted_sums (gmix_nb.py:681-821)
and the last admom_momsums of a converged adaptive-moments fit
(admom_nb.py:131-175) leave in a result record, made the slow way:

  * the pixel grid, its values and inverse errors by oracle.fill_pixels (the
    whole grid, row-major, ierr = 0 where the weight map is <= 0);
  * the coordinates, the weight gaussian(s) with a true exp, the F vector (6,
    17 or 7 moments), w val and w^2 / ierr^2 in np.longdouble from the float64
    inputs (jacobian record, weight record with its norms set);
  * adaptive moments: the per-pixel weight in float64 by the fast exponential
    and the apodisation window of the oracle (oracle.fexp / oracle.apod, held
    bit for bit to fastexp.npz by the host test), in the order of operations of
    gauss2d_eval_pixel_fast; everything after it in np.longdouble;
  * every sum in np.longdouble, and next to every entry the sum of the
    absolute values of its terms: the scale of every comparison.  It bounds
    what any reordering of the additions can change and comes from this
    reference alone.

The case table at the end is data: the host test checks the reference and the
table's own conditions on the CPU, the GPU test walks the same cases.
"""
import numpy as np

from oracle import oracle as ora

LD = np.longdouble
SCALE = 0.263
MAX_CHI2 = 25.0
APOD_CHI2 = 20.0
TILE = 8              # TILE_H = TILE_W of the fused kernels
WS_CHUNK = 256        # pixels per chunk of the exact form
RAD_MARGIN = 1e-9     # no pixel this close (relative) to maxrad^2
CHI2_MARGIN = 1e-6    # no admom pixel this close to the chi2 cut


def jac_record(row0, col0, dvdrow, dvdcol, dudrow, dudcol):
    """the reference's 8-double jacobian record"""
    det = dvdrow * dudcol - dvdcol * dudrow
    return np.array([row0, col0, dvdrow, dvdcol, dudrow, dudcol, det, np.sqrt(abs(det))])


def ora_jac(rec):
    j = np.zeros(1, dtype=ora.JACOBIAN_DTYPE)
    j[0] = tuple(np.asarray(rec, dtype="f8").reshape(8))
    return j


def grid_pixels(stamp):
    """every pixel of the stamp, row-major, as the oracle fills them"""
    nrow, ncol = stamp["image"].shape
    px = np.zeros(nrow * ncol, dtype=ora.PIXEL_DTYPE)
    assert ora.fill_pixels(px, np.asarray(stamp["image"], dtype="f8"),
                           np.asarray(stamp["weight"], dtype="f8"), ora_jac(stamp["jac"]),
                           ignore_zero_weight=False) == ora.OK
    return px


def list_pixels(stamp, izw):
    """the pixel list the seam forms take (ngmix/pixels/pixels.py)"""
    return ora.make_pixels(np.asarray(stamp["image"], dtype="f8"),
                           np.asarray(stamp["weight"], dtype="f8"), ora_jac(stamp["jac"]), izw)


def coords_ld(shape, jac):
    """(v, u, va, ua) of the row-major grid in longdouble; va, ua are the sums
    of the absolute values of the two products behind v and u"""
    nrow, ncol = shape
    j = [LD(x) for x in np.asarray(jac, dtype="f8").reshape(8)]
    rr, cc = np.mgrid[0:nrow, 0:ncol]
    rd = rr.ravel().astype(LD) - j[0]
    cd = cc.ravel().astype(LD) - j[1]
    v = j[2] * rd + j[3] * cd
    u = j[4] * rd + j[5] * cd
    va = np.abs(j[2] * rd) + np.abs(j[3] * cd)
    ua = np.abs(j[4] * rd) + np.abs(j[5] * cd)
    return v, u, va, ua


def make_weight_gmix(rows):
    """(ngauss, 6) 'full' rows [p, row, col, irr, irc, icc] -> the record with
    its norms set"""
    rows = np.asarray(rows, dtype="f8").reshape(-1, 6)
    gm = np.zeros(rows.shape[0], dtype=ora.GAUSS2D_DTYPE)
    assert ora.gmix_fill(gm, rows.ravel(), "full") == ora.OK
    assert ora.gmix_set_norms(gm) == ora.OK
    return gm


def moments_F(nmom, v, u, vmod, umod):
    """the F vector of every pixel, (npix, nmom), gmix_nb.py:715-722 / 780-813"""
    r2 = umod * umod + vmod * vmod
    one = np.ones_like(r2)
    F = [v, u, umod * umod - vmod * vmod, 2 * vmod * umod, r2, one]
    if nmom == 17:
        u2, v2 = umod * umod, vmod * vmod
        u4, v4 = u2 * u2, v2 * v2
        r4 = r2 * r2
        r6 = r4 * r2
        r8 = r6 * r2
        F += [umod * r2, vmod * r2, umod * (u2 - 3 * v2), vmod * (3 * u2 - v2), r4,
              r2 * (u2 - v2), r2 * 2 * umod * vmod, u4 - 6 * u2 * v2 + v4,
              (u2 - v2) * 4 * umod * vmod, r6, r8]
    return np.stack(F, axis=1)


F_DEGREE = {6: [1, 1, 2, 2, 2, 0],
            17: [1, 1, 2, 2, 2, 0, 3, 3, 3, 3, 4, 4, 4, 4, 4, 6, 8],
            7: [1, 1, 2, 2, 2, 0, 4]}


def F_scale(nmom, va, ua, vcen, ucen):
    """the size of one pixel's F with every product taken by its absolute value:
    rho^degree, rho^2 = (va + |vcen|)^2 + (ua + |ucen|)^2.  A double evaluation
    of F_i from double coordinates is within a few ulp of THIS (not of F_i
    itself: v, u^2 - v^2 and their kin cancel)."""
    rho = np.sqrt((va + abs(LD(vcen))) ** 2 + (ua + abs(LD(ucen))) ** 2)
    return np.array([rho ** d for d in F_DEGREE[nmom]], dtype=LD)


def _sums(F, wdata, w2var, weight):
    """(sums, |sums|, cov, |cov|, wsum): longdouble sums over the rows of F and
    the sums of the absolute values of their terms"""
    Fa = np.abs(F)
    sums = (wdata[:, None] * F).sum(axis=0)
    sums_abs = (np.abs(wdata)[:, None] * Fa).sum(axis=0)
    cov = (F * w2var[:, None]).T @ F
    cov_abs = (Fa * w2var[:, None]).T @ Fa
    return sums, sums_abs, cov, cov_abs, weight.sum()


def wsums_reference(stamp, wt, maxrad, nmom, izw):
    """get_weighted_sums (nmom 6) / get_higher_order_weighted_sums (nmom 17) of
    one stamp from a zeroed record.

    Returns a dict: status (0 or oracle.ERR_ZERO_DIV; then nothing else),
    sums / sums_abs (nmom), cov / cov_abs (nmom, nmom), wsum, npix, used (bool
    over the row-major grid), last (grid index of the last pixel used, -1 for
    none), F_last / F_last_scale, margin = min |rad^2 - maxrad^2| / maxrad^2
    over the listed pixels (inf for maxrad == 0)."""
    assert nmom in (6, 17)
    px = grid_pixels(stamp)
    shape = stamp["image"].shape
    v, u, va, ua = coords_ld(shape, stamp["jac"])
    ierr = px["ierr"]
    listed = ierr > 0.0 if izw else np.ones(ierr.size, dtype=bool)
    vcen, ucen = LD(wt["row"][0]), LD(wt["col"][0])
    vmod, umod = v - vcen, u - ucen
    rad2 = umod * umod + vmod * vmod
    mr2 = LD(maxrad) * LD(maxrad)
    used = listed & (rad2 < mr2)
    if nmom == 6:
        used &= ierr > 0.0                      # gmix_nb.py:713
    margin = np.inf
    if mr2 > 0 and listed.any():
        margin = float((np.abs(rad2[listed] - mr2) / mr2).min())
    if nmom == 17 and np.any(ierr[used] == 0.0):
        return {"status": ora.ERR_ZERO_DIV, "margin": margin, "used": used}
    area = LD(stamp["jac"][7]) * LD(stamp["jac"][7])
    weight = np.zeros(v.size, dtype=LD)
    for g in wt:
        vd, ud = v - LD(g["row"]), u - LD(g["col"])
        chi2 = LD(g["dcc"]) * vd * vd + LD(g["drr"]) * ud * ud - 2 * LD(g["drc"]) * vd * ud
        weight += LD(g["pnorm"]) * np.exp(-0.5 * chi2) * area
    F = moments_F(nmom, v, u, vmod, umod)[used]
    w = weight[used]
    ie = ierr[used].astype(LD)
    val = px["val"][used].astype(LD)
    sums, sums_abs, cov, cov_abs, wsum = _sums(F, w * val, w * w / (ie * ie), w)
    idx = np.flatnonzero(used)
    last = int(idx[-1]) if idx.size else -1
    out = {"status": ora.OK, "sums": sums, "sums_abs": sums_abs, "cov": cov, "cov_abs": cov_abs,
           "wsum": wsum, "npix": int(idx.size), "used": used, "last": last, "margin": margin,
           "F_last": None, "F_last_scale": None}
    if last >= 0:
        out["F_last"] = F[-1]
        out["F_last_scale"] = F_scale(nmom, va[last], ua[last], vcen, ucen)
    return out


def fast_weight(wt, v, u, area):
    """gauss2d_eval_pixel_fast (gmix_nb.py:28-63) over float64 arrays, in its
    order of operations, through the oracle's fexp and window.  Returns
    (weight, chi2)."""
    g = wt[0] if np.ndim(wt) else wt
    v = np.asarray(v, dtype="f8")
    u = np.asarray(u, dtype="f8")
    vd, ud = v - g["row"], u - g["col"]
    chi2 = g["dcc"] * vd * vd + g["drr"] * ud * ud - 2.0 * g["drc"] * vd * ud
    w = np.zeros(v.size)
    inside = (chi2 < MAX_CHI2) & (chi2 >= 0.0)
    w[inside] = g["pnorm"] * ora.fexp(-0.5 * chi2[inside]) * area
    ap = inside & (chi2 > APOD_CHI2)
    w[ap] *= ora.apod(chi2[ap])[0]
    return w, chi2


def admom_weight_record(wt):
    """a copy of a returned one-gaussian weight, as the oracle's record, with
    the norms set again from its moments (what every admom pass does first)"""
    src = wt[0] if np.ndim(wt) else wt
    g = np.zeros(1, dtype=ora.GAUSS2D_DTYPE)
    for n in ("p", "row", "col", "irr", "irc", "icc", "det"):
        g[n] = src[n]
    assert ora.gmix_set_norms(g) == ora.OK
    return g


def admom_reference(stamp, wt, izw=True):
    """admom_momsums at the weight `wt` (a converged fit's returned weight IS
    the weight of its last moments pass) from a cleared record: sums (7), cov
    (7, 7), wsum, npix with the sums of absolute terms, F of the last listed
    pixel, and chi2_margin = min |chi2 - 25| over the listed pixels."""
    g = admom_weight_record(wt)
    px = grid_pixels(stamp)
    listed = px["ierr"] > 0.0 if izw else np.ones(px.size, dtype=bool)
    area = px["area"][0]
    w64, chi2_64 = fast_weight(g, px["v"], px["u"], area)
    v, u, va, ua = coords_ld(stamp["image"].shape, stamp["jac"])
    vcen, ucen = LD(g["row"][0]), LD(g["col"][0])
    vmod, umod = v - vcen, u - ucen
    chi2 = LD(g["dcc"][0]) * vmod * vmod + LD(g["drr"][0]) * umod * umod - \
        2 * LD(g["drc"][0]) * vmod * umod
    F = np.stack([v, u, umod * umod - vmod * vmod, 2 * vmod * umod,
                  umod * umod + vmod * vmod, np.ones_like(v), chi2 * chi2], axis=1)[listed]
    w = w64[listed].astype(LD)
    ie = px["ierr"][listed].astype(LD)
    val = px["val"][listed].astype(LD)
    sums, sums_abs, cov, cov_abs, wsum = _sums(F, w * val, w * w / (ie * ie), w)
    idx = np.flatnonzero(listed)
    return {"sums": sums, "sums_abs": sums_abs, "cov": cov, "cov_abs": cov_abs, "wsum": wsum,
            "npix": int(idx.size), "last": int(idx[-1]), "F_last": F[-1],
            "chi2_margin": float(np.abs(chi2_64[listed] - MAX_CHI2).min()),
            "weight64": w64, "listed": listed}


# ------------------------------------------------------------ the case table
WS_SHAPES_A = [(1, 1), (3, 5), (8, 8), (8, 16), (8, 24), (9, 7), (7, 9), (13, 15)]
WS_SHAPES_B = [(15, 17), (16, 16), (1, 257), (17, 19), (32, 32), (33, 31), (70, 1), (1, 70)]
WS_SHAPES_C = [(9, 7), (13, 15), (16, 16), (17, 19), (8, 24), (33, 31)]
JACOBIANS = ["diag", "rot30", "shear", "flip", "aniso", "outside"]
MAXRADS = ["all", "cut", "few", "none"]
MASKS = ["none", "scattered", "zero_row", "last", "one_tile"]


def make_jacobian(kind, shape, rng):
    nrow, ncol = shape
    row0 = (nrow - 1) / 2.0 + rng.uniform(-0.4, 0.4)
    col0 = (ncol - 1) / 2.0 + rng.uniform(-0.4, 0.4)
    s = SCALE
    if kind == "diag":
        m = (s, 0.0, 0.0, s)
    elif kind == "rot30":
        c, sn = np.cos(np.pi / 6), np.sin(np.pi / 6)
        m = (s * c, -s * sn, s * sn, s * c)
    elif kind == "shear":
        m = (1.05 * s, 0.21 * s, 0.13 * s, 0.97 * s)
    elif kind == "flip":                      # det < 0
        m = (s, 0.02 * s, 0.0, -s)
    elif kind == "aniso":                     # 2 : 1
        m = (1.4 * s, 0.1 * s, -0.05 * s, 0.7 * s)
    elif kind == "outside":                   # the origin 3 pixels off a corner
        row0, col0 = nrow + 2.3, -3.4
        m = (s, 0.03 * s, -0.02 * s, s)
    else:
        raise ValueError(kind)
    return jac_record(row0, col0, *m)


def make_mask(kind, shape, weight, rng):
    """zeros written into `weight`; the kind applied (a stamp too small for a
    kind gets the nearest that keeps a pixel)"""
    nrow, ncol = shape
    n = nrow * ncol
    if kind == "scattered" and n >= 4:
        z = rng.uniform(size=shape) < 0.15
        z.flat[rng.randint(n)] = True
        z.flat[(np.flatnonzero(~z.ravel()))[0]] = False
        weight[z] = 0.0
    elif kind == "zero_row" and nrow >= 3:
        weight[nrow // 2, :] = 0.0
    elif kind == "zero_row" and ncol >= 3:    # one line: a run of zeros inside it
        weight[:, ncol // 3:ncol // 3 + max(1, ncol // 8)] = 0.0
    elif kind == "last" and nrow >= 2:        # lastp != n - 1
        weight[-1, :] = 0.0
        weight[-2, -1] = 0.0
    elif kind == "last" and ncol >= 2:
        weight[-1, -max(1, ncol // 4):] = 0.0
    elif kind == "one_tile" and (nrow > TILE or ncol > TILE):
        keep = np.zeros(shape, dtype=bool)
        r0 = TILE * ((nrow - 1) // TILE // 2)
        c0 = TILE * ((ncol - 1) // TILE)      # the last tile column (ragged)
        keep[r0:r0 + TILE, c0:c0 + TILE] = True
        keep &= rng.uniform(size=shape) < 0.8
        keep[min(r0 + 1, nrow - 1), min(c0, ncol - 1)] = True
        weight[~keep] = 0.0
    else:
        kind = "none"
    return kind


def pick_maxrad(rad2, kind):
    """a maxrad that keeps every pixel / about half / three (or all of fewer) /
    none, half way between two well separated neighbours of the sorted rad^2"""
    r = np.sort(np.asarray(rad2, dtype="f8"))
    n = r.size
    if kind == "all":
        return 1.5 * np.sqrt(r[-1]) + 1.0
    if kind == "none":
        return 0.5 * np.sqrt(r[0])
    k = 3 if kind == "few" else max(1, n // 2)
    if k >= n:
        return 1.5 * np.sqrt(r[-1]) + 1.0
    while k < n - 1 and r[k] - r[k - 1] <= 1e-3 * r[k]:
        k += 1
    if r[k] - r[k - 1] <= 1e-3 * r[k]:
        return 1.5 * np.sqrt(r[-1]) + 1.0
    return float(np.sqrt(0.5 * (r[k - 1] + r[k])))


def make_weight_rows(ngauss, shape, jac, rng):
    """'full' rows of a weight of 1..3 gaussians about the uv origin, wide
    enough that no pixel's weight underflows"""
    sig = SCALE * max(1.5, max(shape) / 5.0)
    rows = np.zeros((ngauss, 6))
    frac = np.array([0.6, 0.3, 0.1])[:ngauss]
    for i in range(ngauss):
        T = 2.0 * (sig * (1.0 + 0.6 * i)) ** 2
        e1, e2 = rng.uniform(-0.3, 0.3, size=2)
        rows[i] = [frac[i] / frac.sum(), rng.uniform(-0.7, 0.7) * SCALE,
                   rng.uniform(-0.7, 0.7) * SCALE, 0.5 * T * (1 - e1), 0.5 * T * e2,
                   0.5 * T * (1 + e1)]
    return rows


def _listed_rad2(stamp, wt, izw):
    v, u, _, _ = coords_ld(stamp["image"].shape, stamp["jac"])
    vmod, umod = v - LD(wt["row"][0]), u - LD(wt["col"][0])
    rad2 = (umod * umod + vmod * vmod).astype("f8")
    w = np.asarray(stamp["weight"]).ravel()
    return rad2[w > 0.0] if izw else rad2


def wsums_batch(name, seed):
    """one ragged batch of the table: stamps with image, weight, jac, izw and
    the kinds applied; per ngauss a weight and a maxrad for every stamp"""
    shapes = {"A": WS_SHAPES_A, "B": WS_SHAPES_B, "C": WS_SHAPES_C}[name]
    rng = np.random.RandomState(seed)
    off = {"A": 0, "B": 2, "C": 1}[name]
    stamps = []
    for i, shape in enumerate(shapes):
        jk = JACOBIANS[(i + off) % 6]
        jac = make_jacobian(jk, shape, rng)
        image = rng.normal(size=shape) + 5.0
        weight = rng.uniform(0.5, 2.0, size=shape)
        if name == "B" and shape == (17, 19):           # twelve decades of weight
            weight = 10.0 ** rng.uniform(-6.0, 6.0, size=shape)
        if name == "C":
            mk = make_mask("scattered", shape, weight, rng)
        else:
            mk = make_mask(MASKS[(i + 2 * off) % 5], shape, weight, rng)
        stamps.append({"image": image, "weight": weight, "jac": jac, "shape": shape,
                       "jacobian": jk, "mask": mk, "izw": name != "C"})
    weights, maxrads, kinds = {}, {}, {}
    for ng in (1, 2, 3):
        weights[ng], maxrads[ng], kinds[ng] = [], [], []
        for i, s in enumerate(stamps):
            wt = make_weight_gmix(make_weight_rows(ng, s["shape"], s["jac"], rng))
            mk = MAXRADS[(i + ng + off) % 4]
            weights[ng].append(wt)
            maxrads[ng].append(pick_maxrad(_listed_rad2(s, wt, s["izw"]), mk))
            kinds[ng].append(mk)
    return {"name": name, "stamps": stamps, "weights": weights, "maxrads": maxrads,
            "maxrad_kinds": kinds, "seed": seed}


WS_BATCHES = [("A", 7101), ("B", 7102), ("C", 7103)]


def wsums_cases():
    """(batch, ngauss, nmom): batch C keeps its zero-weight pixels in the list
    (ignore_zero_weight off) and is a case of the 6-moment form alone -- the
    17-moment form raises on them (zero_div_case)"""
    out = []
    for name, _ in WS_BATCHES:
        for ng in (1, 2, 3):
            for nmom in (6, 17):
                if name == "C" and nmom == 17:
                    continue
                out.append((name, ng, nmom))
    return out


def zero_div_case(seed=7201):
    """five stamps with positive weights, ignore_zero_weight off; `k` is the
    stamp and `inside` / `outside` the pixels (row, col) to zero: one inside
    that stamp's maxrad, one outside it"""
    rng = np.random.RandomState(seed)
    shapes = [(9, 7), (17, 19), (16, 16), (13, 15), (8, 24)]
    stamps, wts, maxrads = [], [], []
    for i, shape in enumerate(shapes):
        jac = make_jacobian(JACOBIANS[i % 5], shape, rng)
        stamps.append({"image": rng.normal(size=shape) + 5.0,
                       "weight": rng.uniform(0.5, 2.0, size=shape), "jac": jac, "shape": shape,
                       "izw": False})
        wt = make_weight_gmix(make_weight_rows(1, shape, jac, rng))
        wts.append(wt)
        maxrads.append(pick_maxrad(_listed_rad2(stamps[-1], wt, False), "cut"))
    k = 2
    v, u, _, _ = coords_ld(shapes[k], stamps[k]["jac"])
    rad2 = ((u - LD(wts[k]["col"][0])) ** 2 + (v - LD(wts[k]["row"][0])) ** 2).astype("f8")
    order = np.argsort(rad2)
    inside, outside = int(order[3]), int(order[-2])
    assert rad2[inside] < maxrads[k] ** 2 < rad2[outside]
    ncol = shapes[k][1]
    return {"stamps": stamps, "weights": wts, "maxrads": maxrads, "k": k,
            "inside": divmod(inside, ncol), "outside": divmod(outside, ncol)}


_CACHE = {}


def cached(key, make):
    """cases and references are made once per process and left unchanged"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def get_wsums_batch(name):
    return cached(("wsb", name), lambda: wsums_batch(name, dict(WS_BATCHES)[name]))


def wsums_case_reference(name, ng, nmom):
    def make():
        b = get_wsums_batch(name)
        return [wsums_reference(s, b["weights"][ng][i], b["maxrads"][ng][i], nmom, s["izw"])
                for i, s in enumerate(b["stamps"])]
    return cached(("wsref", name, ng, nmom), make)


# ------------------------------------------------------------------- admom
# (shape, NGMIX_ADMOM_NT or None) -> the launch form of launch_admom_grid
ADMOM_SHAPES = [(16, 16), (22, 22), (25, 25), (31, 32), (40, 44), (47, 48), (56, 60), (65, 65)]
ADMOM_FORCED = [((25, 25), 128), ((25, 25), 256), ((40, 44), 256), ((56, 60), 256)]
ADMOM_CENONLY = [(16, 16), (25, 25), (65, 65)]
ADMOM_KINDS = ["clean_round", "noisy_sheared", "clean_sheared_masked", "noisy_round"]
ADMOM_CONF = {"maxiter": 200, "shiftmax": 5.0, "etol": 1.0e-5, "Ttol": 1.0e-3}
BLOCK = 256


def admom_launch_form(npix, nt_env=0):
    """(NT, PPT) of launch_admom_grid (moments.hip) for a batch whose largest
    stamp has npix pixels; PPT 0 is the streaming form"""
    nt = nt_env
    if nt == 0:
        nt = 64 if npix <= 16 * 64 else (128 if npix <= 16 * 128 else (
            64 if npix <= 36 * 64 else (128 if npix <= 32 * 128 else 256)))
    if nt == 64 and npix <= 8 * 64:
        return 64, 8
    if nt == 64 and npix <= 16 * 64:
        return 64, 16
    if nt <= 128 and npix <= 8 * 128:
        return 128, 8
    if nt <= 128 and npix <= 16 * 128:
        return 128, 16
    if nt == 64 and npix <= 36 * 64:
        return 64, 36
    if nt == 128 and npix <= 32 * 128:
        return 128, 32
    if npix <= 4 * BLOCK:
        return BLOCK, 4
    if npix <= 8 * BLOCK:
        return BLOCK, 8
    if npix <= 16 * BLOCK:
        return BLOCK, 16
    return BLOCK, 0


def admom_all_chunks(npix, nt, ppt):
    """admom_grid_kernel's choice of the compile-time pixel loops"""
    if ppt == 0:
        return False
    if ppt > 16:
        return True
    nchunk = (npix + nt - 1) // nt
    return nt == 64 and nchunk * 8 >= ppt * 7


def render_gauss(pars, shape, jac):
    """a one-gaussian image through the oracle's exact evaluation"""
    gm = np.zeros(1, dtype=ora.GAUSS2D_DTYPE)
    assert ora.gmix_fill(gm, np.asarray(pars, dtype="f8"), "gauss") == ora.OK
    im = np.zeros(shape[0] * shape[1])
    assert ora.render(gm, ora.make_coords(shape, ora_jac(jac)), im, fast_exp=0) == ora.OK
    return im.reshape(shape)


def admom_batch(shape, seed=None):
    """four stamps of one shape: a noise-free round gaussian, a sheared one at
    s/n ~ 50, a noise-free sheared one with masked pixels, a round one at
    s/n ~ 50; every guess off centre and off in size"""
    nrow, ncol = shape
    rng = np.random.RandomState(nrow * 100 + ncol if seed is None else seed)
    stamps, guesses = [], []
    for kind in ADMOM_KINDS:
        jac = jac_record((nrow - 1) / 2.0 + rng.uniform(-0.4, 0.4),
                         (ncol - 1) / 2.0 + rng.uniform(-0.4, 0.4), SCALE, 0.0, 0.0, SCALE)
        T = 2.0 * (SCALE * (1.2 + 0.045 * min(nrow, ncol) * rng.uniform(0.8, 1.1))) ** 2
        g = rng.uniform(0.15, 0.3, size=2) * rng.choice([-1.0, 1.0], size=2) \
            if "sheared" in kind else np.zeros(2)
        cen = rng.uniform(-0.5, 0.5, size=2) * SCALE
        flux = 40.0
        image = render_gauss([cen[0], cen[1], g[0], g[1], T, flux], shape, jac)
        noise = 1.0e-4 * image.max()
        if "noisy" in kind:
            # s/n ~ 50 in the matched filter: sqrt(sum model^2) / noise
            noise = np.sqrt((image ** 2).sum()) / 50.0
            image = image + noise * rng.normal(size=shape)
        weight = np.full(shape, 1.0 / noise ** 2)
        if "masked" in kind:
            weight[nrow // 3, ncol // 2] = 0.0
            weight[-1, -3:] = 0.0                       # the last pixels: last_pos != n - 1
            weight[rng.uniform(size=shape) < 0.03] = 0.0
        stamps.append({"image": image, "weight": weight, "jac": jac, "shape": shape,
                       "kind": kind, "cen": cen})
        guesses.append([cen[0] + rng.uniform(0.4, 0.8) * SCALE * rng.choice([-1.0, 1.0]),
                        cen[1] + rng.uniform(0.4, 0.8) * SCALE * rng.choice([-1.0, 1.0]),
                        0.0, 0.0, T * rng.uniform(0.8, 1.25), 1.0])
    return {"shape": shape, "stamps": stamps, "guess": np.array(guesses)}


def get_admom_batch(shape):
    return cached(("adb", shape), lambda: admom_batch(shape))


def admom_guess_gmix(batch):
    """the (n, 1) weight records of the guesses, norms set"""
    n = len(batch["stamps"])
    gm = np.zeros((n, 1), dtype=ora.GAUSS2D_DTYPE)
    for i in range(n):
        assert ora.gmix_fill(gm[i], batch["guess"][i], "gauss") == ora.OK
        assert ora.gmix_set_norms(gm[i]) == ora.OK
    return gm


def admom_conf(cenonly):
    conf = np.zeros(1, dtype=ora.ADMOM_CONF_DTYPE)
    for k, val in ADMOM_CONF.items():
        conf[k] = val
    conf["cenonly"] = cenonly
    return conf


def admom_oracle(shape, cenonly):
    """the oracle's fit of every stamp of a batch: [(status, result record,
    returned weight)] (cached)"""
    def make():
        b = get_admom_batch(shape)
        gm = admom_guess_gmix(b)
        out = []
        for i, s in enumerate(b["stamps"]):
            w = gm[i].copy()
            r = np.zeros(1, dtype=ora.ADMOM_RESULT_DTYPE)
            st = ora.admom(admom_conf(cenonly), w, list_pixels(s, True), r)
            out.append((st, r, w))
        return out
    return cached(("ado", shape, bool(cenonly)), make)


def admom_cases():
    """(shape, NGMIX_ADMOM_NT or 0, cenonly)"""
    out = [(s, 0, False) for s in ADMOM_SHAPES]
    out += [(s, nt, False) for s, nt in ADMOM_FORCED]
    out += [(s, 0, True) for s in ADMOM_CENONLY]
    return out
