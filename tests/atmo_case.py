"""Cases, inputs and bookkeeping shared by tests/golden/make_golden_atmo.py (which runs the compiled reference) and the tests
of the boundary layer (test_atmo_golden.py, test_gpu_atmo.py).  No GPU here.

A case is one block of 30 x 67 cells (28 x 65 + ghosts) for one surface type, built from a seed: a random part (the fields of
test_gpu_atmo._inputs, 80 % of the interior listed) and a constructed part, the first cells of the interior in storage
order, all listed, CELLS_PER_CLASS cells for each class of BRANCHES: the places where atmo_boundary_layer
(source/ice_atmo.F90:56-384) branches or saturates.  The fixture tests/golden/atmo.npz holds the inputs and what the compiled
reference made of them.

`flip` needs a word: tstar and qstar carry the same factor rh = re, so the sign of hol is that of rh (delt/thva + delq/(1/zvir
+ Qa)) and changes between iterations only where rh turns negative -- where the measurement height lies below the roughness
length.  No model run has such a level; the routine computes it all the same, and the cells are there for the branch.

Conditioning of the fixture (asserted by test_atmo_golden.py, not a tolerance): in every listed cell and every iteration |hol|
is exactly 0 or at least HOL_MIN, so an error of an ulp in log cannot move a cell across the jump of 0.025 psimh has at hol =
0; and atmo_truth takes the stable / unstable side the restatement takes.  For that the `delt0` and `neutral` cells have
surface temperatures that are multiples of 2**-20 (Tsf + Tffresh is then exact, delt is 0 in any precision), and the
`neutral` cells are those candidates whose Qa = fl(qsat / rhoa) does not lie below the quotient in extended precision.

atmo_numpy is the routine restated operation by operation in float64, in the reference's order, with exp, log and atan of
the host's libm.so.6 through ctypes, the reference's own.  atmo_truth is the same sequence in np.longdouble with the inputs
and the named constants promoted, clamps and branches taken on its own values.  Qa of the `neutral` cells depends on the
host libm's exp: the inputs are rebuilt bit for bit only where that is glibc's (conftest.TOL_EXP == 0)."""
import ctypes as C
import ctypes.util
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "atmo.npz")
NY, NX = 30, 67
PUNY = 1.0e-11
HOL_MIN = 1.0e-6
INS = ("Tsf", "potT", "uatm", "vatm", "wind", "zlvl", "Qa", "rhoa")
OUT = ("strx", "stry", "Tref", "Qref", "delt", "delq", "lhcoef", "shcoef")
OUT_EXP = ("delt", "delq")                                        # pass through exp alone
OUT_LOG = ("strx", "stry", "Tref", "Qref", "lhcoef", "shcoef")    # pass through log and atan
CASES = {"ice": dict(sfctype="ice", seed=2026102101), "ocn": dict(sfctype="ocn", seed=2026102102)}
LIST_CASE = "ice"                  # the case that also carries calc_strair = F, the full interior and the sub-lists
SUBLISTS = (1, 255, 256, 257)      # the first cells of the case's list: the workgroup edge of k_atmo_list
BRANCHES = ("stable", "unstable", "flip", "clamp_pos", "clamp_neg", "calm", "at_umin", "still", "alz0", "ztrf", "delt0",
            "neutral", "sst_above", "sst_at", "sst_below")
OCN_ONLY = ("sst_above", "sst_at", "sst_below")
CELLS_PER_CLASS = 12
NEED = 8
SST_FREEZE = -1.8

# ice_constants.F90 and the parameters of the routine
VONKAR, GRAVIT, ZVIR, CP_AIR, CP_WV = 0.4, 9.80616, 0.606, 1005.0, 1.81e3
TFFRESH, ZREF, ICERUF, ZTRF, UMIN = 273.15, 10.0, 0.0005, 2.0, 1.0
PIH = 0.5 * 3.14159265358979323846
CPVIR = CP_WV / CP_AIR - 1.0
QQQ = dict(ice=11637800.0, ocn=627572.4)
TTT = dict(ice=5897.8, ocn=5107.4)
LHEAT = dict(ice=2.835e6, ocn=2.501e6)

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("exp", "log", "atan"):
    getattr(_libm, _n).restype = C.c_double
    getattr(_libm, _n).argtypes = [C.c_double]


def _each(f):
    def g(x):
        x = np.asarray(x, np.float64)
        return np.fromiter((f(v) for v in x.ravel().tolist()), np.float64, x.size).reshape(x.shape)
    return g


class _F64:
    """float64, transcendental functions of the host libm element by element"""
    f = staticmethod(lambda x: np.asarray(x, np.float64))
    exp, log, atan = staticmethod(_each(_libm.exp)), staticmethod(_each(_libm.log)), staticmethod(_each(_libm.atan))


class _LD:
    """np.longdouble; what is handed in is a double and is promoted"""
    f = staticmethod(lambda x: np.asarray(np.asarray(x, np.float64), np.longdouble))
    exp, log, atan = staticmethod(np.exp), staticmethod(np.log), staticmethod(np.arctan)


def _routine(sfctype, c, X):
    """atmo_boundary_layer on the 1-d arrays c[name] of the listed cells in the arithmetic X: the eight outputs (strx, stry as
    calc_strair = T gives them) and hol of the five iterations, after the clamp"""
    f = X.f
    c = {k: f(c[k]) for k in INS}
    c0, c1, c2, c5, c8, c10, c16, p5 = (f(x) for x in (0.0, 1.0, 2.0, 5.0, 8.0, 10.0, 16.0, 0.5))
    vonkar, gravit, zvir, cp_air, cpvir, pih = (f(x) for x in (VONKAR, GRAVIT, ZVIR, CP_AIR, CPVIR, PIH))
    Tffresh, zref, zTrf, umin = (f(x) for x in (TFFRESH, ZREF, ZTRF, UMIN))
    qqq, ttt, Lheat = f(QQQ[sfctype]), f(TTT[sfctype]), f(LHEAT[sfctype])

    def psimhu(xd):                                                                   # :175-176
        return X.log((c1 + xd * (c2 + xd)) * (c1 + xd * xd) / c8) - c2 * X.atan(xd) + pih

    def psixhu(xd):                                                                   # :179
        return c2 * X.log((c1 + xd * xd) / c2)

    al2 = X.log(zref / zTrf)
    vmag = np.maximum(umin, c["wind"])                                                # :215 / :227
    if sfctype == "ice":
        rdn = np.full(vmag.shape, vonkar / X.log(zref / f(ICERUF)), vmag.dtype)
    else:
        rdn = np.sqrt(f(0.0027) / vmag + f(.000142) + f(.0000764) * vmag)
    TsfK = c["Tsf"] + Tffresh                                                         # :242
    qsat = qqq * X.exp(-ttt / TsfK)
    ssq = qsat / c["rhoa"]
    thva = c["potT"] * (c1 + zvir * c["Qa"])
    delt = c["potT"] - TsfK
    delq = c["Qa"] - ssq
    alz = X.log(c["zlvl"] / zref)
    cp = cp_air * (c1 + cpvir * ssq)
    rhn, ren = rdn, rdn
    ustar, tstar, qstar = rdn * vmag, rhn * delt, ren * delq
    hols = []
    for _ in range(5):                                                                # :271
        hol = vonkar * gravit * c["zlvl"] * (tstar / thva + qstar / (c1 / zvir + c["Qa"])) / (ustar * ustar)
        hol = np.copysign(np.minimum(np.abs(hol), c10), hol)
        stable = p5 + np.copysign(p5, hol)
        xqq = np.maximum(np.sqrt(np.abs(c1 - c16 * hol)), c1)
        xqq = np.sqrt(xqq)
        psimhs = -(f(0.7) * hol + f(0.75) * (hol - f(14.3)) * X.exp(f(-0.35) * hol) + f(10.7))
        psimh = psimhs * stable + (c1 - stable) * psimhu(xqq)
        psixh = psimhs * stable + (c1 - stable) * psixhu(xqq)
        rd = rdn / (c1 + rdn / vonkar * (alz - psimh))                                # :297-299
        rh = rhn / (c1 + rhn / vonkar * (alz - psixh))
        re = ren / (c1 + ren / vonkar * (alz - psixh))
        ustar, tstar, qstar = rd * vmag, rh * delt, re * delq
        hols.append(hol)
    tau = c["rhoa"] * ustar * rd                                                      # :334
    o = dict(strx=tau * c["uatm"], stry=tau * c["vatm"], delt=delt, delq=delq)
    o["shcoef"] = c["rhoa"] * ustar * cp * rh + c1                                    # :356-357
    o["lhcoef"] = c["rhoa"] * ustar * Lheat * re
    hol = hol * zTrf / c["zlvl"]                                                      # :362
    xqq = np.maximum(c1, np.sqrt(np.abs(c1 - c16 * hol)))
    xqq = np.sqrt(xqq)
    psix2 = -c5 * hol * stable + (c1 - stable) * psixhu(xqq)
    fac = (rh / vonkar) * (alz + al2 - psixh + psix2)
    Tref = c["potT"] - delt * fac
    o["Tref"] = Tref - f(0.01) * zTrf
    fac = (re / vonkar) * (alz + al2 - psixh + psix2)
    o["Qref"] = c["Qa"] - delq * fac
    return o, np.stack(hols)


def _on_the_list(sfctype, icells, indxi, indxj, a, X, calc_strair, strx, stry):
    ny, nx = a["Tsf"].shape
    q = (np.asarray(indxj[:icells], np.int64) - 1) * nx + (np.asarray(indxi[:icells], np.int64) - 1)
    with np.errstate(all="ignore"):
        o, hols = _routine(sfctype, {k: np.asarray(a[k]).ravel()[q] for k in INS}, X)
    dtype = o["Tref"].dtype
    out = {}
    for k in OUT:
        if k in ("strx", "stry") and not calc_strair:
            out[k] = np.array(strx if k == "strx" else stry, dtype)
            continue
        x = np.zeros(ny * nx, dtype)
        x[q] = o[k]
        out[k] = x.reshape(ny, nx)
    hol = np.zeros((5, ny * nx), dtype)
    hol[:, q] = hols
    return out, hol.reshape(5, ny, nx)


def atmo_numpy(sfctype, icells, indxi, indxj, a, calc_strair=True, strx=None, stry=None):
    """the routine in float64 with the host libm: (outputs, hol of the five iterations (5, ny, nx)); zero off the list"""
    return _on_the_list(sfctype, icells, indxi, indxj, a, _F64, calc_strair, strx, stry)


def atmo_truth(sfctype, icells, indxi, indxj, a, calc_strair=True, strx=None, stry=None):
    """the routine in np.longdouble on the same (double) inputs: (outputs, hol of the five iterations)"""
    return _on_the_list(sfctype, icells, indxi, indxj, a, _LD, calc_strair, strx, stry)


def make_list(mask):
    """cells of a (ny, nx) mask in storage order: icells, indxi, indxj (1-based, padded to the plane)"""
    jj, ii = np.nonzero(mask)
    indxi = np.zeros(mask.size, np.int32); indxj = np.zeros(mask.size, np.int32)
    indxi[:ii.size] = ii + 1; indxj[:ii.size] = jj + 1
    return int(ii.size), indxi, indxj


def interior(ny=NY, nx=NX):
    m = np.zeros((ny, nx), bool)
    m[1:-1, 1:-1] = True
    return m


def constructed(sfctype):
    """{class: (jj, ii)} of the cells built for it: the first cells of the interior in storage order"""
    names = [k for k in BRANCHES if sfctype == "ocn" or k not in OCN_ONLY]
    o = {}
    for n, k in enumerate(names):
        q = np.arange(n * CELLS_PER_CLASS, (n + 1) * CELLS_PER_CLASS)
        o[k] = (q // (NX - 2) + 1, q % (NX - 2) + 1)
    return o


def constructed_mask(sfctype):
    m = np.zeros((NY, NX), bool)
    for jj, ii in constructed(sfctype).values():
        m[jj, ii] = True
    return m


def _ssq(sfctype, Tsf, rhoa, X=_F64):
    f = X.f
    return f(QQQ[sfctype]) * X.exp(-f(TTT[sfctype]) / (f(Tsf) + f(TFFRESH))) / f(rhoa)


def make_inputs(name):
    """the fields of a case, its list mask, and the caller's stresses of the calc_strair = F run"""
    c = CASES[name]
    sfc, ocn = c["sfctype"], c["sfctype"] == "ocn"
    rng = np.random.default_rng(c["seed"])
    shp = (NY, NX)
    U = lambda lo, hi: rng.uniform(lo, hi, shp)  # noqa: E731
    # the random part: test_gpu_atmo._inputs, regime `mixed`
    a = dict(potT=U(238, 280), uatm=U(-15, 15), vatm=U(-15, 15), zlvl=U(8, 40), Qa=U(0.0002, 0.005), rhoa=U(1.2, 1.4))
    a["wind"] = np.sqrt(a["uatm"] ** 2 + a["vatm"] ** 2)
    calm = rng.uniform(0, 1, shp) < 0.1
    for k in ("wind", "uatm", "vatm"):
        a[k][calm] *= 0.02
    a["Tsf"] = np.minimum(a["potT"] - 273.15 + U(-12, 12), 0.0)
    if ocn:
        a["Tsf"] = a["Tsf"] + 2.0 + np.abs(a["Tsf"]) * 0.1
    mask = (rng.uniform(0, 1, shp) < 0.8) & interior()
    # the constructed part
    n = CELLS_PER_CLASS
    u = lambda lo, hi, count=n: rng.uniform(lo, hi, count)  # noqa: E731
    cells = constructed(sfc)
    T0 = (272.0, 295.0) if ocn else (243.0, 262.0)              # air temperatures that leave room for either stratification

    def base(cell, wind=None, dT=None, potT=None):
        """ordinary values on the cells; wind: speeds (the direction is drawn); dT: Tsf minus the air's temperature"""
        a["potT"][cell] = u(*T0) if potT is None else potT
        a["zlvl"][cell] = u(8, 40); a["Qa"][cell] = u(0.0005, 0.004); a["rhoa"][cell] = u(1.2, 1.4)
        w = u(2, 12) if wind is None else wind
        ux, vy = u(-1, 1), u(-1, 1)
        h = np.sqrt(ux * ux + vy * vy)
        a["wind"][cell] = w; a["uatm"][cell] = ux * (w / h); a["vatm"][cell] = vy * (w / h)
        T = a["potT"][cell] - 273.15 + (u(-8, 8) if dT is None else dT)
        a["Tsf"][cell] = T if ocn else np.minimum(T, 0.0)

    def quantised(cell):
        """Tsf a multiple of 2**-20 and potT the very double Tsf + Tffresh"""
        a["Tsf"][cell] = np.round(a["Tsf"][cell] * 2.0 ** 20) / 2.0 ** 20
        a["potT"][cell] = a["Tsf"][cell] + TFFRESH

    base(cells["stable"], dT=-u(4, 12))
    base(cells["unstable"], dT=u(4, 10))
    cold = lambda: u(275, 280) if ocn else u(238, 243)          # ... and for a surface 30 K warmer  # noqa: E731
    cl = cells["flip"]; base(cl, wind=u(0.3, 1.5), dT=np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * u(20, 30), potT=cold())
    a["zlvl"][cl] = u(3.0e-6, 1.0e-5)       # far enough below the roughness length that 1 + rhn / vonkar (alz - psixh) < -0.3
    cl = cells["clamp_pos"]; base(cl, wind=u(0.1, 0.9), dT=-u(20, 30)); a["zlvl"][cl] = u(30, 40)
    cl = cells["clamp_neg"]; base(cl, wind=u(0.1, 0.9), dT=u(20, 30), potT=cold())
    a["zlvl"][cl] = u(30, 40)
    base(cells["calm"], wind=u(0.05, 0.95))
    cl = cells["at_umin"]; base(cl, wind=np.ones(n))
    cl = cells["still"]; base(cl)
    sgn = np.where(np.arange(n) % 2 == 0, 0.0, -0.0)
    a["wind"][cl] = 0.0; a["uatm"][cl] = sgn; a["vatm"][cl] = np.roll(sgn, 1) * np.where(np.arange(n) % 4 < 2, 1.0, -1.0)
    cl = cells["alz0"]; base(cl); a["zlvl"][cl] = ZREF
    cl = cells["ztrf"]; base(cl); a["zlvl"][cl] = ZTRF
    cl = cells["delt0"]; base(cl); quantised(cl)
    a["Qa"][cl] = _ssq(sfc, a["Tsf"][cl], a["rhoa"][cl]) * np.where(np.arange(n) % 2 == 0, 0.5, 1.5)
    # neutral: of 8 n candidates the first n whose Qa = fl(qsat / rhoa) is not below the quotient in extended precision
    cl = cells["neutral"]
    cand_T = np.round((u(*T0, 8 * n) - 273.15 if ocn else np.minimum(u(*T0, 8 * n) - 273.15, 0.0)) * 2.0 ** 20) / 2.0 ** 20
    cand_r = u(1.2, 1.4, 8 * n)
    Qa = _ssq(sfc, cand_T, cand_r)
    keep = np.nonzero(_LD.f(Qa) - _ssq(sfc, cand_T, cand_r, _LD) >= 0)[0][:n]
    assert keep.size == n, "too few neutral candidates"
    base(cl)
    a["Tsf"][cl] = cand_T[keep]; a["rhoa"][cl] = cand_r[keep]; a["Qa"][cl] = Qa[keep]
    a["potT"][cl] = a["Tsf"][cl] + TFFRESH
    if ocn:      # sea-surface temperatures above, at and below freezing, wind speeds on both sides of the minimum of rdn (5.9 m/s)
        w = rng.permutation(np.geomspace(0.3, 45.0, 3 * n))
        base(cells["sst_above"], wind=w[:n]); a["Tsf"][cells["sst_above"]] = u(-1.7, 25.0)
        base(cells["sst_at"], wind=w[n:2 * n]); a["Tsf"][cells["sst_at"]] = SST_FREEZE
        base(cells["sst_below"], wind=w[2 * n:]); a["Tsf"][cells["sst_below"]] = u(-2.5, -1.81)
    mask |= constructed_mask(sfc)
    a = {k: np.ascontiguousarray(a[k]) for k in INS}
    sx, sy = rng.uniform(-1, 1, shp), rng.uniform(-1, 1, shp)
    return a, mask, sx, sy


def digest(a):
    h = hashlib.sha256()
    for k in sorted(a):
        h.update(k.encode())
        h.update(np.ascontiguousarray(a[k]).tobytes())
    return h.hexdigest()


def class_masks(sfctype, a, hol, mask):
    """{class: (ny, nx) bool} over the listed cells, from the inputs and hol of the five iterations"""
    neg = np.signbit(hol)
    TsfK = a["Tsf"] + TFFRESH
    delt0 = a["potT"] == TsfK
    m = dict(stable=~neg[4], unstable=neg[4], flip=neg.any(axis=0) & ~neg.all(axis=0), clamp_pos=hol[4] == 10.0,
             clamp_neg=hol[4] == -10.0, calm=a["wind"] < UMIN, at_umin=a["wind"] == UMIN,
             still=(a["wind"] == 0.0) & (a["uatm"] == 0.0) & (a["vatm"] == 0.0), alz0=a["zlvl"] == ZREF,
             ztrf=a["zlvl"] == ZTRF, delt0=delt0, neutral=delt0 & (a["Qa"] == _ssq(sfctype, a["Tsf"], a["rhoa"])),
             sst_above=a["Tsf"] > SST_FREEZE, sst_at=a["Tsf"] == SST_FREEZE, sst_below=a["Tsf"] < SST_FREEZE)
    return {k: v & mask for k, v in m.items()}


def branch_counts(sfctype, a, mask, ref, ours=None):
    """cells of the constructed part per class of BRANCHES: a cell counts where the inputs and the restatement's hol put it in
    the class AND the reference's outputs show it went that way -- all eight agree with the restatement to 1e-12 of the
    field's magnitude, the stresses are zeros where the air stands still, delt (and delq) are +0 where they are claimed to be"""
    want, hol = atmo_numpy(sfctype, *make_list(mask), a) if ours is None else ours
    agree = np.ones(mask.shape, bool)
    for k in OUT:
        agree &= np.abs(want[k] - ref[k]) <= 1e-12 * max(np.abs(ref[k]).max(), 1e-300)
    zero = lambda x: x.view(np.uint64) == 0  # noqa: E731
    did = dict(still=(ref["strx"] == 0.0) & (ref["stry"] == 0.0), delt0=zero(ref["delt"]),
               neutral=zero(ref["delt"]) & zero(ref["delq"]))
    m = class_masks(sfctype, a, hol, mask)
    con = constructed_mask(sfctype)
    return {k: (int((m[k] & con & agree & did.get(k, True)).sum()) if sfctype == "ocn" or k not in OCN_ONLY else 0)
            for k in BRANCHES}


def needed(sfctype):
    return {k: (NEED if sfctype == "ocn" or k not in OCN_ONLY else 0) for k in BRANCHES}


def ill_conditioned(hol, mask):
    """listed cells with 0 < |hol| < HOL_MIN in some iteration"""
    return (((hol != 0.0) & (np.abs(hol) < HOL_MIN)).any(axis=0)) & mask


def pack(mask, out):
    """what the fixture stores of a run: the values on the listed cells -- the caller has checked the rest"""
    return {k: np.ascontiguousarray(out[k][mask]) for k in OUT}


def unpack(d, prefix, mask, strx=None, stry=None):
    out = {}
    for k in OUT:
        x = np.zeros(mask.shape) if strx is None or k not in ("strx", "stry") else np.array(strx if k == "strx" else stry)
        x[mask] = d[f"{prefix}_{k}"]
        out[k] = x
    return out


def load_case(d, name):
    """from the fixture d (np.load): inputs, list mask and the reference's outputs of the case's run with calc_strair = T"""
    a = {k: np.ascontiguousarray(d[f"{name}_{k}"]) for k in INS}
    mask = np.zeros((NY, NX), bool)
    n = int(d[f"{name}_icells"])
    mask[d[f"{name}_indxj"][:n] - 1, d[f"{name}_indxi"][:n] - 1] = True
    return a, mask, unpack(d, name, mask)


def cell_deviation(x, truth, mask):
    """largest |x - truth| / |truth| over the listed cells, in float64; a cell whose truth is zero must hold a zero of the
    same sign and is not in the maximum (asserted here)"""
    t = truth[mask]
    v = np.asarray(x[mask], truth.dtype)
    z = t == 0
    assert np.array_equal(v[z] == 0, np.ones(int(z.sum()), bool)) and np.array_equal(np.signbit(v[z]), np.signbit(t[z])), \
        "a cell whose true value is a zero holds something else"
    if z.all():
        return 0.0
    return float((np.abs(v[~z] - t[~z]) / np.abs(t[~z])).max())


def reference_error(d, name):
    """E_ref[field] of a case: the reference's (the fixture's) largest per-cell relative deviation from atmo_truth over the
    listed cells, for the six outputs that pass through log and atan; and the truth itself"""
    a, mask, ref = load_case(d, name)
    truth, _ = atmo_truth(CASES[name]["sfctype"], *make_list(mask), a)
    return {k: cell_deviation(ref[k], truth[k], mask) for k in OUT_LOG}, truth
