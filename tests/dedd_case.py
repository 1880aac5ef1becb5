"""Cases, inputs and bookkeeping shared by tests/golden/make_golden_dedd.py (which runs the compiled reference) and the tests
of the delta-Eddington shortwave stage (test_dedd_golden.py, test_gpu_dedd.py).  No GPU here.

A case is the state synth.therm2_state leaves on 4 blocks of 14 x 12 (12 x 10 cells + ghosts, ncat = 5) with seeded edits
that put the branches of shortwave_dEdd, compute_dEdd and solution_dEdd (source/ice_shortwave.F90:1372-3681) on the lists
step_radiation builds: the three surface types, every form of the snow fraction, clamped and unclamped surface scattering
layers, thin and thick ice, deep, shallow and too shallow ponds, snow so thick that the third band's beam dies in it (a
layer skipped by trntdr <= trmin, exp arguments beyond -512, transmissions held at exp_min), low and no sun, no
near-infrared, areas at or below puny, and one block without ice.  The case `tables` is block-wise (shortwave_dEdd alone,
fs, rhosnw, rsnw, fp, hp handed in) and walks the snow grain radius through every interval of the table.  The fixture
tests/golden/dedd.npz holds what the compiled reference made of them.

dedd_numpy is the scheme restated in numpy operation by operation in float64, in the reference's order and with its
parentheses; exp is the host's libm.so.6 through ctypes, the reference's own.  Every step is one correctly rounded IEEE
operation (or that exp), so it is expected to give the bits of the uncontracted Fortran.  The optical tables are READ from
cice4_amd/csrc/dedd_tables.h: what the fixture holds the restatement to, it holds the kernel's tables to."""
import ctypes as C
import ctypes.util
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import shortwave_case as sc  # noqa: E402
import therm_itd_case as tc  # noqa: E402
from cice4_amd import synth  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "dedd.npz")
NX, NY, NB, PUNY = sc.NX, sc.NY, sc.NB, sc.PUNY
NCAT, NILYR, NSLYR = sc.NCAT, sc.NILYR, sc.NSLYR
AWT = sc.AWT
SW = sc.SW
KLEV = NSLYR + NILYR + 1
HPMIN, HP0, HSMIN, HS0, TRMIN = 0.005, 0.2, 0.0001, 0.03, 0.001

CASES = {
    "default": dict(regime="mixed", seed=2026102021, R_ice=0.0, R_pnd=0.0, R_snw=0.0, tr_pond=False, blockwise=False),
    "tuned_pos": dict(regime="melt", seed=2026102022, R_ice=1.0, R_pnd=0.7, R_snw=1.5, tr_pond=False, blockwise=False, thin=0.5),
    # R_ice = -8: 1 + 0.15 R_ice = -0.2, so sigp < 0 in every band and max(sigp, 0) holds it at 0; R_pnd = -2.5 likewise
    "tuned_neg": dict(regime="growth", seed=2026102023, R_ice=-8.0, R_pnd=-2.5, R_snw=-1.0, tr_pond=False, blockwise=False,
                      thin=0.5),
    "tr_pond": dict(regime="melt", seed=2026102024, R_ice=0.0, R_pnd=0.0, R_snw=0.0, tr_pond=True, blockwise=False, thin=0.5),
    "tables": dict(regime="mixed", seed=2026102025, R_ice=0.0, R_pnd=0.0, R_snw=0.0, tr_pond=False, blockwise=True, thin=0.6),
}
DRIVER_CASES = tuple(k for k, c in CASES.items() if not c["blockwise"])
STATE = ("aicen", "vicen", "vsnon", "trcrn")
OUT2 = ("alvdrn", "alvdfn", "alidrn", "alidfn", "fswsfcn", "fswintn", "fswthrun", "albicen", "albsnon", "albpndn")
OUT = OUT2 + ("Sswabsn", "Iswabsn")
LAYERS = dict(Sswabsn=NSLYR, Iswabsn=NILYR)
BRANCHES = ("bare_pass", "snow_pass", "pond_pass", "fs_partial", "fs_one", "hs_below_hsmin", "snow_ssl_clamped",
            "snow_ssl_free", "hi_thin", "hi_thick", "pond_transition", "pond_deep", "pond_too_shallow", "layer_skipped",
            "at_exp_min", "exp_arg_beyond_512", "mu0_clamped", "no_sun", "no_nir", "unlisted_in_used", "sigp_clamped",
            "radius_below_table", "radius_above_table", "empty_block")
NEED = dict({k: 8 for k in BRANCHES}, empty_block=1)
NEED_INTERVALS = 1       # pairs per interval of the radius table, all 31 of them

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.exp.restype = C.c_double
_libm.exp.argtypes = [C.c_double]


def libm_exp(x):
    """the host libm's exp, element by element"""
    x = np.asarray(x, np.float64)
    f = _libm.exp
    return np.fromiter((f(v) for v in x.ravel().tolist()), np.float64, x.size).reshape(x.shape)


def init_kwargs(name):
    """arguments of Context.shortwave_dedd_init for a case"""
    c = CASES[name]
    return dict(R_ice=c["R_ice"], R_pnd=c["R_pnd"], R_snw=c["R_snw"], tr_pond=c["tr_pond"], **AWT)


def tables():
    """the constexpr double arrays of cice4_amd/csrc/dedd_tables.h by name"""
    src = open(os.path.join(ROOT, "cice4_amd", "csrc", "dedd_tables.h")).read()
    t = {}
    for m in re.finditer(r"constexpr double (\w+)\[(\d+)\] = \{(.*?)\};", src, re.S):
        v = np.array([float(x) for x in m.group(3).replace("\n", " ").split(",") if x.strip()])
        assert len(v) == int(m.group(2)), m.group(1)
        t[m.group(1)] = v
    for k in ("Qs_tab", "ws_tab", "gs_tab"):
        t[k] = t[k].reshape(32, 3)
    return t


TAB = tables()
GAUSPT = (.9894009, .9445750, .8656312, .7554044, .6178762, .4580168, .2816036, .0950125)
GAUSWT = (.0271525, .0622535, .0951585, .1246290, .1495960, .1691565, .1826034, .1894506)


def tuned(R_ice, R_pnd):
    """ki, wi, gi of ssl, dl, int, p_ssl, p_int per band (compute_dEdd :2357-2423), and whether max(sigp, 0) changed sigp"""
    one, zero = np.float64(1.0), np.float64(0.0)
    fi = one + np.float64(0.15) * np.float64(R_ice)
    fp = one + (np.float64(2.0) if R_pnd >= 0 else np.float64(0.5)) * np.float64(R_pnd)
    o, clamped = {}, False
    for name, f, neg in (("ssl", fi, R_ice < 0), ("dl", fi, R_ice < 0), ("int", fi, R_ice < 0), ("p_ssl", fp, R_pnd < 0),
                         ("p_int", fp, R_pnd < 0)):
        k_mn, w_mn = TAB[f"ki_{name}_mn"], TAB[f"wi_{name}_mn"]
        sigp = k_mn * w_mn * f
        if neg:
            clamped |= name in ("ssl", "dl", "int") and bool((sigp < 0).any())
            sigp = np.maximum(sigp, zero)
        o["ki_" + name] = sigp + k_mn * (one - w_mn)
        o["wi_" + name] = sigp / o["ki_" + name]
        o["gi_" + name] = TAB[f"gi_{name}_mn"]
    return o, clamped


def block_table(nb=NB, ny=NY, nx=NX):
    return sc.block_table(nb, ny, nx)


def make_inputs(name, nb=NB, ny=NY, nx=NX, seed=None):
    c = CASES[name]
    seed = c["seed"] if seed is None else seed
    blk = block_table(nb, ny, nx)
    raw = synth.therm2_state(c["regime"], nx, ny, nb, seed=seed, ntrcr=1)
    s = {k: raw[k].copy() for k in STATE}
    rng = np.random.default_rng(seed + 7)
    shp = (nb, ny, nx)
    a, v, vs, T = s["aicen"], s["vicen"], s["vsnon"], s["trcrn"][:, :, 0]
    if "thin" in c:                          # fewer pairs with ice: the fixture stores what the lists hold
        drop = rng.random(a.shape) < c["thin"]
        for k in (a, v, vs):
            k[drop] = 0.0
    for k in SW:
        s[k] = rng.uniform(0.0, 120.0, shp)
    s["coszen"] = rng.uniform(0.05, 1.0, shp)
    free = sc.physical(blk, ny, nx)[:, None] & (a > 0.01)
    free[nb - 1] = False
    n_each = 12
    pick = lambda count=n_each: sc._pick(rng, free, count)  # noqa: E731
    cell = lambda t: (t[0], t[2], t[3])  # noqa: E731
    # snow: none to speak of, partial cover, full cover with the ssl at half the layer, full cover with the 4 cm ssl
    t = pick(); vs[t] = a[t] * np.where(rng.random(n_each) < 0.3, 0.0, rng.uniform(1.0e-6, 9.0e-5, n_each))
    t = pick(); vs[t] = a[t] * rng.uniform(1.1e-4, 0.029, n_each)
    t = pick(); vs[t] = a[t] * rng.uniform(0.031, 0.078, n_each)
    t = pick(); vs[t] = a[t] * rng.uniform(0.09, 0.5, n_each)
    # cold snow so thick that the third band's beam dies in it
    t = pick(); vs[t] = a[t] * rng.uniform(1.0, 3.0, n_each); T[t] = -rng.uniform(2.0, 20.0, n_each)
    s["coszen"][cell(t)] = rng.uniform(0.3, 1.0, n_each)
    # thin and thick ice
    t = pick(); v[t] = a[t] * rng.uniform(0.05, 1.4, n_each)
    t = pick(); v[t] = a[t] * rng.uniform(1.6, 4.0, n_each)
    # ponds by surface temperature (set_pond): shallow (the transition), deep, too shallow for a pass
    t = pick(); T[t] = -rng.uniform(0.4, 0.95, n_each); vs[t] = 0.0
    t = pick(); T[t] = 0.0; vs[t] = a[t] * np.where(rng.random(n_each) < 0.5, 0.0, rng.uniform(1.1e-4, 0.009, n_each))
    t = pick(); T[t] = -(1.0 - rng.uniform(1.0e-4, 0.016, n_each)); vs[t] = 0.0
    for tt in (t,):
        s["coszen"][cell(tt)] = rng.uniform(0.2, 1.0, n_each)
    # the sun on the horizon (mu0 held at 0.01), and below it
    t = pick(); s["coszen"][cell(t)] = rng.uniform(2.0e-11, 0.0099, n_each)
    t = pick(); s["coszen"][cell(t)] = rng.choice([0.0, PUNY, -0.2, 5.0e-12], n_each)
    # no near-infrared
    t = pick()
    for k in ("swidr", "swidf"):
        s[k][cell(t)] = 0.0
    # areas at or below puny in categories that other cells hold
    t = pick(); a[t] = np.where(rng.random(n_each) < 0.5, PUNY, rng.uniform(1.0e-13, 9.0e-12, n_each))
    for k in ("aicen", "vicen", "vsnon"):
        s[k][nb - 1] = 0.0
    s["trcrn"][nb - 1, :, 0] = synth.Tocnfrz
    full = (nb, NCAT, ny, nx)
    if c["tr_pond"]:
        s["apondn"] = np.where(rng.random(full) < 0.7, rng.uniform(0.0, 0.5, full), 0.0)
        s["hpondn"] = np.where(rng.random(full) < 0.5, rng.uniform(0.0, 0.4, full), rng.uniform(0.0, 0.012, full))
    if c["blockwise"]:                       # what the caller of shortwave_dEdd hands in
        on = listed(s, blk)
        hs = rng.uniform(0.01, 0.6, full)
        vs[...] = np.where(on, hs * a, vs)
        s["fs"] = np.where(on, np.where(rng.random(full) < 0.8, rng.uniform(0.05, 1.0, full), 1.0), 0.0)
        s["fp"] = np.where(on & (rng.random(full) < 0.3), rng.uniform(0.0, 1.0, full) * (1.0 - s["fs"]), 0.0)
        s["hp"] = np.where(s["fp"] > 0.0, rng.uniform(0.0, 0.4, full), 0.0)
        s["rhosnw"] = np.where(on, rng.uniform(100.0, 500.0, full), 0.0)[:, :, None] + np.zeros((nb, NCAT, NSLYR, ny, nx))
        # the radius: fr * rsnw inside interval (count mod 33) of the table, 0 below the first entry, 32 at or above the last
        tab = TAB["rsnw_tab"]
        edges = np.concatenate([[2.0], tab, [4000.0]])
        which = (np.cumsum(on.ravel()).reshape(full) - 1) % 33
        lo, hi = edges[which], edges[which + 1]
        x = lo + (hi - lo) * rng.uniform(0.1, 0.9, full)
        fn = _fnidr(s["swidr"], s["swidf"])[:, None] + np.zeros(full)
        fr = np.float64(1.0) * fn + np.float64(0.8) * (np.float64(1.0) - fn)
        s["rsnw"] = np.where(on, x / fr, 0.0)[:, :, None] + np.zeros((nb, NCAT, NSLYR, ny, nx))
    return {k: np.ascontiguousarray(x) for k, x in s.items()}


def case_inputs(name):
    return make_inputs(name)


def digest(s):
    return tc.digest(s)


def listed(s, blk=None):
    nb, ncat, ny, nx = s["aicen"].shape
    blk = block_table(nb, ny, nx) if blk is None else blk
    return sc.listed(s, blk)


def _fnidr(swidr, swidf):
    tot = swidr + swidf
    with np.errstate(all="ignore"):
        return np.where(tot > PUNY, swidr / np.where(tot > PUNY, tot, 1.0), 0.0)


def set_snow_numpy(name, s, on):
    """fs, rhosnw, rsnw of shortwave_dEdd_set_snow on the listed pairs (zero elsewhere); (nb, ncat, ny, nx)"""
    one, zero = np.float64(1.0), np.float64(0.0)
    a = np.where(on, s["aicen"], one)
    hs = s["vsnon"] / a
    fs = np.where(hs < HSMIN, zero, np.where(hs <= HS0, hs / np.float64(HS0), one))
    dTs = zero - s["trcrn"][:, :, 0]
    fT = -np.minimum(dTs / one - one, zero)
    r_nm = np.float64(500.0) - np.float64(CASES[name]["R_snw"]) * np.float64(250.0)
    r_nm = min(max(r_nm, np.float64(100.0)), np.float64(1000.0))
    r = r_nm + (np.float64(1000.0) - r_nm) * fT
    r = np.minimum(np.maximum(r, np.float64(100.0)), np.float64(1000.0))
    return np.where(on, fs, zero), np.where(on, np.float64(330.0), zero), np.where(on, r, zero), fT


def _layer(p, exp_min, tau, w0, g, mu0, mu0n_above, fresnel, stats):
    """solution_dEdd's layer solution (:3244-3390) on 1-d arrays; fresnel: bool array"""
    one, c3, c4, p5, p75, c1p5, c2 = (np.float64(x) for x in (1.0, 3.0, 4.0, 0.5, 0.75, 1.5, 2.0))
    refindx = np.float64(1.31)
    ftot = g * g
    ts = (one - w0 * ftot) * tau
    ws = (one - ftot) * w0 / (one - w0 * ftot)
    gs = (g - ftot) / (one - ftot)
    lm = np.sqrt(c3 * (one - ws) * (one - ws * gs))
    ue = c1p5 * (one - ws * gs) / lm
    mu0n = np.sqrt(one - ((one - mu0 * mu0) / (refindx * refindx)))
    mu0n = np.where(mu0n_above, mu0, mu0n)

    def alpha(uu):
        return p75 * ws * uu * ((one + gs * (one - ws)) / (one - lm * lm * uu * uu))

    def gamma(uu):
        return p5 * ws * ((one + c3 * gs * (one - ws) * uu * uu) / (one - lm * lm * uu * uu))

    def ex(arg):
        e = libm_exp(arg)
        stats["at_min"] |= e <= exp_min
        stats["beyond"] |= arg < -512.0
        return np.maximum(exp_min, e)

    extins = ex(-lm * ts)
    ne = ((ue + one) * (ue + one) / extins) - ((ue - one) * (ue - one) * extins)
    rdif_a = (ue + one) * (ue - one) * (one / extins - extins) / ne
    tdif_a = c4 * ue / ne
    trnlay = ex(-ts / mu0n)
    alp, gam = alpha(mu0n), gamma(mu0n)
    apg, amg = alp + gam, alp - gam
    rdir = amg * (tdif_a * trnlay - one) + apg * rdif_a
    tdir = apg * tdif_a + (amg * rdif_a - (apg - one)) * trnlay
    swt, smr, smt = np.float64(0.0), np.zeros_like(tau), np.zeros_like(tau)
    for mu, gwt in zip(GAUSPT, GAUSWT):
        mu, gwt = np.float64(mu), np.float64(gwt)
        swt = swt + mu * gwt
        trn = ex(-ts / mu)
        alp, gam = alpha(mu), gamma(mu)
        apg, amg = alp + gam, alp - gam
        rdr = amg * (tdif_a * trn - one) + apg * rdif_a
        tdr = apg * tdif_a + (amg * rdif_a - (apg - one)) * trn
        smr = smr + mu * rdr * gwt
        smt = smt + mu * tdr * gwt
    rdif_a = smr / swt
    tdif_a = smt / swt
    rdif_b, tdif_b = rdif_a, tdif_a
    # the refracting boundary
    R1 = (mu0 - refindx * mu0n) / (mu0 + refindx * mu0n)
    R2 = (refindx * mu0 - mu0n) / (refindx * mu0 + mu0n)
    T1 = c2 * mu0 / (mu0 + refindx * mu0n)
    T2 = c2 * mu0 / (refindx * mu0 + mu0n)
    Rf_dir_a = p5 * (R1 * R1 + R2 * R2)
    Tf_dir_a = p5 * (T1 * T1 + T2 * T2) * refindx * mu0n / mu0
    Rf_dif_a, Rf_dif_b = np.float64(0.063), np.float64(0.455)
    Tf_dif_a, Tf_dif_b = one - Rf_dif_a, one - Rf_dif_b
    rintfc = one / (one - Rf_dif_b * rdif_a)
    f_tdir = Tf_dir_a * tdir + Tf_dir_a * rdir * Rf_dif_b * rintfc * tdif_a
    f_rdir = Rf_dir_a + Tf_dir_a * rdir * rintfc * Tf_dif_b
    f_rdif_a = Rf_dif_a + Tf_dif_a * rdif_a * rintfc * Tf_dif_b
    f_rdif_b = rdif_b + tdif_b * Rf_dif_b * rintfc * tdif_a
    f_tdif_a = Tf_dif_a * rintfc * tdif_a
    f_tdif_b = tdif_b * rintfc * Tf_dif_b
    f_trnlay = Tf_dir_a * trnlay
    w = lambda x, y: np.where(fresnel, x, y)  # noqa: E731
    return dict(rdir=w(f_rdir, rdir), rdif_a=w(f_rdif_a, rdif_a), rdif_b=w(f_rdif_b, rdif_b), tdir=w(f_tdir, tdir),
                tdif_a=w(f_tdif_a, tdif_a), tdif_b=w(f_tdif_b, tdif_b), trnlay=w(f_trnlay, trnlay))


def _snow_iops(ns, fr, rsnw, rhosnw, stats):
    one = np.float64(1.0)
    tab = TAB["rsnw_tab"]
    x = fr * rsnw
    below, above = x < tab[0], x >= tab[31]
    nr = np.clip(np.searchsorted(tab, x, side="right"), 1, 31)
    stats["below"] |= below
    stats["above"] |= above
    stats["interval"] = np.where(below | above, -1, nr - 1)
    delr = (x - tab[nr - 1]) / (tab[nr] - tab[nr - 1])
    o = []
    for k in ("Qs_tab", "ws_tab", "gs_tab"):
        t = TAB[k][:, ns]
        o.append(np.where(below, t[0], np.where(above, t[31], t[nr - 1] * (one - delr) + t[nr] * delr)))
    ks = o[0] * ((rhosnw / np.float64(917.0)) * np.float64(3.0) / (np.float64(4.0) * fr * rsnw * np.float64(1.0e-6)))
    return ks, o[1], o[2]


def _compute_pass(P, exp_min, srftyp, c, hs, hi, fnidr, stats):
    """compute_dEdd for the surface type on 1-d arrays c[...]; returns avdr, avdf, aidr, aidf, fsfc, fint, fthru, Sabs, Iabs"""
    one, zero, c2 = np.float64(1.0), np.float64(0.0), np.float64(2.0)
    n = len(hi)
    z = np.zeros(n)
    o = dict(avdr=z, avdf=z, aidr=z, aidf=z, fsfc=z, fint=z, fthru=z, Sabs=[z] * NSLYR, Iabs=[z] * NILYR)
    wght = (one, np.float64(0.67) + (np.float64(0.78) - np.float64(0.67)) * (one - fnidr),
            np.float64(0.33) + (np.float64(0.22) - np.float64(0.33)) * (one - fnidr))
    mu0 = np.maximum(c["coszen"], np.float64(0.01))
    stats["mu0_clamped"] |= c["coszen"] < 0.01
    if srftyp == 1:
        dzs = hs / np.float64(NSLYR)
        dzs_ssl = np.minimum(np.float64(0.04), dzs / c2)
        stats["ssl_clamped"] |= dzs / c2 < 0.04
        stats["ssl_free"] |= ~(dzs / c2 < 0.04)
        fr = one * fnidr + np.float64(0.8) * (one - fnidr)
    elif srftyp == 2:
        dzs = c["hp"] / np.float64(NSLYR + 1)
    dz = hi / np.float64(NILYR)
    dz_ssl = np.where(hi < 1.5, hi / np.float64(30.0), np.float64(0.05))
    dz_ssl = np.minimum(dz_ssl, dz / c2)
    fsdl = np.float64(NILYR) / np.float64(4)
    trans = (HPMIN <= c["hp"]) & (c["hp"] <= HP0) if srftyp == 2 else np.zeros(n, bool)
    kii = NSLYR + 1
    for ns in range(3):
        g_ = lambda name: P[name][ns]  # noqa: E731
        tau, w0, g = [], [], []
        for k in range(KLEV + 1):
            if k <= NSLYR:
                if srftyp == 0:
                    t, w, gg = z, z, z
                elif srftyp == 1:
                    ksn = k - 1 if k > 1 else 0
                    ks, w, gg = _snow_iops(ns, fr, c["rsnw"][ksn], c["rhosnw"][ksn], stats)
                    t = ks * dzs_ssl if k == 0 else (ks * (dzs - dzs_ssl) if k == 1 else ks * dzs)
                else:
                    t, w, gg = TAB["kw"][ns] * dzs, z + TAB["ww"][ns], z + TAB["gw"][ns]
            elif srftyp <= 1:
                if k == KLEV:
                    kabs = g_("ki_int") * (one - g_("wi_int"))
                    if ns == 0:
                        kabs = kabs + np.float64(0.6) * (np.float64(0.5) / dz)
                    sig = g_("ki_int") * g_("wi_int")
                    t, w, gg = (kabs + sig) * dz, sig / (sig + kabs) + z, z + g_("gi_int")
                elif k == kii:
                    t, w, gg = g_("ki_ssl") * dz_ssl, z + g_("wi_ssl"), z + g_("gi_ssl")
                elif k == kii + 1:
                    t, w, gg = g_("ki_dl") * (dz - dz_ssl) * fsdl, z + g_("wi_dl"), z + g_("gi_dl")
                else:
                    t, w, gg = g_("ki_int") * dz, z + g_("wi_int"), z + g_("gi_int")
            else:
                if k == kii:
                    t, w, gg = g_("ki_p_ssl") * dz_ssl, z + g_("wi_p_ssl"), z + g_("gi_p_ssl")
                    sig_i, sig_p, kab, thick = g_("ki_ssl") * g_("wi_ssl"), g_("ki_p_ssl") * g_("wi_p_ssl"), \
                        g_("ki_p_ssl") * (one - g_("wi_p_ssl")), dz_ssl
                elif k == kii + 1:
                    t, w, gg = g_("ki_p_int") * (dz - dz_ssl), z + g_("wi_p_int"), z + g_("gi_p_int")
                    sig_i, sig_p, kab, thick = g_("ki_dl") * g_("wi_dl") * fsdl, g_("ki_p_int") * g_("wi_p_int"), \
                        g_("ki_p_int") * (one - g_("wi_p_int")), dz - dz_ssl
                else:
                    t, w, gg = g_("ki_p_int") * dz, z + g_("wi_p_int"), z + g_("gi_p_int")
                    sig_i, sig_p, kab, thick = g_("ki_int") * g_("wi_int"), g_("ki_p_int") * g_("wi_p_int"), \
                        g_("ki_p_int") * (one - g_("wi_p_int")), dz
                sig = sig_i + (sig_p - sig_i) * (c["hp"] / np.float64(HP0))
                kext = sig + kab
                t = np.where(trans, kext * thick, t)
                w = np.where(trans, sig / kext, w)
                gg = np.where(trans, g_("gi_p_int"), gg)
            tau.append(t); w0.append(w); g.append(gg)
        # downward sweep
        trndir, trntdr, trndif, rdndif = [z + one], [z + one], [z + one], [z]
        L = []
        kfr = NSLYR + 2 if srftyp < 2 else 0
        with np.errstate(all="ignore"):
            for k in range(KLEV + 2):
                if k > 0:
                    m = L[k - 1]
                    trndir.append(trndir[k - 1] * m["trnlay"])
                    refkm1 = one / (one - rdndif[k - 1] * m["rdif_a"])
                    tdrrdir = trndir[k - 1] * m["rdir"]
                    tdndif = trntdr[k - 1] - trndir[k - 1]
                    trntdr.append(trndir[k - 1] * m["tdir"] + (tdndif + tdrrdir * rdndif[k - 1]) * refkm1 * m["tdif_a"])
                    rdndif.append(m["rdif_b"] + (m["tdif_b"] * rdndif[k - 1] * refkm1 * m["tdif_a"]))
                    trndif.append(trndif[k - 1] * refkm1 * m["tdif_a"])
                if k == KLEV + 1:
                    break
                go = trntdr[k] > TRMIN
                stats["skipped"] |= ~go
                sub = dict(at_min=np.zeros(n, bool), beyond=np.zeros(n, bool))
                sol = _layer(P, exp_min, tau[k], w0[k], g[k], mu0, np.full(n, srftyp < 2 and k < kfr), np.full(n, k == kfr), sub)
                stats["at_min"] |= sub["at_min"] & go
                stats["beyond"] |= sub["beyond"] & go
                L.append({q: np.where(go, x, zero) for q, x in sol.items()})
            # upward sweep and interface fluxes
            swdr, swdf = (c["swvdr"], c["swvdf"]) if ns == 0 else (c["swidr"], c["swidf"])
            rupdir = z + (np.float64(0.01) if ns == 0 else zero)
            rupdif = rupdir
            F = [None] * (KLEV + 2)
            for k in range(KLEV + 1, -1, -1):
                if k <= KLEV:
                    m = L[k]
                    refkp1 = one / (one - m["rdif_b"] * rupdif)
                    rupdir = m["rdir"] + (m["trnlay"] * rupdir + (m["tdir"] - m["trnlay"]) * rupdif) * refkp1 * m["tdif_b"]
                    rupdif = m["rdif_a"] + m["tdif_a"] * rupdif * refkp1 * m["tdif_b"]
                refk = one / (one - rdndif[k] * rupdif)
                fdirup = (trndir[k] * rupdir + (trntdr[k] - trndir[k]) * rupdif) * refk
                fdirdn = trndir[k] + (trntdr[k] - trndir[k] + trndir[k] * rupdir * rdndif[k]) * refk
                fdifup = trndif[k] * rupdif * refk
                fdifdn = trndif[k] * refk
                F[k] = (fdirdn - fdirup) * swdr + (fdifdn - fdifup) * swdf
        Fsrf = F[1] if srftyp == 1 else F[NSLYR + 2]
        bot = KLEV + 1
        if ns == 0:
            o["avdr"], o["avdf"] = rupdir, rupdif
            o["fsfc"] = o["fsfc"] + F[0] - Fsrf
            o["fint"] = o["fint"] + Fsrf - F[bot]
            o["fthru"] = o["fthru"] + F[bot]
            if srftyp == 1:
                o["Sabs"] = [o["Sabs"][k - 1] + F[k] - F[k + 1] for k in range(1, NSLYR + 1)]
            o["Iabs"] = [o["Iabs"][k - NSLYR - 2] + (F[k - 1] if srftyp == 1 and k == NSLYR + 2 else F[k]) - F[k + 1]
                         for k in range(NSLYR + 2, NSLYR + 2 + NILYR)]
        else:
            w = wght[ns]
            o["aidr"] = o["aidr"] + rupdir * w
            o["aidf"] = o["aidf"] + rupdif * w
            o["fsfc"] = o["fsfc"] + (F[0] - Fsrf) * w
            o["fint"] = o["fint"] + (Fsrf - F[bot]) * w
            o["fthru"] = o["fthru"] + F[bot] * w
            if srftyp == 1:
                o["Sabs"] = [o["Sabs"][k - 1] + (F[k] - F[k + 1]) * w for k in range(1, NSLYR + 1)]
            o["Iabs"] = [o["Iabs"][k - NSLYR - 2] + ((F[k - 1] if srftyp == 1 and k == NSLYR + 2 else F[k]) - F[k + 1]) * w
                         for k in range(NSLYR + 2, NSLYR + 2 + NILYR)]
    return o


def dedd_numpy(name, s, blk=None):
    """the scheme for every (block, category) of a case: the arrays of OUT ((nb, ncat[, layers], ny, nx)) and the branch
    masks `m` ((nb, ncat, ny, nx) bool by name, `interval` int: the radius table's interval the snow pass used, -1 none)"""
    c = CASES[name]
    nb, ncat, ny, nx = s["aicen"].shape
    full = (nb, ncat, ny, nx)
    on = listed(s, blk)
    P, sig_clamped = tuned(c["R_ice"], c["R_pnd"])
    exp_min = np.float64(_libm.exp(-10.0))
    one, zero = np.float64(1.0), np.float64(0.0)
    bc = lambda x: x[:, None] + np.zeros(full)  # noqa: E731
    cosz = bc(s["coszen"])
    if c["blockwise"]:
        fs, fp, hp = s["fs"], s["fp"], s["hp"]
        rhosnw, rsnw = s["rhosnw"], s["rsnw"]
    else:
        fs, rho1, r1, fT = set_snow_numpy(name, s, on)
        rhosnw = np.stack([rho1] * NSLYR, axis=2)
        rsnw = np.stack([r1] * NSLYR, axis=2)
        if c["tr_pond"]:
            fp, hp = s["apondn"], s["hpondn"]
        else:
            fp = np.where(on, np.float64(0.3) * fT * (one - fs), zero)
            hp = fp
    act = on & (cosz > PUNY)
    idx = np.nonzero(act.ravel())[0]
    flat = lambda x: x.ravel()[idx]  # noqa: E731
    col = dict(coszen=flat(cosz), hp=flat(hp), rsnw=[flat(rsnw[:, :, k]) for k in range(NSLYR)],
               rhosnw=[flat(rhosnw[:, :, k]) for k in range(NSLYR)], **{k: flat(bc(s[k])) for k in SW})
    aice, vice, vsno = flat(s["aicen"]), flat(s["vicen"]), flat(s["vsnon"])
    fsf, fpf = flat(fs), flat(fp)
    fnidr = _fnidr(col["swidr"], col["swidf"])
    hi = vice / aice
    hs = vsno / aice
    fi = one - fsf - fpf
    n = len(idx)
    res = {k: np.zeros(n) for k in OUT2}
    res["Sswabsn"] = [np.zeros(n) for _ in range(NSLYR)]
    res["Iswabsn"] = [np.zeros(n) for _ in range(NILYR)]
    names = ("mu0_clamped", "ssl_clamped", "ssl_free", "skipped", "at_min", "beyond", "below", "above")
    m = {k: np.zeros(n, bool) for k in names}
    interval = np.full(n, -1)
    took = {}
    for srftyp, frac, take, hist in ((0, fi, fi > zero, "albicen"), (1, fsf, fsf > zero, "albsnon"),
                                     (2, fpf, (fpf > PUNY) & (col["hp"] > HPMIN), "albpndn")):
        took[srftyp] = take
        sel = np.nonzero(take)[0]
        if not len(sel):
            continue
        cs = {k: ([x[sel] for x in v] if isinstance(v, list) else v[sel]) for k, v in col.items()}
        st = {k: np.zeros(len(sel), bool) for k in names}
        st["interval"] = np.full(len(sel), -1)
        o = _compute_pass(P, exp_min, srftyp, cs, hs[sel] if srftyp else np.zeros(len(sel)), hi[sel], fnidr[sel], st)
        f = frac[sel]
        for k in names:
            m[k][sel] |= st[k]
        if srftyp == 1:
            interval[sel] = st["interval"]
        for dst, src in (("fswsfcn", "fsfc"), ("fswintn", "fint"), ("fswthrun", "fthru"), ("alvdrn", "avdr"), ("alvdfn", "avdf"),
                         ("alidrn", "aidr"), ("alidfn", "aidf")):
            res[dst][sel] = res[dst][sel] + o[src] * f
        for k in range(NSLYR):
            res["Sswabsn"][k][sel] = res["Sswabsn"][k][sel] + o["Sabs"][k] * f
        for k in range(NILYR):
            res["Iswabsn"][k][sel] = res["Iswabsn"][k][sel] + o["Iabs"][k] * f
        w = {k: np.float64(AWT[k]) for k in AWT}
        res[hist][sel] = zero + w["awtvdr"] * o["avdr"] + w["awtidr"] * o["aidr"] + w["awtvdf"] * o["avdf"] + w["awtidf"] * o["aidf"]

    def unflat(x, dtype=np.float64, fill=0):
        a = np.full(act.size, fill, dtype)
        a[idx] = x
        return a.reshape(full)

    out = {k: unflat(res[k]) for k in OUT2}
    for k in ("Sswabsn", "Iswabsn"):
        out[k] = np.stack([unflat(x) for x in res[k]], axis=2)
    hpf = col["hp"]
    M = dict(on=on, active=act,
             bare_pass=unflat(took[0], bool), snow_pass=unflat(took[1], bool), pond_pass=unflat(took[2], bool),
             fs_partial=unflat((fsf > 0) & (fsf < 1), bool), fs_one=unflat(fsf == 1, bool),
             hs_below_hsmin=unflat((hs < HSMIN) & (fsf == 0), bool),
             snow_ssl_clamped=unflat(m["ssl_clamped"], bool), snow_ssl_free=unflat(m["ssl_free"], bool),
             hi_thin=unflat(hi < 1.5, bool), hi_thick=unflat(hi >= 1.5, bool),
             pond_transition=unflat(took[2] & (hpf >= HPMIN) & (hpf <= HP0), bool), pond_deep=unflat(took[2] & (hpf > HP0), bool),
             pond_too_shallow=unflat((fpf > PUNY) & (hpf <= HPMIN), bool),
             layer_skipped=unflat(m["skipped"], bool), at_exp_min=unflat(m["at_min"], bool),
             exp_arg_beyond_512=unflat(m["beyond"], bool), mu0_clamped=unflat(m["mu0_clamped"], bool),
             no_sun=on & ~(cosz > PUNY), no_nir=unflat(~(col["swidr"] + col["swidf"] > PUNY), bool),
             radius_below_table=unflat(m["below"], bool), radius_above_table=unflat(m["above"], bool),
             sigp_clamped=act & sig_clamped, interval=unflat(interval, np.int64, -1))
    used = on.reshape(nb, ncat, -1).any(axis=2)[:, :, None, None]
    M["unlisted_in_used"] = sc.physical(block_table(nb, ny, nx) if blk is None else blk, ny, nx)[:, None] & ~on & used
    return {k: np.ascontiguousarray(x) for k, x in out.items()}, M


def rel_err(got, want):
    """largest deviation in units of the field's magnitude"""
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def branch_counts(name, s, out, m=None):
    """(cell, category) pairs per branch of BRANCHES (blocks for empty_block), and pairs per interval of the radius table:
    a pair counts where the inputs put it on the branch (the restatement's masks) AND the recorded outputs show the
    reference went that way -- its history albedo of the pass is positive where a pass is claimed, it left zeros where
    none is, and all its outputs of the pair agree with the restatement to 1e-12 of the field's magnitude."""
    if m is None:
        ours, m = dedd_numpy(name, s)
    else:
        ours, m = m
    nb = s["aicen"].shape[0]
    agree = np.ones(m["on"].shape, bool)
    for k in OUT:
        d = np.abs(ours[k] - out[k]) <= 1e-12 * max(np.abs(out[k]).max(), 1e-300)
        agree &= d.all(axis=2) if k in LAYERS else d
    dark = np.ones(m["on"].shape, bool)
    for k in OUT:
        zk = out[k] == 0.0
        dark &= zk.all(axis=2) if k in LAYERS else zk
    lit = (out["albicen"] > 0) | (out["albsnon"] > 0) | (out["albpndn"] > 0)
    did = dict(bare_pass=out["albicen"] > 0, snow_pass=out["albsnon"] > 0, pond_pass=out["albpndn"] > 0,
               pond_transition=out["albpndn"] > 0, pond_deep=out["albpndn"] > 0,
               pond_too_shallow=(out["albpndn"] == 0) & lit, hs_below_hsmin=(out["albsnon"] == 0) & lit,
               fs_partial=out["albsnon"] > 0, fs_one=out["albsnon"] > 0, snow_ssl_clamped=out["albsnon"] > 0,
               snow_ssl_free=out["albsnon"] > 0, radius_below_table=out["albsnon"] > 0, radius_above_table=out["albsnon"] > 0,
               no_sun=dark, unlisted_in_used=dark)
    c = {}
    for k in BRANCHES:
        if k == "empty_block":
            continue
        c[k] = int((m[k] & did.get(k, lit) & agree).sum())
    c["empty_block"] = int(sum(1 for b in range(nb) if not m["on"][b].any() and dark[b].all()))
    iv = np.array([int(((m["interval"] == i) & (out["albsnon"] > 0) & agree).sum()) for i in range(31)], np.int64)
    return c, iv


def pack(name, s, out):
    """what the fixture stores of a case's outputs: the values on the pairs where the scheme ran (the lists, sun up) -- the
    minter has checked that every other word is +0"""
    act = listed(s) & ((s["coszen"] > PUNY)[:, None])
    d = {}
    for k in OUT:
        x = np.moveaxis(out[k], 2, -1) if k in LAYERS else out[k]
        rest = x[~act]
        assert not rest.view(np.uint64).any(), (name, k, "a word off the lists is not +0")
        d[f"{name}_{k}"] = np.ascontiguousarray(x[act]).view(np.uint64)
    return d


def load_case(d, name):
    """inputs and what the reference left, from the fixture d (np.load) and the case module"""
    s = case_inputs(name)
    act = listed(s) & ((s["coszen"] > PUNY)[:, None])
    out = {}
    for k in OUT:
        shp = act.shape + ((LAYERS[k],) if k in LAYERS else ())
        x = np.zeros(shp)
        x[act] = d[f"{name}_{k}"].view(np.float64).reshape((-1,) + shp[4:])
        out[k] = np.ascontiguousarray(np.moveaxis(x, -1, 2)) if k in LAYERS else x
    return s, out
