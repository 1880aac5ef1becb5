"""Cases, inputs and bookkeeping shared by tests/golden/make_golden_coupling.py (which runs the compiled reference) and the
tests of the coupling stage (test_coupling_golden.py, test_gpu_coupling.py).  No GPU here.

A case is a set of seeded fields on 4 blocks of 14 x 12 (12 x 10 cells + ghosts, ncat = 5; 168 cells per plane) that puts
every branch of coupling_prep (drivers/cice4/CICE_RunMod.F90:643-755), scale_fluxes (source/ice_flux.F90:776-888) and
ocean_mixed_layer (source/ice_ocean.F90:64-234) on physical AND ghost cells: the routines run on every cell of a block.
The fixture tests/golden/coupling.npz holds what the compiled reference made of them: scale_fluxes called on the 13 fluxes
and the merged albedos, ocean_mixed_layer called through its module arrays, and atmo_boundary_layer('ocn') for the four
arrays ocean_mixed_layer keeps local (delt, delq, shcoef, lhcoef).

merge_numpy is the EXPECTED VALUE of the loops of coupling_prep themselves: they live in the driver file, which cannot be
compiled here (it drags in ice_history and ice_forcing, which need netCDF), so they are restated operation by operation in
the reference's order.  Every step is one correctly rounded IEEE operation -- products summed left to right from c0, one
subtraction and one product per term of scale_factor -- so float64 numpy gives the bits of the uncontracted Fortran.
scale_fluxes_numpy and mixed_tail_numpy are restatements of the same kind and ARE held to the compiled reference's bits
(test_coupling_golden.py); x**4 is ((x*x)*x)*x, the form that passes there ((x*x)*(x*x) does not).

Conditioning (asserted by the minter and again by test_coupling_golden.py; not a tolerance): on every ocean cell the
reference's sst differs from Tf by at least SST_MARGIN at both comparisons (ice_ocean.F90:219, :229), an unclamped frzmlt
differs from +-1000 by at least FRZMLT_MARGIN, and |hol| of the boundary layer is 0 or at least atmo_case.HOL_MIN in every
iteration: an error of an ulp in the device's log cannot move a cell across a branch.  No cell is left out of any
comparison."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import atmo_case as ac  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "coupling.npz")
NX, NY, NB, NCAT = 14, 12, 4, 5
PUNY = 1.0e-11
DT = 3600.0
ALBOCN = 0.06
# ice_constants.F90 (the stand-alone build)
STEFAN_BOLTZMANN, TFFRESH, LVAP, CPRHO, FRZMLT_MAX = 567.0e-10, 273.15, 2.501e6, 4218.0 * 1026.0, 1000.0
SST_MARGIN, FRZMLT_MARGIN = 1.0e-9, 1.0e-6
NSTREAMS_MAX = 2

CASES = {
    "standalone": dict(seed=2026102201, scale_fluxes=True, oceanmixed_ice=True, albpndn=False),
    "auscom": dict(seed=2026102202, scale_fluxes=False, oceanmixed_ice=False, albpndn=True),
    "nomix": dict(seed=2026102203, scale_fluxes=True, oceanmixed_ice=False, albpndn=True),
}
CAT_ALB = ("alvdrn", "alidrn", "alvdfn", "alidfn", "albicen", "albsnon", "albpndn")
IN2 = ("coszen", "aice", "Tf", "Tair", "Qa", "swvdr", "swvdf", "swidr", "swidf")
FLUXES = ("strairxT", "strairyT", "fsens", "flat", "fswabs", "flwout", "evap", "Tref", "Qref", "fresh", "fsalt", "fhocn",
          "fswthru")
ALB4 = ("alvdr", "alidr", "alvdf", "alidf")
SCALED = FLUXES + ALB4                         # the 17 arguments of scale_fluxes behind Qa, in its order
MERGED = ALB4 + ("albice", "albsno", "albpnd")
GBM = ("alvdf_gbm", "alidf_gbm", "alvdr_gbm", "alidr_gbm", "fresh_gbm", "fsalt_gbm", "fhocn_gbm", "fswthru_gbm")
OUT = MERGED + GBM + ("scale_factor",)
MIX_IN = ("potT", "uatm", "vatm", "wind", "zlvl", "rhoa", "flw", "hmix")
MIX_IO = ("sst", "qdp")
MIX_OUT = ("frzmlt", "flwout_ocn", "fsens_ocn", "flat_ocn", "evap_ocn", "strairx_ocn", "strairy_ocn", "Tref_ocn", "Qref_ocn",
           "alvdr_ocn", "alidr_ocn", "alvdf_ocn", "alidf_ocn")
MIX_OPT = ("delt", "delq", "shcoef", "lhcoef")
# the order of coupling_capture.F90's `in` planes
MIX_CAPTURE_IN = ("potT", "uatm", "vatm", "wind", "zlvl", "Qa", "rhoa", "flw", "hmix", "Tf", "aice", "fhocn", "fswthru",
                  "swvdr", "swvdf", "swidr", "swidf")
MIX_TAIL = ("sst", "qdp", "frzmlt", "flwout_ocn", "fsens_ocn", "flat_ocn", "evap_ocn")   # what :190-231 write
MIX_LOG = ("strairx_ocn", "strairy_ocn", "Tref_ocn", "Qref_ocn", "lhcoef", "shcoef")    # pass through log and atan
ATMO_NAME = dict(strairx_ocn="strx", strairy_ocn="stry", Tref_ocn="Tref", Qref_ocn="Qref", lhcoef="lhcoef", shcoef="shcoef",
                 delt="delt", delq="delq")
MIX_MASKS = ("qdp_zeroed", "clamp_hi", "clamp_lo", "reset")
BRANCHES = ("coszen_above", "coszen_at", "coszen_zero", "no_ice", "sf_scaled", "sf_ocean_noice", "sf_land_ice", "sf_tiny",
            "ml_land", "ml_qdp_zeroed", "ml_cold_qdp_kept", "ml_clamp_hi", "ml_clamp_lo", "ml_unclamped", "ml_reset",
            "ml_not_reset", "ml_aice_one", "ml_aice_zero")
NEED = 8


def physical(nb=NB, ny=NY, nx=NX):
    m = np.zeros((nb, ny, nx), bool)
    m[:, 1:-1, 1:-1] = True
    return m


def make_inputs(name, nb=NB, ny=NY, nx=NX, seed=None):
    """the fields of a case on (nb, ny, nx) blocks: tmask int32, per-category arrays (nb, ncat, ny, nx), 2-d fields
    (nb, ny, nx), albcnt (NSTREAMS_MAX, nb, ny, nx)"""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"] if seed is None else seed)
    shp, shc = (nb, ny, nx), (nb, NCAT, ny, nx)
    U = lambda lo, hi, shape=shp: rng.uniform(lo, hi, shape)  # noqa: E731
    s = dict(tmask=(rng.random(shp) < 0.8).astype(np.int32))
    # the thickness distribution: empty cells, cells that hold puny or less, cells that are full
    a = np.where(rng.random(shc) < 0.6, U(0.0, 0.19, shc), 0.0)
    a[rng.random(shc) < 0.04] = PUNY
    a[rng.random(shc) < 0.04] = 5.0e-12
    r = rng.random(shp)
    noice, tiny, full = r < 0.15, (r >= 0.15) & (r < 0.25), (r >= 0.25) & (r < 0.33)
    a = np.where((noice | tiny)[:, None], 0.0, a)
    cat = rng.integers(0, NCAT, shp)
    speck = np.where(rng.random(shp) < 0.4, PUNY, U(1.0e-13, 9.0e-12))
    for n in range(NCAT):
        a[:, n] = np.where(tiny & (cat == n), speck, a[:, n])
    a = np.where(full[:, None], 0.2, a)
    aice = np.zeros(shp)
    for n in range(NCAT):
        aice = aice + a[:, n]
    aice[full] = 1.0
    aice[(rng.random(shp) < 0.05) & ~full & ~tiny] = 0.0      # the aggregate says "no ice" while a category holds some
    s["aicen"], s["aice"] = a, aice
    ice = a > PUNY
    for k in CAT_ALB[:4]:
        s[k] = np.where(ice, U(0.06, 0.9, shc), ALBOCN)
    for k in CAT_ALB[4:]:
        s[k] = np.where(ice, U(0.0, 0.9, shc), 0.0)
    if not c["albpndn"]:
        del s["albpndn"]
    r = rng.random(shp)
    s["coszen"] = np.where(r < 0.6, U(0.05, 1.0), np.where(r < 0.8, PUNY, 0.0))
    s["Tf"] = np.where(rng.random(shp) < 0.5, -1.8, U(-1.95, -1.6))
    s["Tair"], s["Qa"] = U(240.0, 285.0), U(0.0005, 0.005)
    night = rng.random(shp) < 0.12
    for k in ("swvdr", "swvdf", "swidr", "swidf"):
        s[k] = np.where(night, 0.0, U(0.0, 120.0))
    rng_f = dict(strairxT=(-0.3, 0.3), strairyT=(-0.3, 0.3), fsens=(-50.0, 50.0), flat=(-30.0, 5.0), fswabs=(0.0, 200.0),
                 flwout=(-320.0, -200.0), evap=(-1.0e-5, 1.0e-6), Tref=(240.0, 285.0), Qref=(0.0005, 0.005),
                 fresh=(-1.0e-4, 1.0e-4), fsalt=(-1.0e-6, 1.0e-6), fhocn=(-150.0, 0.0), fswthru=(0.0, 30.0))
    for k in FLUXES:                         # grid box means: times the ice area
        s[k] = U(*rng_f[k]) * aice
    s["albcnt"] = rng.integers(0, 10, (NSTREAMS_MAX,) + shp).astype(np.float64)
    # the mixed layer: warm water, water within a few hundredths of a degree of freezing, supercooled water
    r = rng.random(shp)
    off = np.where(r < 0.35, U(0.5, 12.0), np.where(r < 0.7, U(-0.015, 0.015), -U(0.1, 0.6)))
    s["sst"] = s["Tf"] + off
    s["qdp"] = np.where(rng.random(shp) < 0.1, 0.0, U(-40.0, 40.0))
    s["hmix"], s["flw"] = U(10.0, 60.0), U(150.0, 350.0)
    s["potT"] = s["sst"] + TFFRESH + U(-12.0, 8.0)
    s["uatm"], s["vatm"] = U(-15.0, 15.0), U(-15.0, 15.0)
    calm = rng.random(shp) < 0.1
    for k in ("uatm", "vatm"):
        s[k] = np.where(calm, 0.02 * s[k], s[k])
    s["wind"] = np.sqrt(s["uatm"] ** 2 + s["vatm"] ** 2)
    s["zlvl"], s["rhoa"] = U(8.0, 40.0), U(1.2, 1.4)
    return {k: np.ascontiguousarray(x) for k, x in s.items()}


def case_inputs(name):
    return make_inputs(name)


def digest(s):
    h = hashlib.sha256()
    for k in sorted(s):
        h.update(k.encode())
        h.update(np.ascontiguousarray(s[k]).tobytes())
    return h.hexdigest()


def pow4(x):
    """x**4 as the reference's compiler evaluates it"""
    return ((x * x) * x) * x


def merge_numpy(s, nstreams=0):
    """coupling_prep :649-716 on every cell: the arrays of OUT (the four albedos unscaled) and albcnt"""
    shp = s["coszen"].shape
    lit = s["coszen"] > PUNY
    o = {k: np.zeros(shp) for k in MERGED}
    pnd = s.get("albpndn")
    for n in range(s["aicen"].shape[1]):
        a = s["aicen"][:, n]
        o["alvdf"] = o["alvdf"] + s["alvdfn"][:, n] * a
        o["alidf"] = o["alidf"] + s["alidfn"][:, n] * a
        o["alvdr"] = o["alvdr"] + s["alvdrn"][:, n] * a
        o["alidr"] = o["alidr"] + s["alidrn"][:, n] * a
        o["albice"] = np.where(lit, o["albice"] + s["albicen"][:, n] * a, o["albice"])
        o["albsno"] = np.where(lit, o["albsno"] + s["albsnon"][:, n] * a, o["albsno"])
        o["albpnd"] = np.where(lit, o["albpnd"] + (pnd[:, n] if pnd is not None else 0.0) * a, o["albpnd"])
    for k in ("alvdf", "alidf", "alvdr", "alidr"):
        o[k + "_gbm"] = o[k].copy()
    for k in ("fresh", "fsalt", "fhocn", "fswthru"):
        o[k + "_gbm"] = s[k].copy()
    one = np.float64(1.0)
    sf = s["swvdr"] * (one - o["alvdr_gbm"])
    sf = sf + s["swvdf"] * (one - o["alvdf_gbm"])
    sf = sf + s["swidr"] * (one - o["alidr_gbm"])
    o["scale_factor"] = sf + s["swidf"] * (one - o["alidf_gbm"])
    if nstreams:
        o["albcnt"] = s["albcnt"][:nstreams] + np.where(lit, 1.0, 0.0)[None]
    return o


def scale_fluxes_numpy(s, alb):
    """scale_fluxes on every cell: the 17 arrays of SCALED from the 13 fluxes of s and the four merged albedos `alb`"""
    scaled = (s["tmask"] != 0) & (s["aice"] > 0.0)
    with np.errstate(all="ignore"):
        ar = np.float64(1.0) / np.where(scaled, s["aice"], 1.0)
    src = {k: (s[k] if k in FLUXES else alb[k]) for k in SCALED}
    other = {k: np.zeros(s["aice"].shape) for k in SCALED}
    other["flwout"] = -STEFAN_BOLTZMANN * pow4(s["Tf"] + TFFRESH)
    other["Tref"], other["Qref"] = s["Tair"], s["Qa"]
    with np.errstate(all="ignore"):
        return {k: np.where(scaled, src[k] * ar, other[k]) for k in SCALED}


def expected(name, s, nstreams=0):
    """what cice_coupling_prep leaves of k_coupling_prep's outputs for a case's configuration"""
    o = merge_numpy(s, nstreams)
    if CASES[name]["scale_fluxes"]:
        o.update(scale_fluxes_numpy(s, o))
    return o


def mixed_tail_numpy(s, local, dt=DT, albocn=ALBOCN):
    """ice_ocean.F90:190-231 on the ocean cells and :125-130 on land, from the boundary layer's delt, delq, shcoef, lhcoef
    (`local`): the arrays of MIX_TAIL, the branch masks of MIX_MASKS, and what the conditioning looks at"""
    ocean = s["tmask"] != 0
    one, a = np.float64(1.0), np.float64(albocn)
    swabs = (one - a) * s["swvdr"] + (one - a) * s["swidr"] + (one - a) * s["swvdf"] + (one - a) * s["swidf"]
    TsfK = s["sst"] + TFFRESH
    flwout = -STEFAN_BOLTZMANN * pow4(TsfK)
    fsens = local["shcoef"] * local["delt"]
    flat = local["lhcoef"] * local["delq"]
    evap = -flat / LVAP
    sst1 = s["sst"] + dt * ((fsens + flat + flwout + s["flw"] + swabs) * (one - s["aice"]) + s["fhocn"] + s["fswthru"]) / \
        (CPRHO * s["hmix"])
    zeroed = (sst1 <= s["Tf"]) & (s["qdp"] > 0.0)
    qdp = np.where(zeroed, 0.0, s["qdp"])
    sst2 = sst1 - qdp * dt / (CPRHO * s["hmix"])
    raw = (s["Tf"] - sst2) * CPRHO * s["hmix"] / dt
    frzmlt = np.minimum(np.maximum(raw, -FRZMLT_MAX), FRZMLT_MAX)
    reset = sst2 <= s["Tf"]
    sst = np.where(reset, s["Tf"], sst2)
    o = dict(sst=sst, qdp=qdp, frzmlt=frzmlt, flwout_ocn=flwout, fsens_ocn=fsens, flat_ocn=flat, evap_ocn=evap)
    o = {k: np.where(ocean, v, s["qdp"] if k == "qdp" else 0.0) for k, v in o.items()}
    m = dict(qdp_zeroed=ocean & zeroed, cold_qdp_kept=ocean & (sst1 <= s["Tf"]) & ~zeroed, clamp_hi=ocean & (raw > FRZMLT_MAX),
             clamp_lo=ocean & (raw < -FRZMLT_MAX), reset=ocean & reset)
    m["unclamped"] = ocean & ~m["clamp_hi"] & ~m["clamp_lo"]
    return o, m, dict(sst1=sst1, sst2=sst2, raw=raw)


def masks_from_outputs(s, o):
    """the three branches of the tail as a run's OUTPUTS show them, (nb, ny, nx) bool each"""
    ocean = s["tmask"] != 0
    return dict(qdp_zeroed=ocean & (s["qdp"] > 0.0) & (o["qdp"] == 0.0),
                clamp_hi=ocean & (o["frzmlt"] == FRZMLT_MAX), clamp_lo=ocean & (o["frzmlt"] == -FRZMLT_MAX),
                reset=ocean & (o["sst"] == s["Tf"]))


def atmo_inputs(s, b):
    """block b's fields under atmo_case's names, and the list of its ocean cells"""
    a = {k: np.ascontiguousarray(s[k][b]) for k in ("potT", "uatm", "vatm", "wind", "zlvl", "Qa", "rhoa")}
    a["Tsf"] = np.ascontiguousarray(s["sst"][b])
    return a, ac.make_list(s["tmask"][b] != 0)


def atmo_all(s, fn):
    """fn = atmo_case.atmo_numpy or atmo_truth on the ocean cells of every block: ({coupling name: (nb, ny, nx)}, hol
    (nb, 5, ny, nx)); zero on land"""
    outs, hols = [], []
    for b in range(s["sst"].shape[0]):
        a, lst = atmo_inputs(s, b)
        o, hol = fn("ocn", *lst, a)
        outs.append(o); hols.append(hol)
    return {k: np.stack([o[v] for o in outs]) for k, v in ATMO_NAME.items()}, np.stack(hols)


def ill_conditioned(s, cond, m, hol):
    """ocean cells that break the conditioning, by rule"""
    ocean = s["tmask"] != 0
    return dict(sst_219=ocean & (np.abs(cond["sst1"] - s["Tf"]) < SST_MARGIN),
                sst_229=ocean & (np.abs(cond["sst2"] - s["Tf"]) < SST_MARGIN),
                frzmlt=m["unclamped"] & (np.abs(np.abs(cond["raw"]) - FRZMLT_MAX) < FRZMLT_MARGIN),
                hol=((hol != 0.0) & (np.abs(hol) < ac.HOL_MIN)).any(axis=1) & ocean)


def reference_error(s, mixed):
    """E_ref[field]: the reference's largest per-cell relative deviation from atmo_case.atmo_truth over the ocean cells, for
    the six outputs that pass through log and atan; and the truth itself"""
    truth, _ = atmo_all(s, ac.atmo_truth)
    ocean = s["tmask"] != 0
    return {k: ac.cell_deviation(mixed[k], truth[k], ocean) for k in MIX_LOG}, truth


def branch_counts(name, s, ref_scaled=None, ref_mixed=None):
    """{branch: (physical cells, ghost cells)}.  The branches of the merge are read from the inputs; those of scale_fluxes
    and of the mixed layer count a cell where the inputs put it on the branch AND the reference's outputs (ref_scaled: the 17
    of SCALED, ref_mixed: MIX_IO + MIX_OUT) show it went that way."""
    c = CASES[name]
    phys = physical(*s["coszen"].shape)
    ocean = s["tmask"] != 0
    m = dict(coszen_above=s["coszen"] > PUNY, coszen_at=s["coszen"] == PUNY, coszen_zero=s["coszen"] == 0.0,
             no_ice=(s["aicen"] == 0.0).all(axis=1))
    if c["scale_fluxes"]:
        r = ref_scaled
        went = (r["Tref"] == s["Tair"]) & (r["Qref"] == s["Qa"]) & (r["fresh"] == 0.0) & (r["alvdr"] == 0.0)
        did = (s["aice"] > 0.0) & ocean
        with np.errstate(all="ignore"):
            scaled = did & (r["fswabs"] == s["fswabs"] * (1.0 / np.where(did, s["aice"], 1.0)))
        m.update(sf_scaled=scaled, sf_ocean_noice=ocean & (s["aice"] == 0.0) & went, sf_land_ice=~ocean & (s["aice"] > 0.0) & went,
                 sf_tiny=scaled & (s["aice"] <= PUNY))      # 1 / aice is 1e11 or more
    if c["oceanmixed_ice"]:
        r = ref_mixed
        d = masks_from_outputs(s, r)
        land = ~ocean
        for k in ("sst", "frzmlt", "flwout_ocn", "fsens_ocn", "flat_ocn", "evap_ocn"):
            land = land & (r[k].view(np.uint64) == 0)
        cold = ocean & (r["sst"] == s["Tf"]) & (r["frzmlt"] > 0.0)
        m.update(ml_land=land, ml_qdp_zeroed=d["qdp_zeroed"], ml_cold_qdp_kept=cold & (s["qdp"] <= 0.0) & (r["qdp"] == s["qdp"]),
                 ml_clamp_hi=d["clamp_hi"], ml_clamp_lo=d["clamp_lo"],
                 ml_unclamped=ocean & (np.abs(r["frzmlt"]) < FRZMLT_MAX), ml_reset=d["reset"], ml_not_reset=ocean & ~d["reset"],
                 ml_aice_one=ocean & (s["aice"] == 1.0), ml_aice_zero=ocean & (s["aice"] == 0.0))
    return {k: (int((m[k] & phys).sum()), int((m[k] & ~phys).sum())) if k in m else (0, 0) for k in BRANCHES}


def short_of(total):
    """branches of {branch: (physical, ghost)} that occur too rarely"""
    return {k: v for k, v in total.items() if v[0] + v[1] < NEED or v[0] < 1 or v[1] < 1}


def u64(x):
    return np.ascontiguousarray(x).view(np.uint64)


def load_case(d, name):
    """inputs, and from the fixture d (np.load) what the reference left: (s, the 17 of SCALED or None, the mixed layer's
    MIX_IO + MIX_OUT + MIX_OPT or None)"""
    s = case_inputs(name)
    shp = s["coszen"].shape
    get = lambda k: d[f"{name}_{k}"].view(np.float64).reshape(shp)  # noqa: E731
    scaled = {k: get("sf_" + k) for k in SCALED} if CASES[name]["scale_fluxes"] else None
    mixed = {k: get("ml_" + k) for k in MIX_IO + MIX_OUT + MIX_OPT} if CASES[name]["oceanmixed_ice"] else None
    return s, scaled, mixed
