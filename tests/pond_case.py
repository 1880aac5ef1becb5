"""Cases, inputs and bookkeeping shared by tests/golden/make_golden_pond.py (which runs the compiled reference) and the tests
of the pond stage (test_pond_golden.py, test_gpu_pond.py).  No GPU here.

A case is a seeded state on 4 blocks of 14 x 12 (12 x 10 cells + ghosts, ncat = 5: the shape of shortwave_case / dedd_case)
that puts the branches of compute_ponds (source/ice_meltpond.F90:88-229) and the list of increment_age (source/ice_age.F90:
87-123) on the table: thin ice that keeps its pond tracer, surfaces warmer and colder than Tp = -2, volumes that transport
round-off left slightly negative, pond fractions clamped at 1 and depths limited by 0.9 hi, snow over a pond, volumes of
exactly zero.  Ghost cells, ice-free cells and thin ice carry stale non-zero apondn, hpondn and volpn, and every tracer plane
the routines do not own carries random words, so that a wrong store shows.  The cases differ in their tracer slots on purpose.

pond_numpy and age_numpy restate the two routines in numpy operation by operation in float64, in the reference's order; min
and max are the compare-and-select of the reference's compiler; exp is the host's libm.so.6 through ctypes (dedd_case), the
reference's own.  Every step is one correctly rounded IEEE operation (or that exp), so they are expected to give the bits of
the uncontracted Fortran: the minter asserts that in every word before it writes tests/golden/pond.npz."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import dedd_case as dc  # noqa: E402
import shortwave_case as sc  # noqa: E402
import therm_itd_case as tc  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "pond.npz")
NX, NY, NB, NCAT, PUNY = sc.NX, sc.NY, sc.NB, sc.NCAT, sc.PUNY
NTRCR = 5                                # max_ntrcr of ice_domain_size
DT = 3600.0
# drivers/cice4/ice_constants.F90 and the parameters of compute_ponds (:141-147)
RHOS, RHOI, RHOFRESH, TIMELT = 330.0, 917.0, 1000.0, 0.0
HICEMIN, TD, RFRAC, REXP, DPTHHI, DPTHFRAC = 0.1, 2.0, 0.1, 0.01, 0.9, 0.8

CASES = {
    # surface at or near 0 C, top melt, snow melt and rain; snow-free and snow-covered columns
    "melt": dict(seed=2026102101, regime="melt", tr_iage=True, nt_Tsfc=1, nt_iage=2, nt_volpn=3, ponds=True, age=True),
    # surface down to -40 C, no rain, ponds inherited from before
    "freeze": dict(seed=2026102102, regime="freeze", tr_iage=True, nt_Tsfc=1, nt_iage=3, nt_volpn=5, ponds=True, age=True),
    "age_only": dict(seed=2026102103, regime="melt", tr_iage=True, nt_Tsfc=1, nt_iage=2, nt_volpn=0, ponds=False, age=True),
    # a tracer set without iage, the surface temperature not in the first slot
    "no_age": dict(seed=2026102104, regime="melt", tr_iage=False, nt_Tsfc=2, nt_iage=0, nt_volpn=1, ponds=True, age=False),
}
IN_CAT = ("aicen", "vicen", "vsnon", "melttn", "meltsn")
OUT = ("apondn", "hpondn", "volpn", "iage")
BRANCHES = ("off_list_stale", "ghost_stale", "thin_with_tracer", "dTs_zero", "dTs_pos", "clamp_negative", "frac_clamped",
            "frac_free", "depth_limited", "depth_free", "snow_with_hpond", "no_snow", "zero_volume")
NEED = {k: 8 for k in BRANCHES}          # the project's figure (make_golden_coupling.py)
MARGIN = 1e-9                            # conditioning of the four comparisons


def block_table(nb=NB, ny=NY, nx=NX):
    return sc.block_table(nb, ny, nx)


def outputs_of(name):
    """the members of OUT a case's flags make the routines write"""
    c = CASES[name]
    return (("apondn", "hpondn", "volpn") if c["ponds"] else ()) + (("iage",) if c["age"] else ())


def make_inputs(name, nb=NB, ny=NY, nx=NX, seed=None, fill=0.55):
    c = CASES[name]
    rng = np.random.default_rng(c["seed"] if seed is None else seed)
    full, shp = (nb, NCAT, ny, nx), (nb, ny, nx)
    u = lambda lo, hi, s=full: rng.uniform(lo, hi, s)  # noqa: E731
    pick = lambda p, s=full: rng.random(s) < p  # noqa: E731
    warm = c["regime"] == "melt"
    a = np.where(pick(fill), u(0.02, 0.3), 0.0)
    a[pick(0.04)] = PUNY                                   # at and below the list's threshold
    a[pick(0.04)] = 5.0e-12
    hi = np.where(pick(0.25), u(0.12, 0.6), u(0.6, 3.0))   # thin-ish ice: where 0.9 hi limits the depth
    hi = np.where(pick(0.12), u(0.01, 0.095), hi)          # below hicemin
    hs = np.where(pick(0.5), 0.0, u(0.01, 0.5))            # snow-free (exactly) and snow-covered
    s = dict(aicen=a, vicen=hi * a, vsnon=hs * a)
    s["trcrn"] = u(-50.0, 50.0, (nb, NCAT, NTRCR, ny, nx))  # what the routines must leave alone
    T = u(-1.5, 0.0) if warm else u(-40.0, -0.1)
    if warm:
        T[pick(0.3)] = 0.0
        T = np.where(pick(0.15), u(-12.0, -2.5), T)        # a few cold surfaces: dTs > 0 in the melt case too
    s["trcrn"][:, :, c["nt_Tsfc"] - 1] = T
    if c["tr_iage"]:
        s["trcrn"][:, :, c["nt_iage"] - 1] = u(0.0, 1.0e7)
    if c["nt_volpn"]:
        vol = np.where(pick(0.35), 0.0, u(0.0, 0.3))
        vol = np.where(pick(0.12), u(0.8, 1.6), vol)       # more than the fraction can hold
        vol[pick(0.04)] = -1.0e-12                         # what transport round-off leaves
        s["trcrn"][:, :, c["nt_volpn"] - 1] = vol
    if warm:
        s["melttn"] = np.where(pick(0.6), u(0.0, 0.02), 0.0)
        s["meltsn"] = np.where((hs > 0.0) & pick(0.6), u(0.0, 0.01), 0.0)
        s["frain"] = np.where(pick(0.7, shp), u(0.0, 1.0e-4, shp), 0.0)
    else:
        s["melttn"] = np.where(pick(0.1), u(0.0, 0.001), 0.0)
        s["meltsn"] = np.zeros(full)
        s["frain"] = np.zeros(shp)
    # stale ponds everywhere: ghost cells, ice-free cells, thin ice
    s["apondn"] = u(0.01, 0.5)
    s["hpondn"] = u(0.01, 0.4)
    return {k: np.ascontiguousarray(v) for k, v in s.items()}


def case_inputs(name):
    return make_inputs(name)


def digest(s):
    return tc.digest(s)


def listed(s, blk=None):
    """(nb, ncat, ny, nx): aicen > puny on the physical cells -- the list of both routines"""
    nb, ncat, ny, nx = s["aicen"].shape
    return sc.listed(s, block_table(nb, ny, nx) if blk is None else blk)


def pond_numpy(name, s, dt=DT, blk=None):
    """compute_ponds for every (block, category): apondn, hpondn and the volpn plane as the routine leaves them (inputs off
    the list), and the branch masks m ((nb, ncat, ny, nx) bool by name; `cond`: the four conditioning margins)"""
    c = CASES[name]
    on = listed(s, blk)
    f8 = np.float64
    zero, one = f8(0.0), f8(1.0)
    a = np.where(on, s["aicen"], one)
    vol0 = s["trcrn"][:, :, c["nt_volpn"] - 1]
    T = s["trcrn"][:, :, c["nt_Tsfc"] - 1]
    frain = s["frain"][:, None] + np.zeros(on.shape)
    with np.errstate(all="ignore"):
        hi = s["vicen"] / a
        hs = s["vsnon"] / a
        thin = on & (hi < f8(HICEMIN))
        run = on & ~thin
        v1 = vol0 + f8(RFRAC) * (s["melttn"] * f8(RHOI) / f8(RHOFRESH) + s["meltsn"] * f8(RHOS) / f8(RHOFRESH) +
                                 frain * f8(dt) / f8(RHOFRESH))
        Tp = f8(TIMELT) - f8(TD)
        d = Tp - T
        dTs = np.where(d > zero, d, zero)
        arg = f8(REXP) * dTs / Tp
        e = np.ones(on.shape)
        e[run] = dc.libm_exp(arg[run])
        v2 = v1 * e
        v3 = np.where(v2 > zero, v2, zero)
        r = np.sqrt(v3 / f8(DPTHFRAC))
        ap = np.where(r < one, r, one)
        hp = f8(DPTHFRAC) * ap
        lim = f8(DPTHHI) * hi
        hp2 = np.where(hp < lim, hp, lim)
        v4 = hp2 * ap
        snow = hs > f8(PUNY)
        ap2 = np.where(snow, zero, ap)
    out = dict(apondn=np.where(run, ap2, np.where(thin, zero, s["apondn"])),
               hpondn=np.where(run, hp2, np.where(thin, zero, s["hpondn"])),
               volpn=np.where(run, v4, vol0))
    nb, ncat, ny, nx = on.shape
    phys = sc.physical(block_table(nb, ny, nx) if blk is None else blk, ny, nx)[:, None] & np.ones(on.shape, bool)
    stale = (s["apondn"] != 0) & (s["hpondn"] != 0) & (vol0 != 0)
    m = dict(on=on, run=run,
             off_list_stale=phys & ~on & stale, ghost_stale=~phys & stale,
             thin_with_tracer=thin & (vol0 != 0),
             dTs_zero=run & (dTs == 0), dTs_pos=run & (dTs > 0),
             clamp_negative=run & (v2 < 0), frac_clamped=run & ~(r < one), frac_free=run & (r < one),
             depth_limited=run & ~(hp < lim), depth_free=run & (hp < lim),
             snow_with_hpond=run & snow & (hp2 != 0), no_snow=run & ~snow, zero_volume=run & (v3 == 0))
    # an exactly snow-free column (vsnon = 0, hs = 0 with no rounding anywhere) cannot change sides of hs > puny
    cond = dict(hi=np.abs(hi - HICEMIN)[on], hs=np.abs(hs - PUNY)[run & (s["vsnon"] != 0)], frac=np.abs(r - 1.0)[run],
                depth=np.abs(hp - lim)[run])
    m["cond"] = cond
    return {k: np.ascontiguousarray(v) for k, v in out.items()}, m


def age_numpy(name, s, dt=DT, on=None):
    """increment_age on the list `on` (default: the ice list): the iage plane"""
    on = listed(s) if on is None else on
    iage = s["trcrn"][:, :, CASES[name]["nt_iage"] - 1]
    return np.ascontiguousarray(np.where(on, iage + np.float64(dt), iage))


def restate(name, s):
    """what the case's flags make of s: the members of outputs_of(name), and pond_numpy's masks (None without ponds)"""
    c = CASES[name]
    out, m = pond_numpy(name, s) if c["ponds"] else ({}, None)
    if c["age"]:
        out["iage"] = age_numpy(name, s)
    return out, m


def branch_counts(name, s, out):
    """(cell, category) pairs per branch: where the inputs put a pair on the branch (the restatement's masks) AND the
    reference's words of the pair are the restatement's, in every output"""
    if not CASES[name]["ponds"]:
        return {k: 0 for k in BRANCHES}
    ours, m = pond_numpy(name, s)
    agree = np.ones(m["on"].shape, bool)
    for k in ("apondn", "hpondn", "volpn"):
        agree &= ours[k].view(np.uint64) == np.ascontiguousarray(out[k]).view(np.uint64)
    return {k: int((m[k] & agree).sum()) for k in BRANCHES}


def pack(name, s, out):
    """what the fixture stores of a case's outputs: the words on the pairs where the list ran"""
    on = listed(s)
    return {f"{name}_{k}": np.ascontiguousarray(out[k][on]).view(np.uint64) for k in outputs_of(name)}


def load_case(d, name):
    """inputs and what the reference left -- the recorded words on the list, the inputs everywhere else -- from the fixture
    d (np.load) and the case module"""
    c = CASES[name]
    s = case_inputs(name)
    on = listed(s)
    src = dict(apondn=s["apondn"], hpondn=s["hpondn"])
    if c["nt_volpn"]:
        src["volpn"] = s["trcrn"][:, :, c["nt_volpn"] - 1]
    if c["tr_iage"]:
        src["iage"] = s["trcrn"][:, :, c["nt_iage"] - 1]
    out = {}
    for k in outputs_of(name):
        x = np.array(src[k])
        x[on] = d[f"{name}_{k}"].view(np.float64)
        out[k] = x
    return s, out
