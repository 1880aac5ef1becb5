"""Cases, inputs and bookkeeping shared by tests/golden/make_golden_ridge.py (which runs the compiled reference) and the
tests of ridging (test_ridge_golden.py, test_gpu_ridge.py).  No GPU here.

A case starts from the state s3 of a case of tests/golden/therm_itd.npz (what lateral_melt leaves on 4 blocks of 14 x 12),
brought to a sum of areas <= 0.98 as in cleanup_itd_case, and applies seeded edits so that the transport "has run": the
sum of areas and open water is off 1 by up to a few per cent, rdg_conv and rdg_shear are of the size the dynamics gives.
The list of a block is its physical tmask cells, ice or not (ice_step_mod.F90:621-631).  Block 1 is gentle (one
iteration), block 2 has cells whose open water runs out, block 3 cells whose thin categories run out one after the other,
block 4 the thin ice whose exp arguments leave the normal range; in the first case block 4 is all land instead.
The fixture stores what ridge_ice left as the XOR of its bit patterns with the inputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import cleanup_itd_case as cc  # noqa: E402
import therm_itd_case as tc  # noqa: E402
from cice4_amd import synth  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "ridge.npz")
NX, NY, NB, DT, PUNY = tc.NX, tc.NY, tc.NB, tc.DT, tc.PUNY
ILO, IHI, JLO, JHI = tc.ILO, tc.IHI, tc.JLO, tc.JHI
NCAT, NILYR, NSLYR = synth.NCAT, synth.NILYR, synth.NSLYR
TOCNFRZ = synth.Tocnfrz
MU_RDG = 4.0
# ice_mechred.F90:82-100
CS, GSTAR, ASTAR, MAXRAFT = 0.25, 0.15, 0.05, 1.0
DENORM = 2.2250738585072014e-308

CASES = {
    "ntr1": dict(base="growth", seed=2026102001, ntrcr=1, dep=(0,), partic=1, land_block=True),
    "ntr4": dict(base="tracers", seed=2026102002, ntrcr=4, dep=(0, 1, 0, 1), partic=1, land_block=False),
    "snow": dict(base="melt", seed=2026102003, ntrcr=2, dep=(0, 2), partic=1, land_block=False),
    "partic0": dict(base="growth", seed=2026102004, ntrcr=1, dep=(0,), partic=0, land_block=False),
}
ORDINARY = tuple(CASES)
STOP = "stop_aice0"
STOP_SEED = 2026102005
STATE = tc.STATE
DIAG = ("dardg1dt", "dardg2dt", "dvirdgdt", "opening")
OPTIONAL = DIAG + ("fresh", "fhocn")
IN_ONLY = ("rdg_conv", "rdg_shear")
OUT = STATE + ("aice0",) + OPTIONAL                    # what ridge_ice writes
BRANCHES = ("iter1_block", "iter2_block", "iter3_block", "bystander_roundtrip", "unlisted_zeroed", "untouched_block",
            "cut_open_water", "cut_category", "aice0_clamped", "convergent", "divergent_opening_only", "into_empty",
            "farea_zero", "exp_below_512", "exp_denormal", "exp_zero", "hi_clamped", "snow_to_ocean")
NEED = dict({k: 8 for k in BRANCHES}, iter1_block=1, iter2_block=1, iter3_block=1, untouched_block=1, exp_denormal=1,
            exp_zero=1, aice0_clamped=0)


def itd_kwargs(name):
    c = CASES[name] if name in CASES else CASES["ntr1"]
    four = c["ntrcr"] == 4
    return dict(hin_max=synth.hin_max(), ntrcr=c["ntrcr"], trcr_depend=c["dep"], nt_Tsfc=1, nt_iage=2 if four else 0,
                nt_alvl=3 if four else 0, nt_vlvl=4 if four else 0, tr_iage=four, tr_lvl=four, update_ocn_f=True,
                hi_min=tc.HI_MIN)


def ridge_kwargs(name):
    c = CASES[name] if name in CASES else CASES["ntr1"]
    return dict(krdg_partic=c["partic"], krdg_redist=1, mu_rdg=MU_RDG)


def tmask_list(tmask_b):
    """the physical tmask cells of a block, j then i: icells and 1-based indxi, indxj"""
    jj, ii = np.nonzero(tmask_b[JLO - 1:JHI, ILO - 1:IHI])
    return len(ii), tc.pad(ii + ILO), tc.pad(jj + JLO)


def listed_mask(tmask):
    inner = np.zeros(tmask.shape, bool)
    inner[..., JLO - 1:JHI, ILO - 1:IHI] = True
    return inner & (tmask != 0)


def _base(c):
    raw, chain = tc.load_chain(np.load(tc.FIXTURE), c["base"])
    s = {k: chain[3][k].copy() for k in STATE + ("fresh", "fhocn")}
    s["tmask"] = raw["tmask"].copy()
    tot = cc.cat_sum(s["aicen"])
    f = np.where(tot > 1.0, 0.98 / np.where(tot > 1.0, tot, 1.0), 1.0)
    for k, per in (("aicen", 1), ("vicen", 1), ("vsnon", 1), ("eicen", NILYR), ("esnon", NSLYR)):
        s[k] = s[k] * np.repeat(f[:, None], NCAT * per, axis=1)
    none = s["aicen"] == 0.0
    s["trcrn"][:, :, 1:][np.broadcast_to(none[:, :, None], s["trcrn"][:, :, 1:].shape)] = 0.0
    s["trcrn"][:, :, 0][none] = TOCNFRZ
    rng = np.random.default_rng(c["seed"])
    if c["dep"] == (0, 2):                   # a snow-volume tracer
        s["trcrn"][:, :, 1] = np.where(s["vsnon"] > 0.0, rng.uniform(0.1, 5.0, s["vsnon"].shape), 0.0)
    return s, rng


def _close(s, b, j, i, target):
    """aice0 of the cell such that aice0 + sum of areas is `target` (up to rounding)"""
    s["aice0"][b, j, i] = max(target - cc.cat_sum(s["aicen"][b][:, j:j + 1, i:i + 1])[0, 0], 0.0)


def _fill(s, b, n, j, i, a, h, rng):
    """category n of the cell: area a, thickness h, some snow, cold"""
    s["aicen"][b, n, j, i] = a
    s["vicen"][b, n, j, i] = a * h
    s["vsnon"][b, n, j, i] = a * 0.1
    s["eicen"][b, n * NILYR:(n + 1) * NILYR, j, i] = -3.0e8 * a * h / NILYR
    s["esnon"][b, n * NSLYR:(n + 1) * NSLYR, j, i] = -1.1e8 * a * 0.1 / NSLYR
    s["trcrn"][b, n, :, j, i] = 0.0
    s["trcrn"][b, n, 0, j, i] = -float(rng.uniform(1.0, 15.0))


def _edit(s, rng, c):
    shp = s["tmask"].shape
    a = s["aicen"]
    s["_used"] = np.zeros(shp, bool)
    # what the transport leaves: the total area off 1 by up to 2e-3 either way, on every cell
    s["aice0"] = np.maximum(1.0 - cc.cat_sum(a), 0.0) + rng.uniform(-2.0e-3, 2.0e-3, shp)
    s["aice0"] = np.where(s["aice0"] < 0.0, 0.0, s["aice0"])
    s["rdg_conv"] = np.where(rng.random(shp) < 0.5, rng.uniform(0.0, 2.0e-7, shp), 0.0)
    s["rdg_shear"] = rng.uniform(0.0, 4.0e-7, shp)
    for k in DIAG:
        s[k] = rng.uniform(-1.0, 1.0, shp)       # what was there before: kept on the cells that are not listed
    any_ice = (a > 0.05).any(axis=1)
    # block 1: divergent cells with opening only; receiving categories emptied
    b = 0
    for j, i in cc._cells(rng, s, b, any_ice[b], 10):
        s["rdg_conv"][b, j, i] = s["rdg_shear"][b, j, i] = 0.0
        _close(s, b, j, i, 1.0 - float(rng.uniform(1.0e-3, 2.0e-2)))
    for j, i in cc._cells(rng, s, b, a[b, 0] > 0.05, 10):
        for n in (3, 4):
            cc._empty(s, b, n, j, i)
        _close(s, b, j, i, 1.0 + float(rng.uniform(1.0e-3, 1.0e-2)))
    # block 2: little open water under strong convergence -- the open water runs out; and cells exactly at rest
    b = 1
    for j, i in cc._cells(rng, s, b, any_ice[b], 10):
        s["rdg_conv"][b, j, i] = float(rng.uniform(1.0e-5, 3.0e-5))
        tot = cc.cat_sum(a[b][:, j:j + 1, i:i + 1])[0, 0]
        r = (1.0 - float(rng.uniform(2.0e-3, 1.0e-2))) / tot
        for n in range(NCAT):
            cc._scale(s, b, n, j, i, r)
        _close(s, b, j, i, 1.0 + float(rng.uniform(0.0, 2.0e-3)))
    # blocks 2 and 3: cells at rest (total area exactly 1, no forcing): converged bystanders of the repeats
    for b in (1, 2):
        for j, i in cc._cells(rng, s, b, any_ice[b], 25):
            s["rdg_conv"][b, j, i] = s["rdg_shear"][b, j, i] = 0.0
            for _ in range(60):
                tot = s["aice0"][b, j, i]
                for n in range(NCAT):
                    tot = tot + a[b, n, j, i]
                if tot == 1.0:
                    break
                s["aice0"][b, j, i] = max(s["aice0"][b, j, i] + (1.0 - tot), 0.0)
                if s["aice0"][b, j, i] == 0.0:
                    n = int(np.argmax(a[b, :, j, i]))
                    a[b, n, j, i] += 1.0 - tot
    # block 3: two thin categories of little area, no open water, strong convergence: one runs out per iteration
    b = 2
    for j, i in cc._cells(rng, s, b, any_ice[b], 10):
        s["rdg_conv"][b, j, i] = float(rng.uniform(1.5e-5, 3.0e-5))
        _fill(s, b, 0, j, i, float(rng.uniform(2.0e-3, 4.0e-3)), float(rng.uniform(0.1, 0.5)), rng)
        _fill(s, b, 1, j, i, float(rng.uniform(3.0e-3, 6.0e-3)), float(rng.uniform(0.7, 1.3)), rng)
        if not (a[b, 2:, j, i] > 0.05).any():
            _fill(s, b, 3, j, i, 0.5, 3.0, rng)
        # (a cut scales closing and opening alike: only a total area off 1 makes the block repeat)
        r = (1.0 + float(rng.uniform(0.07, 0.09)) - a[b, 0, j, i] - a[b, 1, j, i]) / float(a[b, 2:, j, i].sum())
        for n in range(2, NCAT):
            cc._scale(s, b, n, j, i, r)
        s["aice0"][b, j, i] = 0.0
    # block 4: all land in the first case; else ice much thinner than anything the thermodynamics leaves, under empty
    # thicker categories: exp arguments below -512, results denormal or zero; hi below puny
    b = 3
    if c["land_block"]:
        s["tmask"][b] = 0
    else:
        for group in ("thin", "puny"):
            for j, i in cc._cells(rng, s, b, s["tmask"][b] != 0, 12):
                for n in range(NCAT):
                    cc._empty(s, b, n, j, i)
                if group == "puny":
                    hi = float(rng.uniform(1.0e-13, 9.0e-12))
                elif rng.random() < 0.5:
                    hi = float(np.exp(rng.uniform(np.log(1.0e-7), np.log(4.0e-6))))
                else:                    # exp(-hin_max(k)/hrexp) lands among the denormal numbers
                    hi = (float(synth.hin_max()[int(rng.integers(1, NCAT))]) / float(rng.uniform(700.0, 725.0)) / MU_RDG) ** 2
                _fill(s, b, 0, j, i, float(rng.uniform(0.2, 0.6)), hi, rng)   # alone: what it gives is all there is
                s["rdg_conv"][b, j, i] = float(rng.uniform(1.0e-6, 5.0e-6))
                _close(s, b, j, i, 1.0 + float(rng.uniform(0.0, 2.0e-3)))
    # every listed cell has something above puny (the reference divides by that sum)
    lm = listed_mask(s["tmask"])
    big = (s["aice0"] > PUNY) | (a > PUNY).any(axis=1)
    s["aice0"][lm & ~big] = 1.0
    del s["_used"]
    return {k: np.ascontiguousarray(v) for k, v in s.items()}


def case_inputs(name):
    """the edited state of an ordinary case, all blocks"""
    c = CASES[name]
    s, rng = _base(c)
    return _edit(s, rng, c)


def stop_inputs():
    """one block (block 1 of the first case's edits) with rdg_conv < 0 in two cells without open water: the new aice0 is
    below -puny there.  Returns the block and the two cells (i, j), 1-based, in list order."""
    c = dict(CASES["ntr1"], seed=STOP_SEED, land_block=False)
    s, rng = _base(c)
    s = _edit(s, rng, c)
    b = 0
    s["_used"] = np.zeros(s["tmask"].shape, bool)
    cells = cc._cells(rng, s, b, (s["aicen"][b] > 0.05).any(axis=0) & (s["tmask"][b] != 0), 2)
    for j, i in cells:
        tot = cc.cat_sum(s["aicen"][b][:, j:j + 1, i:i + 1])[0, 0]
        for n in range(NCAT):
            cc._scale(s, b, n, j, i, 0.999 / tot)
        s["aice0"][b, j, i] = 0.0
        s["rdg_conv"][b, j, i] = -1.0e-5
        s["rdg_shear"][b, j, i] = 0.0
    del s["_used"]
    blk = {k: np.ascontiguousarray(v[b]) for k, v in s.items()}
    cells = sorted(cells)                    # list order: j then i
    return blk, [(i + 1, j + 1) for j, i in cells]


def digest(s):
    return tc.digest(s)


def first_iteration(name, s):
    """ridge_prep, ridge_itd and the cuts of ridge_shift for the FIRST iteration, in numpy, on every cell (nb, ny, nx):
    what is needed to say which branch a cell took -- not a parity model (numpy's exp, no care for the last bit)."""
    kw = ridge_kwargs(name)
    hm = synth.hin_max()
    a, v, a0 = s["aicen"], s["vicen"], s["aice0"]
    with np.errstate(all="ignore"):
        asum = a0.copy()
        for n in range(NCAT):
            asum = asum + a[:, n]
        closing = CS * s["rdg_shear"] + s["rdg_conv"]
        divu = (1.0 - asum) / DT
        closing = np.where(divu < 0.0, np.maximum(closing, -divu), closing)
        opning = closing + divu
        G = [np.zeros_like(a0), np.where(a0 > PUNY, a0, 0.0)]
        for n in range(NCAT):
            G.append(np.where(a[:, n] > PUNY, G[-1] + a[:, n], G[-1]))
        w = 1.0 / G[-1]
        G = [G[0]] + [g * w for g in G[1:]]
        ap = []
        if kw["krdg_partic"] == 0:
            for n in range(NCAT + 1):
                gm, gn = G[n], G[n + 1]
                x = np.where(gn < GSTAR, (gn - gm) / GSTAR * (2.0 - (gm + gn) / GSTAR),
                             np.where(gm < GSTAR, (GSTAR - gm) / GSTAR * (2.0 - (gm + GSTAR) / GSTAR), 0.0))
                ap.append(x)
        else:
            x = 1.0 / (1.0 - np.exp(-1.0 / ASTAR))
            E = [np.exp(-g / ASTAR) * x for g in G]
            ap = [E[n] - E[n + 1] for n in range(NCAT + 1)]
        has = a > PUNY
        hraw = np.where(has, v / np.where(has, a, 1.0), 0.0)
        hi = np.maximum(hraw, PUNY)
        hrmin = np.where(has, np.minimum(2.0 * hi, hi + MAXRAFT), 0.0)
        hrexp = np.where(has, kw["mu_rdg"] * np.sqrt(hi), 0.0)
        krdg = np.where(has, (hrmin + hrexp) / hi, 1.0)
        aksum = ap[0].copy()
        for n in range(NCAT):
            aksum = aksum + ap[n + 1] * (1.0 - 1.0 / krdg[:, n])
        cg = closing / aksum
        wk = ap[0] * cg * DT
        cut0 = (ap[0] > 0.0) & (wk > a0)
        f = np.where(cut0, a0 / np.where(cut0, wk, 1.0), 1.0)
        cg, opn = cg * f, opning * f
        cutn = np.zeros_like(cut0)
        for n in range(NCAT):
            wk = ap[n + 1] * cg * DT
            cut = has[:, n] & (ap[n + 1] > 0.0) & (wk > a[:, n])
            f = np.where(cut, a[:, n] / np.where(cut, wk, 1.0), 1.0)
            cg, opn = cg * f, opn * f
            cutn |= cut
        aice0n = a0 - ap[0] * cg * DT + opn * DT
        rdg = has & (np.stack(ap[1:], axis=1) > 0.0) & (cg > 0.0)[:, None]
        # smallest exp argument of a ridging category: -(hin_max(ncat-1) - hrmin)/hrexp
        arg = np.where(rdg, -(np.maximum(hrmin, hm[NCAT - 1]) - hrmin) / np.where(rdg, hrexp, 1.0), 0.0)
        farea0 = rdg & (hrmin >= hm[1])
    return dict(asum=asum, closing=closing, opning=opning, cut0=cut0, cutn=cutn, aice0n=aice0n, rdg=rdg,
                argmin=arg.min(axis=1), farea0=farea0.any(axis=1), hi_clamped=(rdg & (hraw < PUNY)).any(axis=1))


def branch_counts(name, s, out, niter):
    """cells (or blocks) per branch of BRANCHES from the inputs s, what ridge_ice left and the iterations per block"""
    ntr = CASES[name]["ntrcr"]
    lm = listed_mask(s["tmask"])
    called = lm.reshape(NB, -1).any(axis=1)
    m = first_iteration(name, s)
    bits = cc.bits
    a0, a1 = s["aicen"], out["aicen"]
    t0, t1 = bits(s["trcrn"][:, :, :ntr]), bits(out["trcrn"][:, :, :ntr])
    tchg = (t0 != t1).reshape(NB, -1, NY, NX).any(axis=1)
    same_av = ((bits(a0) == bits(a1)) & (bits(s["vicen"]) == bits(out["vicen"]))).all(axis=1)
    rep = (np.asarray(niter) >= 2)[:, None, None]
    untouched = 0
    for b in range(NB):
        if not called[b] and all(tc.same(s[k][b], out[k][b]) for k in OUT) and (s["trcrn"][b] != 0.0).any():
            untouched += 1
    sn = (s["vsnon"] > 0.0) & (s["esnon"].reshape(NB, NCAT, NSLYR, NY, NX).sum(axis=2) < 0.0) & m["rdg"]
    c = dict(
        iter1_block=int(sum(1 for b in range(NB) if called[b] and niter[b] == 1)),
        iter2_block=int(sum(1 for b in range(NB) if called[b] and niter[b] == 2)),
        iter3_block=int(sum(1 for b in range(NB) if called[b] and niter[b] >= 3)),
        bystander_roundtrip=int((lm & rep & same_av & (m["closing"] == 0.0) & (m["opning"] == 0.0) & tchg).sum()),
        unlisted_zeroed=int((~lm & called[:, None, None] & ((s["trcrn"][:, :, 0] == TOCNFRZ) &
                                                            (bits(out["trcrn"][:, :, 0]) == 0)).any(axis=1)).sum()),
        untouched_block=untouched,
        cut_open_water=int((lm & m["cut0"]).sum()),
        cut_category=int((lm & m["cutn"]).sum()),
        # (the open water ran out and the new aice0 came out below zero by rounding; afterwards it takes no part)
        aice0_clamped=int((lm & m["cut0"] & (m["aice0n"] < 0.0) & (m["aice0n"] >= -PUNY) & (out["aice0"] == 0.0)).sum()),
        convergent=int((lm & (m["asum"] > 1.0)).sum()),
        divergent_opening_only=int((lm & (m["closing"] == 0.0) & (m["opning"] > 0.0) & (out["aice0"] > s["aice0"])).sum()),
        into_empty=int((lm & ((a0 == 0.0) & (a1 >= DENORM)).any(axis=1)).sum()),
        farea_zero=int((lm & m["farea0"]).sum()),
        exp_below_512=int((lm & (m["argmin"] < -512.0)).sum()),
        exp_denormal=int((lm & (m["argmin"] < -512.0) & ((a0 == 0.0) & (a1 > 0.0) & (a1 < DENORM)).any(axis=1)).sum()),
        exp_zero=int((lm & (m["argmin"] < -746.0) & (a0[:, NCAT - 1] == 0.0) & (a1[:, NCAT - 1] == 0.0)).sum()),
        hi_clamped=int((lm & m["hi_clamped"]).sum()),
        snow_to_ocean=int((lm & sn.any(axis=1) & (bits(out["fresh"]) != bits(s["fresh"])) &
                           (bits(out["fhocn"]) != bits(s["fhocn"]))).sum()),
    )
    return c


def load_case(d, name):
    """inputs, what ridge_ice left, the iterations per block -- from the fixture d (np.load) and the case module"""
    s = case_inputs(name)
    out = {k: v.copy() for k, v in s.items()}
    for k in OUT:
        out[k] = tc.unxor(d[f"{name}_out_{k}"], s[k]).reshape(s[k].shape)
    return s, out, d[f"{name}_niter"]
