"""Cases, inputs and bookkeeping shared by tests/golden/make_golden_therm_itd.py (which runs the compiled reference) and
the tests of the thickness-distribution stage (test_therm_itd_golden.py, test_gpu_therm_itd.py).  No GPU here.

A case is a chain per block, as step_therm2 runs it (ice_step_mod.F90:286-422): s0 = synth.therm2_state after the rain
term and aggregate_area (done here in numpy: one multiply-add, one sum in category order), s1 after linear_itd, s2 after
add_new_ice, s3 after lateral_melt.  The fixture stores s1, s2, s3 as the XOR of their bit patterns with the state in
front (most of a state does not change in a step, and zeros compress), plus seeds, hashes and what the reference
reported."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from cice4_amd import synth  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "therm_itd.npz")
NX, NY, NB = 14, 12, 4          # configuration small: 12 x 10 cells + ghosts, 4 blocks
DT, YDAY, HI_MIN = 3600.0, 100.5, 0.01
PUNY = 1.0e-11
ILO, IHI, JLO, JHI = 2, NX - 1, 2, NY - 1

CASES = {
    "growth": dict(regime="growth", seed=2026101801, ntrcr=1, dep=(0,), update_ocn_f=True),
    "melt": dict(regime="melt", seed=2026101802, ntrcr=1, dep=(0,), update_ocn_f=True),
    "tracers": dict(regime="mixed", seed=2026101803, ntrcr=4, dep=(0, 1, 0, 1), update_ocn_f=True),
    "noflux": dict(regime="growth", seed=2026101801, ntrcr=1, dep=(0,), update_ocn_f=False),
}
ORDINARY = tuple(CASES)
STOP_SEED = 2026101804
STATE = ("aicen", "vicen", "vsnon", "trcrn", "eicen", "esnon")
OUT1 = STATE + ("aice", "aice0")                                            # what linear_itd writes
OUT2 = ("aicen", "vicen", "trcrn", "eicen", "aice0", "frazil", "frz_onset", "fresh", "fsalt")   # add_new_ice
OUT3 = ("aicen", "vicen", "vsnon", "eicen", "esnon", "fresh", "fsalt", "fhocn", "meltl")        # lateral_melt
CHAIN = STATE + ("aice", "aice0", "fresh", "fsalt", "fhocn", "frazil", "meltl", "frz_onset")
BRANCHES = ("thicker", "thinner", "cat1_loss", "emptied", "unchanged", "new_cat1", "new_spread", "surplus_only",
            "ghost_new", "melt_snow", "melt_nosnow")


def itd_kwargs(c):
    """arguments of Context.itd_init / cap_set for a case"""
    four = c["ntrcr"] == 4
    return dict(hin_max=synth.hin_max(), ntrcr=c["ntrcr"], trcr_depend=c["dep"], nt_Tsfc=1, nt_iage=2 if four else 0,
                nt_alvl=3 if four else 0, nt_vlvl=4 if four else 0, tr_iage=four, tr_lvl=four,
                update_ocn_f=c["update_ocn_f"], hi_min=HI_MIN)


def case_inputs(name):
    """(raw synth state, s0): s0 = the state after the rain term and aggregate_area, all blocks"""
    c = CASES[name]
    raw = synth.therm2_state(c["regime"], NX, NY, NB, seed=c["seed"], ntrcr=c["ntrcr"])
    s0 = {k: v.copy() for k, v in raw.items()}
    s0["fresh"] = raw["fresh"] + raw["frain"] * raw["aice"]
    aice = np.zeros_like(raw["aice"])
    for n in range(synth.NCAT):
        aice = aice + raw["aicen"][:, n]
    s0["aice"] = aice
    s0["aice0"] = np.maximum(1.0 - aice, 0.0)
    return raw, s0


def digest(s):
    h = hashlib.sha256()
    for k in sorted(s):
        h.update(k.encode())
        h.update(np.ascontiguousarray(s[k]).tobytes())
    return h.hexdigest()


def ice_list(aice_b):
    """cells with aice > puny on the physical domain, j then i (ice_step_mod.F90:316-325): 1-based indxi, indxj"""
    jj, ii = np.nonzero(aice_b[JLO - 1:JHI, ILO - 1:IHI] > PUNY)
    return len(ii), pad(ii + ILO), pad(jj + JLO)


def ocean_list(tmask_b):
    """every tmask cell of the whole block (ice_step_mod.F90:366-376)"""
    jj, ii = np.nonzero(tmask_b)
    return len(ii), pad(ii + 1), pad(jj + 1)


def pad(a):
    out = np.zeros(NX * NY, np.int32)
    out[:len(a)] = a
    return out


def block(s, b, names=None):
    """contiguous copies of block b of the named arrays"""
    return {k: np.ascontiguousarray(s[k][b]) for k in (names or s)}


def xor(a, b):
    return np.ascontiguousarray(a).view(np.uint64) ^ np.ascontiguousarray(b).view(np.uint64)


def unxor(x, b):
    return (x ^ np.ascontiguousarray(b).view(np.uint64)).view(np.float64)


def load_chain(d, name):
    """s0..s3 of a case from the fixture d (np.load) -- s0 from synth -- and the raw inputs"""
    raw, s0 = case_inputs(name)
    chain = [s0]
    for k in (1, 2, 3):
        prev = chain[-1]
        cur = {key: v.copy() for key, v in prev.items()}
        for key in CHAIN:
            cur[key] = unxor(d[f"{name}_s{k}_{key}"], prev[key]).reshape(prev[key].shape)
        chain.append(cur)
    return raw, chain


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def branch_counts(chain, ntrcr):
    """cells per branch of BRANCHES, from the states of one case"""
    s0, s1, s2, s3 = chain
    a0, a1, a2 = s0["aicen"], s1["aicen"], s2["aicen"]
    v1, v2 = s1["vicen"], s2["vicen"]
    inner = np.zeros(s0["aice"].shape, bool)
    inner[:, JLO - 1:JHI, ILO - 1:IHI] = True
    listed = inner & (s0["aice"] > PUNY)
    up = np.zeros_like(inner)
    down = np.zeros_like(inner)
    for n in range(synth.NCAT - 1):
        up |= (a1[:, n] < a0[:, n]) & (a1[:, n + 1] > a0[:, n + 1])
        down |= (a1[:, n + 1] < a0[:, n + 1]) & (a1[:, n] > a0[:, n])
    bits = lambda x: np.ascontiguousarray(x).view(np.uint64)
    rest_same = (bits(a1[:, 1:]) == bits(a0[:, 1:])).all(axis=1)
    changed = np.zeros_like(inner)
    for k in STATE:
        x0, x1 = s0[k], s1[k]
        if k == "trcrn":
            x0, x1 = x0[:, :, :ntrcr], x1[:, :, :ntrcr]
        ne = bits(x0) != bits(x1)
        changed |= ne.reshape(ne.shape[0], -1, NY, NX).any(axis=1)
    grew = (v2 > v1)
    out = dict(
        thicker=listed & up, thinner=listed & down,
        cat1_loss=listed & (s1["aice"] < s0["aice"]) & (a1[:, 0] < a0[:, 0]) & rest_same,
        emptied=listed & ((a0 > PUNY) & (a1 == 0.0)).any(axis=1),
        unchanged=listed & ~changed,
        new_cat1=(a2[:, 0] > a1[:, 0]) & ~grew[:, 1:].any(axis=1),
        new_spread=(a2[:, 0] > a1[:, 0]) & grew[:, 1:].any(axis=1),
        surplus_only=(s1["aice0"] < PUNY) & grew.any(axis=1) & (bits(a2) == bits(a1)).all(axis=1),
        ghost_new=~inner & grew.any(axis=1),
        melt_snow=inner & (s0["rside"] > 0) & (v2.sum(axis=1) > 0) & (s2["vsnon"].sum(axis=1) > 0),
        melt_nosnow=inner & (s0["rside"] > 0) & (v2.sum(axis=1) > 0) & (s2["vsnon"].sum(axis=1) == 0),
    )
    return {k: int(v.sum()) for k, v in out.items()}


def stop_add_inputs():
    """one block; in cell (5, 6) aice is half of the sum of aicen, aice0 = 0, frzmlt > 0: add_new_ice spreads twice the
    new volume over the categories and its conservation check fires there (ice_therm_itd.F90:1102, 1238)"""
    raw = synth.therm2_state("growth", NX, NY, 1, seed=STOP_SEED, ntrcr=1)
    s = block(raw, 0)
    i, j = 5, 6
    a = s["aicen"][:, j - 1, i - 1]
    if a.sum() <= 0.1:
        a[0] = 0.5
        s["vicen"][0, j - 1, i - 1] = 0.2
    s["aice"][j - 1, i - 1] = 0.5 * sum(s["aicen"][:, j - 1, i - 1])
    s["aice0"][j - 1, i - 1] = 0.0
    s["frzmlt"][j - 1, i - 1] = 60.0
    s["tmask"][j - 1, i - 1] = 1
    return s, (i, j)


def stop_shift_inputs():
    """one block; shift_ice with daice = 2 aicen(nd) across boundary 2 in two cells of the list: the reference names
    the later one (ice_itd.F90:1143-1163)"""
    raw = synth.therm2_state("growth", NX, NY, 1, seed=STOP_SEED, ntrcr=1)
    s = block(raw, 0, STATE)
    icells, indxi, indxj = ice_list(raw["aice"][0])
    a = np.stack([s["aicen"][:, indxj[k] - 1, indxi[k] - 1] for k in range(icells)], axis=1)   # (ncat, icells)
    v = np.stack([s["vicen"][:, indxj[k] - 1, indxi[k] - 1] for k in range(icells)], axis=1)
    s["hicen"] = np.where(a > PUNY, v / np.where(a > PUNY, a, 1.0), 0.0)
    s["donor"] = np.zeros((synth.NCAT, icells), np.int32)
    s["daice"] = np.zeros((synth.NCAT, icells))
    s["dvice"] = np.zeros((synth.NCAT, icells))
    have = np.nonzero(a[1] > 0.01)[0]
    k1, k2 = int(have[1]), int(have[-2])
    assert k1 < k2
    for k in (k1, k2):
        s["donor"][1, k] = 2
        s["daice"][1, k] = 2.0 * a[1, k]
        s["dvice"][1, k] = 0.5 * v[1, k]
    s = {k: np.ascontiguousarray(x) for k, x in s.items()}
    return s, icells, indxi, indxj, (int(indxi[k2]), int(indxj[k2]))
