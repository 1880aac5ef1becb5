"""Inputs and bookkeeping shared by the tests of the column thermodynamics that drive it into the branches the three
regimes of synth.thermo_columns never reach (test_thermo_branches.py, test_oracle_vs_ref.py, test_gpu_thermo.py): columns
that melt through whole layers from above and from below, columns that melt away, interior layers that reach their
melting temperature so that the solver scales kh inside its iteration.  No GPU here.

A recipe changes summer columns in three ways: vicen and eicen are scaled by s (thinner ice of the same temperature),
`extra` W m-2 are added to fswsfc, and fbot becomes a constant where one is given.  The reference accepts all of them.

branch_counts() counts, per branch, the columns of one thermo_vertical call that took it: from the arrays before and
after the call and from the per-column trace of the checker (oracle/cice_oracle.h: ORC_TR_*).  Every input set of the GPU
tests is listed here with the branches it is meant to reach; test_thermo_branches.py holds each of them to FLOOR columns."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from cice4_amd import lib, synth  # noqa: E402

DT = 3600.0
YDAY = 200.0
PUNY = 1.0e-11
HS_MIN = 1.0e-4
NC, NI, NS = 5, 4, 1
FLOOR = 8            # columns every named branch of a set must hold

# name -> (s, extra, fbot)
RECIPES = {
    "thin_top": (0.05, 1000.0, None),       # top melt through layers of thin ice
    "thin_bottom": (0.05, 0.0, -1500.0),    # bottom melt through everything; snow left on water -> snow-ice in freeboard
    "both": (0.2, 5000.0, -1500.0),         # melt from both sides
    "thick_top": (1.0, 20000.0, None),      # top melt through layers of thick ice
}

TRACE = dict(tsf_reset=0x100, tsf_halved=0x200, cond2b_halved=0x400, layer_at_Tmlt=0x800, kh_reduced=0x1000,
             cold=0x2000, melting=0x4000, bottom_into_snow=0x8000, snoice_after_ice_gone=0x10000,
             stopped=0x20000000, listed=0x40000000)

BRANCHES = ("melted_away", "top_through_layer", "bottom_through_layer", "bottom_into_snow", "snow_gone", "snoice",
            "snoice_after_ice_gone", "thin_snow", "new_snow_on_bare", "condense", "sublime",
            "snow_cold", "snow_melting", "bare_cold", "bare_melting", "mlt_onset_set", "frz_onset_set",
            "tsf_reset", "tsf_halved", "cond2b_halved", "layer_at_Tmlt", "kh_reduced", "iters_ge_20")


def apply_recipe(a, recipe):
    """the three changes of a recipe, in place, on the arrays of synth.thermo_columns"""
    s, extra, fbot = RECIPES[recipe]
    a["vicen"] *= s
    a["eicen"] *= s
    a["fswsfc"] += extra
    if fbot is not None:
        a["fbot"][:] = fbot
    return a


def extreme_columns(ny, nx, n, recipe, seed=3, ice_frac=0.9):
    """synth.thermo_columns(regime="summer") of category n under a recipe: (a, icells, indxi, indxj)"""
    a, icells, ii, jj = synth.thermo_columns(ny, nx, n, regime="summer", seed=seed, ice_frac=ice_frac)
    return apply_recipe(a, recipe), icells, ii, jj


def branch_masks(before, after, trace):
    """{branch: boolean (ny, nx) mask of the listed columns that took it}.  before / after: the arrays of one
    thermo_vertical call (one category); trace: the checker's per-column words of that call (zero outside the list)."""
    listed = (trace & TRACE["listed"]) != 0
    ai = np.where(listed, before["aicen"], 1.0)
    hi0 = np.where(listed, before["vicen"] / ai, 0.0)
    hs0 = np.where(listed, before["vsnon"] / ai, 0.0)
    gone = listed & (after["aicen"] == 0.0)
    bit = lambda k: listed & ((trace & TRACE[k]) != 0)
    snow = hs0 > HS_MIN / NS                      # l_snow of temperature_changes
    m = dict(
        melted_away=gone,
        top_through_layer=listed & (after["meltt"] > hi0 / NI),
        bottom_through_layer=listed & (after["meltb"] > hi0 / NI),
        bottom_into_snow=bit("bottom_into_snow"),
        snow_gone=listed & ~gone & (hs0 > 0.0) & (after["vsnon"] == 0.0),
        snoice=listed & (after["snoice"] > 0.0),
        snoice_after_ice_gone=bit("snoice_after_ice_gone"),
        thin_snow=listed & (hs0 > 0.0) & (hs0 <= HS_MIN),
        new_snow_on_bare=listed & (hs0 == 0.0) & (before["fsnow"] > 0.0),
        condense=listed & (after["flatn"] > 0.0),
        sublime=listed & (after["flatn"] < 0.0),
        snow_cold=bit("cold") & snow, snow_melting=bit("melting") & snow,
        bare_cold=bit("cold") & ~snow, bare_melting=bit("melting") & ~snow,
        mlt_onset_set=listed & (before["mlt_onset"] != after["mlt_onset"]),
        frz_onset_set=listed & (before["frz_onset"] != after["frz_onset"]),
        iters_ge_20=listed & ((trace & 0xff) >= 20),
    )
    for k in ("tsf_reset", "tsf_halved", "cond2b_halved", "layer_at_Tmlt", "kh_reduced"):
        m[k] = bit(k)
    assert set(m) == set(BRANCHES)
    return m


def branch_counts(before, after, trace):
    """{branch: number of listed columns that took it} (see branch_masks)"""
    return {k: int(v.sum()) for k, v in branch_masks(before, after, trace).items()}


def add_counts(total, counts):
    for k, v in counts.items():
        total[k] = total.get(k, 0) + v
    return total


def traced_call(orc, a, icells, ii, jj, yday=YDAY, dt=DT):
    """one checker call on a copy of `a`: (l_stop tuple, arrays after, trace)"""
    out = {k: v.copy() for k, v in a.items()}
    trace = np.zeros(a["aicen"].shape, np.int32)
    ls = orc.thermo_vertical(dt, icells, ii, jj, out, yday=yday, trace=trace)
    return ls, out, trace


# ---- list kernel: the sets of test_gpu_thermo.py ----------------------------------------------------------------------
_SOLVER = ("layer_at_Tmlt", "kh_reduced", "tsf_reset")
_FORMS = ("snow_cold", "snow_melting", "bare_cold", "bare_melting")
_SMALL = dict(ny=12, nx=20, cats=tuple(range(NC)), ice_frac=0.9, seed=3)
LIST_SETS = {
    # every recipe x five categories at 12 x 20
    "thin_top": dict(_SMALL, recipe="thin_top",
                     branches=("melted_away", "top_through_layer", "snow_gone", "snoice", "new_snow_on_bare", "condense",
                               "sublime", "mlt_onset_set", "frz_onset_set", "iters_ge_20") + _FORMS + _SOLVER),
    "thin_bottom": dict(_SMALL, recipe="thin_bottom",
                        branches=("melted_away", "bottom_through_layer", "bottom_into_snow", "snoice",
                                  "snoice_after_ice_gone", "new_snow_on_bare", "condense", "sublime", "mlt_onset_set",
                                  "tsf_reset", "tsf_halved") + _FORMS),
    "both": dict(_SMALL, recipe="both",
                 branches=("melted_away", "top_through_layer", "bottom_through_layer", "snow_gone", "snoice",
                           "snoice_after_ice_gone", "mlt_onset_set") + _FORMS + _SOLVER),
    "thick_top": dict(_SMALL, recipe="thick_top",
                      branches=("melted_away", "top_through_layer", "snow_gone", "snoice_after_ice_gone",
                                "mlt_onset_set", "frz_onset_set") + _FORMS + _SOLVER),
    # 37 x 70: a column count that is no multiple of 64 or 256; ice_frac 0.3 goes the compact way, 0.9 the full one
    "compact": dict(recipe="both", ny=37, nx=70, cats=(0, 3), ice_frac=0.3, seed=3,
                    branches=("melted_away", "top_through_layer", "bottom_through_layer", "bottom_into_snow",
                              "thin_snow") + _SOLVER),
    "full": dict(recipe="thin_top", ny=37, nx=70, cats=(0, 2), ice_frac=0.9, seed=3,
                 branches=("melted_away", "top_through_layer", "thin_snow", "iters_ge_20") + _SOLVER),
}
RECIPE_SETS = tuple(RECIPES)


def list_set(name):
    """[(n, a, icells, indxi, indxj)] of a set of LIST_SETS"""
    s = LIST_SETS[name]
    return [(n,) + extreme_columns(s["ny"], s["nx"], n, s["recipe"], seed=s["seed"], ice_frac=s["ice_frac"])
            for n in s["cats"]]


# ---- calc_Tsfc = F on the recipe sets ----------------------------------------------------------------------------------
# (an interior layer at its melting temperature is not among them: with the converged fluxes handed in, no column of
# these sets reaches it -- 0 of 3,200 -- and the fluxes are perturbed on cold surfaces only)
KNOWN_BRANCHES = {
    "thin_top": ("melted_away", "top_through_layer", "snow_gone", "cond2b_halved"),
    "thin_bottom": ("melted_away", "bottom_through_layer", "bottom_into_snow", "snoice_after_ice_gone",
                    "cond2b_halved"),
    "both": ("melted_away", "top_through_layer", "bottom_through_layer", "snow_gone", "cond2b_halved"),
    "thick_top": ("melted_away", "top_through_layer", "snow_gone"),
}
MAX_LEFT_OUT = 0.05


def without(icells, ii, jj, drop):
    """the list without the columns of the boolean (ny, nx) mask `drop`, in its order"""
    keep = ~drop[jj[:icells] - 1, ii[:icells] - 1]
    i2 = np.zeros_like(ii); j2 = np.zeros_like(jj)
    m = int(keep.sum())
    i2[:m] = ii[:icells][keep]; j2[:m] = jj[:icells][keep]
    return m, i2, j2


def known_tsfc_set(orc, name, conduct, keep_stops=False):
    """A recipe set as inputs of calc_Tsfc = F: [(n, b, icells, indxi, indxj, left_out)].  The surface fluxes and Tsfc
    come from the checker's calc_Tsfc = T solution of the same columns, perturbed by synth.known_tsfc_inputs.  Some of
    the perturbed columns cannot conserve energy and the reference stops there: the checker's trace names them and
    they leave the list (at most MAX_LEFT_OUT of a set) -- unless keep_stops.  Leaves the checker at calc_Tsfc = F."""
    out = []
    for n, a, icells, ii, jj in list_set(name):
        orc.init_thermo(conduct=conduct)
        ls, t, _ = traced_call(orc, a, icells, ii, jj)
        assert ls[0] == 0, (name, conduct, n, ls)
        b = synth.known_tsfc_inputs(a, t, seed=n)
        orc.init_thermo(calc_Tsfc=False, conduct=conduct)
        left_out = 0
        if not keep_stops:
            _, _, tr = traced_call(orc, b, icells, ii, jj)
            stops = (tr & TRACE["stopped"]) != 0
            left_out = int(stops.sum())
            icells, ii, jj = without(icells, ii, jj, stops)
        out.append((n, b, icells, ii, jj, left_out))
    return out


# ---- dense batch: module-array-shaped inputs of the batched step -------------------------------------------------------
def batch_inputs(ny, nx, nb, seed, recipe=None):
    """Module-array-shaped inputs of the batched step from per-category column sets: (batch, percat).  recipe: None
    (mixed regime), the name of a recipe for every block, or one name per block (summer columns under it)."""
    out = {k: None for k in lib.THERMO_STATE + lib.THERMO_FORCING + lib.THERMO_CAT_IN + lib.THERMO_SW
           + lib.THERMO_OUT + lib.THERMO_ONSET}
    z = lambda *shape: np.zeros(shape)
    out.update(aicen=z(nb, NC, ny, nx), trcrn=z(nb, NC, 5, ny, nx), vicen=z(nb, NC, ny, nx),
               vsnon=z(nb, NC, ny, nx), eicen=z(nb, NC * NI, ny, nx), esnon=z(nb, NC * NS, ny, nx),
               lhcoef=z(nb, NC, ny, nx), shcoef=z(nb, NC, ny, nx), fswsfc=z(nb, NC, ny, nx),
               fswint=z(nb, NC, ny, nx), fswthrun=z(nb, NC, ny, nx), Sswabs=z(nb, NC, NS, ny, nx),
               Iswabs=z(nb, NC, NI, ny, nx), mlt_onset=z(nb, ny, nx), frz_onset=z(nb, ny, nx))
    for k in lib.THERMO_FORCING:
        out[k] = z(nb, ny, nx)
    for k in lib.THERMO_OUT:
        out[k] = np.full((nb, NC, ny, nx), 9.0)
    percat = {}
    for b in range(nb):
        rb = recipe if recipe is None or isinstance(recipe, str) else recipe[b]
        for n in range(NC):
            a, icells, ii, jj = synth.thermo_columns(ny, nx, n, regime="mixed" if rb is None else "summer",
                                                     seed=seed + 17 * b, ice_frac=0.8)
            if rb is not None:
                apply_recipe(a, rb)
            percat[(b, n)] = (a, icells, ii, jj)
            for k in ("aicen", "vicen", "vsnon", "lhcoef", "shcoef", "fswsfc", "fswint", "fswthrun"):
                out[k][b, n] = a[k]
            out["trcrn"][b, n] = a["trcrn"]
            out["eicen"][b, n * NI:(n + 1) * NI] = a["eicen"]
            out["esnon"][b, n * NS:(n + 1) * NS] = a["esnon"]
            out["Sswabs"][b, n] = a["Sswabs"]; out["Iswabs"][b, n] = a["Iswabs"]
            if n == 0:
                for k in lib.THERMO_FORCING + ("mlt_onset", "frz_onset"):
                    out[k][b] = a[k]
    return out, percat


# the extreme batch of the dense, sorted, step_therm1 and hand-off tests: 14 x 22 x 2 blocks, one recipe per block
BATCH = dict(ny=14, nx=22, nb=2, seed=21, recipe=("both", "thin_top"), yday=150.0,
             branches=("melted_away", "top_through_layer", "bottom_through_layer", "iters_ge_20") + _SOLVER)


# the same recipes at the size of test_sorted_columns_give_the_same_bits (planes that are no multiple of a chunk)
SORTED = dict(ny=29, nx=43, nb=2, seed=33, recipe=BATCH["recipe"], yday=150.0,
              branches=("melted_away", "iters_ge_20", "kh_reduced"))


def batch_checker_calls(orc, percat, nb, yday, forcing=None, dt=DT):
    """The n = 1..ncat loop of step_therm1 on the checker: the categories of a block share the forcing of its first
    category (or `forcing`: {name: (nb, ny, nx)}) and the onset dates, which travel from one category to the next.
    Returns {(b, n): (before, after, trace, l_stop tuple)}."""
    res = {}
    for b in range(nb):
        mlt = percat[(b, 0)][0]["mlt_onset"].copy(); frz = percat[(b, 0)][0]["frz_onset"].copy()
        for n in range(NC):
            a, icells, ii, jj = percat[(b, n)]
            ac = {k: v.copy() for k, v in a.items()}
            for k in lib.THERMO_FORCING:
                ac[k] = (forcing[k][b] if forcing and k in forcing else percat[(b, 0)][0][k]).copy()
            ac["mlt_onset"], ac["frz_onset"] = mlt, frz
            before = {k: v.copy() for k, v in ac.items()}
            trace = np.zeros(ac["aicen"].shape, np.int32)
            ls = orc.thermo_vertical(dt, icells, ii, jj, ac, yday=yday, trace=trace)
            res[(b, n)] = (before, ac, trace, ls)
    return res


# ---- step_therm1 in one call: frzmlt_bottom_lateral makes fbot, so the recipe's constant goes in through frzmlt ---------
THERM1 = dict(ny=14, nx=22, nb=2, seed=35, recipe=("both", "thin_top"), yday=150.0, frzmlt=-3000.0, dsst=3.0,
              branches=("melted_away", "top_through_layer", "bottom_through_layer") + _SOLVER)


def therm1_inputs(ny, nx, nb, seed, recipe=None, frzmlt=None, dsst=None):
    """inputs of cice_step_therm1: (batch, percat, fz, pc, acc0).  recipe None: the mixed regime with moderate ocean
    heat; else frzmlt and sst - Tf are the constants given (a strong melt potential: fbot of the order of -1500 W m-2)."""
    batch, percat = batch_inputs(ny, nx, nb, seed=seed, recipe=recipe)
    rng = np.random.default_rng(6)
    aice = np.ascontiguousarray(batch["aicen"].sum(axis=1))
    fz = dict(aice=aice, frzmlt=np.ascontiguousarray(rng.uniform(-60, 20, (nb, ny, nx))),
              Tf=np.full((nb, ny, nx), -1.8), strocnxT=np.ascontiguousarray(rng.uniform(-0.2, 0.2, (nb, ny, nx))),
              strocnyT=np.ascontiguousarray(rng.uniform(-0.2, 0.2, (nb, ny, nx))))
    fz["sst"] = fz["Tf"] + rng.uniform(0, 0.5, (nb, ny, nx))
    if frzmlt is not None:
        fz["frzmlt"][:] = frzmlt
        fz["sst"] = fz["Tf"] + dsst
    pc = {k: np.ascontiguousarray(rng.uniform(-1, 1, batch["aicen"].shape))
          for k in ("strairxn", "strairyn", "Trefn", "Qrefn")}
    acc0 = {k: np.ascontiguousarray(rng.uniform(-1, 1, (nb, ny, nx))) for k in lib.MERGE_ORDER}
    return batch, percat, fz, pc, acc0


# ---- the thermo state handed to the dynamics on the device: one block of the dynamics' 70 x 44 grid ---------------------
ADOPT = dict(nxg=70, nyg=44, ny=46, nx=72, seed=9, recipe="both", yday=150.0, branches=("melted_away",))


def adopt_batch(ny, nx, recipe=None, seed=9):
    """one-block batch whose concentrations add up to at most 0.95 per cell: (batch, percat), both scaled"""
    batch, percat = batch_inputs(ny, nx, 1, seed=seed, recipe=recipe)
    tot = batch["aicen"].sum(axis=1, keepdims=True)
    sc = np.where(tot > 0.95, 0.95 / np.maximum(tot, 1e-30), 1.0)
    for k in ("aicen", "vicen", "vsnon", "eicen", "esnon"):
        batch[k] = np.ascontiguousarray(batch[k] * sc)
    for n in range(NC):
        a = percat[(0, n)][0]
        for k in ("aicen", "vicen", "vsnon"):
            a[k] = np.ascontiguousarray(batch[k][0, n])
        a["eicen"] = np.ascontiguousarray(batch["eicen"][0, n * NI:(n + 1) * NI])
        a["esnon"] = np.ascontiguousarray(batch["esnon"][0, n * NS:(n + 1) * NS])
    return batch, percat
