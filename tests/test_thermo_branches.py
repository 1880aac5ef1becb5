"""Census of the input sets that test_gpu_thermo.py drives the device with (tests/thermo_case.py): the checker runs every
set without a stop, and every branch a set is meant to reach holds at least FLOOR of its columns -- so that a GPU test
that passes has compared columns in that branch.  The counts come from the arrays before and after the call and from the
checker's per-column trace, which a test here shows to change no result.  No GPU.

`pytest -s` prints the counts of every set."""
import ctypes

import numpy as np
import pytest

import thermo_case as tc

CONDUCT = ("MU71", "bubbly")


def _hold(tag, total, branches, ncol):
    print(tag, "columns", ncol, {k: v for k, v in total.items() if v})
    short = {k: total.get(k, 0) for k in branches if total.get(k, 0) < tc.FLOOR}
    assert not short, (tag, short)


@pytest.mark.parametrize("calc_Tsfc", [True, False])
def test_trace_changes_no_result(orc, calc_Tsfc):
    """every array of the call is the same bit for bit with and without the trace; the trace marks exactly the listed
    columns, holds each one's iteration count, and leaves the other cells alone"""
    orc.init_thermo()
    for recipe, n in (("both", 0), ("thin_top", 2), ("thin_bottom", 4)):
        a, icells, ii, jj = tc.extreme_columns(12, 20, n, recipe)
        if not calc_Tsfc:
            a = tc.known_tsfc_set(orc, recipe, "MU71", keep_stops=True)[n][1]
        hist0 = np.ctypeslib.as_array((ctypes.c_long * 101).in_dll(orc.lib, "orc_iter_hist")).copy()
        plain = {k: v.copy() for k, v in a.items()}
        l0 = orc.thermo_vertical(tc.DT, icells, ii, jj, plain, yday=tc.YDAY)
        hist1 = np.ctypeslib.as_array((ctypes.c_long * 101).in_dll(orc.lib, "orc_iter_hist")).copy()
        trace = np.full(a["aicen"].shape, -7, np.int32)
        traced = {k: v.copy() for k, v in a.items()}
        l1 = orc.thermo_vertical(tc.DT, icells, ii, jj, traced, yday=tc.YDAY, trace=trace)
        assert l0 == l1
        for k in a:
            assert np.array_equal(plain[k], traced[k]), (recipe, k)
        listed = np.zeros(a["aicen"].shape, bool)
        listed[jj[:icells] - 1, ii[:icells] - 1] = True
        assert np.all(trace[~listed] == -7)
        assert np.all((trace[listed] & tc.TRACE["listed"]) != 0)
        # the iteration counts of the trace are those of orc_iter_hist, which stays
        assert np.array_equal(np.bincount(trace[listed] & 0xff, minlength=101), hist1 - hist0)
        # a later call without a trace writes none
        again = {k: v.copy() for k, v in a.items()}
        before = trace.copy()
        orc.thermo_vertical(tc.DT, icells, ii, jj, again, yday=tc.YDAY)
        assert np.array_equal(trace, before)
    orc.init_thermo()


def test_recipes_leave_synth_alone():
    """a recipe changes vicen, eicen, fswsfc and fbot and nothing else of synth.thermo_columns"""
    base, icells, ii, jj = tc.synth.thermo_columns(12, 20, 1, regime="summer", seed=3)
    for recipe, (s, extra, fbot) in tc.RECIPES.items():
        a, ic2, i2, j2 = tc.extreme_columns(12, 20, 1, recipe)
        assert ic2 == icells and np.array_equal(i2, ii) and np.array_equal(j2, jj)
        for k in base:
            if k in ("vicen", "eicen"):
                assert np.array_equal(a[k], base[k] * s)
            elif k == "fswsfc":
                assert np.array_equal(a[k], base[k] + extra)
            elif k == "fbot" and fbot is not None:
                assert np.all(a[k] == fbot)
            else:
                assert np.array_equal(a[k], base[k]), (recipe, k)


@pytest.mark.parametrize("conduct", CONDUCT)
@pytest.mark.parametrize("name", list(tc.LIST_SETS))
def test_census_list_sets(orc, name, conduct):
    orc.init_thermo(conduct=conduct)
    total, ncol = {}, 0
    for n, a, icells, ii, jj in tc.list_set(name):
        ls, out, trace = tc.traced_call(orc, a, icells, ii, jj)
        assert ls == (0, 0, 0), (name, n, ls)
        tc.add_counts(total, tc.branch_counts(a, out, trace))
        ncol += icells
    s = tc.LIST_SETS[name]
    if name in ("compact", "full"):     # which way cice_thermo_vertical takes them, and no multiple of the tile
        for n, a, icells, ii, jj in tc.list_set(name):
            assert (2 * icells <= s["nx"] * s["ny"]) == (name == "compact")
            assert icells % 64 and icells % 256
    _hold(("list", name, conduct), total, s["branches"], ncol)
    orc.init_thermo()


@pytest.mark.parametrize("conduct", CONDUCT)
@pytest.mark.parametrize("name", tc.RECIPE_SETS)
def test_census_known_Tsfc_sets(orc, name, conduct):
    """calc_Tsfc = F: the columns the perturbed fluxes stop are named by the checker and leave the list, at most 5 % of
    the set; the census counts what is left."""
    total, ncol, left_out = {}, 0, 0
    for n, b, icells, ii, jj, lo in tc.known_tsfc_set(orc, name, conduct):
        ls, out, trace = tc.traced_call(orc, b, icells, ii, jj)
        assert ls == (0, 0, 0), (name, n, ls)
        assert not ((trace & tc.TRACE["stopped"]) != 0).any()
        tc.add_counts(total, tc.branch_counts(b, out, trace))
        ncol += icells; left_out += lo
    assert left_out <= tc.MAX_LEFT_OUT * (ncol + left_out), (left_out, ncol)
    for k in ("snow_cold", "snow_melting", "bare_cold", "bare_melting", "tsf_reset", "tsf_halved"):
        assert total[k] == 0          # no surface solve on this path
    _hold(("known_Tsfc", name, conduct, "left out", left_out), total, tc.KNOWN_BRANCHES[name], ncol)
    orc.init_thermo()


def _batch_census(orc, tag, percat, nb, yday, branches, forcing=None):
    total, ncol = {}, 0
    for (b, n), (before, after, trace, ls) in tc.batch_checker_calls(orc, percat, nb, yday, forcing=forcing).items():
        assert ls == (0, 0, 0), (tag, b, n, ls)
        tc.add_counts(total, tc.branch_counts(before, after, trace))
        ncol += percat[(b, n)][1]
    _hold(tag, total, branches, ncol)
    return total


@pytest.mark.parametrize("conduct", CONDUCT)
def test_census_batches(orc, conduct):
    """the dense / permuted batch, the one of the sorted-columns test, the batch of step_therm1 (its fbot from the checker's frzmlt_bottom_lateral) and the
    batch behind the hand-off to the dynamics"""
    orc.init_thermo(conduct=conduct)
    s = tc.BATCH
    _, percat = tc.batch_inputs(s["ny"], s["nx"], s["nb"], s["seed"], s["recipe"])
    total = _batch_census(orc, ("batch", conduct), percat, s["nb"], s["yday"], s["branches"])
    assert total["iters_ge_20"] >= tc.FLOOR      # the spread the sort gets
    s = tc.SORTED
    _, percat = tc.batch_inputs(s["ny"], s["nx"], s["nb"], s["seed"], s["recipe"])
    total = _batch_census(orc, ("sorted", conduct), percat, s["nb"], s["yday"], s["branches"])
    s = tc.THERM1
    ny, nx, nb = s["ny"], s["nx"], s["nb"]
    batch, percat, fz, _, _ = tc.therm1_inputs(ny, nx, nb, s["seed"], s["recipe"], s["frzmlt"], s["dsst"])
    forcing = dict(Tbot=np.zeros((nb, ny, nx)), fbot=np.zeros((nb, ny, nx)))
    for b in range(nb):
        forcing["Tbot"][b], forcing["fbot"][b], _ = orc.frzmlt_bottom_lateral(
            2, nx - 1, 2, ny - 1, tc.DT, fz["aice"][b], fz["frzmlt"][b], np.ascontiguousarray(batch["eicen"][b]),
            np.ascontiguousarray(batch["esnon"][b]), fz["sst"][b], fz["Tf"][b], fz["strocnxT"][b], fz["strocnyT"][b])
    assert forcing["fbot"].min() < -1000.0
    _batch_census(orc, ("step_therm1", conduct), percat, nb, s["yday"], s["branches"], forcing=forcing)
    s = tc.ADOPT
    _, percat = tc.adopt_batch(s["ny"], s["nx"], s["recipe"], s["seed"])
    _batch_census(orc, ("adopt", conduct), percat, 1, s["yday"], s["branches"])
    orc.init_thermo()


def test_branch_counts_on_a_hand_made_column(orc):
    """branch_counts on columns whose fate is known: 1 cm of ice under 1000 W m-2 melts away from above through all
    its layers; the same ice without the heat does neither"""
    orc.init_thermo()
    a, icells, ii, jj = tc.synth.thermo_columns(6, 8, 0, regime="summer", seed=1, ice_frac=1.0)
    a["vsnon"][:] = 0.0; a["esnon"][:] = 0.0; a["Sswabs"][:] = 0.0
    a["fswint"] = np.ascontiguousarray(a["Iswabs"].sum(axis=0))
    h = np.where(a["aicen"] > 0, a["vicen"] / np.where(a["aicen"] > 0, a["aicen"], 1.0), 1.0)
    thin = {k: v.copy() for k, v in a.items()}
    thin["vicen"] = a["vicen"] * 0.01 / h; thin["eicen"] = a["eicen"] * 0.01 / h
    hot = {k: v.copy() for k, v in thin.items()}
    hot["fswsfc"] = hot["fswsfc"] + 1000.0
    hot["fsnow"][:] = 0.0                      # (new snow on open water would turn into ice again)
    ls, out, trace = tc.traced_call(orc, hot, icells, ii, jj)
    c = tc.branch_counts(hot, out, trace)
    assert ls == (0, 0, 0) and c["melted_away"] == c["top_through_layer"] == icells and c["snow_gone"] == 0
    ls, out, trace = tc.traced_call(orc, a, icells, ii, jj)
    c = tc.branch_counts(a, out, trace)
    assert ls == (0, 0, 0) and c["melted_away"] == c["top_through_layer"] == c["bottom_through_layer"] == 0
