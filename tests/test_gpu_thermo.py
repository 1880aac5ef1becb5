"""GPU parity tests of the column thermodynamics (through the C-ABI) against the CPU
checker.  Each iteration of the temperature solve evaluates exp() (saturation humidity); the
device evaluates it with glibc's own algorithm (cice4_amd/csrc/libm_exact.h), so the results are
BIT-IDENTICAL to the checker's (conftest.TOL_EXP = 0 on a host with glibc's FMA build of exp, 1e-10
elsewhere); only frzmlt_bottom_lateral (`**1.36` -> pow) keeps the 1e-10 bound.  Error reporting
(l_stop, istop, jstop) must be identical."""
import numpy as np
import pytest

import thermo_case as tc
from cice4_amd import lib, synth
from conftest import relerr, TOL_EXP, TOL_POW

pytestmark = pytest.mark.gpu
DT = 3600.0
TOL = TOL_EXP
CHECK = ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon", "fswsfc", "fswint", "Sswabs", "Iswabs",
         "fsurfn", "fcondtopn", "fsensn", "flatn", "fswabsn", "flwoutn", "evapn", "freshn", "fsaltn",
         "fhocnn", "meltt", "melts", "meltb", "congel", "snoice", "mlt_onset", "frz_onset")


# Field-level relative error = max|gpu - cpu| / max(max|cpu|, floor): the floor keeps
# fields that are physically ~0 in a given regime (e.g. top melt in winter, ~1e-18 m of
# round-off) from being compared digit by digit.  Floors are 3+ orders below values that matter.
FLOOR = dict(meltt=1e-4, melts=1e-4, meltb=1e-4, congel=1e-4, snoice=1e-4,      # m per step
             evapn=1e-7, freshn=1e-6, fsaltn=1e-8,                               # kg m-2 s-1
             fsurfn=1.0, fcondtopn=1.0, fsensn=1.0, flatn=1.0, fswabsn=1.0, flwoutn=1.0, fhocnn=1.0,
             fswsfc=1.0, fswint=1.0, Sswabs=1.0, Iswabs=1.0)                     # W m-2


def frel(k, a, b):
    den = max(np.abs(b).max(), FLOOR.get(k, 0.0))
    return np.abs(np.asarray(a) - np.asarray(b)).max() / den if den > 0 else 0.0


def _cmp(a_gpu, a_cpu, tag=""):
    for k in CHECK:
        e = frel(k, a_gpu[k], a_cpu[k])
        assert e <= TOL, (tag, k, e)


def _melted_come_back_exactly(a, ag, ac, icells, ii, jj):
    """the columns of the list that the checker melts away: the device returns aicen = vicen = vsnon = eicen = esnon = 0
    and Tsfc = Tbot there, exactly.  Returns their number."""
    listed = np.zeros(a["aicen"].shape, bool)
    listed[jj[:icells] - 1, ii[:icells] - 1] = True
    gone = listed & (ac["aicen"] == 0.0)
    for k in ("aicen", "vicen", "vsnon"):
        assert np.array_equal(ag[k][gone], np.zeros(gone.sum())), k
    for k in ("eicen", "esnon"):
        assert np.array_equal(ag[k][:, gone], np.zeros((ag[k].shape[0], gone.sum()))), k
    assert np.array_equal(ag["trcrn"][0][gone], a["Tbot"][gone])
    assert np.array_equal(ag["aicen"] == 0.0, ac["aicen"] == 0.0)       # and no other column
    return int(gone.sum())


def _outside_untouched(a, ag, icells, ii, jj, flux_in=()):
    """cells outside the list keep what they held; the outputs are zero there"""
    outside = np.ones(a["aicen"].shape, bool)
    outside[jj[:icells] - 1, ii[:icells] - 1] = False
    for k in CHECK:
        if k in lib.THERMO_OUT and k not in flux_in:
            assert np.all(ag[k][outside] == 0.0), k
        else:
            assert np.array_equal(ag[k][..., outside], a[k][..., outside]), k


@pytest.mark.parametrize("name", list(tc.LIST_SETS))
@pytest.mark.parametrize("conduct", ["MU71", "bubbly"])
def test_extreme_columns_match_oracle(ctx, orc, name, conduct):
    """The list kernel on the sets of tests/thermo_case.py: columns that melt through whole layers from above and from
    below, columns that melt away, interior layers at their melting temperature with kh scaled inside the solver's
    iteration (tests/test_thermo_branches.py holds every set to its branches; tests/test_oracle_vs_ref.py pins the
    checker to the reference on the same sets).  Four recipes x five categories at 12 x 20, and at 37 x 70 one set the
    compact way and one the full way, with column counts that are no multiple of 64 or 256."""
    ctx.thermo_init(conduct=conduct); orc.init_thermo(conduct=conduct)
    gone = 0
    for n, a, icells, ii, jj in tc.list_set(name):
        ag = {k: v.copy() for k, v in a.items()}; ac = {k: v.copy() for k, v in a.items()}
        lg = ctx.thermo_vertical(DT, icells, ii, jj, ag, yday=tc.YDAY)
        lc = orc.thermo_vertical(DT, icells, ii, jj, ac, yday=tc.YDAY)
        assert lg == lc == (0, 0, 0), (name, n, lg, lc)
        _cmp(ag, ac, (name, conduct, n))
        gone += _melted_come_back_exactly(a, ag, ac, icells, ii, jj)
        _outside_untouched(a, ag, icells, ii, jj)
    assert gone >= 8
    ctx.thermo_init(); orc.init_thermo()


@pytest.mark.parametrize("name", tc.RECIPE_SETS)
@pytest.mark.parametrize("conduct", ["MU71", "bubbly"])
def test_extreme_columns_known_Tsfc_bit_exact(ctx, orc, name, conduct):
    """calc_Tsfc = F on the recipe sets (the columns the perturbed fluxes stop have left the lists: tc.known_tsfc_set):
    no exp() on this path, so device == checker bit for bit."""
    sets = tc.known_tsfc_set(orc, name, conduct)
    ctx.thermo_init(calc_Tsfc=False, conduct=conduct)
    for n, b, icells, ii, jj, _ in sets:
        bg = {k: v.copy() for k, v in b.items()}; bc = {k: v.copy() for k, v in b.items()}
        lg = ctx.thermo_vertical(DT, icells, ii, jj, bg, yday=tc.YDAY)
        lc = orc.thermo_vertical(DT, icells, ii, jj, bc, yday=tc.YDAY)
        assert lg == lc == (0, 0, 0), (name, n, lg, lc)
        for k in CHECK:
            assert np.array_equal(bg[k], bc[k]), (name, conduct, n, k)
        _melted_come_back_exactly(b, bg, bc, icells, ii, jj)
        _outside_untouched(b, bg, icells, ii, jj, flux_in=("fsurfn", "fcondtopn", "flatn"))
    ctx.thermo_init(); orc.init_thermo()


@pytest.mark.parametrize("regime", ["winter", "summer", "mixed"])
@pytest.mark.parametrize("conduct", ["MU71", "bubbly"])
def test_thermo_vertical_matches_oracle(ctx, orc, regime, conduct):
    ctx.thermo_init(conduct=conduct)
    so, to = orc.init_thermo(conduct=conduct)
    sg, tg = ctx.thermo_init(conduct=conduct)
    assert np.array_equal(sg, so) or relerr(sg, so) < 1e-15
    for n in range(5):
        a, icells, ii, jj = synth.thermo_columns(37, 70, n, regime=regime, seed=11)
        ag = {k: v.copy() for k, v in a.items()}; ac = {k: v.copy() for k, v in a.items()}
        lg = ctx.thermo_vertical(DT, icells, ii, jj, ag, yday=200.0)
        lc = orc.thermo_vertical(DT, icells, ii, jj, ac, yday=200.0)
        assert lg == lc == (0, 0, 0)
        _cmp(ag, ac, (regime, conduct, n))
        # cells outside the list keep their state; out-fields are zero there
        outside = np.ones_like(a["aicen"], bool)
        outside[jj[:icells] - 1, ii[:icells] - 1] = False
        assert np.array_equal(ag["vicen"][outside], a["vicen"][outside])
        assert np.all(ag["fsensn"][outside] == 0.0)
    orc.init_thermo()


@pytest.mark.parametrize("conduct", ["MU71", "bubbly"])
def test_known_Tsfc_variant_bit_exact(ctx, orc, conduct):
    """calc_Tsfc = F (surface fluxes and Tsfc are the caller's; get_matrix_elements_know_Tsfc,
    ice_therm_vertical.F90:2777): no exp() on this path, so device == checker bit for bit."""
    for regime in ("winter", "summer", "mixed"):
        for n in (0, 2, 4):
            a, icells, ii, jj = synth.thermo_columns(37, 70, n, regime=regime, seed=11)
            orc.init_thermo(conduct=conduct)
            t = {k: v.copy() for k, v in a.items()}
            assert orc.thermo_vertical(DT, icells, ii, jj, t, yday=200.0)[0] == 0
            b = synth.known_tsfc_inputs(a, t, seed=n)
            orc.init_thermo(calc_Tsfc=False, conduct=conduct)
            ctx.thermo_init(calc_Tsfc=False, conduct=conduct)
            bg = {k: v.copy() for k, v in b.items()}; bc = {k: v.copy() for k, v in b.items()}
            lg = ctx.thermo_vertical(DT, icells, ii, jj, bg, yday=200.0)
            lc = orc.thermo_vertical(DT, icells, ii, jj, bc, yday=200.0)
            assert lg == lc == (0, 0, 0), (regime, n, lg, lc)
            for k in CHECK:
                assert np.array_equal(bg[k], bc[k]), (regime, conduct, n, k)
            assert not np.array_equal(bc["eicen"], t["eicen"])
    ctx.thermo_init(); orc.init_thermo()


def test_known_Tsfc_batched(ctx, orc):
    """The device-resident batch with calc_Tsfc = F: fsurfn, fcondtopn, flatn travel in with the state."""
    ny, nx, nb = 26, 40, 2
    batch, percat = _batch_inputs(ny, nx, nb, seed=33)
    orc.init_thermo()
    inputs = {}
    for b in range(nb):
        for n in range(5):
            a, icells, ii, jj = percat[(b, n)]
            a = {k: v.copy() for k, v in a.items()}
            for k in lib.THERMO_FORCING:
                a[k] = percat[(b, 0)][0][k].copy()
            t = {k: v.copy() for k, v in a.items()}
            assert orc.thermo_vertical(DT, icells, ii, jj, t, yday=150.0)[0] == 0
            t["mlt_onset"] = a["mlt_onset"]; t["frz_onset"] = a["frz_onset"]
            kb = synth.known_tsfc_inputs(a, t, seed=5 * b + n)
            inputs[(b, n)] = kb
            for k in ("fsurfn", "fcondtopn", "flatn"):
                batch[k][b, n] = kb[k]
            batch["trcrn"][b, n] = kb["trcrn"]
    ctx.thermo_init(calc_Tsfc=False); orc.init_thermo(calc_Tsfc=False)
    ctx.thermo_batch_alloc(nx, ny, nb)
    ctx.thermo_batch_upload(batch)
    st = ctx.thermo_batch_step(DT, yday=150.0)
    assert st["l_stop"] == 0
    ctx.thermo_batch_download(batch)
    for b in range(nb):
        mlt = percat[(b, 0)][0]["mlt_onset"].copy(); frz = percat[(b, 0)][0]["frz_onset"].copy()
        for n in range(5):
            _, icells, ii, jj = percat[(b, n)]
            ac = inputs[(b, n)]
            ac["mlt_onset"], ac["frz_onset"] = mlt, frz
            assert orc.thermo_vertical(DT, icells, ii, jj, ac, yday=150.0)[0] == 0
            for k in ("aicen", "vicen", "vsnon", "fswsfc", "fswint") + lib.THERMO_OUT:
                assert np.array_equal(batch[k][b, n], ac[k]), (b, n, k)
            assert np.array_equal(batch["eicen"][b, n * 4:(n + 1) * 4], ac["eicen"])
            assert np.array_equal(batch["trcrn"][b, n], ac["trcrn"])
    ctx.thermo_init(); orc.init_thermo()


@pytest.mark.parametrize("calc_Tsfc", [True, False])
def test_sparse_list_travels_compact(ctx, orc, calc_Tsfc):
    """Fewer than half of the block's cells listed (the rule on a real grid): cice_thermo_vertical gathers the listed
    cells on the host, moves them in one copy each way and runs the list kernel on the compact block.  Same bits as
    the checker, cells outside the list untouched, outputs zero there, the first failing column reported with its
    (i, j) of the full block."""
    ctx.thermo_init(calc_Tsfc=calc_Tsfc); orc.init_thermo(calc_Tsfc=calc_Tsfc)
    for n, frac in ((0, 0.3), (3, 0.05)):
        a, icells, ii, jj = synth.thermo_columns(37, 70, n, regime="mixed", seed=19 + n, ice_frac=frac)
        assert 0 < icells * 2 <= 37 * 70
        if not calc_Tsfc:
            orc.init_thermo(); t = {k: v.copy() for k, v in a.items()}
            assert orc.thermo_vertical(DT, icells, ii, jj, t, yday=120.0)[0] == 0
            a = synth.known_tsfc_inputs(a, t, seed=4)
            orc.init_thermo(calc_Tsfc=False)
        ag = {k: v.copy() for k, v in a.items()}; ac = {k: v.copy() for k, v in a.items()}
        lg = ctx.thermo_vertical(DT, icells, ii, jj, ag, yday=120.0)
        lc = orc.thermo_vertical(DT, icells, ii, jj, ac, yday=120.0)
        assert lg == lc == (0, 0, 0)
        for k in CHECK:
            assert np.array_equal(ag[k], ac[k]) or frel(k, ag[k], ac[k]) <= TOL, (n, k)
        outside = np.ones_like(a["aicen"], bool)
        outside[jj[:icells] - 1, ii[:icells] - 1] = False
        for k in ("aicen", "vicen", "vsnon", "fswsfc", "mlt_onset"):
            assert np.array_equal(ag[k][outside], a[k][outside]), k
        assert np.all(ag["fsensn"][outside] == 0.0) and np.all(ag["meltb"][outside] == 0.0)
    # error order in the compact form
    a, icells, ii, jj = synth.thermo_columns(20, 30, 2, regime="winter", seed=5, ice_frac=0.3)
    for e in (icells - 2, icells // 2):
        a["eicen"][2, jj[e] - 1, ii[e] - 1] *= 1e-3          # layer-3 enthalpy far too warm
    ag = {k: v.copy() for k, v in a.items()}; ac = {k: v.copy() for k, v in a.items()}
    ctx.thermo_init(); orc.init_thermo()
    lg = ctx.thermo_vertical(DT, icells, ii, jj, ag); lc = orc.thermo_vertical(DT, icells, ii, jj, ac)
    assert lg == lc and lg[0] == 1 and (lg[1], lg[2]) == (ii[icells // 2], jj[icells // 2])


@pytest.mark.parametrize("calc_Tsfc", [True, False])
def test_compact_and_full_path_agree_at_the_switch(ctx, orc, calc_Tsfc):
    """cice_thermo_vertical takes the compact path while 2 * icells <= nx * ny and the full one above.  On a block of
    120 cells the first 60 entries of one list go the compact way and the first 61 the full way: the 60 common cells
    come out bit for bit the same, each call equals the checker on its own list, and cells outside a list keep what
    they held, with zero in the outputs (calc_Tsfc = F: fsurfn, fcondtopn, flatn are inputs and stay)."""
    ny, nx = 10, 12
    ctx.thermo_init(calc_Tsfc=calc_Tsfc); orc.init_thermo(calc_Tsfc=calc_Tsfc)
    a, icells, ii, jj = synth.thermo_columns(ny, nx, 0, regime="mixed", seed=56, ice_frac=0.9)
    assert icells >= 61
    if not calc_Tsfc:
        orc.init_thermo(); t = {k: v.copy() for k, v in a.items()}
        assert orc.thermo_vertical(DT, icells, ii, jj, t, yday=120.0)[0] == 0
        a = synth.known_tsfc_inputs(a, t, seed=4)
        orc.init_thermo(calc_Tsfc=False)
    flux_in = () if calc_Tsfc else ("fsurfn", "fcondtopn", "flatn")
    got = {}
    for m in (60, 61):
        assert (2 * m <= nx * ny) == (m == 60)
        ag = {k: v.copy() for k, v in a.items()}; ac = {k: v.copy() for k, v in a.items()}
        lg = ctx.thermo_vertical(DT, m, ii, jj, ag, yday=120.0)
        lc = orc.thermo_vertical(DT, m, ii, jj, ac, yday=120.0)
        assert lg == lc == (0, 0, 0), (m, lg, lc)
        _cmp(ag, ac, ("switch", m))
        outside = np.ones((ny, nx), bool)
        outside[jj[:m] - 1, ii[:m] - 1] = False
        for k in CHECK:
            if k in lib.THERMO_OUT and k not in flux_in:
                assert np.all(ag[k][outside] == 0.0), (m, k)
            else:
                assert np.array_equal(ag[k][..., outside], a[k][..., outside]), (m, k)
        got[m] = ag
    common = np.zeros((ny, nx), bool)
    common[jj[:60] - 1, ii[:60] - 1] = True
    for k in CHECK:
        assert np.array_equal(got[60][k][..., common], got[61][k][..., common]), k
    assert not np.array_equal(got[60]["eicen"][..., common], a["eicen"][..., common])
    ctx.thermo_init(); orc.init_thermo()


def test_empty_list_and_all_melt(ctx, orc):
    ctx.thermo_init(); orc.init_thermo()
    a, icells, ii, jj = synth.thermo_columns(12, 20, 0, regime="summer", seed=3)
    ag = {k: v.copy() for k, v in a.items()}
    assert ctx.thermo_vertical(DT, 0, ii, jj, ag) == (0, 0, 0)
    assert np.array_equal(ag["vicen"], a["vicen"]) and np.all(ag["flatn"] == 0.0)
    # very thin ice under strong heating melts away completely: state is zeroed, Tsfc = Tbot.  The snow stays (without
    # it Sswabs and fswint would be shortwave absorbed by nothing, and the reference stops in its energy check).
    a["vicen"] *= 0.02; a["eicen"] *= 0.02
    a["fbot"][:] = -400.0
    ag = {k: v.copy() for k, v in a.items()}; ac = {k: v.copy() for k, v in a.items()}
    lg = ctx.thermo_vertical(DT, icells, ii, jj, ag); lc = orc.thermo_vertical(DT, icells, ii, jj, ac)
    assert lg == lc == (0, 0, 0)
    _cmp(ag, ac, "melt")
    assert _melted_come_back_exactly(a, ag, ac, icells, ii, jj) >= 8


def test_error_reporting_matches_reference_order(ctx, orc):
    """Bad enthalpy in several cells: the FIRST failure in the reference's order
    (stage, then list position) is the one reported."""
    ctx.thermo_init(); orc.init_thermo()
    a, icells, ii, jj = synth.thermo_columns(20, 30, 2, regime="winter", seed=5)
    bad = [icells // 3, icells // 2, icells - 2]
    # layer-3 enthalpy far too warm (Tin > Tmlt) in one cell, snow too cold (Tsn < Tmin) in a
    # later-listed one, and layer-1 too warm in the last: snow check comes first.
    q = lambda e: (jj[e] - 1, ii[e] - 1)
    a["eicen"][2][q(bad[0])] *= 1e-3
    a["esnon"][0][q(bad[1])] *= 3.0
    a["vsnon"][q(bad[1])] = max(a["vsnon"][q(bad[1])], 0.05)
    a["esnon"][0][q(bad[1])] = -330.0 * (3.34e5 + 2106.0 * 150.0) * a["vsnon"][q(bad[1])]
    a["eicen"][0][q(bad[2])] *= 1e-3
    ag = {k: v.copy() for k, v in a.items()}; ac = {k: v.copy() for k, v in a.items()}
    lg = ctx.thermo_vertical(DT, icells, ii, jj, ag); lc = orc.thermo_vertical(DT, icells, ii, jj, ac)
    assert lc[0] == 1 and lg == lc
    assert (lc[1], lc[2]) == (ii[bad[1]], jj[bad[1]])


def _batch_inputs(ny, nx, nb, seed, recipe=None):
    """Module-array-shaped inputs of the batched step from per-category column sets (recipe: see tc.batch_inputs)."""
    return tc.batch_inputs(ny, nx, nb, seed, recipe=recipe)


def test_batched_step_equals_per_category_calls(ctx, orc):
    """cice_thermo_batch_step = the n = 1..ncat loop of step_therm1 around thermo_vertical."""
    ctx.thermo_init(); orc.init_thermo()
    ny, nx, nb = 26, 40, 2
    batch, percat = _batch_inputs(ny, nx, nb, seed=21)
    ctx.thermo_batch_alloc(nx, ny, nb)
    ctx.thermo_batch_upload(batch)
    st = ctx.thermo_batch_step(DT, yday=150.0, timed=True)
    assert st["l_stop"] == 0 and st["ms"] > 0
    # of trcrn only the surface temperature travels (the column physics touches no other tracer): whatever the host
    # holds in the other planes when the batch comes back stays there
    orig = batch["trcrn"][:, :, 1:].copy()
    batch["trcrn"][:, :, 1:] = 7.0
    ctx.thermo_batch_download(batch)
    assert np.all(batch["trcrn"][:, :, 1:] == 7.0)
    batch["trcrn"][:, :, 1:] = orig
    nupd = 0
    for b in range(nb):
        mlt = percat[(b, 0)][0]["mlt_onset"].copy(); frz = percat[(b, 0)][0]["frz_onset"].copy()
        for n in range(5):
            a, icells, ii, jj = percat[(b, n)]
            ac = {k: v.copy() for k, v in a.items()}
            for k in lib.THERMO_FORCING:          # forcing is shared by the categories of a block
                ac[k] = percat[(b, 0)][0][k].copy()
            ac["mlt_onset"], ac["frz_onset"] = mlt, frz
            assert orc.thermo_vertical(DT, icells, ii, jj, ac, yday=150.0)[0] == 0
            nupd += icells
            for k in ("aicen", "vicen", "vsnon", "fswsfc", "fswint") + lib.THERMO_OUT:
                assert frel(k, batch[k][b, n], ac[k]) <= TOL, (b, n, k)
            assert relerr(batch["trcrn"][b, n], ac["trcrn"]) <= TOL
            assert relerr(batch["eicen"][b, n * 4:(n + 1) * 4], ac["eicen"]) <= TOL
            assert relerr(batch["esnon"][b, n:n + 1], ac["esnon"]) <= TOL
            assert relerr(batch["Iswabs"][b, n], ac["Iswabs"]) <= TOL
        assert np.array_equal(batch["mlt_onset"][b], mlt) and np.array_equal(batch["frz_onset"][b], frz)
    assert st["n_updates"] == nupd


@pytest.mark.parametrize("sort_chunk", [0, 256])
@pytest.mark.parametrize("conduct", ["MU71", "bubbly"])
def test_extreme_batch_equals_per_category_calls(ctx, orc, conduct, sort_chunk):
    """cice_thermo_batch_step on the extreme batch (tc.BATCH: one recipe per block), as k_thermo_dense and with the
    columns dealt to the lanes in sorted order (k_thermo_perm), against the per-category calls of the checker: every
    field, n_updates, the onset dates the categories of a cell share, the melted-away columns exactly, and the solver
    iterations the device keeps per column against the checker's trace."""
    ctx.thermo_init(conduct=conduct); orc.init_thermo(conduct=conduct)
    s = tc.BATCH
    ny, nx, nb = s["ny"], s["nx"], s["nb"]
    batch, percat = _batch_inputs(ny, nx, nb, seed=s["seed"], recipe=s["recipe"])
    ctx.thermo_batch_alloc(nx, ny, nb)
    ctx.thermo_set_option("sort_chunk", sort_chunk); ctx.thermo_set_option("sort_group", 8)
    ctx.thermo_batch_upload(batch)
    st = ctx.thermo_batch_step(DT, yday=s["yday"])
    ctx.thermo_set_option("sort_chunk", 0)
    assert st["l_stop"] == 0
    ctx.thermo_batch_download(batch)
    niter = ctx.evp_debug("thermo_niter").view(np.uint8)[:nb * 5 * ny * nx].reshape(nb, 5, ny, nx)
    res = tc.batch_checker_calls(orc, percat, nb, s["yday"])
    nupd = gone = 0
    for (b, n), (before, ac, trace, lc) in res.items():
        assert lc == (0, 0, 0)
        icells = percat[(b, n)][1]
        nupd += icells
        for k in ("aicen", "vicen", "vsnon", "fswsfc", "fswint") + lib.THERMO_OUT:
            assert frel(k, batch[k][b, n], ac[k]) <= TOL, (b, n, k)
        assert relerr(batch["trcrn"][b, n], ac["trcrn"]) <= TOL
        assert relerr(batch["eicen"][b, n * 4:(n + 1) * 4], ac["eicen"]) <= TOL
        assert relerr(batch["esnon"][b, n:n + 1], ac["esnon"]) <= TOL
        assert relerr(batch["Iswabs"][b, n], ac["Iswabs"]) <= TOL
        assert relerr(batch["Sswabs"][b, n], ac["Sswabs"]) <= TOL
        ag = dict(aicen=batch["aicen"][b, n], vicen=batch["vicen"][b, n], vsnon=batch["vsnon"][b, n],
                  eicen=batch["eicen"][b, n * 4:(n + 1) * 4], esnon=batch["esnon"][b, n:n + 1], trcrn=batch["trcrn"][b, n])
        gone += _melted_come_back_exactly(before, ag, ac, *percat[(b, n)][1:])
        listed = (trace & tc.TRACE["listed"]) != 0
        assert np.array_equal(niter[b, n][listed], (trace & 0xff)[listed].astype(np.uint8)), (b, n)
        if n == 4:
            assert np.array_equal(batch["mlt_onset"][b], ac["mlt_onset"])
            assert np.array_equal(batch["frz_onset"][b], ac["frz_onset"])
            assert not np.array_equal(ac["mlt_onset"], percat[(b, 0)][0]["mlt_onset"])
    assert st["n_updates"] == nupd and gone >= 8
    ctx.thermo_init(); orc.init_thermo()


@pytest.mark.parametrize("chunk,group,recipe", [(256, 1, None), (512, 8, None), (2048, 16, None), (256, 32, None),
                                                (512, 8, tc.BATCH["recipe"])],
                         ids=["256-1", "512-8", "2048-16", "256-32", "512-8-extreme"])
def test_sorted_columns_give_the_same_bits(ctx, chunk, group, recipe):
    """cice_thermo_set_option("sort_chunk", C): the columns of every chunk are dealt to the lanes in the order of the
    work they are expected to take (previous step's solver iterations, snow, cold / melting).  Which lane a column sits
    in changes nothing in its arithmetic: every field equals the unsorted step bit for bit, in the first step (no
    iteration counts yet) and in a second one (sorted by the first step's counts); planes that are no multiple of the
    chunk, two blocks, ice-free and ghost cells inside the chunks.  On the extreme batch (tc.BATCH at this size) the
    columns take 1 to 40 and more iterations and the second step's sort has a real spread."""
    ctx.thermo_init()
    ny, nx, nb = 29, 43, 2
    assert (ny, nx, nb, 33) == tuple(tc.SORTED[k] for k in ("ny", "nx", "nb", "seed"))
    batch, _ = _batch_inputs(ny, nx, nb, seed=33, recipe=recipe)
    keys = ("aicen", "vicen", "vsnon", "trcrn", "eicen", "esnon", "fswsfc", "fswint", "Sswabs", "Iswabs", "mlt_onset",
            "frz_onset") + lib.THERMO_OUT
    res = {}
    for sort in (0, chunk):
        ctx.thermo_batch_alloc(nx, ny, nb)
        ctx.thermo_set_option("sort_chunk", sort); ctx.thermo_set_option("sort_group", group)
        outs = []
        for step in range(2):
            b = {k: v.copy() for k, v in batch.items()}
            ctx.thermo_batch_upload(b)
            st = ctx.thermo_batch_step(DT, yday=150.0)
            assert st["l_stop"] == 0
            ctx.thermo_batch_download(b)
            outs.append((b, st["n_updates"]))
        res[sort] = outs
    ctx.thermo_set_option("sort_chunk", 0)
    for step in range(2):
        assert res[0][step][1] == res[chunk][step][1] > 0
        if recipe is not None:
            assert ((batch["aicen"] > 0) & (res[chunk][step][0]["aicen"] == 0)).sum() >= 8
        for k in keys:
            assert np.array_equal(res[0][step][0][k], res[chunk][step][0][k]), (step, k)


def test_batch_settings_hold_before_and_across_allocations():
    """On a context of its own: the sort options and the stage's timing switch set BEFORE the first cice_thermo_batch_alloc
    take effect, and survive re-allocations to another shape and back (the sorted step's permutation is there both times,
    every field of the second visit equals the first bit for bit); cice_thermo_batch_upload forgets the concentrations
    cice_step_therm1 kept, so the stage without aicen_init is refused behind it."""
    import therm_itd_case as ti
    c = lib.Context()
    try:
        c.thermo_set_option("sort_chunk", 256); c.thermo_set_option("sort_group", 8)
        c.therm2_itd_times(True)
        c.thermo_init()
        ny, nx, nb = 29, 43, 2
        batch, _ = _batch_inputs(ny, nx, nb, seed=33)
        keys = ("aicen", "vicen", "vsnon", "trcrn", "eicen", "esnon", "fswsfc", "fswint", "Sswabs", "Iswabs", "mlt_onset",
                "frz_onset") + lib.THERMO_OUT

        def shape_a():
            c.thermo_batch_alloc(nx, ny, nb)
            b = {k: v.copy() for k, v in batch.items()}
            c.thermo_batch_upload(b)
            st = c.thermo_batch_step(DT, yday=150.0)
            assert st["l_stop"] == 0 and st["n_updates"] > 0
            c.thermo_batch_download(b)
            assert c.evp_debug("thermo_perm").size > 0
            return b, st["n_updates"]

        r1 = shape_a()
        nyb, nxb = 12, 14
        small, _ = _batch_inputs(nyb, nxb, nb, seed=35)
        c.thermo_batch_alloc(nxb, nyb, nb)
        c.thermo_batch_upload({k: v.copy() for k, v in small.items()})
        assert c.thermo_batch_step(DT, yday=150.0)["l_stop"] == 0
        r2 = shape_a()
        assert r1[1] == r2[1]
        for k in keys:
            assert np.array_equal(r1[0][k], r2[0][k]), k
        # shape B again: cice_step_therm1 keeps the concentrations it found, an upload of the batch drops them
        c.itd_init(**ti.itd_kwargs(ti.CASES["growth"]))
        rng = np.random.default_rng(6)
        U = lambda lo, hi: np.ascontiguousarray(rng.uniform(lo, hi, (nb, nyb, nxb)))
        aice = np.ascontiguousarray(small["aicen"].sum(axis=1))
        fz = dict(aice=aice, frzmlt=U(-40, 60), Tf=np.full((nb, nyb, nxb), -1.8), strocnxT=U(-0.2, 0.2), strocnyT=U(-0.2, 0.2))
        fz["sst"] = fz["Tf"] + U(0, 0.5)
        pc = {k: np.ascontiguousarray(rng.uniform(-1, 1, small["aicen"].shape)) for k in ("strairxn", "strairyn", "Trefn", "Qrefn")}
        acc = {k: U(-1, 1) for k in lib.MERGE_ORDER}
        st = {k: v.copy() for k, v in small.items()}
        c.thermo_batch_alloc(nxb, nyb, nb)
        assert c.step_therm1(DT, ti.YDAY, st, fz, pc, acc)["l_stop"] == 0
        c.thermo_batch_upload(st)
        ice = st["aicen"].sum(axis=1) > ti.PUNY
        a = dict({k: st[k].copy() for k in ti.STATE}, vicen_init=small["vicen"].copy(), frain=U(0, 1e-5),
                 frzmlt=fz["frzmlt"].copy(), Tf=fz["Tf"].copy(),
                 rside=np.ascontiguousarray(np.where(ice & (fz["frzmlt"] < 0), U(0.005, 0.05), 0.0)),
                 tmask=np.ones((nb, nyb, nxb), np.int32), aice=aice.copy(), aice0=np.maximum(1 - aice, 0),
                 fresh=U(0, 1e-5), fsalt=U(0, 1e-7), fhocn=U(-5, 0), frazil=np.zeros((nb, nyb, nxb)),
                 meltl=np.zeros((nb, nyb, nxb)), frz_onset=np.zeros((nb, nyb, nxb)))
        with pytest.raises(lib.CiceError):
            c.step_therm2_itd(DT, ti.YDAY, {k: v.copy() for k, v in a.items()}, state_resident=True)
        a["aicen_init"] = small["aicen"].copy()
        assert c.step_therm2_itd(DT, ti.YDAY, a, state_resident=True)["l_stop"] == 0
        assert sum(c.therm2_itd_times()) > 0
    finally:
        c.close()


def test_batch_merge_equals_merge_fluxes(ctx, orc):
    """cice_thermo_batch_merge = merge_fluxes (ice_flux.F90:613) called once per category with
    that category's list and aicen_init, on the batch's own per-category outputs: bit for bit."""
    ctx.thermo_init(); orc.init_thermo()
    ny, nx, nb = 22, 34, 2
    batch, percat = _batch_inputs(ny, nx, nb, seed=33)
    aicen_init = batch["aicen"].copy()
    ctx.thermo_batch_alloc(nx, ny, nb)
    ctx.thermo_batch_upload(batch)
    assert ctx.thermo_batch_step(DT, yday=150.0)["l_stop"] == 0
    ctx.thermo_batch_download(batch)
    rng = np.random.default_rng(4)
    pc = dict(aicen_init=aicen_init)
    for k in ("strairxn", "strairyn", "Trefn", "Qrefn"):
        pc[k] = np.ascontiguousarray(rng.uniform(-1, 1, aicen_init.shape))
    acc0 = {k: np.ascontiguousarray(rng.uniform(-1, 1, (nb, ny, nx))) for k in lib.MERGE_ORDER}
    got = {k: v.copy() for k, v in acc0.items()}
    ctx.thermo_batch_merge(pc, got)
    src = dict(strairx="strairxn", strairy="strairyn", Tref="Trefn", Qref="Qrefn", fsurf="fsurfn",
               fcondtop="fcondtopn", fsens="fsensn", flat="flatn", fswabs="fswabsn", flwout="flwoutn",
               evap="evapn", fresh="freshn", fsalt="fsaltn", fhocn="fhocnn", fswthru="fswthrun",
               meltt="meltt", meltb="meltb", melts="melts", congel="congel", snoice="snoice")
    okeys = orc.MERGE_ORDER
    for b in range(nb):
        want = {ok: acc0[lk][b].copy() for ok, lk in zip(okeys, lib.MERGE_ORDER)}
        for n in range(5):
            a, icells, ii, jj = percat[(b, n)]
            catn = {ok: np.ascontiguousarray((pc if src[ok] in pc else batch)[src[ok]][b, n]) for ok in okeys}
            orc.merge_fluxes(icells, ii, jj, np.ascontiguousarray(aicen_init[b, n]),
                             np.ascontiguousarray(batch["flw"][b]), catn, want)
        for ok, lk in zip(okeys, lib.MERGE_ORDER):
            assert np.array_equal(got[lk][b], want[ok]), (b, lk)


def test_step_therm1_single_call_equals_the_separate_calls(ctx):
    """cice_step_therm1 (one upload, frzmlt_bottom_lateral -> thermo_vertical x ncat -> merge_fluxes on the device, one
    download) against the same work through the separate entries (frzmlt per block, batch upload / step / merge /
    download), which the tests above pin to the checker: every field bit for bit."""
    _step_therm1_both_ways(ctx, 22, 34, 2, 150.0, *tc.therm1_inputs(22, 34, 2, seed=35))


def test_step_therm1_single_call_on_the_extreme_batch(ctx):
    """the same on tc.THERM1: a melt potential that makes fbot of the order of -1500 W m-2 under the recipes' thin ice
    and strong shortwave, so that both ways melt columns through their layers and away"""
    s = tc.THERM1
    a, b_ = _step_therm1_both_ways(ctx, s["ny"], s["nx"], s["nb"], s["yday"],
                                   *tc.therm1_inputs(s["ny"], s["nx"], s["nb"], s["seed"], s["recipe"], s["frzmlt"], s["dsst"]))
    assert a["fbot"].min() < -1000.0
    assert ((b_["aicen_in"] > 0) & (b_["aicen"] == 0)).sum() >= 8


def _step_therm1_both_ways(ctx, ny, nx, nb, yday, batch, percat, fz, pc, acc0):
    ctx.thermo_init()
    # (a) separate entries
    a = {k: v.copy() for k, v in batch.items()}
    rs = np.zeros((nb, ny, nx))
    for b in range(nb):
        tb, fb, r = ctx.frzmlt_bottom_lateral(2, nx - 1, 2, ny - 1, DT, fz["aice"][b], fz["frzmlt"][b],
                                               np.ascontiguousarray(a["eicen"][b]), np.ascontiguousarray(a["esnon"][b]),
                                               fz["sst"][b], fz["Tf"][b], fz["strocnxT"][b], fz["strocnyT"][b])
        a["Tbot"][b] = tb; a["fbot"][b] = fb; rs[b] = r
    ctx.thermo_batch_alloc(nx, ny, nb)
    ctx.thermo_batch_upload(a)
    st_a = ctx.thermo_batch_step(DT, yday=yday)
    acc_a = {k: v.copy() for k, v in acc0.items()}
    ctx.thermo_batch_merge(dict(pc, aicen_init=batch["aicen"].copy()), acc_a)
    ctx.thermo_batch_download(a)
    # (b) one call
    b_ = {k: v.copy() for k, v in batch.items()}
    fzb = dict(fz, Tbot=np.zeros((nb, ny, nx)), fbot=np.zeros((nb, ny, nx)), rside=np.zeros((nb, ny, nx)))
    acc_b = {k: v.copy() for k, v in acc0.items()}
    st_b = ctx.step_therm1(DT, yday, b_, fzb, pc, acc_b)
    assert st_b["l_stop"] == st_a["l_stop"] == 0 and st_b["n_updates"] == st_a["n_updates"] > 0
    assert np.array_equal(fzb["Tbot"], a["Tbot"]) and np.array_equal(fzb["fbot"], a["fbot"]) and np.array_equal(fzb["rside"], rs)
    assert np.abs(fzb["fbot"]).max() > 0 and np.abs(rs).max() > 0
    for k in lib.THERMO_STATE + lib.THERMO_SW + lib.THERMO_OUT + lib.THERMO_ONSET:
        if k == "fswthrun":
            continue
        assert np.array_equal(b_[k], a[k]), k
    for k in lib.MERGE_ORDER:
        assert np.array_equal(acc_b[k], acc_a[k]), k
    b_["aicen_in"] = batch["aicen"]
    return a, b_


def test_thermo_state_handed_to_the_dynamics_on_the_device(ctx):
    """cice_thermo_batch_step leaves aicen, vicen, vsnon on the device;
    cice_evp_adopt_thermo_state makes them the dynamics' input there (aggregates formed on the device in the order of
    `aggregate`, ice_itd.F90:279) and the next evp(dt) uploads neither them nor aice, vice, vsno, aice0.  The result
    equals the two PCIe calls -- download the thermo state, aggregate on the host, evp(dt) with everything uploaded --
    bit for bit."""
    _hand_off_both_ways(ctx, None)


def test_thermo_state_of_an_extreme_step_handed_to_the_dynamics(ctx):
    """the same behind tc.ADOPT, a step that empties categories: they reach the dynamics as zeros, and the aggregates the
    device forms equal the sum in category order that the host forms in numpy (the dynamics' results are the same bits)"""
    before, after = _hand_off_both_ways(ctx, tc.ADOPT["recipe"])
    emptied = (before["aicen"] > 0) & (after["aicen"] == 0)
    assert emptied.sum() >= 8 and np.all(after["vicen"][emptied] == 0) and np.all(after["vsnon"][emptied] == 0)


def _hand_off_both_ways(ctx, recipe):
    DTE, NDTE_ = 3600.0, 24
    nxg, nyg = tc.ADOPT["nxg"], tc.ADOPT["nyg"]
    dom = ctx.domain_create(nxg, nyg, nxg, nyg, ew=1, ns=0)
    ny, nx, nb = dom["ny"], dom["nx"], 1
    assert (ny, nx) == (tc.ADOPT["ny"], tc.ADOPT["nx"])
    gg = synth.global_grid(nxg, nyg, perturb=0.1, land_frac=0.03, seed=5)
    grid = synth.block_fields(gg, dom)
    ctx.thermo_init()
    batch, _ = tc.adopt_batch(ny, nx, recipe, seed=tc.ADOPT["seed"])   # concentrations of a cell add up to at most 0.95
    before = {k: batch[k].copy() for k in ("aicen", "vicen", "vsnon")}
    ctx.thermo_batch_alloc(nx, ny, nb)
    ctx.thermo_batch_upload(batch)
    assert ctx.thermo_batch_step(DTE, yday=150.0)["l_stop"] == 0
    ctx.thermo_batch_download(batch)
    st = synth.evp_state(grid, dom, seed=5, cover="patchy")
    # path A: over PCIe -- the host aggregates (n = 1..ncat in order, ice_itd.F90:279) and uploads everything
    a = {k: v.copy() for k, v in st.items()}
    a["aicen"] = batch["aicen"].copy(); a["vicen"] = batch["vicen"].copy()
    for name, src in (("aice", "aicen"), ("vice", "vicen"), ("vsno", "vsnon")):
        acc = np.zeros((nb, ny, nx))
        for n in range(5):
            acc = acc + batch[src][:, n]
        a[name] = acc
    a["aice0"] = np.maximum(1.0 - a["aice"], 0.0)
    ctx.evp_init(grid, ndte=NDTE_)
    ctx.evp(DTE, a)
    # path B: on the device
    b = {k: v.copy() for k, v in st.items()}
    for k in ("aice", "vice", "vsno", "aice0", "aicen", "vicen"):
        b[k] = None
    ctx.evp_init(grid, ndte=NDTE_)
    ctx.evp_adopt_thermo_state()
    ctx.evp(DTE, b)
    for k in ("uvel", "vvel", "strength", "divu", "shear", "strocnxT", "strocnyT", "stressp_1", "stress12_4", "iceumask"):
        assert np.array_equal(a[k], b[k]), k
    assert np.abs(a["uvel"]).max() > 1e-4 and a["strength"].max() > 0
    with pytest.raises(lib.CiceError):       # without a fresh hand-off the six fields are required again
        ctx.evp(DTE, b)
    return before, batch


def test_frzmlt_bottom_lateral(ctx, orc):
    ctx.thermo_init(); orc.init_thermo()
    ny, nx = 30, 44
    rng = np.random.default_rng(8)
    aice = np.where(rng.uniform(0, 1, (ny, nx)) < 0.8, rng.uniform(0.01, 1, (ny, nx)), 0.0)
    frzmlt = rng.uniform(-60, 20, (ny, nx))
    eicen = -rng.uniform(1e6, 3e8, (20, ny, nx)); esnon = -rng.uniform(0, 5e7, (5, ny, nx))
    Tf = np.full((ny, nx), -1.8); sst = Tf + rng.uniform(0, 1.5, (ny, nx))
    sx = rng.uniform(-0.2, 0.2, (ny, nx)); sy = rng.uniform(-0.2, 0.2, (ny, nx))
    g = ctx.frzmlt_bottom_lateral(2, nx - 1, 2, ny - 1, DT, aice, frzmlt, eicen, esnon, sst, Tf, sx, sy)
    c = orc.frzmlt_bottom_lateral(2, nx - 1, 2, ny - 1, DT, aice, frzmlt, eicen, esnon, sst, Tf, sx, sy)
    for a, b, nm in zip(g, c, ("Tbot", "fbot", "rside")):
        assert relerr(a, b) <= TOL_POW, nm


def test_fortran_dropin_thermo_module(orc):
    """The reference's callers + wrapper linked with OUR cice4_amd/fortran/ice_therm_vertical.F90:
    `call thermo_vertical(...)` / `call frzmlt_bottom_lateral(...)` go Fortran -> ISO_C_BINDING
    shim -> GPU and must reproduce the checker; init_thermo_vertical hands back the salinity
    profile."""
    from oracle import refapi
    if not refapi.available("gx3b4", "dropin"):
        pytest.skip("oracle/_ref/libcice_dropin_gx3b4.so not built")
    ref = refapi.Ref("gx3b4", kind="dropin")
    sr, tr = ref.init_thermo(); so, to = orc.init_thermo()
    assert relerr(sr, so) < 1e-15 and relerr(tr, to) < 1e-15
    for n in (0, 2, 4):
        a, icells, ii, jj = synth.thermo_columns(30, 44, n, regime="mixed", seed=77)
        ag = {k: v.copy() for k, v in a.items()}; ac = {k: v.copy() for k, v in a.items()}
        assert ref.thermo_vertical(DT, icells, ii, jj, ag, yday=100.0) == \
            orc.thermo_vertical(DT, icells, ii, jj, ac, yday=100.0) == (0, 0, 0)
        _cmp(ag, ac, ("dropin", n))
    # calc_Tsfc = F through the module variable (namelist calc_Tsfc, ice_init.F90:107)
    a, icells, ii, jj = synth.thermo_columns(30, 44, 1, regime="mixed", seed=78)
    t = {k: v.copy() for k, v in a.items()}
    assert orc.thermo_vertical(DT, icells, ii, jj, t, yday=100.0)[0] == 0
    b = synth.known_tsfc_inputs(a, t, seed=3)
    ref.init_thermo(calc_Tsfc=False); orc.init_thermo(calc_Tsfc=False)
    bg = {k: v.copy() for k, v in b.items()}; bc = {k: v.copy() for k, v in b.items()}
    assert ref.thermo_vertical(DT, icells, ii, jj, bg, yday=100.0) == \
        orc.thermo_vertical(DT, icells, ii, jj, bc, yday=100.0) == (0, 0, 0)
    for k in CHECK:
        assert np.array_equal(bg[k], bc[k]), ("dropin calc_Tsfc=F", k)
    ref.init_thermo(); orc.init_thermo()
    # error path through the Fortran logical
    a, icells, ii, jj = synth.thermo_columns(20, 30, 2, regime="winter", seed=5)
    a["eicen"][1][jj[7] - 1, ii[7] - 1] *= 40.0
    ag = {k: v.copy() for k, v in a.items()}; ac = {k: v.copy() for k, v in a.items()}
    lg = ref.thermo_vertical(DT, icells, ii, jj, ag); lc = orc.thermo_vertical(DT, icells, ii, jj, ac)
    assert lc[0] == 1 and lg == lc
    ny, nx = 30, 44
    rng = np.random.default_rng(8)
    aice = np.where(rng.uniform(0, 1, (ny, nx)) < 0.8, rng.uniform(0.01, 1, (ny, nx)), 0.0)
    args = (2, nx - 1, 2, ny - 1, DT, aice, rng.uniform(-60, 20, (ny, nx)), -rng.uniform(1e6, 3e8, (20, ny, nx)),
            -rng.uniform(0, 5e7, (5, ny, nx)), np.full((ny, nx), -1.8) + rng.uniform(0, 1.5, (ny, nx)),
            np.full((ny, nx), -1.8), rng.uniform(-0.2, 0.2, (ny, nx)), rng.uniform(-0.2, 0.2, (ny, nx)))
    for x, y, nm in zip(ref.frzmlt_bottom_lateral(*args), orc.frzmlt_bottom_lateral(*args), ("Tbot", "fbot", "rside")):
        assert relerr(x, y) <= TOL_POW, nm

