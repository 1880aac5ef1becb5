"""atmo_boundary_layer (source/ice_atmo.F90:56-384) on the device against the compiled reference
(oracle/_ref, ref_atmo_boundary_layer).  The kernel evaluates exp with glibc's algorithm but log and atan with the
device library (<= 1 ulp): the five stability iterations are contractive, so the outputs agree to ~1e-14; the bound
asserted here is 1e-12 relative to each field's magnitude (north_star: <= 1e-10).  The same stage inside the one-call
thermodynamic half-step (cice_step_therm1_abl) against the reference's routine feeding cice_step_therm1.

The tests from test_list_kernel_against_the_fixture on need no compiled reference: they hold k_atmo_list to
tests/golden/atmo.npz (minted from it; cases and classes: tests/atmo_case.py) word class by word class -- zeros off the list,
the caller's stresses under calc_strair = F, delt and delq bit for bit, and the six outputs that pass through log and atan
per cell against the extended-precision restatement, within 4 E_ref + 2**-52 where E_ref is the reference's own largest
per-cell deviation from it (computed here from the fixture) -- and k_atmo_dense to k_atmo_list bit for bit."""
import numpy as np
import pytest

import atmo_case as ac
from cice4_amd import lib, synth
from conftest import TOL_EXP

pytestmark = pytest.mark.gpu
TOL = 1e-12
DT = 3600.0


def _inputs(ny, nx, seed, regime):
    rng = np.random.default_rng(seed)
    U = lambda lo, hi: rng.uniform(lo, hi, (ny, nx))
    a = dict(potT=U(238, 280), uatm=U(-15, 15), vatm=U(-15, 15), zlvl=U(8, 40), Qa=U(0.0002, 0.005), rhoa=U(1.2, 1.4))
    a["wind"] = np.sqrt(a["uatm"] ** 2 + a["vatm"] ** 2)
    calm = rng.uniform(0, 1, (ny, nx)) < 0.1                  # below umin (:201)
    a["wind"][calm] *= 0.02; a["uatm"][calm] *= 0.02; a["vatm"][calm] *= 0.02
    TairC = a["potT"] - 273.15
    if regime == "stable":          # surface colder than the air
        a["Tsf"] = np.minimum(TairC - U(0.5, 15), 0.0)
    elif regime == "unstable":      # surface warmer
        a["Tsf"] = np.minimum(TairC + U(0.5, 25), 0.0)
    else:
        a["Tsf"] = np.minimum(TairC + U(-12, 12), 0.0)
    mask = rng.uniform(0, 1, (ny, nx)) < 0.8
    mask[0, :] = mask[-1, :] = False; mask[:, 0] = mask[:, -1] = False
    jj, ii = np.nonzero(mask)
    indxi = np.zeros(ny * nx, np.int32); indxj = np.zeros(ny * nx, np.int32)
    indxi[:ii.size] = ii + 1; indxj[:ii.size] = jj + 1
    return a, int(ii.size), indxi, indxj, mask


def _close(g, c, tag):
    for k in g:
        den = np.abs(c[k]).max()
        err = np.abs(g[k] - c[k]).max() / den if den > 0 else np.abs(g[k]).max()
        assert err <= TOL, (tag, k, err)


@pytest.mark.parametrize("sfctype", ["ice", "ocn"])
@pytest.mark.parametrize("regime", ["stable", "unstable", "mixed"])
def test_atmo_boundary_layer_matches_reference(ctx, ref_gx3, sfctype, regime):
    a, icells, ii, jj, mask = _inputs(37, 70, 5, regime)
    if sfctype == "ocn":
        a["Tsf"] = a["Tsf"] + 2.0 + np.abs(a["Tsf"]) * 0.1     # sea-surface temperatures around and above freezing
    g = ctx.atmo_boundary_layer(sfctype, icells, ii, jj, a)
    c = ref_gx3.atmo_boundary_layer(sfctype, icells, ii, jj, a)
    _close(g, c, (sfctype, regime))
    for k in g:                                                # zero outside the list, exactly
        assert np.all(g[k][~mask] == 0.0), k
    assert np.abs(c["lhcoef"]).max() > 0
    if regime != "unstable":
        assert (c["delt"] > 0).any()            # stable stratification exercised (psimhs branch)
    if regime != "stable":
        assert (c["delt"] < 0).any()            # unstable (log / atan branch)


def test_atmo_data_stresses_and_empty_list(ctx, ref_gx3):
    """calc_strair = F: strx, stry are the caller's and stay untouched (:309); an empty list zeroes the outputs."""
    a, icells, ii, jj, mask = _inputs(20, 31, 9, "mixed")
    rng = np.random.default_rng(2)
    sx, sy = rng.uniform(-1, 1, mask.shape), rng.uniform(-1, 1, mask.shape)
    g = ctx.atmo_boundary_layer("ice", icells, ii, jj, a, calc_strair=False, strx=sx, stry=sy)
    c = ref_gx3.atmo_boundary_layer("ice", icells, ii, jj, a, calc_strair=False, strx=sx, stry=sy)
    assert np.array_equal(g["strx"], sx) and np.array_equal(c["strx"], sx) and np.array_equal(g["stry"], sy)
    _close(g, c, "data stresses")
    g = ctx.atmo_boundary_layer("ice", 0, ii, jj, a)
    assert all(np.all(v == 0.0) for v in g.values())


@pytest.mark.parametrize("calc_strair", [True, False])
def test_step_therm1_with_boundary_layer_on_the_device(ctx, ref_gx3, calc_strair):
    """cice_step_therm1_abl = the reference's atmo_boundary_layer per category (CICE_RunMod.F90:402-439) feeding
    cice_step_therm1 (which the thermo tests pin bit for bit)."""
    from test_gpu_thermo import _batch_inputs
    ctx.thermo_init()
    ny, nx, nb, NC = 22, 34, 2, 5
    batch, percat = _batch_inputs(ny, nx, nb, seed=41)
    rng = np.random.default_rng(12)
    U = lambda lo, hi: np.ascontiguousarray(rng.uniform(lo, hi, (nb, ny, nx)))
    atm = dict(uatm=U(-12, 12), vatm=U(-12, 12), zlvl=U(8, 30), strax=U(-0.3, 0.3), stray=U(-0.3, 0.3),
               calc_strair=calc_strair)
    atm["wind"] = np.sqrt(atm["uatm"] ** 2 + atm["vatm"] ** 2)
    fz = dict(aice=np.ascontiguousarray(batch["aicen"].sum(axis=1)), frzmlt=U(-60, 20), Tf=np.full((nb, ny, nx), -1.8),
              strocnxT=U(-0.2, 0.2), strocnyT=U(-0.2, 0.2))
    fz["sst"] = fz["Tf"] + U(0, 0.5)
    acc0 = {k: U(-1, 1) for k in lib.MERGE_ORDER}
    # (a) the reference's routine per block and category, then the one-call step with its outputs as inputs
    a = {k: v.copy() for k, v in batch.items()}
    pc = {k: np.zeros((nb, NC, ny, nx)) for k in ("strairxn", "strairyn", "Trefn", "Qrefn")}
    for b in range(nb):
        for n in range(NC):
            act = a["aicen"][b, n] > 1e-11
            act[0, :] = act[-1, :] = False; act[:, 0] = act[:, -1] = False
            jj, ii = np.nonzero(act)
            indxi = np.zeros(ny * nx, np.int32); indxj = np.zeros(ny * nx, np.int32)
            indxi[:ii.size] = ii + 1; indxj[:ii.size] = jj + 1
            ins = dict(Tsf=a["trcrn"][b, n, 0], potT=a["potT"][b], uatm=atm["uatm"][b], vatm=atm["vatm"][b],
                       wind=atm["wind"][b], zlvl=atm["zlvl"][b], Qa=a["Qa"][b], rhoa=a["rhoa"][b])
            o = ref_gx3.atmo_boundary_layer("ice", int(ii.size), indxi, indxj, ins, calc_strair=calc_strair,
                                            strx=atm["strax"][b], stry=atm["stray"][b])
            pc["strairxn"][b, n], pc["strairyn"][b, n] = o["strx"], o["stry"]
            pc["Trefn"][b, n], pc["Qrefn"][b, n] = o["Tref"], o["Qref"]
            a["lhcoef"][b, n], a["shcoef"][b, n] = o["lhcoef"], o["shcoef"]
    ctx.thermo_batch_alloc(nx, ny, nb)
    acc_a = {k: v.copy() for k, v in acc0.items()}
    st_a = ctx.step_therm1(DT, 150.0, a, dict(fz), pc, acc_a)
    # (b) everything on the device
    b_ = {k: v.copy() for k, v in batch.items()}
    b_["lhcoef"][...] = np.nan; b_["shcoef"][...] = np.nan          # must not be read
    outs = {k: np.full((nb, NC, ny, nx), 7.0) for k in ("strairxn", "strairyn", "Trefn", "Qrefn", "lhcoef", "shcoef")}
    acc_b = {k: v.copy() for k, v in acc0.items()}
    st_b = ctx.step_therm1(DT, 150.0, b_, dict(fz), {}, acc_b, atm=dict(atm, **outs))
    assert st_a["l_stop"] == st_b["l_stop"] == 0 and st_a["n_updates"] == st_b["n_updates"] > 0

    def close(x, y, k):
        den = np.abs(y).max()
        assert (np.abs(x - y).max() / den if den > 0 else np.abs(x).max()) <= 1e-10, k
    for k in ("strairxn", "strairyn", "Trefn", "Qrefn"):
        close(outs[k], pc[k], k)
    close(outs["lhcoef"], a["lhcoef"], "lhcoef"); close(outs["shcoef"], a["shcoef"], "shcoef")
    for k in lib.THERMO_STATE + lib.THERMO_SW + lib.THERMO_OUT + lib.THERMO_ONSET:
        if k != "fswthrun":
            close(b_[k], a[k], k)
    for k in lib.MERGE_ORDER:
        close(acc_b[k], acc_a[k], k)


# ---- the list kernel against tests/golden/atmo.npz --------------------------------------------------------------------

def _device_list(ctx, sfctype, icells, indxi, indxj, a, calc_strair=True, strx=None, stry=None):
    """cice_atmo_boundary_layer with every array it only writes handed in full of NaN: an unwritten word shows"""
    ny, nx = a["Tsf"].shape
    o = {k: np.full((ny, nx), np.nan) for k in ac.OUT}
    if not calc_strair:
        o["strx"][...] = strx; o["stry"][...] = stry
    ins = [np.ascontiguousarray(a[k], np.float64) for k in ac.INS]
    ctx._ck(ctx.lib.cice_atmo_boundary_layer(
        ctx.h, nx, ny, 0 if sfctype == "ice" else 1, icells, lib._i4(indxi), lib._i4(indxj), *[lib._f8(x) for x in ins],
        int(calc_strair), *[lib._f8(o[k]) for k in ac.OUT]))
    return o


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.fixture(scope="module")
def golden():
    """the fixture, and per case: inputs, list, the reference's outputs, E_ref per field and the extended-precision
    restatement it is measured against -- computed once, on the host"""
    d = np.load(ac.FIXTURE)
    g = {}
    for name in ac.CASES:
        a, mask, ref = ac.load_case(d, name)
        e_ref, truth = ac.reference_error(d, name)
        g[name] = dict(a=a, mask=mask, ref=ref, e_ref=e_ref, truth=truth, lst=ac.make_list(mask))
    return d, g


@pytest.fixture(scope="module")
def device(ctx, golden):
    """per case the device's run on the case's list with calc_strair = T; the inputs must come back as they went in"""
    r = {}
    for name, c in ac.CASES.items():
        g = golden[1][name]
        a = {k: v.copy() for k, v in g["a"].items()}
        r[name] = _device_list(ctx, c["sfctype"], *g["lst"], a)
        for k in ac.INS:
            assert np.array_equal(_bits(a[k]), _bits(g["a"][k])), (name, k, "an input array changed")
    return r


@pytest.mark.parametrize("name", tuple(ac.CASES))
def test_list_kernel_against_the_fixture(golden, device, name):
    """k_atmo_list on a case's list, word class by word class (the module's docstring); the measured figures are printed
    before anything is asserted on them (DESIGN.md 3.6 has those of the MI355X)."""
    g, dev = golden[1][name], device[name]
    mask, ref = g["mask"], g["ref"]
    for k in ac.OUT:
        assert np.isfinite(dev[k]).all(), (name, k, "a word was not written")
        assert not _bits(dev[k][~mask]).any(), (name, k, "a word off the list is not +0")
    for k in ac.OUT_EXP:                        # exp alone: glibc's algorithm on the device
        if TOL_EXP == 0.0:
            assert np.array_equal(_bits(dev[k]), _bits(ref[k])), (name, k, int((_bits(dev[k]) != _bits(ref[k])).sum()))
        else:
            assert np.abs(dev[k] - ref[k]).max() <= TOL_EXP * np.abs(ref[k]).max(), (name, k)
    e_dev = {k: ac.cell_deviation(dev[k], g["truth"][k], mask) for k in ac.OUT_LOG}      # zeros: same sign, asserted there
    differ = {k: int((_bits(dev[k]) != _bits(ref[k])).sum()) for k in ac.OUT}
    print(f"{name}: E_ref  " + ", ".join(f"{k} {v:.3e}" for k, v in g["e_ref"].items()))
    print(f"{name}: device " + ", ".join(f"{k} {v:.3e}" for k, v in e_dev.items()))
    print(f"{name}: words that differ bitwise from the reference, of {int(mask.sum())} listed cells per field: {differ}")
    nz = {k: mask & (ref[k] != 0) for k in ac.OUT_LOG}
    print(f"{name}: largest per-cell deviation from the reference " +
          ", ".join(f"{k} {(np.abs(dev[k][nz[k]] - ref[k][nz[k]]) / np.abs(ref[k][nz[k]])).max():.3e}" for k in ac.OUT_LOG))
    for k in ac.OUT_LOG:
        assert e_dev[k] <= 4.0 * g["e_ref"][k] + 2.0 ** -52, (name, k, e_dev[k], g["e_ref"][k])
    _close(dev, ref, ("fixture", name))


def test_list_kernel_data_stresses_against_the_fixture(ctx, golden, device):
    """calc_strair = F: strx, stry come back bit for bit as they went in, on the list and off it; nothing else changes"""
    d, g = golden[0], golden[1][ac.LIST_CASE]
    sx, sy = d[f"{ac.LIST_CASE}_F_strx_in"], d[f"{ac.LIST_CASE}_F_stry_in"]
    dev = _device_list(ctx, ac.CASES[ac.LIST_CASE]["sfctype"], *g["lst"], g["a"], calc_strair=False, strx=sx, stry=sy)
    assert np.array_equal(_bits(dev["strx"]), _bits(sx)) and np.array_equal(_bits(dev["stry"]), _bits(sy))
    for k in ac.OUT[2:]:
        assert np.array_equal(_bits(dev[k]), _bits(device[ac.LIST_CASE][k])), k
    _close(dev, ac.unpack(d, ac.LIST_CASE + "_F", g["mask"], sx, sy), "fixture, data stresses")


@pytest.mark.parametrize("count", ac.SUBLISTS + ("interior",))
def test_sublists_give_the_bits_of_the_full_list(ctx, golden, device, count):
    """1, 255, 256 and 257 cells (the workgroup edge of k_atmo_list) and the full interior: a cell's result does not depend
    on the list it is on, and a cell that is on none is +0"""
    d, g, full = golden[0], golden[1][ac.LIST_CASE], device[ac.LIST_CASE]
    sfc = ac.CASES[ac.LIST_CASE]["sfctype"]
    icells, indxi, indxj = g["lst"]
    if count == "interior":
        sub = ac.interior()
        dev = _device_list(ctx, sfc, *ac.make_list(sub), g["a"])
        _close(dev, ac.unpack(d, ac.LIST_CASE + "_interior", sub), "fixture, interior")
        assert (sub & ~g["mask"]).sum() >= 100
    else:
        assert count < icells
        sub = np.zeros(g["mask"].shape, bool)
        sub[indxj[:count] - 1, indxi[:count] - 1] = True
        dev = _device_list(ctx, sfc, count, indxi, indxj, g["a"])
    shared = sub & g["mask"]
    assert shared.sum() == (icells if count == "interior" else count)
    for k in ac.OUT:
        assert np.isfinite(dev[k]).all(), (count, k)
        assert np.array_equal(_bits(dev[k][shared]), _bits(full[k][shared])), (count, k)
        assert not _bits(dev[k][~sub]).any(), (count, k)


# ---- the dense kernel against the list kernel --------------------------------------------------------------------------

DENSE_OUT = dict(strairxn="strx", strairyn="stry", Trefn="Tref", Qrefn="Qref", lhcoef="lhcoef", shcoef="shcoef")
PUNY = 1.0e-11


def _dense_inputs(nx, ny, nb, seed):
    """the inputs of cice_step_therm1_abl on nb blocks of ny x nx; in every (block, category) two cells of the interior are
    scaled down to aicen == puny exactly (not on the list) and two to the next double above it (on the list), thicknesses
    and enthalpies per unit area kept"""
    from test_gpu_thermo import _batch_inputs
    NC = 5
    batch, _ = _batch_inputs(ny, nx, nb, seed=seed)
    rng = np.random.default_rng(seed + 1)
    at, above = [], []
    for b in range(nb):
        for n in range(NC):
            jj, ii = np.nonzero(batch["aicen"][b, n] > 0.02)
            pick = rng.choice(jj.size, 4, replace=False)
            for m, p in enumerate(pick):
                j, i = jj[p], ii[p]
                new = PUNY if m < 2 else np.nextafter(PUNY, 1.0)
                f = new / batch["aicen"][b, n, j, i]
                batch["aicen"][b, n, j, i] = new
                batch["vicen"][b, n, j, i] *= f; batch["vsnon"][b, n, j, i] *= f
                batch["eicen"][b, n * 4:(n + 1) * 4, j, i] *= f; batch["esnon"][b, n, j, i] *= f
                (at if m < 2 else above).append((b, n, j, i))
    U = lambda lo, hi: np.ascontiguousarray(rng.uniform(lo, hi, (nb, ny, nx)))  # noqa: E731
    atm = dict(uatm=U(-12, 12), vatm=U(-12, 12), zlvl=U(8, 30), strax=U(-0.3, 0.3), stray=U(-0.3, 0.3))
    atm["wind"] = np.sqrt(atm["uatm"] ** 2 + atm["vatm"] ** 2)
    fz = dict(aice=np.ascontiguousarray(batch["aicen"].sum(axis=1)), frzmlt=U(-60, 20), Tf=np.full((nb, ny, nx), -1.8),
              strocnxT=U(-0.2, 0.2), strocnyT=U(-0.2, 0.2))
    fz["sst"] = fz["Tf"] + U(0, 0.5)
    acc = {k: U(-1, 1) for k in lib.MERGE_ORDER}
    return batch, atm, fz, acc, at, above


@pytest.mark.parametrize("calc_strair", [True, False])
@pytest.mark.parametrize("nx,ny", [(64, 5), (66, 5), (67, 4)])
def test_dense_kernel_gives_the_list_kernels_bits(ctx, nx, ny, calc_strair):
    """k_atmo_dense (what cice_step_therm1_abl runs on every category of every block) = k_atmo_list per (block, category) on
    the list {interior, aicen > puny} with Tsf from tracer plane 0, bit for bit: rows of 64, 66 and 67 cells, cells with
    aicen == puny (off the list) and one ulp above (on it), both settings of calc_strair.  Off the list +0, but for the
    stresses under calc_strair = F, which are strax / stray on every cell, ghost cells included."""
    nb, NC = 2, 5
    ctx.thermo_init()
    batch, atm, fz, acc, at, above = _dense_inputs(nx, ny, nb, seed=300 + nx)
    assert len(at) >= 8 and len(above) >= 8 and len({n for _, n, _, _ in at}) == len({n for _, n, _, _ in above}) == NC
    before = {k: batch[k].copy() for k in ("aicen", "trcrn", "potT", "Qa", "rhoa")}
    batch["lhcoef"][...] = np.nan; batch["shcoef"][...] = np.nan          # must not be read
    outs = {k: np.full((nb, NC, ny, nx), 7.0) for k in DENSE_OUT}
    ctx.thermo_batch_alloc(nx, ny, nb)
    st = ctx.step_therm1(DT, 150.0, batch, dict(fz), {}, acc, atm=dict(atm, calc_strair=calc_strair, **outs))
    assert st["l_stop"] == 0 and st["n_updates"] > 0
    inside = np.zeros((ny, nx), bool)
    inside[1:-1, 1:-1] = True
    for k in DENSE_OUT:
        assert np.isfinite(outs[k]).all() and (outs[k] != 7.0).all(), (k, "a word was not written")
    listed = np.zeros((nb, NC, ny, nx), bool)
    for b in range(nb):
        for n in range(NC):
            act = inside & (before["aicen"][b, n] > PUNY)
            listed[b, n] = act
            ins = dict(Tsf=before["trcrn"][b, n, 0], potT=before["potT"][b], Qa=before["Qa"][b], rhoa=before["rhoa"][b],
                       **{k: atm[k][b] for k in ("uatm", "vatm", "wind", "zlvl")})
            o = ctx.atmo_boundary_layer("ice", *ac.make_list(act), ins, calc_strair=calc_strair, strx=atm["strax"][b],
                                        stry=atm["stray"][b])
            for k, src in DENSE_OUT.items():
                assert np.array_equal(_bits(outs[k][b, n]), _bits(o[src])), (b, n, k)
            for k in DENSE_OUT:
                if calc_strair or k not in ("strairxn", "strairyn"):
                    assert not _bits(outs[k][b, n][~act]).any(), (b, n, k, "a word off the list is not +0")
            if not calc_strair:
                assert np.array_equal(_bits(outs["strairxn"][b, n]), _bits(atm["strax"][b]))
                assert np.array_equal(_bits(outs["strairyn"][b, n]), _bits(atm["stray"][b]))
    for b, n, j, i in at:
        assert not listed[b, n, j, i] and outs["lhcoef"][b, n, j, i] == 0.0 and outs["Trefn"][b, n, j, i] == 0.0
    for b, n, j, i in above:
        assert listed[b, n, j, i] and outs["lhcoef"][b, n, j, i] != 0.0 and outs["Trefn"][b, n, j, i] > 100.0
    assert listed.sum() >= 100 and (~listed & inside).sum() >= 100
