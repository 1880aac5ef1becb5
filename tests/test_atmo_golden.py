"""tests/golden/atmo.npz (minted from the compiled reference by tests/golden/make_golden_atmo.py): it loads, says how it was
made, belongs to the inputs tests/atmo_case.py builds today, holds every class of atmo_case.BRANCHES in at least 8 cells of
each case's constructed part, obeys the conditioning rule of atmo_case (|hol| exactly 0 or >= 1e-6 in every listed cell and
iteration; the extended-precision restatement on the same side of hol = 0), is what the compiled reference gives today (where
that is built), and agrees with atmo_case.atmo_numpy -- the routine restated in float64 with the host libm's exp, log and
atan -- to 1e-12 of each field's magnitude and per cell to the bound the device is held to (4 E_ref + 2**-52).  The words
that differ bitwise between restatement and reference are counted and printed, not asserted; delt and delq
pass through exp alone and are bit-equal where conftest.TOL_EXP == 0.  E_ref, the reference's own per-cell deviation from the
extended-precision restatement, is computed here from the committed data and printed."""
import importlib.util
import os

import numpy as np
import pytest

import atmo_case as ac
from conftest import TOL_EXP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def d():
    return np.load(ac.FIXTURE)


@pytest.fixture(scope="module")
def restated(d):
    """per case: inputs, list mask, the reference's outputs, (outputs, hol) of the restatement, (outputs, hol) of the
    extended-precision restatement -- computed once"""
    r = {}
    for name, c in ac.CASES.items():
        a, mask, ref = ac.load_case(d, name)
        lst = ac.make_list(mask)
        r[name] = (a, mask, ref, ac.atmo_numpy(c["sfctype"], *lst, a), ac.atmo_truth(c["sfctype"], *lst, a))
    return r


def test_fixture_meta(d):
    meta = str(d["meta"][0])
    assert "flang" in meta and "-ffp-contract=off" in meta and "-fdefault-real-8" in meta and "-O2" in meta
    assert "make_golden_atmo.py" in meta and "ice_atmo" in meta and "atmo_boundary_layer" in meta
    assert os.path.getsize(ac.FIXTURE) < (1 << 20)
    assert tuple(str(x) for x in d["branches"]) == ac.BRANCHES
    assert tuple(ac.CASES) == ("ice", "ocn") and [c["sfctype"] for c in ac.CASES.values()] == ["ice", "ocn"]
    assert ac.NY * ac.NX <= 4000 and tuple(int(x) for x in d[f"{ac.LIST_CASE}_sublists"]) == ac.SUBLISTS == (1, 255, 256, 257)


@pytest.mark.parametrize("name", tuple(ac.CASES))
def test_inputs_match_seeds(d, name):
    assert int(d[f"{name}_seed"]) == ac.CASES[name]["seed"]
    a, mask, sx, sy = ac.make_inputs(name)
    for k in ac.INS:
        assert np.array_equal(a[k].view(np.uint64), d[f"{name}_{k}"].view(np.uint64)), k
    assert ac.digest(a) == str(d[f"{name}_sha256"])
    icells, indxi, indxj = ac.make_list(mask)
    assert icells == int(d[f"{name}_icells"]) > max(ac.SUBLISTS)
    assert np.array_equal(indxi[:icells], d[f"{name}_indxi"]) and np.array_equal(indxj[:icells], d[f"{name}_indxj"])
    assert (mask & ~ac.interior()).sum() == 0 and (ac.interior() & ~mask).sum() >= 100      # unlisted cells inside the block
    if name == ac.LIST_CASE:
        assert np.array_equal(sx, d[f"{name}_F_strx_in"]) and np.array_equal(sy, d[f"{name}_F_stry_in"])


def test_branch_counts(d, restated):
    for name, c in ac.CASES.items():
        a, mask, ref, ours, _ = restated[name]
        counts = ac.branch_counts(c["sfctype"], a, mask, ref, ours)
        assert [counts[k] for k in ac.BRANCHES] == [int(x) for x in d[f"{name}_counts"]], name
        short = {k: v for k, v in counts.items() if v < ac.needed(c["sfctype"])[k]}
        assert not short, (name, short)
        print(f"{name}: cells of the constructed part per class: {counts}")
    assert ac.NEED >= 8 and all(ac.needed("ocn")[k] >= 8 for k in ac.BRANCHES)
    assert all(ac.needed("ice")[k] >= 8 for k in ac.BRANCHES if k not in ac.OCN_ONLY)


def test_constructed_cells_are_what_they_are_called(restated):
    """the cells built for a class are in it, flips go both ways, still air has zeros of both signs, delq of both signs on
    delt0, and the ocean case spans both sides of the minimum of rdn"""
    for name, c in ac.CASES.items():
        a, mask, ref, (want, hol), _ = restated[name]
        m = ac.class_masks(c["sfctype"], a, hol, mask)
        for k, cell in ac.constructed(c["sfctype"]).items():
            assert m[k][cell].all(), (name, k)
        cell = ac.constructed(c["sfctype"])["flip"]
        assert (hol[0][cell] < 0).any() and (hol[0][cell] > 0).any()
        cell = ac.constructed(c["sfctype"])["still"]
        for k in ("strx", "stry"):
            assert (ref[k][cell] == 0).all() and np.signbit(ref[k][cell]).any() and not np.signbit(ref[k][cell]).all(), (name, k)
        cell = ac.constructed(c["sfctype"])["delt0"]
        assert (ref["delq"][cell] < 0).any() and (ref["delq"][cell] > 0).any() and not ref["delt"][cell].view(np.uint64).any()
        cell = ac.constructed(c["sfctype"])["neutral"]
        assert not hol[:, cell[0], cell[1]].view(np.uint64).any()          # hol = +0 in all five iterations
        if name == "ocn":
            w = np.concatenate([a["wind"][ac.constructed("ocn")[k]] for k in ac.OCN_ONLY])
            assert w.min() < ac.UMIN and ((w > ac.UMIN) & (w < 5.0)).sum() >= 8 and (w > 7.0).sum() >= 8 and w.max() > 40.0


def test_conditioning(restated):
    for name in ac.CASES:
        a, mask, ref, (want, hol), (truth, hol_t) = restated[name]
        bad = ac.ill_conditioned(hol, mask)
        assert not bad.any(), (name, np.argwhere(bad).tolist())
        # the extended-precision restatement is on the same side of hol = 0 in every iteration, and clamped where this one is
        assert np.array_equal(np.signbit(hol_t)[:, mask], np.signbit(hol)[:, mask]), name
        assert np.array_equal((np.abs(hol_t) == 10)[:, mask], (np.abs(hol) == 10)[:, mask]), name


def test_fixture_is_what_the_reference_gives():
    from oracle import refapi
    if not refapi.available("gx3"):
        pytest.skip("oracle/_ref/libcice_ref_gx3.so not built")
    spec = importlib.util.spec_from_file_location("make_golden_atmo", os.path.join(ROOT, "tests", "golden", "make_golden_atmo.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    new = m.mint()
    old = np.load(ac.FIXTURE)
    assert set(new) == set(old.files)
    for k, v in new.items():
        assert old[k].dtype == np.asarray(v).dtype and old[k].shape == np.asarray(v).shape, k
        assert old[k].tobytes() == np.asarray(v).tobytes(), k


@pytest.mark.parametrize("name", tuple(ac.CASES))
def test_numpy_restatement_agrees(d, restated, name):
    a, mask, ref, (want, hol), (truth, _) = restated[name]
    differ = {k: int((want[k].view(np.uint64) != ref[k].view(np.uint64)).sum()) for k in ac.OUT}
    print(f"{name}: words that differ bitwise between the numpy restatement and the compiled reference, of {int(mask.sum())} "
          f"listed cells per field: {differ}")
    for k in ac.OUT:
        assert np.abs(ref[k]).max() > 0.0
        err = np.abs(want[k] - ref[k]).max() / np.abs(ref[k]).max()
        assert err <= 1.0e-12, (name, k, err)
        assert not want[k][~mask].view(np.uint64).any() and not ref[k][~mask].view(np.uint64).any(), (name, k)
    for k in ac.OUT_EXP:
        if TOL_EXP == 0.0:
            assert differ[k] == 0, (name, k, differ[k])
        else:
            assert np.abs(want[k] - ref[k]).max() <= TOL_EXP * np.abs(ref[k]).max(), (name, k)
    e_ref = {k: ac.cell_deviation(ref[k], truth[k], mask) for k in ac.OUT_LOG}
    e_np = {k: ac.cell_deviation(want[k], truth[k], mask) for k in ac.OUT_LOG}
    print(f"{name}: E_ref (largest per-cell relative deviation of the reference from the extended-precision restatement): "
          + ", ".join(f"{k} {v:.3e}" for k, v in e_ref.items()))
    print(f"{name}: the same of the numpy restatement: " + ", ".join(f"{k} {v:.3e}" for k, v in e_np.items()))
    for k in ac.OUT_LOG:
        assert e_np[k] <= 4.0 * e_ref[k] + 2.0 ** -52, (name, k, e_np[k], e_ref[k])
    assert ac.reference_error(d, name)[0] == e_ref


def test_calc_strair_false_and_interior_runs(d, restated):
    """the other two runs of the list case: the caller's stresses come back, everything else is the bits of the first run; the
    run on the full interior gives the first run's bits on the cells they share and agrees with the restatement"""
    name = ac.LIST_CASE
    a, mask, ref, (want, hol), _ = restated[name]
    sx, sy = d[f"{name}_F_strx_in"], d[f"{name}_F_stry_in"]
    f = ac.unpack(d, name + "_F", mask, sx, sy)
    assert np.array_equal(f["strx"], sx) and np.array_equal(f["stry"], sy)
    for k in ac.OUT[2:]:
        assert np.array_equal(f[k].view(np.uint64), ref[k].view(np.uint64)), k
    full = ac.unpack(d, name + "_interior", ac.interior())
    ours, _ = ac.atmo_numpy(ac.CASES[name]["sfctype"], *ac.make_list(ac.interior()), a)
    for k in ac.OUT:
        assert np.array_equal(full[k][mask].view(np.uint64), ref[k][mask].view(np.uint64)), k
        assert np.abs(ours[k] - full[k]).max() <= 1.0e-12 * np.abs(full[k]).max(), k
