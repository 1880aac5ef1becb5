"""tests/golden/ridge.npz (minted from the compiled reference by tests/golden/make_golden_ridge.py): it loads, says how it was
made, belongs to the inputs tests/ridge_case.py builds today, and holds every branch of ridge_ice the case module asks for
in the number of cells it asks for.  And the C header, lib.py and the library agree on the ridging entries."""
import os
import re

import numpy as np
import pytest

import cleanup_itd_case as cc
import ridge_case as rc
from cice4_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"cice_ridge_init": 4, "cice_ridge_ice": 28, "cice_step_ridge": 8, "cice_ridge_times": 3}


@pytest.fixture(scope="module")
def d():
    return np.load(rc.FIXTURE)


def test_fixture_meta(d):
    meta = str(d["meta"][0])
    assert "flang" in meta and "-ffp-contract=off" in meta and "-fdefault-real-8" in meta and "-O2" in meta
    assert "make_golden_ridge.py" in meta and "ice_mechred" in meta
    assert os.path.getsize(rc.FIXTURE) < (1 << 20)


@pytest.mark.parametrize("name", rc.ORDINARY)
def test_inputs_match_seeds(d, name):
    assert int(d[f"{name}_seed"]) == rc.CASES[name]["seed"]
    s = rc.case_inputs(name)
    assert rc.digest(s) == str(d[f"{name}_sha256"])
    # what the reference divides by is positive on every listed cell, and everything it left is finite
    lm = rc.listed_mask(s["tmask"])
    assert (((s["aice0"] > rc.PUNY) | (s["aicen"] > rc.PUNY).any(axis=1)) | ~lm).all()
    _, out, _ = rc.load_case(d, name)
    assert all(np.isfinite(out[k]).all() for k in rc.OUT)


def test_the_four_configurations():
    c = rc.CASES
    assert c["ntr1"]["ntrcr"] == 1 and rc.itd_kwargs("ntr4")["tr_lvl"] and 2 in c["snow"]["dep"]
    assert rc.ridge_kwargs("partic0")["krdg_partic"] == 0 and all(rc.ridge_kwargs(n)["krdg_redist"] == 1 for n in c)
    assert (rc.NX, rc.NY, rc.NB) == (14, 12, 4)


def test_stop_case(d):
    blk, cells = rc.stop_inputs()
    assert rc.digest(blk) == str(d[f"{rc.STOP}_sha256"])
    assert tuple(int(x) for x in d[f"{rc.STOP}_stop"]) == (1,) + cells[0]
    assert [tuple(int(v) for v in c) for c in d[f"{rc.STOP}_cells"]] == cells and int(d[f"{rc.STOP}_niter"]) == 1
    (i1, j1), (i2, j2) = cells
    assert (blk["rdg_conv"][j1 - 1, i1 - 1] < 0) and (blk["rdg_conv"][j2 - 1, i2 - 1] < 0)
    a0 = d[f"{rc.STOP}_out_aice0"]
    assert a0[j1 - 1, i1 - 1] < -rc.PUNY                      # the first failing cell holds its negative value
    assert a0[j2 - 1, i2 - 1] == blk["aice0"][j2 - 1, i2 - 1]  # the second is untouched
    icells, ii, jj = rc.tmask_list(blk["tmask"])
    pos = {(int(ii[k]), int(jj[k])): k for k in range(icells)}
    changed = cc.bits(a0) != cc.bits(blk["aice0"])
    for j, i in zip(*np.nonzero(changed)):                     # only cells up to the failing one hold a new aice0
        assert pos[(i + 1, j + 1)] <= pos[cells[0]]
    assert changed.sum() > 1
    for k in rc.STATE + rc.OPTIONAL:                           # nothing else of the iteration happened
        assert np.array_equal(cc.bits(d[f"{rc.STOP}_out_{k}"]), cc.bits(blk[k])), k


def test_every_branch_is_in_the_fixture(d):
    total = {k: 0 for k in rc.BRANCHES}
    for name in rc.ORDINARY:
        s, out, niter = rc.load_case(d, name)
        counts = rc.branch_counts(name, s, out, niter)
        assert [counts[k] for k in rc.BRANCHES] == [int(x) for x in d[f"{name}_counts"]], name
        for b in range(rc.NB):
            assert (niter[b] == 0) == (rc.tmask_list(s["tmask"][b])[0] == 0)
        for k, v in counts.items():
            total[k] += v
    short = {k: v for k, v in total.items() if v < rc.NEED[k]}
    assert not short, short
    need = rc.NEED
    assert all(need[k] >= 8 for k in rc.BRANCHES if k not in ("iter1_block", "iter2_block", "iter3_block", "untouched_block",
                                                              "exp_denormal", "exp_zero", "aice0_clamped"))
    assert min(need[k] for k in ("iter1_block", "iter2_block", "iter3_block", "untouched_block", "exp_denormal",
                                 "exp_zero")) >= 1


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "cice4_amd.h")).read()
    src = open(os.path.join(ROOT, "cice4_amd", "lib.py")).read()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, len(m.group(1).split(",")))
        assert "self.lib." + name + "(" in src, name
    L = lib.load()
    for name in ENTRIES:
        assert hasattr(L, name), name
    m = re.search(r"typedef struct \{([^}]*)\} cice_ridge_fields;", text)
    members = re.findall(r"\*?(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert members == ["ncat", "bound"] + list(lib.RIDGE_PTRS)
    assert len(lib.RIDGE_TIMES) == 41
    assert "krdg_redist = 0 is CICE_EUNSUPPORTED" in text
