"""tests/golden/cleanup_itd.npz (minted from the compiled reference by tests/golden/make_golden_cleanup_itd.py): it loads,
says how it was made, belongs to the inputs tests/cleanup_itd_case.py builds today, and holds every branch of cleanup_itd
(rebin with its block-wide flag, zap_small_areas) in the number of cells the case module asks for.  And the C header,
lib.py and the library agree on the entries of the second half of step_therm2."""
import os
import re

import numpy as np
import pytest

import cleanup_itd_case as cc
from cice4_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"cice_cleanup_itd": 26, "cice_aggregate": 19, "cice_step_therm2_cleanup": 8, "cice_therm2_cleanup_times": 3}


@pytest.fixture(scope="module")
def d():
    return np.load(cc.FIXTURE)


def test_fixture_meta(d):
    meta = str(d["meta"][0])
    assert "flang" in meta and "-ffp-contract=off" in meta and "-fdefault-real-8" in meta and "-O2" in meta
    assert "make_golden_cleanup_itd.py" in meta
    assert os.path.getsize(cc.FIXTURE) < (1 << 20)


@pytest.mark.parametrize("name", cc.ORDINARY)
def test_inputs_match_seeds(d, name):
    assert int(d[f"{name}_seed"]) == cc.CASES[name]["seed"]
    assert cc.digest(cc.case_inputs(name)) == str(d[f"{name}_sha256"])


@pytest.mark.parametrize("which", cc.STOPS)
def test_stop_inputs_match(d, which):
    blk, cell = cc.stop_inputs(which)
    assert cc.digest(blk) == str(d[f"{which}_sha256"])
    assert tuple(int(x) for x in d[f"{which}_stop"]) == (1,) + cell
    if which == "stop_area":                                   # the state untouched, the fluxes too
        for k in cc.STATE + cc.FLUX:
            assert np.array_equal(cc.bits(d[f"{which}_out_{k}"]), cc.bits(blk[k])), k
    else:                                                      # categories 1-2 zapped where tiny, 3-5 and the fluxes untouched
        a0, a1 = blk["aicen"], d[f"{which}_out_aicen"]
        tiny = (a0 != 0) & (np.abs(a0) <= cc.PUNY)
        assert tiny[:2].sum() >= 2 and (a1[:2][tiny[:2]] == 0).all() and np.array_equal(cc.bits(a1[2:]), cc.bits(a0[2:]))
        for k in cc.FLUX:
            assert np.array_equal(cc.bits(d[f"{which}_out_{k}"]), cc.bits(blk[k])), k


def test_every_branch_is_in_the_fixture(d):
    total = {k: 0 for k in cc.BRANCHES}
    for name in cc.ORDINARY:
        s, out, _ = cc.load_case(d, name)
        counts, quiet = cc.branch_counts(name, s, out)
        assert [counts[k] for k in cc.BRANCHES] == [int(x) for x in d[f"{name}_counts"]], name
        assert quiet == [int(b) for b in d[f"{name}_quiet"]] and 2 in quiet, (name, quiet)
        ntr = cc.ntrcr(name)
        for b in quiet:                                        # every tracer bit of a quiet block stays
            assert np.array_equal(cc.bits(out["trcrn"][b][:, :ntr]), cc.bits(s["trcrn"][b][:, :ntr])), (name, b)
        if cc.CASES[name]["hin0"] == 0.0:                      # the lift of category 1 is dead with hin_max(0) = 0
            assert counts["floor_cat1"] == 0
        for k, v in counts.items():
            total[k] += v
    short = {k: v for k, v in total.items() if v < cc.NEED[k]}
    assert not short, short


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
    m = re.search(r"typedef struct \{([^}]*)\} cice_therm2_cleanup_fields;", text)
    members = re.findall(r"\*?(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert members == ["ncat", "state_resident", "bound"] + list(lib.CLEANUP_PTRS)
    assert "cleanup_itd, bound_state, aggregate, ridging and shortwave stay with the caller" not in text
