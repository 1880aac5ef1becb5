"""tests/golden/therm_itd.npz (minted from the compiled reference by tests/golden/make_golden_therm_itd.py): it loads,
says how it was made, belongs to the inputs synth.therm2_state produces today, and holds every branch of linear_itd /
add_new_ice / lateral_melt in at least 8 cells.  And the C header, lib.py and the library agree on the six entries."""
import os
import re

import numpy as np
import pytest

import therm_itd_case as tc
from cice4_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"cice_itd_init": 2, "cice_linear_itd": 22, "cice_add_new_ice": 25, "cice_lateral_melt": 18,
           "cice_shift_ice": 21, "cice_step_therm2_itd": 9}


@pytest.fixture(scope="module")
def d():
    return np.load(tc.FIXTURE)


def test_fixture_meta(d):
    meta = str(d["meta"][0])
    assert "flang" in meta and "-ffp-contract=off" in meta and "-fdefault-real-8" in meta and "-O2" in meta
    assert os.path.getsize(tc.FIXTURE) < (1 << 20)


@pytest.mark.parametrize("name", tc.ORDINARY)
def test_inputs_match_seeds(d, name):
    raw, _ = tc.case_inputs(name)
    assert int(d[f"{name}_seed"]) == tc.CASES[name]["seed"]
    assert tc.digest(raw) == str(d[f"{name}_sha256"])


def test_stop_inputs_match(d):
    assert tc.digest(tc.stop_add_inputs()[0]) == str(d["stop_add_sha256"])
    assert tc.digest(tc.stop_shift_inputs()[0]) == str(d["stop_shift_sha256"])
    assert tuple(d["stop_add_stop"])[0] == 1 and tuple(d["stop_shift_stop"])[0] == 1


def test_every_branch_is_in_the_fixture(d):
    total = {k: 0 for k in tc.BRANCHES}
    for name in tc.ORDINARY:
        _, chain = tc.load_chain(d, name)
        for k, v in tc.branch_counts(chain, tc.CASES[name]["ntrcr"]).items():
            total[k] += v
    assert all(v >= 8 for v in total.values()), total
    assert max(int(d[f"{name}_not_remapped"]) for name in tc.ORDINARY) > 0


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
