"""tests/golden/shortwave.npz (minted from the compiled reference by tests/golden/make_golden_shortwave.py): it loads, says how
it was made, belongs to the inputs tests/shortwave_case.py builds today, holds every branch of shortwave_ccsm3 the case
module asks for in the number of (cell, category) pairs it asks for, and agrees with a plain numpy restatement of the scheme
(numpy's arctan and exp) to 1e-12 of each field's magnitude -- which a fixture minted with the wrong namelist, list or
argument order would not.  And the C header, lib.py and the library agree on the shortwave entries."""
import os
import re

import numpy as np
import pytest

import shortwave_case as sc
from cice4_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"cice_shortwave_init": 2, "cice_shortwave_ccsm3": 25, "cice_step_radiation": 2, "cice_prep_radiation": 2,
           "cice_radiation_chain": 2, "cice_radiation_times": 3}


@pytest.fixture(scope="module")
def d():
    return np.load(sc.FIXTURE)


def test_fixture_meta(d):
    meta = str(d["meta"][0])
    assert "flang" in meta and "-ffp-contract=off" in meta and "-fdefault-real-8" in meta and "-O2" in meta
    assert "make_golden_shortwave.py" in meta and "ice_shortwave" in meta and "AusCOM" in meta
    assert os.path.getsize(sc.FIXTURE) < (1 << 20)


def test_the_three_cases():
    c = sc.CASES
    assert tuple(c) == ("default", "constant", "auscom")
    assert c["constant"]["albedo_type"] == "constant" and c["auscom"]["flavour"] == "auscom"
    assert (c["auscom"]["dT_mlt"], c["auscom"]["dalb_mlt"], c["auscom"]["snowpatch"]) == (1.5, -0.05, 0.01)
    assert (sc.NX, sc.NY, sc.NB, sc.NCAT) == (14, 12, 4, 5)
    ocn = sc.case_inputs("auscom")["ocn_albedo"]
    assert ocn.std() > 1.0e-3 and "ocn_albedo" not in sc.case_inputs("default")


@pytest.mark.parametrize("name", tuple(sc.CASES))
def test_inputs_match_seeds(d, name):
    assert int(d[f"{name}_seed"]) == sc.CASES[name]["seed"]
    s, out = sc.load_case(d, name)
    assert sc.digest(s) == str(d[f"{name}_sha256"])
    assert all(np.isfinite(out[k]).all() for k in sc.OUT)
    on = sc.listed(s, sc.block_table())
    assert not on[sc.NB - 1].any() and all(on[b].any() for b in range(sc.NB - 1))   # one whole block has no ice at all


def test_branch_counts(d):
    total = {k: 0 for k in sc.BRANCHES}
    for name in sc.CASES:
        s, out = sc.load_case(d, name)
        counts = sc.branch_counts(name, s, out)
        assert [counts[k] for k in sc.BRANCHES] == [int(x) for x in d[f"{name}_counts"]], name
        for k, v in counts.items():
            total[k] += v
    short = {k: v for k, v in total.items() if v < sc.NEED[k]}
    assert not short, short
    assert all(sc.NEED[k] >= 8 for k in sc.BRANCHES if k != "empty_block")


@pytest.mark.parametrize("name", tuple(sc.CASES))
def test_numpy_restatement_agrees(d, name):
    s, out = sc.load_case(d, name)
    want, m = sc.ccsm3_numpy(name, s)
    for k in sc.OUT:
        mag = np.abs(out[k]).max()
        assert mag > 0.0, k
        err = np.abs(want[k] - out[k]).max() / mag
        assert err <= 1.0e-12, (name, k, err)
    # off the list: bit for bit what the whole-block initialisation leaves (no arithmetic)
    off = ~m["on"]
    for k in sc.OUT2:
        assert np.array_equal(out[k][off], want[k][off]), (name, k)
    assert np.array_equal(out["alvdrn"], out["alvdfn"]) and np.array_equal(out["alidrn"], out["alidfn"])


def test_prep_radiation_inputs_cover_both_sides():
    p = sc.prep_inputs()
    want, m = sc.prep_radiation_numpy(p)
    phys = sc.physical(sc.block_table(), sc.NY, sc.NX)
    assert (phys & (p["aice"] > 0.0)).sum() >= 8 and (phys & ~(p["aice"] > 0.0)).sum() >= 8
    assert (phys & (p["aice"] > 0.0) & (p["scale_factor"] > sc.PUNY)).sum() >= 8
    assert (phys & (p["aice"] > 0.0) & ~(p["scale_factor"] > sc.PUNY)).sum() >= 8
    assert m["on"].sum() >= 8 and (phys[:, None] & ~m["on"]).sum() >= 8
    assert m["scaled"].sum() >= 8 and m["unit"].sum() >= 8
    assert (want["scale_factor"][m["unit"]] == 1.0).all()
    assert np.array_equal(want["fswsfcn"][~m["on"]], p["fswsfcn"][~m["on"]])
    assert not np.array_equal(want["Iswabsn"], p["Iswabsn"])


def test_header_lib_and_library_agree():
    head = open(os.path.join(ROOT, "include", "cice4_amd.h")).read()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", head)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
    for struct, cls in (("cice_shortwave_config", lib.ShortwaveConfig), ("cice_radiation_fields", lib.RadiationFields),
                        ("cice_prep_radiation_fields", lib.PrepRadiationFields)):
        body = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", head).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        members = re.findall(r"\*?(\w+)\s*[,;]", body)
        assert members == [n for n, _t in cls._fields_], struct
    for flavour in ("standalone", "auscom"):
        path = lib.LIBPATH if flavour == "standalone" else lib.LIBPATH.replace(".so", "_auscom.so")
        if os.path.exists(path):
            L = lib.load(flavour)
            assert all(hasattr(L, name) for name in ENTRIES), flavour
