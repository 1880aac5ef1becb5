"""tests/golden/dedd.npz (minted from the compiled reference by tests/golden/make_golden_dedd.py): it loads, says how it was
made, belongs to the inputs tests/dedd_case.py builds today, holds every branch of the delta-Eddington scheme the case
module asks for in the number of (cell, category) pairs it asks for -- every interval of the snow grain radius table
included -- and agrees with dedd_case.dedd_numpy, the scheme restated operation by operation in float64 with the host
libm's exp, to 1e-12 of each field's magnitude (the bound of test_shortwave_golden.py).  Every step of the restatement is one
correctly rounded operation, so it is expected to give the reference's bits: the test counts the words that differ bitwise
and reports the count (0 on the host that minted the fixture: DESIGN.md 8.7) -- the advance evidence that the device, whose
exp restates the same libm, can be bit-exact.  And the C header, lib.py and the library agree on the entries."""
import os
import re

import numpy as np
import pytest

import dedd_case as dc
from cice4_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"cice_shortwave_dedd_init": 2, "cice_shortwave_dEdd": 31, "cice_step_radiation_dedd": 2, "cice_dedd_times": 3}


@pytest.fixture(scope="module")
def d():
    return np.load(dc.FIXTURE)


@pytest.fixture(scope="module")
def restated(d):
    """per case: inputs, the reference's outputs, the restatement's outputs and masks -- computed once"""
    r = {}
    for name in dc.CASES:
        s, out = dc.load_case(d, name)
        r[name] = (s, out, dc.dedd_numpy(name, s))
    return r


def test_fixture_meta(d):
    meta = str(d["meta"][0])
    assert "flang" in meta and "-ffp-contract=off" in meta and "-fdefault-real-8" in meta and "-O2" in meta
    assert "make_golden_dedd.py" in meta and "ice_shortwave" in meta and "shortwave_dEdd_set_snow" in meta
    assert os.path.getsize(dc.FIXTURE) < (1 << 20)
    assert tuple(str(x) for x in d["branches"]) == dc.BRANCHES


def test_the_five_cases():
    c = dc.CASES
    assert tuple(c) == ("default", "tuned_pos", "tuned_neg", "tr_pond", "tables")
    assert all(c["default"][k] == 0.0 for k in ("R_ice", "R_pnd", "R_snw"))
    assert all(c["tuned_pos"][k] > 0.0 and c["tuned_neg"][k] < 0.0 for k in ("R_ice", "R_pnd", "R_snw"))
    assert c["tr_pond"]["tr_pond"] and c["tables"]["blockwise"] and dc.DRIVER_CASES == ("default", "tuned_pos", "tuned_neg", "tr_pond")
    assert (dc.NX, dc.NY, dc.NB, dc.NCAT) == (14, 12, 4, 5)
    # R_ice of tuned_neg is negative enough that max(sigp, 0) is not a no-op: the reference's constants allow it
    _, clamped = dc.tuned(c["tuned_neg"]["R_ice"], c["tuned_neg"]["R_pnd"])
    assert clamped and not dc.tuned(c["tuned_pos"]["R_ice"], c["tuned_pos"]["R_pnd"])[1]


def test_tables_header_has_the_shape_the_scheme_needs():
    t = dc.TAB
    assert t["rsnw_tab"].shape == (32,) and (np.diff(t["rsnw_tab"]) > 0).all() and t["rsnw_tab"][0] == 5.0 and t["rsnw_tab"][-1] == 2500.0
    for k in ("Qs_tab", "ws_tab", "gs_tab"):
        assert t[k].shape == (32, 3)
    assert (t["ws_tab"] <= 1.0).all() and (t["ws_tab"] > 0.7).all() and (t["Qs_tab"] > 2.0).all() and (t["gs_tab"] < 1.0).all()
    assert (np.diff(t["ws_tab"], axis=0) < 0).all() and (np.diff(t["Qs_tab"], axis=0) < 0).all()      # a mistyped digit breaks these
    for k in ("ki_ssl_mn", "wi_ssl_mn", "gi_ssl_mn", "ki_dl_mn", "wi_dl_mn", "gi_dl_mn", "ki_int_mn", "wi_int_mn", "gi_int_mn",
              "ki_p_ssl_mn", "wi_p_ssl_mn", "gi_p_ssl_mn", "ki_p_int_mn", "wi_p_int_mn", "gi_p_int_mn", "kw", "ww", "gw"):
        assert t[k].shape == (3,), k


@pytest.mark.parametrize("name", tuple(dc.CASES))
def test_inputs_match_seeds(d, name):
    assert int(d[f"{name}_seed"]) == dc.CASES[name]["seed"]
    s, out = dc.load_case(d, name)
    assert dc.digest(s) == str(d[f"{name}_sha256"])
    assert all(np.isfinite(out[k]).all() for k in dc.OUT)
    on = dc.listed(s)
    assert not on[dc.NB - 1].any() and all(on[b].any() for b in range(dc.NB - 1))   # one whole block has no ice at all


def test_branch_counts(d, restated):
    total = {k: 0 for k in dc.BRANCHES}
    intervals = np.zeros(31, np.int64)
    for name in dc.CASES:
        s, out, ours = restated[name]
        counts, iv = dc.branch_counts(name, s, out, ours)
        assert [counts[k] for k in dc.BRANCHES] == [int(x) for x in d[f"{name}_counts"]], name
        assert np.array_equal(iv, d[f"{name}_intervals"]), name
        for k, v in counts.items():
            total[k] += v
        if dc.CASES[name]["blockwise"]:
            intervals += iv
    short = {k: v for k, v in total.items() if v < dc.NEED[k]}
    assert not short, short
    assert all(dc.NEED[k] >= 8 for k in dc.BRANCHES if k != "empty_block")
    assert (intervals >= 1).all(), intervals.tolist()        # every interval of the radius table, in the block-wise case
    print("branch counts over the cases:", total, "pairs per interval of the radius table:", intervals.tolist())


@pytest.mark.parametrize("name", tuple(dc.CASES))
def test_numpy_restatement_agrees(restated, name):
    s, out, (want, m) = restated[name]
    differ, words = 0, 0
    for k in dc.OUT:
        mag = np.abs(out[k]).max()
        assert mag > 0.0 or (k == "albpndn" and not m["pond_pass"].any()), k
        differ += int((want[k].view(np.uint64) != out[k].view(np.uint64)).sum())
        words += out[k].size
    print(f"{name}: {differ} of {words} words differ bitwise between the numpy restatement and the compiled reference")
    for k in dc.OUT:
        err = np.abs(want[k] - out[k]).max() / max(np.abs(out[k]).max(), 1e-300)
        assert err <= 1.0e-12, (name, k, err)
    # off the lists and without sun: bit for bit the zeros of the whole-block initialisation (no arithmetic)
    off = ~m["active"]
    for k in dc.OUT:
        x = out[k][np.broadcast_to(off[:, :, None], out[k].shape)] if k in dc.LAYERS else out[k][off]
        assert not x.view(np.uint64).any(), (name, k)
    assert m["active"].sum() >= 100


def test_header_lib_and_library_agree():
    head = open(os.path.join(ROOT, "include", "cice4_amd.h")).read()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", head)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
    for struct, cls in (("cice_dedd_config", lib.DeddConfig), ("cice_radiation_dedd_fields", lib.RadiationDeddFields)):
        body = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", head).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        members = re.findall(r"\*?(\w+)\s*[,;]", body)
        assert members == [n for n, _t in cls._fields_], struct
