"""tests/golden/pond.npz is what it says: the inputs rebuilt from the seeds hash to what the minter hashed; the numpy
restatements of compute_ponds and increment_age give the compiled reference's bits in every word; the branch counts,
re-derived from the fixture, are the ones the minter stored and meet pond_case.NEED; the four comparisons are conditioned.
And the cell routine itself, cice4_amd/csrc/pond_cell.h, compiled for the host under the address and undefined-behaviour
sanitizers into the stand-alone tests/pond_probe.cpp, gives the fixture's words on every listed pair of every case.  No GPU,
no compiled reference."""
import os
import subprocess

import numpy as np
import pytest

import pond_case as pc
import therm_itd_case as tc
from conftest import TOL_EXP
from test_libm_exact import _host_has_fma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def d():
    return np.load(pc.FIXTURE)


@pytest.fixture(scope="module")
def cases(d):
    return {name: pc.load_case(d, name) for name in pc.CASES}


def test_fixture_meta(d):
    meta = str(d["meta"][0])
    assert "flang" in meta and "-ffp-contract=off" in meta and "-fdefault-real-8" in meta and "-O2" in meta
    assert "compute_ponds" in meta and "increment_age" in meta and "configuration small" in meta
    assert tuple(d["branches"]) == pc.BRANCHES
    assert os.path.getsize(pc.FIXTURE) <= os.path.getsize(os.path.join(os.path.dirname(pc.FIXTURE), "coupling.npz"))


@pytest.mark.parametrize("name", tuple(pc.CASES))
def test_inputs_match_seeds(d, cases, name):
    assert int(d[f"{name}_seed"]) == pc.CASES[name]["seed"]
    s = cases[name][0]
    assert pc.digest(s) == str(d[f"{name}_sha256"])
    assert s["aicen"].shape == (pc.NB, pc.NCAT, pc.NY, pc.NX) == (4, 5, 12, 14) and (pc.NY * pc.NX) % 64 != 0
    assert s["trcrn"].shape == (pc.NB, pc.NCAT, pc.NTRCR, pc.NY, pc.NX)
    assert set(k[len(name) + 1:] for k in d.files if k.startswith(name + "_")) == set(pc.outputs_of(name)) | {
        "seed", "sha256", "counts"}


@pytest.mark.parametrize("name", tuple(pc.CASES))
def test_restatement_gives_the_reference_bits(cases, name):
    s, want = cases[name]
    ours, m = pc.restate(name, s)
    assert set(ours) == set(want) == set(pc.outputs_of(name))
    on = pc.listed(s)
    assert on.sum() >= 1000
    for k in want:
        through_exp = k != "iage" and TOL_EXP != 0.0
        sel = ~m["run"] if through_exp else np.ones(on.shape, bool)
        assert tc.same(ours[k][sel], want[k][sel]), (name, k, int((ours[k] != want[k]).sum()))
        if through_exp:
            assert np.abs(ours[k] - want[k]).max() <= TOL_EXP * np.abs(want[k]).max(), (name, k)


def test_stale_words_off_the_list_are_there_to_be_kept(cases):
    for name, (s, want) in cases.items():
        on = pc.listed(s)
        phys = pc.sc.physical(pc.block_table(), pc.NY, pc.NX)[:, None] & np.ones(on.shape, bool)
        assert (~phys).sum() > 0 and (phys & ~on).sum() >= 100
        assert (s["apondn"][~on] != 0).all() and (s["hpondn"][~on] != 0).all()
        for k, v in want.items():
            src = s[k] if k in s else s["trcrn"][:, :, pc.CASES[name]["nt_" + k] - 1]
            assert tc.same(v[~on], src[~on]), (name, k)
        if pc.CASES[name]["ponds"]:
            vol = s["trcrn"][:, :, pc.CASES[name]["nt_volpn"] - 1]
            assert (vol[~on] != 0).sum() >= 100 and (vol == -1.0e-12).sum() >= 8


def test_branch_counts(d, cases):
    total = {k: 0 for k in pc.BRANCHES}
    for name, (s, want) in cases.items():
        counts = pc.branch_counts(name, s, want)
        if TOL_EXP == 0.0:
            assert [counts[k] for k in pc.BRANCHES] == d[f"{name}_counts"].tolist(), name
        for k in pc.BRANCHES:
            total[k] += int(d[f"{name}_counts"][pc.BRANCHES.index(k)])
    print("(cell, category) pairs per branch:", total)
    assert all(total[k] >= pc.NEED[k] >= 8 for k in pc.BRANCHES), total


def test_conditioning(cases):
    low = {}
    for name, (s, _) in cases.items():
        if not pc.CASES[name]["ponds"]:
            continue
        _, m = pc.pond_numpy(name, s)
        for k, v in m["cond"].items():
            assert len(v) >= 100, (name, k)
            low[k] = min(low.get(k, np.inf), float(v.min()))
        # the columns left out of the hs margin are exactly snow-free: no rounding can move them across hs > puny
        assert (s["vsnon"][m["run"] & (s["vsnon"] == 0)] == 0).all()
    print("smallest margins at the four comparisons:", low)
    assert set(low) == {"hi", "hs", "frac", "depth"} and all(v >= pc.MARGIN == 1e-9 for v in low.values()), low


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not _host_has_fma():
        pytest.skip("host CPU without FMA: glibc selects its non-FMA exp build here")
    exe = str(tmp_path_factory.mktemp("pond_probe") / "pond_probe")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "pond_probe.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", tuple(pc.CASES))
def test_cell_routine_on_the_host_gives_the_fixture_words(probe, cases, name, tmp_path):
    c = pc.CASES[name]
    s, want = cases[name]
    on = pc.listed(s)
    n = int(on.sum())
    zeros = np.zeros(n)
    plane = lambda nt: s["trcrn"][:, :, nt - 1][on] if nt else zeros  # noqa: E731
    frain = (s["frain"][:, None] + np.zeros(on.shape))[on]
    rec = np.stack([s["aicen"][on], s["vicen"][on], s["vsnon"][on], plane(c["nt_Tsfc"]), s["melttn"][on], s["meltsn"][on], frain,
                    plane(c["nt_volpn"]), plane(c["nt_iage"] if c["tr_iage"] else 0)], axis=1)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([[float(n), float(c["ponds"]), float(c["age"]), pc.DT], rec.ravel()]).astype(np.float64).tofile(fin)
    r = subprocess.run([probe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and f"cells={n}" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])
    got = np.fromfile(fout, np.float64).reshape(n, 5)
    st = got[:, 4].astype(int)
    bit = dict(apondn=1, hpondn=1, volpn=2, iage=4)
    col = dict(apondn=0, hpondn=1, volpn=2, iage=3)
    src = dict(apondn=s["apondn"][on], hpondn=s["hpondn"][on], volpn=plane(c["nt_volpn"]), iage=rec[:, 8])
    assert (st == st & (3 * c["ponds"] + 4 * c["age"])).all()
    if c["ponds"]:
        hi = s["vicen"][on] / s["aicen"][on]
        assert ((st & 1) == 1).all() and np.array_equal((st & 2) != 0, ~(hi < pc.HICEMIN)) and ((st & 2) == 0).sum() >= 8
    for k in pc.outputs_of(name):
        stored = (st & bit[k]) != 0
        res = np.where(stored, got[:, col[k]], src[k])
        assert tc.same(res, want[k][on]), (name, k, int((res != want[k][on]).sum()))
    for k in set(pc.OUT) - set(pc.outputs_of(name)):
        assert not (st & bit[k]).any(), (name, k, "a word the flags do not ask for")
