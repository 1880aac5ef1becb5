"""tests/golden/coupling.npz is what it says: the inputs rebuilt from the seeds hash to what the minter hashed; the numpy
restatements of scale_fluxes and of the mixed layer's tail (ice_ocean.F90:190-231, :125-130) give the compiled reference's
bits in EVERY word; the branch counts, re-derived from the fixture, are the ones the minter stored and occur often enough on
physical and on ghost cells; the conditioning of the mixed layer's cells holds with no cell left out.  E_ref, the reference's
own largest per-cell deviation from the extended-precision restatement of the boundary layer on this fixture's ocean cells,
is computed from the committed data and printed (DESIGN.md 8.8 quotes it).  No GPU, no compiled reference."""
import numpy as np
import pytest

import atmo_case as ac
import coupling_case as cc


@pytest.fixture(scope="module")
def d():
    return np.load(cc.FIXTURE)


@pytest.fixture(scope="module")
def cases(d):
    return {name: cc.load_case(d, name) for name in cc.CASES}


def test_fixture_meta(d):
    meta = str(d["meta"][0])
    assert "flang" in meta and "-ffp-contract=off" in meta and "-fdefault-real-8" in meta and "-O2" in meta
    assert "scale_fluxes" in meta and "ocean_mixed_layer" in meta and "configuration small" in meta
    assert tuple(d["branches"]) == cc.BRANCHES


@pytest.mark.parametrize("name", tuple(cc.CASES))
def test_inputs_match_seeds(d, cases, name):
    assert int(d[f"{name}_seed"]) == cc.CASES[name]["seed"]
    s = cases[name][0]
    assert cc.digest(s) == str(d[f"{name}_sha256"])
    assert s["coszen"].shape == (cc.NB, cc.NY, cc.NX) and cc.NY * cc.NX == 168 and (cc.NY * cc.NX) % 64 != 0
    assert ("albpndn" in s) == cc.CASES[name]["albpndn"]


@pytest.mark.parametrize("name", [n for n, c in cc.CASES.items() if c["scale_fluxes"]])
def test_scale_fluxes_restatement_gives_the_reference_bits(cases, name):
    s, scaled, _ = cases[name]
    want = cc.scale_fluxes_numpy(s, cc.merge_numpy(s))
    for k in cc.SCALED:
        assert np.array_equal(cc.u64(want[k]), cc.u64(scaled[k])), (name, k)


def test_mixed_layer_tail_restatement_gives_the_reference_bits(cases):
    s, _, mixed = cases["standalone"]
    want, m, _ = cc.mixed_tail_numpy(s, mixed)
    for k in cc.MIX_TAIL:
        assert np.array_equal(cc.u64(want[k]), cc.u64(mixed[k])), k
    from_outputs = cc.masks_from_outputs(s, mixed)
    for k in cc.MIX_MASKS:
        assert np.array_equal(m[k], from_outputs[k]), k
    ocean = s["tmask"] != 0
    for k in cc.MIX_OUT[-4:]:
        assert (mixed[k] == cc.ALBOCN).all(), k
    for k in cc.MIX_OUT[5:9] + cc.MIX_OPT:           # atmo_boundary_layer zeroes its block first
        assert not cc.u64(mixed[k])[~ocean].any(), k
    assert np.array_equal(cc.u64(mixed["qdp"])[~ocean], cc.u64(s["qdp"])[~ocean])


def test_boundary_layer_restatement_agrees(cases):
    """delt and delq pass through exp alone: bit for bit where the host libm is the one the fixture was minted with; the six
    that pass through log and atan to 1e-12 of the field's magnitude"""
    from conftest import TOL_EXP
    s, _, mixed = cases["standalone"]
    ours, _ = cc.atmo_all(s, ac.atmo_numpy)
    for k in ("delt", "delq"):
        if TOL_EXP == 0.0:
            assert np.array_equal(cc.u64(ours[k]), cc.u64(mixed[k])), k
        else:
            assert np.abs(ours[k] - mixed[k]).max() <= TOL_EXP * np.abs(mixed[k]).max(), k
    for k in cc.MIX_LOG:
        assert np.abs(ours[k] - mixed[k]).max() <= 1e-12 * np.abs(mixed[k]).max(), k


def test_branch_counts(d, cases):
    total = {k: (0, 0) for k in cc.BRANCHES}
    for name, (s, scaled, mixed) in cases.items():
        counts = cc.branch_counts(name, s, scaled, mixed)
        assert [list(counts[k]) for k in cc.BRANCHES] == d[f"{name}_counts"].tolist(), name
        total = {k: (total[k][0] + v[0], total[k][1] + v[1]) for k, v in counts.items()}
    print("cells per branch (physical, ghost):", total)
    assert not cc.short_of(total)
    assert all(v[0] + v[1] >= cc.NEED and v[0] >= 1 and v[1] >= 1 for v in total.values())


def test_conditioning(cases):
    s, _, mixed = cases["standalone"]
    _, m, cond = cc.mixed_tail_numpy(s, mixed)
    _, hol = cc.atmo_all(s, ac.atmo_numpy)
    _, hol_t = cc.atmo_all(s, ac.atmo_truth)
    bad = cc.ill_conditioned(s, cond, m, hol)
    assert not any(v.any() for v in bad.values()), {k: int(v.sum()) for k, v in bad.items()}
    ocean = (s["tmask"] != 0)[:, None]
    assert np.array_equal(np.signbit(hol)[ocean & (hol != 0)], np.signbit(np.asarray(hol_t, np.float64))[ocean & (hol != 0)])
    margin = np.abs(cond["sst2"] - s["Tf"])[s["tmask"] != 0].min()
    print(f"smallest |sst - Tf| at :229 over the ocean cells: {margin:.3e} K; cells left out of any comparison: 0")


def test_reference_error_is_measured(cases):
    s, _, mixed = cases["standalone"]
    e_ref, _ = cc.reference_error(s, mixed)
    print("E_ref: " + ", ".join(f"{k} {v:.3e}" for k, v in e_ref.items()))
    for k, v in e_ref.items():
        assert 0.0 <= v < 1.0e-12, (k, v)          # a deviation of rounding errors, not of a different routine
