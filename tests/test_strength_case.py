"""The catalogue of tests/strength_case.py on the CPU: the checker's ice_strength equals the compiled reference bit for bit
on every distribution and in every configuration, every guard of the routine is taken, and the checker's whole evp(dt)
stays finite on a state seeded with the catalogue.  (The same inputs on the device: test_gpu_strength.py.)"""
import numpy as np
import pytest

import strength_case as sc
from cice4_amd import lib

DT = 3600.0


@pytest.fixture(scope="module")
def row():
    return sc.as_row()


@pytest.mark.parametrize("cfg", sc.CONFIGS, ids=sc.cfg_id)
def test_checker_equals_reference_on_the_catalogue(ref_gx3, orc, row, cfg):
    ref_gx3.set_strength_parameters(*cfg); orc.set_strength_parameters(*cfg)
    try:
        want, got = ref_gx3.ice_strength(*row), orc.ice_strength(*row)
    finally:
        ref_gx3.set_strength_parameters(); orc.set_strength_parameters()
    ne = np.argwhere(sc.bits(want) != sc.bits(got))
    assert len(ne) == 0, [(sc.CATALOGUE[i - 1][0], want[j, i].hex(), got[j, i].hex()) for j, i in ne[:5]]
    assert np.isfinite(got).all()
    st = got[1, 1:-1]
    a, v, a0 = sc.catalogue_arrays()
    counts = sc.branch_counts(a, v, a0, cfg)
    for k in sc.reachable(cfg):
        for c in (counts[k] if isinstance(counts[k], list) else [counts[k]]):
            assert c >= 1, (k, counts[k])
    if cfg[0] == 1:
        ice = (a > 0.0).any(axis=1)
        assert int((ice & (st == 0.0)).sum()) == counts["ice_with_zero_strength"]     # ... and branch_counts knows the routine
        assert not (st[~ice] != 0.0).any()
        distinct = len(np.unique(st[st != 0.0]))
        assert distinct >= (60 if cfg[1] == 1 else 25), distinct      # (a later edit must not hollow the catalogue out)
    else:
        assert (st[(a > 0.0).any(axis=1)] > 0.0).all()


def test_catalogue_is_what_the_tests_rely_on():
    a, v, a0 = sc.catalogue_arrays()
    kinds = [c[0] for c in sc.CATALOGUE]
    assert ((a > sc.PUNY).any(axis=1) | (a0 > sc.PUNY)).all()
    for n in range(sc.NCAT):
        k = kinds.index(f"at_puny{n}")
        assert a[k, n] == sc.PUNY and not a[k, n] > sc.PUNY and v[k, n] > 0.0
        assert 0.0 < a[kinds.index(f"below_puny{n}"), n] < sc.PUNY < a[kinds.index(f"above_puny{n}"), n]
    k = kinds.index("raft")
    hi = v[k] / a[k]
    assert (2.0 * hi == hi + 1.0).sum() == 2 and (2.0 * hi < hi + 1.0).sum() == 1 and (2.0 * hi > hi + 1.0).sum() == 2
    k = kinds.index("film")
    assert v[k, 0] / a[k, 0] < sc.PUNY


@pytest.mark.parametrize("bs", [(24, 20), (12, 10), (64, 20)], ids=["one_block", "2x2_blocks", "wide_block"])
def test_seeded_state_places_the_catalogue(bs):
    nxg = 64 if bs[0] == 64 else sc.NXG
    dom, grid, s, which = sc.seeded_case(lib.Context(), bs[0], bs[1], nxg=nxg)
    assert np.bincount(which[which >= 0], minlength=len(sc.CATALOGUE)).min() >= 4
    ca, cv, c0 = sc.catalogue_arrays()
    for b in range(dom["nblocks"]):
        jj, ii = sc.global_coords(dom, b)
        w = np.where(jj[:, None] >= 0, which[np.ix_(np.maximum(jj, 0), ii)], -1)
        phys = w[dom["jlo"][b] - 1:dom["jhi"][b], dom["ilo"][b] - 1:dom["ihi"][b]]
        for edge in (phys[0], phys[-1], phys[:, 0], phys[:, -1]):
            assert (edge >= 0).any(), b
        m = w >= 0                    # ghost cells agree with their owners
        assert m[:, [0, -1]].any(), b
        for n in range(sc.NCAT):
            assert sc.same(s["aicen"][b, n][m], ca[w[m], n]) and sc.same(s["vicen"][b, n][m], cv[w[m], n])
        assert sc.same(s["aice0"][b][m], c0[w[m]])
    assert sc.same(s["aice"], sc.aggregate(s["aicen"], s["vicen"])[0])


@pytest.mark.parametrize("bs", [(24, 20), (12, 10)], ids=["one_block", "2x2_blocks"])
@pytest.mark.parametrize("cfg", sc.CONFIGS, ids=sc.cfg_id)
def test_checker_whole_evp_stays_finite_on_the_seeded_state(orc, cfg, bs):
    dom, grid, s, which = sc.seeded_case(lib.Context(), *bs)
    orc.set_evp_parameters(DT, 4, False); orc.set_strength_parameters(*cfg)
    try:
        orc.evp(orc.make_domain(dom, grid), s)
    finally:
        orc.set_strength_parameters()
    for k, x in s.items():
        assert np.isfinite(x).all(), k
    ocean = moving = 0
    for b in range(dom["nblocks"]):
        js, is_ = slice(dom["jlo"][b] - 1, dom["jhi"][b]), slice(dom["ilo"][b] - 1, dom["ihi"][b])
        ocean += int((grid["tmask"][b][js, is_] != 0).sum())
        moving += int((s["iceumask"][b][js, is_] != 0).sum())
    assert moving > ocean // 2, (moving, ocean)
    assert s["strength"].max() > 1.0e5 and np.abs(s["uvel"]).max() > 0.0
