"""cice_coupling_prep on the device against tests/golden/coupling.npz (minted from the compiled reference; cases and
restatements: tests/coupling_case.py).

k_coupling_prep: every output bit for bit on all four blocks, ghost and land cells included, for the three cases, the albcnt
increment with nstreams 1 and 2; intent(in) arrays come back unchanged; the same on the nine padded blocks of configuration
`pad` against the restatement.  k_ocean_mixed_layer: delt and delq bit for bit; the six outputs that pass through log and atan
per cell within 4 E_ref + 2**-52 of the extended-precision restatement, E_ref being the reference's own largest per-cell
deviation from it on this fixture, zeros of the truth zeros of the same sign; the tail (ice_ocean.F90:
190-231) evaluated in numpy on the DEVICE's own delt, delq, shcoef, lhcoef equals the device's sst, qdp, frzmlt and the four
ocean fluxes bit for bit; the branch masks equal the fixture's in every cell; land cells hold the zeros.  Residence (albedos
behind either radiation entry, aicen behind cice_step_ridge, host arrays full of NaN), the ghost-cell update of scale_factor,
the order of the two kernels, the refusals."""
import functools

import numpy as np
import pytest

import atmo_case as ac
import coupling_case as cc
import dedd_case as dc
import shortwave_case as sc
from cice4_amd import lib

pytestmark = pytest.mark.gpu

DT = cc.DT
IN_KEYS = ("tmask", "aicen") + cc.CAT_ALB + cc.IN2 + cc.MIX_IN


@functools.lru_cache(maxsize=None)
def _gold(name):
    return cc.load_case(np.load(cc.FIXTURE), name)


def _context(name, batch=(cc.NX, cc.NY, cc.NB), flavour="standalone", domain=None):
    c = lib.Context(flavour=flavour)
    c.sync()
    if domain:
        c.domain_create(*domain, ew=1, ns=0)
        batch = (c.nx, c.ny, c.nblocks)
    c.thermo_init()
    cfg = cc.CASES[name]
    c.coupling_init(scale_fluxes=cfg["scale_fluxes"], oceanmixed_ice=cfg["oceanmixed_ice"], albocn=cc.ALBOCN)
    if batch:
        c.thermo_batch_alloc(*batch)
    return c


def _call(ctx, s, nstreams=0, **flags):
    """one cice_coupling_prep on copies of the in / out arrays of s and outputs full of NaN; the arrays that are intent(in)
    in the reference must come back as they went in.  Returns the dict the call was given."""
    a = {k: s[k] for k in IN_KEYS if k in s}
    for k in cc.FLUXES + cc.MIX_IO:
        a[k] = s[k].copy()
    shp = s["coszen"].shape
    for k in cc.OUT + cc.MIX_OUT + cc.MIX_OPT:           # (NaN sentinels: fhocn_gbm, fswthru_gbm among them)
        a[k] = np.full(shp, np.nan)
    if nstreams:
        a["albcnt"] = s["albcnt"][:nstreams].copy()
    before = {k: a[k].copy() for k in IN_KEYS if k in a}
    ctx.coupling_prep(DT, a, nstreams=nstreams, **flags)
    for k, v in before.items():
        assert np.array_equal(cc.u64(a[k]) if v.dtype == np.float64 else a[k], cc.u64(v) if v.dtype == np.float64 else v), \
            ("intent(in)", k)
    return a


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = cc.u64(got) != cc.u64(want)
    assert not bad.any(), (what, int(bad.sum()), "words differ", np.argwhere(bad)[:4].tolist())


def _check_prep(name, s, a, nstreams, scaled=None):
    """k_coupling_prep's outputs against the restatement and, for the 17 of scale_fluxes, the fixture"""
    want = cc.expected(name, s, nstreams)
    for k in cc.OUT:
        _same(a[k], want[k], (name, k))
    for k in cc.FLUXES:                          # scale_fluxes = 0: neither read (but for the *_gbm) nor written
        _same(a[k], want[k] if cc.CASES[name]["scale_fluxes"] else s[k], (name, k))
    if scaled is not None:
        for k in cc.SCALED:
            _same(a[k], scaled[k], (name, k, "fixture"))
    if nstreams:
        _same(a["albcnt"], want["albcnt"], (name, "albcnt"))
        assert (a["albcnt"] != s["albcnt"][:nstreams]).any()
    if not cc.CASES[name]["oceanmixed_ice"]:
        for k in cc.MIX_OUT + cc.MIX_OPT:
            assert np.isnan(a[k]).all(), (name, k, "written with oceanmixed_ice = 0")
        for k in cc.MIX_IO:
            _same(a[k], s[k], (name, k))


def _check_tail(s, a):
    """ice_ocean.F90:190-231 in numpy on the device's own delt, delq, shcoef, lhcoef"""
    want, m, _ = cc.mixed_tail_numpy(s, {k: a[k] for k in cc.MIX_OPT})
    for k in cc.MIX_TAIL:
        _same(a[k], want[k], ("tail", k))
    ocean = s["tmask"] != 0
    for k in cc.MIX_OUT[-4:]:
        assert (a[k] == cc.ALBOCN).all(), k
    for k in ("sst", "frzmlt", "flwout_ocn", "fsens_ocn", "flat_ocn", "evap_ocn") + cc.MIX_OUT[5:9] + cc.MIX_OPT:
        assert not cc.u64(a[k])[~ocean].any(), (k, "not +0 on land")
    _same(a["qdp"][~ocean], s["qdp"][~ocean], "qdp passes through on land")
    return m


@pytest.mark.parametrize("nstreams", (1, 2))
@pytest.mark.parametrize("name", tuple(cc.CASES))
def test_fields_bit_for_bit(name, nstreams):
    s, scaled, _ = _gold(name)
    ctx = _context(name, flavour="auscom" if name == "auscom" else "standalone")
    try:
        a = _call(ctx, s, nstreams)
    finally:
        ctx.close()
    _check_prep(name, s, a, nstreams, scaled)
    phys = cc.physical()
    lit = s["coszen"] > cc.PUNY
    assert (a["albice"][lit & ~phys] > 0).sum() >= 8 and not cc.u64(a["albice"])[~lit].any()    # ghost cells are merged too
    if "albpndn" not in s:
        assert not cc.u64(a["albpnd"]).any()


def test_padded_blocks_against_the_restatement():
    """configuration pad: 3 x 3 blocks of 12 x 10 on 26 x 22 cells, the last column and row of blocks padded"""
    ctx = _context("standalone", domain=(26, 22, 12, 10))
    try:
        assert (ctx.nx, ctx.ny, ctx.nblocks) == (14, 12, 9)
        s = cc.make_inputs("standalone", nb=9, seed=2026102209)
        a = _call(ctx, s, 2)
    finally:
        ctx.close()
    _check_prep("standalone", s, a, 2)
    m = _check_tail(s, a)
    assert all(m[k].sum() >= 8 for k in cc.MIX_MASKS)


@pytest.fixture(scope="module")
def mixed_run():
    s, _, ref = _gold("standalone")
    ctx = _context("standalone")
    try:
        a = _call(ctx, s)
    finally:
        ctx.close()
    return s, ref, a


def test_mixed_layer_boundary_layer(mixed_run):
    s, ref, a = mixed_run
    for k in ("delt", "delq"):
        _same(a[k], ref[k], k)
    e_ref, truth = cc.reference_error(s, ref)
    ocean = s["tmask"] != 0
    e_dev = {k: ac.cell_deviation(a[k], truth[k], ocean) for k in cc.MIX_LOG}     # zeros: same sign, asserted there
    print("E_ref  " + ", ".join(f"{k} {v:.3e}" for k, v in e_ref.items()))
    print("device " + ", ".join(f"{k} {v:.3e}" for k, v in e_dev.items()))
    print("words that differ bitwise from the reference, of", int(ocean.sum()), "ocean cells per field:",
          {k: int((cc.u64(a[k]) != cc.u64(ref[k])).sum()) for k in cc.MIX_LOG + cc.MIX_TAIL})
    for k in cc.MIX_LOG:
        assert e_dev[k] <= 4.0 * e_ref[k] + 2.0 ** -52, (k, e_dev[k], e_ref[k])


def test_mixed_layer_tail_on_the_device_s_own_coefficients(mixed_run):
    s, ref, a = mixed_run
    _check_tail(s, a)


def test_mixed_layer_masks_equal_the_fixture_s(mixed_run):
    s, ref, a = mixed_run
    got, want = cc.masks_from_outputs(s, a), cc.masks_from_outputs(s, ref)
    for k in cc.MIX_MASKS:
        assert want[k].sum() >= 8 and np.array_equal(got[k], want[k]), k


def test_mixed_layer_land(mixed_run):
    s, ref, a = mixed_run
    land = s["tmask"] == 0
    assert land.sum() >= 8 and (land & ~cc.physical()).sum() >= 1
    for k in ("sst", "frzmlt", "flwout_ocn", "fsens_ocn", "flat_ocn", "evap_ocn"):
        assert not cc.u64(a[k])[land].any(), k
    assert (s["sst"][land] != 0).all()
    _same(a["qdp"][land], s["qdp"][land], "qdp")
    for k in cc.MIX_IO + cc.MIX_OUT + cc.MIX_OPT:          # and everything the reference leaves there
        _same(a[k][land], ref[k][land], (k, "land"))


def test_call_order_mixed_layer_sees_the_unscaled_fluxes(mixed_run):
    """the *_gbm outputs started as NaN and hold the unscaled inputs; fhocn and fswthru came back scaled; the tail, which reads
    them, reproduces from the UNSCALED ones (test_mixed_layer_tail_on_the_device_s_own_coefficients) and not from the scaled"""
    s, ref, a = mixed_run
    for k in ("fhocn", "fswthru", "fresh", "fsalt"):
        _same(a[k + "_gbm"], s[k], k + "_gbm")
    moved = (s["tmask"] != 0) & (s["aice"] > 0) & (s["aice"] < 1) & (s["fhocn"] != 0)
    assert moved.sum() >= 8 and (a["fhocn"][moved] != s["fhocn"][moved]).all()
    after, _, _ = cc.mixed_tail_numpy(dict(s, fhocn=a["fhocn"], fswthru=a["fswthru"]), {k: a[k] for k in cc.MIX_OPT})
    assert (cc.u64(after["sst"]) != cc.u64(a["sst"]))[moved].sum() >= 8


def _swap_state(s, aicen, albedos):
    """the case's 2-d fields around another call's aicen and per-category albedos"""
    t = {k: v for k, v in s.items() if k not in cc.CAT_ALB + ("aicen",)}
    t["aicen"] = aicen
    t.update(albedos)
    return t


def _nan_like(t, keys):
    return dict(t, **{k: np.full_like(t[k], np.nan) for k in keys if k in t})


def _equal_runs(a, b, what):
    for k in cc.OUT + cc.FLUXES:
        _same(a[k], b[k], (what, k))


def test_alb_resident_behind_step_radiation():
    from test_gpu_shortwave import _one_call as radiation
    s, _, _ = _gold("nomix")
    ctx = _context("nomix")
    try:
        with pytest.raises(lib.CiceError, match="error -1: cice_coupling_prep: alb_resident needs"):
            _call(ctx, s, alb_resident=True)                                    # no record yet
        ctx.shortwave_init(**sc.init_kwargs("default"))
        r = sc.case_inputs("default")
        rad = radiation(ctx, r)
        t = _swap_state(s, r["aicen"], {k: rad[k] for k in cc.CAT_ALB[:6]})      # (no albpndn: zeros after the ccsm3 scheme)
        up = _call(ctx, t, 1)
        res = _call(ctx, _nan_like(dict(t, albpndn=rad["albicen"]), cc.CAT_ALB), 1, alb_resident=True)
        res2 = _call(ctx, _nan_like(t, cc.CAT_ALB), 1, alb_resident=True)        # the record stays
        ctx.prep_radiation(sc.prep_inputs())                                     # stages its aicen in that buffer
        with pytest.raises(lib.CiceError, match="error -1: cice_coupling_prep: alb_resident needs"):
            _call(ctx, t, alb_resident=True)
    finally:
        ctx.close()
    _check_prep("nomix", t, up, 1)
    assert (up["albice"] > 0).sum() >= 8 and not cc.u64(up["albpnd"]).any()
    _equal_runs(res, up, "alb_resident"); _equal_runs(res2, up, "alb_resident again")


def test_alb_resident_behind_step_radiation_dedd():
    from test_gpu_dedd import _one_call as radiation
    s, _, _ = _gold("nomix")
    ctx = _context("nomix")
    try:
        ctx.shortwave_dedd_init(**dc.init_kwargs("default"))
        r = dc.case_inputs("default")
        rad = radiation(ctx, r)
        t = _swap_state(dict(s, coszen=r["coszen"]), r["aicen"], {k: rad[k] for k in cc.CAT_ALB})
        up = _call(ctx, t)
        res = _call(ctx, _nan_like(t, cc.CAT_ALB), alb_resident=True)
        with pytest.raises(lib.CiceError, match="error -1: cice_step_radiation_dedd"):     # a failing radiation call ...
            ctx.step_radiation_dedd(dict(r, swvdr=None, **{k: np.zeros_like(v) for k, v in rad.items()}))
        with pytest.raises(lib.CiceError, match="error -1: cice_coupling_prep: alb_resident needs"):   # ... ends the record
            _call(ctx, t, alb_resident=True)
    finally:
        ctx.close()
    _check_prep("nomix", t, up, 0)
    assert (up["albpnd"] > 0).sum() >= 8
    _equal_runs(res, up, "alb_resident")


def test_state_resident_behind_step_ridge():
    from test_gpu_ridge_chain import DT as RIDGE_DT, _context as ridge_context, _inputs
    ctx, dom, grid = ridge_context("3x2pad", "ntr4")
    try:
        _, _, st = _inputs(dom, grid)
        ctx.thermo_init()
        ctx.coupling_init(oceanmixed_ice=False)
        s = cc.make_inputs("nomix", dom["nblocks"], dom["ny"], dom["nx"], seed=2026102210)
        with pytest.raises(lib.CiceError, match="error -1: cice_coupling_prep: state_resident needs"):
            _call(ctx, s, state_resident=True)
        r = ctx.step_ridge(RIDGE_DT, st, bound=True)
        assert r["l_stop"] == 0, r
        t = dict(s, aicen=st["aicen"])
        res = _call(ctx, _nan_like(t, ("aicen",)), state_resident=True)
        up = _call(ctx, t)                                                       # uploads into a buffer of its own:
        res2 = _call(ctx, _nan_like(t, ("aicen",)), state_resident=True)         # the record is left alone
    finally:
        ctx.close()
    assert (t["aicen"] > cc.PUNY).sum() > 100
    _check_prep("nomix", t, up, 0)
    _equal_runs(res, up, "state_resident"); _equal_runs(res2, up, "state_resident again")


def test_bound_updates_the_ghost_cells_of_scale_factor():
    s, _, _ = _gold("standalone")
    ctx = _context("standalone", domain=(24, 20, 12, 10))
    try:
        assert (ctx.nx, ctx.ny, ctx.nblocks) == (cc.NX, cc.NY, cc.NB)
        a0 = _call(ctx, s, bound=False)
        a1 = _call(ctx, s, bound=True)
        want = a0["scale_factor"].copy()
        ctx.halo_update(want)
    finally:
        ctx.close()
    _same(a1["scale_factor"], want, "scale_factor")
    assert (cc.u64(want) != cc.u64(a0["scale_factor"]))[~cc.physical()].sum() >= 8
    _same(want[cc.physical()], a0["scale_factor"][cc.physical()], "physical cells")
    for k in cc.OUT[:-1] + cc.FLUXES + cc.MIX_IO + cc.MIX_OUT + cc.MIX_OPT:
        _same(a1[k], a0[k], k)
    ctx = _context("standalone")                         # no domain
    try:
        with pytest.raises(lib.CiceError, match="error -1: cice_coupling_prep: bound = 1 needs cice_domain_create"):
            _call(ctx, s, bound=True)
    finally:
        ctx.close()


def test_refusals():
    s, _, _ = _gold("standalone")
    ctx = lib.Context()
    try:
        ctx.sync()
        ctx.thermo_init()
        with pytest.raises(lib.CiceError, match=r"error -4: cice_coupling_init: atmbndy = 'constant'"):
            ctx.coupling_init(atmbndy="constant")
        ctx.thermo_batch_alloc(cc.NX, cc.NY, cc.NB)
        with pytest.raises(lib.CiceError, match="error -1: cice_coupling_prep: cice_coupling_init has not been called"):
            _call(ctx, s)
        ctx.coupling_init()
        with pytest.raises(lib.CiceError, match="error -1: cice_coupling_prep: ncat is not the library's"):
            _call(ctx, s, ncat=lib.NCAT + 1)
        with pytest.raises(lib.CiceError, match="error -1: cice_coupling_prep: nstreams must not be negative"):
            _call(ctx, s, nstreams=-1)
        with pytest.raises(lib.CiceError, match="error -1: cice_coupling_prep: albcnt is given with nstreams = 0"):
            ctx.coupling_prep(DT, dict(_call(ctx, s), albcnt=s["albcnt"][:1].copy()), nstreams=0)
        for k in ("coszen", "swidf", "aicen", "albsnon", "tmask", "fsens", "fhocn", "scale_factor", "albpnd", "hmix", "sst",
                  "Qref_ocn", "alidf_ocn"):
            with pytest.raises(lib.CiceError, match="error -1: cice_coupling_prep: NULL field"):
                ctx.coupling_prep(DT, dict(_call(ctx, s), **{k: None}))
        for k in ("albpndn", "albcnt") + cc.MIX_OPT:      # optional
            ctx.coupling_prep(DT, dict(_call(ctx, s), **{k: None}))
        with pytest.raises(lib.CiceError, match="error -1: cice_coupling_prep: state_resident needs"):
            _call(ctx, s, state_resident=True)
        with pytest.raises(lib.CiceError, match="error -1: cice_coupling_prep: alb_resident needs"):
            _call(ctx, s, alb_resident=True)
        with pytest.raises(lib.CiceError, match="error -1: cice_coupling_prep: state_resident must be 0 or 1"):
            _call(ctx, s, state_resident=2)
        ctx.coupling_init(scale_fluxes=False, oceanmixed_ice=False)     # then only these are looked at
        few = {k: v for k, v in _call(ctx, s).items() if k in ("aicen", "coszen", "swvdr", "swvdf", "swidr", "swidf", "fresh",
                                                                "fsalt", "fhocn", "fswthru") + cc.CAT_ALB + cc.OUT}
        ctx.coupling_prep(DT, few)
        ms = ctx.coupling_times(True)
        ctx.coupling_prep(DT, few)
        assert ctx.coupling_times(False)[1] > 0.0 and ms == (0.0, 0.0)
    finally:
        ctx.close()
    want = cc.merge_numpy(s)                              # the pointers left out were not needed
    for k in cc.OUT:
        _same(few[k], want[k], ("few pointers", k))
