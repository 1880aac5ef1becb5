"""Shortwave (ccsm3) on the device -- cice_shortwave_ccsm3, cice_step_radiation, cice_prep_radiation -- against what the
compiled reference recorded in tests/golden/shortwave.npz, ghost and land cells included.  Agreement by class of word:

  bit for bit, unconditionally: every word that passes through neither atan nor exp -- the snow albedos (albsnon), all
    albedos of the case `constant`, Sswabsn, every cell that is not on a list, the intent(in) arrays;
  bit for bit where conftest.TOL_EXP == 0 (the host libm that minted the fixture is the restated one), else to TOL_EXP:
    every output of the listed cells with hi > ahmax (1 + 1e-6), where fh = 1 exactly, and of every listed cell of the case
    `constant` -- fswintn, fswthrun, Iswabsn pass through exp;
  within TOL = 1e-12 of the field's magnitude (the project's bound for device-library transcendentals, TOL of
    test_gpu_atmo.py): the remaining cells, whose bare-ice albedo passes through the device library's atan (1 ulp of atan
    moves fh by <= 2 ulp and an albedo by < 1e-15).

cice_prep_radiation is held bit for bit to shortwave_case.prep_radiation_numpy (see there why that is the expected value).
The multi-block layout (3 x 2 blocks of 10 x 10 with a padded last column) is held to the block-wise entry, which is itself
held to the fixture."""
import functools

import numpy as np
import pytest

import shortwave_case as sc
import therm_itd_case as tc
from conftest import TOL_EXP
from cice4_amd import lib

pytestmark = pytest.mark.gpu
TOL = 1.0e-12
ALBEDOS = ("alvdrn", "alidrn", "alvdfn", "alidfn", "albicen", "albsnon")
ALL_OUT = sc.OUT + ("Sswabsn",)


@functools.lru_cache(maxsize=None)
def _gold(name):
    return sc.load_case(np.load(sc.FIXTURE), name)


def _context(name, flavour="standalone", calc_Tsfc=True, batch=None):
    c = lib.Context(flavour=flavour)
    c.sync()
    c.thermo_init(calc_Tsfc=calc_Tsfc)
    c.shortwave_init(**sc.init_kwargs(name))
    if batch:
        c.thermo_batch_alloc(*batch)
    return c


def _outputs(shape):
    nb, ncat, ny, nx = shape
    o = {k: np.full(shape, np.nan) for k in sc.OUT2}
    o["Iswabsn"] = np.full((nb, ncat, sc.NILYR, ny, nx), np.nan)
    o["Sswabsn"] = np.full((nb, ncat, sc.NSLYR, ny, nx), np.nan)
    return o


def _classes(name, s, blk=None):
    """(nb, ncat, ny, nx) masks: unlisted, exact (no atan), loose (atan)"""
    on = sc.listed(s, sc.block_table(*[s["aicen"].shape[k] for k in (0, 2, 3)]) if blk is None else blk)
    if sc.CASES[name]["albedo_type"] == "constant":
        return ~on, on, np.zeros_like(on)
    hi = s["vicen"] / np.where(on, s["aicen"], 1.0)
    thick = on & (hi > sc.NAMELIST["ahmax"] * (1.0 + 1.0e-6))
    return ~on, thick, on & ~thick


def _check(name, s, got, want, where, blk=None):
    """got against want by class of word; returns the number of (cell, category) pairs compared under TOL"""
    off, exact, loose = _classes(name, s, blk)
    assert np.array_equal(got["Sswabsn"], np.zeros_like(got["Sswabsn"])), (where, "Sswabsn")
    assert tc.same(got["albsnon"], want["albsnon"]), (where, "albsnon")
    if sc.CASES[name]["albedo_type"] == "constant":
        for k in ALBEDOS:
            assert tc.same(got[k], want[k]), (where, k)
    for k in sc.OUT:
        g, w = got[k], want[k]
        sel = (lambda m: m[:, :, None] & np.ones(g.shape, bool)) if k == "Iswabsn" else (lambda m: m)
        assert g.shape == w.shape and np.isfinite(g).all(), (where, k)
        assert tc.same(g[sel(off)], w[sel(off)]), (where, k, "unlisted")
        if TOL_EXP == 0.0:
            assert tc.same(g[sel(exact)], w[sel(exact)]), (where, k, "fh = 1", int((g[sel(exact)] != w[sel(exact)]).sum()))
        else:
            assert np.abs(g[sel(exact)] - w[sel(exact)]).max() <= TOL_EXP * np.abs(w).max(), (where, k, "fh = 1")
        if loose.any():
            err = np.abs(g[sel(loose)] - w[sel(loose)]).max() / np.abs(w).max()
            assert err <= max(TOL, TOL_EXP), (where, k, "atan", err)
    return int(loose.sum())


def _blockwise(ctx, name, s, blk=None):
    """cice_shortwave_ccsm3 per (block, category) on step_radiation's lists: the arrays of ALL_OUT (Sswabsn as the caller
    zeroes it), and the inputs the calls were given"""
    nb, ncat, ny, nx = s["aicen"].shape
    blk = sc.block_table(nb, ny, nx) if blk is None else blk
    out = _outputs(s["aicen"].shape)
    out["Sswabsn"][...] = 0.0
    names = dict(alvdrn="alvdrn", alidrn="alidrn", alvdfn="alvdfn", alidfn="alidfn", fswsfc="fswsfcn", fswint="fswintn",
                 fswthru="fswthrun", Iswabs="Iswabsn", albin="albicen", albsn="albsnon")
    on = sc.listed(s, blk)
    for b in range(nb):
        for n in range(ncat):
            jj, ii = np.nonzero(on[b, n])
            indxi, indxj = np.zeros(nx * ny, np.int32), np.zeros(nx * ny, np.int32)
            indxi[:len(ii)], indxj[:len(ii)] = ii + 1, jj + 1
            a = {k: np.ascontiguousarray(s[k][b, n]) for k in ("aicen", "vicen", "vsnon")}
            a["Tsfcn"] = np.ascontiguousarray(s["trcrn"][b, n, 0])
            for k in sc.SW:
                a[k] = np.ascontiguousarray(s[k][b])
            ins = {k: v.copy() for k, v in a.items()}
            for k, big in names.items():
                a[k] = np.full((sc.NILYR, ny, nx) if k == "Iswabs" else (ny, nx), np.nan)
            ocn = np.ascontiguousarray(s["ocn_albedo"][b]) if "ocn_albedo" in s else None
            ctx.shortwave_ccsm3(len(ii), indxi, indxj, a, ocn_albedo=ocn)
            for k, v in ins.items():
                assert tc.same(a[k], v), ("intent(in)", k, b, n)
            for k, big in names.items():
                out[big][b, n] = a[k]
    return out


def _one_call(ctx, s, state_resident=False, coszen=None):
    a = dict(s)
    a.update(_outputs(s["aicen"].shape))
    a["coszen"] = coszen
    before = {k: s[k].copy() for k in s}
    ctx.step_radiation(a, state_resident=state_resident)
    for k, v in before.items():
        assert tc.same(s[k], v), ("intent(in)", k)
    return {k: a[k] for k in ALL_OUT}


@pytest.mark.parametrize("name", ("default", "constant"))
def test_blockwise_entry_reproduces_the_reference(name):
    s, want = _gold(name)
    ctx = _context(name)
    try:
        got = _blockwise(ctx, name, s)
    finally:
        ctx.close()
    n = _check(name, s, got, want, ("block-wise", name))
    assert (n >= 8) == (name == "default"), n


def test_auscom_flavour_with_the_ocean_albedo_plane():
    name = "auscom"
    s, want = _gold(name)
    ctx = _context(name, flavour="auscom", batch=(sc.NX, sc.NY, sc.NB))
    try:
        got = _blockwise(ctx, name, s)
        one = _one_call(ctx, s)
    finally:
        ctx.close()
    assert _check(name, s, got, want, ("block-wise", name)) >= 8
    assert _check(name, s, one, want, ("one call", name)) >= 8
    for k in ALL_OUT:
        assert tc.same(one[k], got[k]), k


@pytest.mark.parametrize("name", ("default", "constant"))
def test_one_call_on_the_four_blocks(name):
    s, want = _gold(name)
    ctx = _context(name, batch=(sc.NX, sc.NY, sc.NB))
    try:
        coszen = np.full((sc.NB, sc.NY, sc.NX), np.nan)
        got = _one_call(ctx, s, coszen=coszen)
    finally:
        ctx.close()
    n = _check(name, s, got, want, ("one call", name))
    assert (n >= 8) == (name == "default"), n
    assert (coszen == 0.5).all()


def test_one_call_on_padded_blocks_equals_the_blockwise_entry():
    """3 x 2 blocks of 10 x 10 on 24 x 20 cells: the last column of blocks holds 4 columns of cells"""
    ctx = lib.Context()
    try:
        ctx.sync()
        dom = ctx.domain_create(24, 20, 10, 10, ew=1, ns=0)
        nb, ny, nx = dom["nblocks"], dom["ny"], dom["nx"]
        assert (nb, ny, nx) == (6, 12, 12)
        blk = np.stack([dom[k] for k in ("ilo", "ihi", "jlo", "jhi")], axis=1).astype(np.int32)
        assert len({tuple(r) for r in blk}) > 1
        ctx.thermo_init()
        ctx.shortwave_init(**sc.init_kwargs("default"))
        ctx.thermo_batch_alloc(nx, ny, nb)
        s = sc.make_inputs("default", nb, ny, nx, blk)
        want = _blockwise(ctx, "default", s, blk)
        got = _one_call(ctx, s)
    finally:
        ctx.close()
    off, exact, loose = _classes("default", s, blk)
    assert loose.sum() >= 8 and exact.sum() >= 8 and (off & (s["aicen"] > sc.PUNY)).sum() >= 8   # (ice on ghost / padding cells)
    for k in ALL_OUT:
        assert np.array_equal(got[k], want[k]), k


def test_state_resident_after_step_ridge():
    from test_gpu_ridge_chain import DT, _context as ridge_context, _inputs

    def sw(dom):
        rng = np.random.default_rng(20261020)
        return {k: rng.uniform(0.0, 120.0, (dom["nblocks"], dom["ny"], dom["nx"])) for k in sc.SW}

    ctx, dom, grid = ridge_context("3x2pad", "ntr4")
    try:
        _, _, a = _inputs(dom, grid)
        ctx.thermo_init()
        ctx.shortwave_init(**sc.init_kwargs("default"))
        r = ctx.step_ridge(DT, a, bound=True)
        assert r["l_stop"] == 0, r
        s = dict({k: a[k] for k in sc.STATE}, **sw(dom))
        spoilt = dict(s, **{k: np.full_like(a[k], np.nan) for k in sc.STATE})   # resident: the state pointers are not read
        res = _one_call(ctx, spoilt, state_resident=True)
        res2 = _one_call(ctx, spoilt, state_resident=True)                      # ... and the record stays
        up = _one_call(ctx, s, state_resident=False)
        with pytest.raises(lib.CiceError, match="error -1"):                    # the upload ended the record
            _one_call(ctx, s, state_resident=True)
    finally:
        ctx.close()
    assert (s["aicen"] > sc.PUNY).sum() > 100 and up["fswsfcn"].max() > 0.0
    for k in ALL_OUT:
        assert np.array_equal(res[k], up[k]) and np.array_equal(res2[k], up[k]), k


@pytest.mark.parametrize("resident", (False, True))
def test_prep_radiation_bit_for_bit(resident):
    s, _ = _gold("default")
    ctx = _context("default", batch=(sc.NX, sc.NY, sc.NB))
    try:
        if resident:
            rad = _one_call(ctx, s)
            p = sc.prep_inputs(sw_arrays={k: rad[k].copy() for k in sc.PREP_SW}, aicen=s["aicen"])
            want, m = sc.prep_radiation_numpy(p)
            for k in sc.PREP_SW:             # download targets only
                p[k] = np.full_like(p[k], np.nan)
        else:
            p = sc.prep_inputs()
            want, m = sc.prep_radiation_numpy(p)
        ins = {k: p[k].copy() for k in sc.SW + ("alvdr_gbm", "alvdf_gbm", "alidr_gbm", "alidf_gbm", "aice", "aicen")}
        ctx.prep_radiation(p, sw_resident=resident)
    finally:
        ctx.close()
    assert m["scaled"].sum() >= 8 and m["unit"].sum() >= 8 and m["on"].sum() >= 8
    for k in ("scale_factor", "fswfac") + sc.PREP_SW:
        assert np.array_equal(p[k], want[k]), (k, int((p[k] != want[k]).sum()))
    for k, v in ins.items():
        assert tc.same(p[k], v), ("intent(in)", k)


def test_refusals():
    ctx = lib.Context()
    try:
        ctx.sync()
        with pytest.raises(lib.CiceError, match="error -1"):      # no cice_thermo_init
            ctx.shortwave_init(**sc.init_kwargs("default"))
        with pytest.raises(lib.CiceError, match="error -4"):      # heat_capacity = 0
            ctx.thermo_init(heat_capacity=False)
        with pytest.raises(lib.CiceError, match="error -1"):      # ... which leaves the context without thermo parameters
            ctx.shortwave_init(**sc.init_kwargs("default"))
        ctx.thermo_init()
        with pytest.raises(lib.CiceError, match="error -4"):
            ctx.shortwave_init(**dict(sc.init_kwargs("default"), shortwave="dEdd"))
        ctx.shortwave_init(**sc.init_kwargs("default"))
        ctx.thermo_batch_alloc(sc.NX, sc.NY, sc.NB)
        s, _ = _gold("default")
        with pytest.raises(lib.CiceError, match="error -1"):      # no resident state
            _one_call(ctx, s, state_resident=True)
        p = sc.prep_inputs()
        with pytest.raises(lib.CiceError, match="error -1"):      # no resident shortwave
            ctx.prep_radiation(p, sw_resident=True)
        ctx.prep_radiation(p, sw_resident=False)
        ctx.prep_radiation(p, sw_resident=True)                   # ... now there is
    finally:
        ctx.close()


def test_calc_Tsfc_false_zero_fills():
    s, _ = _gold("default")
    ctx = _context("default", calc_Tsfc=False, batch=(sc.NX, sc.NY, sc.NB))
    try:
        coszen = np.full((sc.NB, sc.NY, sc.NX), 0.25)
        got = _one_call(ctx, s, coszen=coszen)
        for k in ALL_OUT:
            if k in ("albicen", "albsnon"):
                assert np.isnan(got[k]).all(), k     # not touched, as in the reference
            else:
                assert np.array_equal(got[k], np.zeros_like(got[k])), k
        assert (coszen == 0.25).all()
        p = sc.prep_inputs()
        before = {k: p[k].copy() for k in ("scale_factor", "fswfac")}
        ctx.prep_radiation(p)
        for k in sc.PREP_SW:
            assert np.array_equal(p[k], np.zeros_like(p[k])), k
        for k, v in before.items():
            assert tc.same(p[k], v), k
    finally:
        ctx.close()
