"""Delta-Eddington shortwave on the device -- cice_shortwave_dEdd, cice_step_radiation_dedd -- against what the compiled
reference recorded in tests/golden/dedd.npz, ghost and land cells included.  The scheme's only transcendental functions are
exp (restated bit for bit in libm_exact.h) and sqrt (correctly rounded), so the agreement is

  bit for bit, unconditionally: every word that passes through no exp -- the cells off the lists and the listed cells
    without sun, which hold zeros -- and the intent(in) arrays;
  bit for bit where conftest.TOL_EXP == 0 (the host libm that minted the fixture is the restated one), else to TOL_EXP of
    the field's magnitude: every other word.

Behind cice_step_radiation_dedd, cice_prep_radiation(sw_resident = 1) is held to shortwave_case.prep_radiation_numpy on the
downloaded arrays, and cice_radiation_chain(1) to the unchained calls."""
import functools

import numpy as np
import pytest

import dedd_case as dc
import shortwave_case as sc
import therm_itd_case as tc
import thermo_case as tcase
from conftest import TOL_EXP
from cice4_amd import lib

pytestmark = pytest.mark.gpu
IN_2D = dc.SW + ("coszen",)


@functools.lru_cache(maxsize=None)
def _gold(name):
    return dc.load_case(np.load(dc.FIXTURE), name)


def _context(name, calc_Tsfc=True, batch=None):
    c = lib.Context()
    c.sync()
    c.thermo_init(calc_Tsfc=calc_Tsfc)
    c.shortwave_dedd_init(**dc.init_kwargs(name))
    if batch:
        c.thermo_batch_alloc(*batch)
    return c


def _outputs(shape):
    nb, ncat, ny, nx = shape
    o = {k: np.full(shape, np.nan) for k in dc.OUT2}
    for k, n in dc.LAYERS.items():
        o[k] = np.full((nb, ncat, n, ny, nx), np.nan)
    return o


def _check(s, got, want, where):
    """got against want by class of word; returns the number of (cell, category) pairs the scheme ran on"""
    act = dc.listed(s) & (s["coszen"] > dc.PUNY)[:, None]
    for k in dc.OUT:
        g, w = got[k], want[k]
        sel = (lambda m: m[:, :, None] & np.ones(g.shape, bool)) if k in dc.LAYERS else (lambda m: m)
        assert g.shape == w.shape and np.isfinite(g).all(), (where, k)
        assert tc.same(g[sel(~act)], w[sel(~act)]) and not g[sel(~act)].view(np.uint64).any(), (where, k, "no exp")
        if TOL_EXP == 0.0:
            assert tc.same(g[sel(act)], w[sel(act)]), (where, k, int((g[sel(act)] != w[sel(act)]).sum()), dc.rel_err(g, w))
        else:
            assert dc.rel_err(g, w) <= TOL_EXP, (where, k, dc.rel_err(g, w))
    return int(act.sum())


def _one_call(ctx, s, state_resident=False):
    a = {k: v for k, v in s.items() if k in dc.STATE + IN_2D + ("apondn", "hpondn")}
    a.update(_outputs(s["aicen"].shape))
    before = {k: v.copy() for k, v in a.items() if k not in dc.OUT}
    ctx.step_radiation_dedd(a, state_resident=state_resident)
    for k, v in before.items():
        assert tc.same(a[k], v), ("intent(in)", k)
    return {k: a[k] for k in dc.OUT}


def _blockwise(ctx, name, s, pairs=None):
    """cice_shortwave_dEdd per (block, category) on step_radiation's lists.  For a driver case fs, rhosnw, rsnw, fp, hp are
    what the restatement's set_snow / set_pond give (each one IEEE operation after another: the reference's bits)."""
    nb, ncat, ny, nx = s["aicen"].shape
    on = dc.listed(s)
    if dc.CASES[name]["blockwise"]:
        given = {k: s[k] for k in ("fs", "rhosnw", "rsnw", "fp", "hp")}
    else:
        fs, rho, r, fT = dc.set_snow_numpy(name, s, on)
        fp = np.where(on, np.float64(0.3) * fT * (np.float64(1.0) - fs), 0.0)
        given = dict(fs=fs, fp=fp, hp=fp.copy(), rhosnw=np.stack([rho] * dc.NSLYR, axis=2), rsnw=np.stack([r] * dc.NSLYR, axis=2))
    names = dict(alvdr="alvdrn", alvdf="alvdfn", alidr="alidrn", alidf="alidfn", fswsfc="fswsfcn", fswint="fswintn",
                 fswthru="fswthrun", Sswabs="Sswabsn", Iswabs="Iswabsn", albice="albicen", albsno="albsnon", albpnd="albpndn")
    out = {}
    for b, n in (pairs or [(b, n) for b in range(nb) for n in range(ncat)]):
        jj, ii = np.nonzero(on[b, n])
        indxi, indxj = np.zeros(nx * ny, np.int32), np.zeros(nx * ny, np.int32)
        indxi[:len(ii)], indxj[:len(ii)] = ii + 1, jj + 1
        a = dict(aice=s["aicen"][b, n], vice=s["vicen"][b, n], vsno=s["vsnon"][b, n], coszen=s["coszen"][b],
                 **{k: s[k][b] for k in dc.SW}, **{k: v[b, n] for k, v in given.items()})
        a = {k: np.ascontiguousarray(v) for k, v in a.items()}
        ins = {k: v.copy() for k, v in a.items()}
        for k, big in names.items():
            a[k] = np.full((dc.LAYERS[big], ny, nx) if big in dc.LAYERS else (ny, nx), np.nan)
        ctx.shortwave_dEdd(len(ii), indxi, indxj, a)
        for k, v in ins.items():
            assert tc.same(a[k], v), ("intent(in)", k, b, n)
        out[b, n] = {big: a[k] for k, big in names.items()}
    return out


@pytest.mark.parametrize("name", dc.DRIVER_CASES)
def test_one_call_reproduces_the_reference(name):
    s, want = _gold(name)
    ctx = _context(name, batch=(dc.NX, dc.NY, dc.NB))
    try:
        got = _one_call(ctx, s)
    finally:
        ctx.close()
    assert _check(s, got, want, ("one call", name)) >= 100


def test_blockwise_entry_on_the_tables_case():
    s, want = _gold("tables")
    ctx = _context("tables")
    try:
        got = _blockwise(ctx, "tables", s)
    finally:
        ctx.close()
    full = {k: np.stack([np.stack([got[b, n][k] for n in range(dc.NCAT)]) for b in range(dc.NB)]) for k in dc.OUT}
    assert _check(s, full, want, ("block-wise", "tables")) >= 100


def test_blockwise_entry_on_one_pair_of_default():
    s, want = _gold("default")
    on = dc.listed(s) & (s["coszen"] > dc.PUNY)[:, None]
    b, n = np.unravel_index(np.argmax(on.reshape(dc.NB, dc.NCAT, -1).sum(axis=2)), (dc.NB, dc.NCAT))
    assert on[b, n].sum() >= 8
    ctx = _context("default")
    try:
        got = _blockwise(ctx, "default", s, pairs=[(int(b), int(n))])[int(b), int(n)]
    finally:
        ctx.close()
    for k in dc.OUT:
        g, w = got[k], want[k][b, n]
        off = ~(on[b, n] & np.ones(g.shape, bool))
        assert not g[off].view(np.uint64).any(), (k, "no exp")
        if TOL_EXP == 0.0:
            assert tc.same(g, w), (k, int((g != w).sum()))
        else:
            assert dc.rel_err(g, want[k]) <= TOL_EXP, k


def test_state_resident_after_step_ridge():
    from test_gpu_ridge_chain import DT, _context as ridge_context, _inputs

    ctx, dom, grid = ridge_context("3x2pad", "ntr4")
    try:
        _, _, a = _inputs(dom, grid)
        ctx.thermo_init()
        ctx.shortwave_dedd_init(**dc.init_kwargs("default"))
        r = ctx.step_ridge(DT, a, bound=True)
        assert r["l_stop"] == 0, r
        rng = np.random.default_rng(20261022)
        shp = (dom["nblocks"], dom["ny"], dom["nx"])
        f2 = dict({k: rng.uniform(0.0, 120.0, shp) for k in dc.SW}, coszen=rng.uniform(-0.1, 1.0, shp))
        s = dict({k: a[k] for k in dc.STATE}, **f2)
        spoilt = dict(s, **{k: np.full_like(a[k], np.nan) for k in dc.STATE})   # resident: the state pointers are not read
        res = _one_call(ctx, spoilt, state_resident=True)
        res2 = _one_call(ctx, spoilt, state_resident=True)                      # ... and the record stays
        up = _one_call(ctx, s, state_resident=False)
        with pytest.raises(lib.CiceError, match="error -1"):                    # the upload ended the record
            _one_call(ctx, s, state_resident=True)
    finally:
        ctx.close()
    assert (s["aicen"] > dc.PUNY).sum() > 100 and up["fswsfcn"].max() > 0.0 and up["albpndn"].max() >= 0.0
    for k in dc.OUT:
        assert np.array_equal(res[k], up[k]) and np.array_equal(res2[k], up[k]), k


def test_prep_radiation_behind_it_bit_for_bit():
    s, _ = _gold("default")
    ctx = _context("default", batch=(dc.NX, dc.NY, dc.NB))
    try:
        rad = _one_call(ctx, s)
        p = sc.prep_inputs(sw_arrays={k: rad[k].copy() for k in sc.PREP_SW}, aicen=s["aicen"])
        want, m = sc.prep_radiation_numpy(p)
        for k in sc.PREP_SW:             # download targets only
            p[k] = np.full_like(p[k], np.nan)
        ctx.prep_radiation(p, sw_resident=True)
    finally:
        ctx.close()
    assert m["scaled"].sum() >= 8 and m["unit"].sum() >= 8 and m["on"].sum() >= 8 and np.abs(want["Sswabsn"]).max() > 0.0
    for k in ("scale_factor", "fswfac") + sc.PREP_SW:
        assert np.array_equal(p[k], want[k]), (k, int((p[k] != want[k]).sum()))


def _therm1_behind(mode):
    """cice_step_radiation_dedd -> cice_prep_radiation(sw_resident = 1) -> cice_step_therm1 on thermo_case.therm1_inputs'
    state, the five shortwave arrays of cice_thermo_fields being the arrays the radiation calls write"""
    NY, NX, NB = 14, 22, 2
    ctx = lib.Context()
    try:
        ctx.sync()
        ctx.thermo_init()
        ctx.shortwave_dedd_init(**dc.init_kwargs("default"))
        ctx.thermo_batch_alloc(NX, NY, NB)
        ctx.radiation_chain(mode)
        batch, _, fz, pc, acc = tcase.therm1_inputs(NY, NX, NB, seed=35)
        rng = np.random.default_rng(20261023)
        shp = (NB, NY, NX)
        sw = {k: rng.uniform(0.0, 15.0, shp) for k in dc.SW}       # (what the cold columns of the state can take)
        gbm = {k: rng.uniform(0.05, 0.9, shp) for k in ("alvdr_gbm", "alvdf_gbm", "alidr_gbm", "alidf_gbm")}
        extra = dict(scale_factor=rng.uniform(10.0, 40.0, shp), fswfac=np.zeros(shp))
        alb = {k: np.zeros(batch["aicen"].shape) for k in ("alvdrn", "alidrn", "alvdfn", "alidfn", "albicen", "albsnon", "albpndn")}
        five = dict(fswsfcn=batch["fswsfc"], fswintn=batch["fswint"], fswthrun=batch["fswthrun"], Sswabsn=batch["Sswabs"],
                    Iswabsn=batch["Iswabs"])
        fzb = dict(fz, Tbot=np.zeros(shp), fbot=np.zeros(shp), rside=np.zeros(shp))
        ctx.step_radiation_dedd(dict({k: batch[k] for k in dc.STATE}, **sw, **alb, **five, coszen=rng.uniform(0.1, 1.0, shp)))
        assert batch["fswsfc"].max() > 0.0
        ctx.prep_radiation(dict(sw, **gbm, **extra, **five, aice=fz["aice"], aicen=batch["aicen"]), sw_resident=True)
        if mode:                             # the device copies are what is read
            batch["fswthrun"][...] = np.nan
        r = ctx.step_therm1(tcase.DT, 150.0, batch, fzb, pc, acc)
        assert r["l_stop"] == 0 and r["n_updates"] > 0, r
        snap = lambda d: {k: v.copy() for k, v in d.items() if isinstance(v, np.ndarray)}  # noqa: E731
        return snap(batch), snap(acc), snap(fzb)
    finally:
        ctx.close()


def test_radiation_chain_gives_the_bits_of_the_unchained_step_therm1():
    want, got = _therm1_behind(0), _therm1_behind(1)
    assert np.isfinite(want[0]["fswsfc"]).all() and np.abs(want[1]["fswabs"]).max() > 0.0
    assert np.isnan(got[0]["fswthrun"]).all()
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for k in w:
            if k != "fswthrun":
                assert np.array_equal(g[k], w[k], equal_nan=True), (k, int((g[k] != w[k]).sum()))


def test_refusals():
    s, _ = _gold("tr_pond")
    ctx = lib.Context()
    try:
        ctx.sync()
        with pytest.raises(lib.CiceError, match="error -1"):      # no cice_thermo_init
            ctx.shortwave_dedd_init(**dc.init_kwargs("default"))
        ctx.thermo_init()
        ctx.thermo_batch_alloc(dc.NX, dc.NY, dc.NB)
        with pytest.raises(lib.CiceError, match="error -1: cice_shortwave_dedd_init"):      # no init
            _one_call(ctx, s)
        ctx.shortwave_init(**sc.init_kwargs("default"))           # the other scheme's init is not this one's
        with pytest.raises(lib.CiceError, match="error -1: cice_shortwave_dedd_init"):
            _one_call(ctx, s)
        ctx.shortwave_dedd_init(**dc.init_kwargs("tr_pond"))
        with pytest.raises(lib.CiceError, match="error -1"):      # no resident state
            _one_call(ctx, s, state_resident=True)
        with pytest.raises(lib.CiceError, match="error -1"):      # tr_pond without the pond planes
            _one_call(ctx, {k: v for k, v in s.items() if k not in ("apondn", "hpondn")})
        _one_call(ctx, s)
        with pytest.raises(lib.CiceError, match="error -4"):      # the old refusal stays
            ctx.shortwave_init(**dict(sc.init_kwargs("default"), shortwave="dEdd"))
    finally:
        ctx.close()
    nobatch = lib.Context()
    try:
        nobatch.sync()
        nobatch.thermo_init()
        nobatch.shortwave_dedd_init(**dc.init_kwargs("default"))
        with pytest.raises(lib.CiceError, match="error -1: cice_thermo_batch_alloc"):      # no batch
            _one_call(nobatch, _gold("default")[0])
    finally:
        nobatch.close()


def test_calc_Tsfc_false_zero_fills():
    s, _ = _gold("default")
    ctx = _context("default", calc_Tsfc=False, batch=(dc.NX, dc.NY, dc.NB))
    try:
        got = _one_call(ctx, s)
    finally:
        ctx.close()
    for k in dc.OUT:
        if k in ("albicen", "albsnon", "albpndn"):
            assert np.isnan(got[k]).all(), k     # not touched, as in the reference
        else:
            assert np.array_equal(got[k], np.zeros_like(got[k])), k
