"""The strength stage that opens every evp(dt) on the device -- k_strength, the device form of ice_strength with
asum_ridging / ridge_itd -- in every configuration, on thickness distributions that sit on the routine's guards
(tests/strength_case.py; test_strength_case.py pins the checker to the compiled reference on the same inputs), and the
device compile of exp() and pow() (cice4_amd/csrc/libm_exact.h) argument by argument against the host's libm.

Bounds: the exp-free configurations bit for bit on any host; everything else conftest.TOL_EXP / TOL_POW, which is 0 --
compared through the bit patterns -- where the host's glibc runs its FMA build."""
import math

import numpy as np
import pytest

import strength_case as sc
from cice4_amd import lib, synth
from conftest import relerr, TOL_EXP, TOL_POW
from test_gpu_evp import EVP_OUT_FIELDS, tol_of

pytestmark = pytest.mark.gpu

DT, NDTE = 3600.0, 4
STAGE = ("strength", "strairx", "strairy", "fm", "strtltx", "strtlty")     # what evp_prepare leaves final
LAYOUTS = {"one_block": (24, 20, 24), "2x2_blocks": (12, 10, 24), "wide_block": (64, 20, 64)}   # bsx, bsy, nxg


def _close(got, want, tol, what):
    """tol 0: the same bit patterns; else the field-level relative error"""
    if tol == 0.0:
        ne = np.argwhere(sc.bits(got) != sc.bits(want))
        assert len(ne) == 0, (what, len(ne), [(tuple(q), float(got[tuple(q)]).hex(), float(want[tuple(q)]).hex()) for q in ne[:4]])
    else:
        assert np.isfinite(got).all() and relerr(got, want) <= tol, (what, relerr(got, want))


def _kw(cfg, ndte=NDTE):
    return dict(ndte=ndte, kstrength=cfg[0], krdg_partic=cfg[1], krdg_redist=cfg[2], mu_rdg=cfg[3])


def _checker(orc, dom, grid, s, cfg):
    orc.set_evp_parameters(DT, NDTE, False); orc.set_strength_parameters(*cfg)
    so = {k: v.copy() for k, v in s.items()}
    try:
        orc.evp(orc.make_domain(dom, grid), so)
    finally:
        orc.set_strength_parameters()
    return so


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("cfg", sc.CONFIGS, ids=sc.cfg_id)
def test_strength_stage_alone(ctx, orc, cfg, layout):
    """upload, prepare, download: the six fields the stage leaves final, ghost cells and all, in every block"""
    bsx, bsy, nxg = LAYOUTS[layout]
    dom, grid, s, _ = sc.seeded_case(ctx, bsx, bsy, nxg=nxg)
    so = _checker(orc, dom, grid, s, cfg)
    sg = {k: v.copy() for k, v in s.items()}
    ctx.evp_init(grid, **_kw(cfg))
    ctx.evp_upload(sg); ctx.evp_prepare(DT); ctx.evp_download(sg)
    tol = 0.0 if cfg[:3] in sc.EXP_FREE else TOL_EXP
    for k in STAGE:
        _close(sg[k], so[k], tol, (cfg, layout, k))
    assert so["strength"].max() > 1.0e5


@pytest.mark.parametrize("layout", ["one_block", "2x2_blocks"])
@pytest.mark.parametrize("cfg", sc.CONFIGS, ids=sc.cfg_id)
def test_whole_step_on_edge_distributions(ctx, orc, cfg, layout):
    """evp(dt): the stress kernel sees zero strength under ice, 1e-13 and 2.9e5 side by side"""
    bsx, bsy, nxg = LAYOUTS[layout]
    dom, grid, s, _ = sc.seeded_case(ctx, bsx, bsy, nxg=nxg)
    so = _checker(orc, dom, grid, s, cfg)
    sg = {k: v.copy() for k, v in s.items()}
    ctx.evp_init(grid, **_kw(cfg))
    ctx.evp(DT, sg)
    assert np.array_equal(sg["iceumask"], so["iceumask"])
    for k in EVP_OUT_FIELDS:
        _close(sg[k], so[k], 0.0 if cfg[:3] in sc.EXP_FREE else tol_of(k), (cfg, layout, k))
    assert np.abs(so["uvel"]).max() > 0.0


def test_whole_step_on_edge_distributions_auscom(orc_aus):
    """the same through the coupled flavour of the library, on the configuration that no other test runs there"""
    c = lib.Context(flavour="auscom")
    c.sync()
    c.set_auscom(); orc_aus.set_auscom(True)
    cfg = (1, 1, 0, 4.0)
    dom, grid, s, _ = sc.seeded_case(c, 24, 20)
    so = _checker(orc_aus, dom, grid, s, cfg)
    sg = {k: v.copy() for k, v in s.items()}
    c.evp_init(grid, **_kw(cfg))
    c.evp(DT, sg)
    assert np.array_equal(sg["iceumask"], so["iceumask"])
    for k in EVP_OUT_FIELDS:
        _close(sg[k], so[k], tol_of(k), k)


def _exp_arguments():
    """three sets of x in [-20, 0] (and a little beyond), 128 x 64 each"""
    rng = np.random.default_rng(2026101902)
    n = 128 * 64
    uniform = rng.uniform(-20.0, 0.0, n)
    small = -np.exp(rng.uniform(np.log(1e-15), np.log(20.0), n))
    small[0] = 0.0                                        # aice = 1 exactly
    # where the argument reduction k = round(x 128 / ln2) rounds up or down
    k = np.resize(np.arange(-3700, 0), n).astype(np.float64)
    x = (k + 0.5) * (math.log(2.0) / 128.0)
    edge = (sc.bits(x).astype(np.int64) + rng.integers(-64, 65, n)).view(np.float64)
    return uniform, small, edge


def test_device_exp_against_host_libm(ctx, orc):
    """Hibler's strength with vice = 1 / 27500 is exp(-20 (1 - aice)) and nothing else: about 25 k arguments of the
    device's exp against the host's libm itself.  The ghost cells are compared as well: the routine computes the physical
    cells only, and the halo update fills the rest."""
    nxg, nyg = 128, 64
    assert 2.75e4 * (1.0 / 27500.0) == 1.0
    dom = ctx.domain_create(nxg, nyg, nxg, nyg, ew=1, ns=0)
    grid = synth.block_fields(synth.global_grid(nxg, nyg, land_rows=0), dom)
    s = synth.evp_state(grid, dom, cover="full")
    ny, nx = dom["ny"], dom["nx"]
    s["vice"][...] = 1.0 / 27500.0
    ctx.evp_init(grid, ndte=NDTE, kstrength=0)
    orc.set_strength_parameters(0, 1, 1, 4.0)
    li = np.zeros(nx * ny, np.int32); lj = np.zeros(nx * ny, np.int32)
    try:
        for name, x in zip(("uniform", "small", "edge"), _exp_arguments()):
            s["aice"][...] = 1.0
            s["aice"][0, 1:-1, 1:-1] = 1.0 + x.reshape(nyg, nxg) / 20.0
            aice = s["aice"][0, 1:-1, 1:-1]
            arg = -20.0 * (1.0 - aice)
            want = np.array([math.exp(v) for v in arg.ravel()]).reshape(nyg, nxg)
            assert len(np.unique(arg)) > arg.size // 2, name
            chk = orc.ice_strength(2, nx - 1, 2, ny - 1, 0, li, lj, s["aice"][0], s["vice"][0], s["aice0"][0],
                                   np.ascontiguousarray(s["aicen"][0]), np.ascontiguousarray(s["vicen"][0]))
            assert sc.same(chk[1:-1, 1:-1], want), name          # the checker calls the same libm
            sg = {k: v.copy() for k, v in s.items()}
            ctx.evp_upload(sg); ctx.evp_prepare(DT); ctx.evp_download(sg)
            _close(sg["strength"][0, 1:-1, 1:-1], want, TOL_EXP, name)
            full = np.zeros((1, ny, nx))
            full[0, 1:-1, 1:-1] = want
            full.reshape(-1)[dom["hdst"]] = full.reshape(-1)[dom["hsrc"]]
            _close(sg["strength"], full, TOL_EXP, name + ", ghost cells")
    finally:
        orc.set_strength_parameters()


def _pow_arguments(n):
    rng = np.random.default_rng(2026101903)
    one = (sc.bits(np.ones(129)).astype(np.int64) + np.arange(-64, 65)).view(np.float64)      # 1 +- 64 ulp, and 1
    p2 = 2.0 ** np.arange(-20, 10)
    # ... and where the log step's 128-entry table changes its entry (glibc: the top 7 mantissa bits of ix - OFF), +- 1 ulp
    off = np.int64(0x3FE6955500000000) + (np.arange(128, dtype=np.int64) << 45)
    tab = np.concatenate([off - 1, off, off + 1]).view(np.float64)
    special = np.concatenate([one, np.zeros(4), p2, np.nextafter(p2, 0.0), np.nextafter(p2, np.inf), tab, 8.0 * tab])
    nlog = (n - len(special)) // 2
    logu = np.exp(rng.uniform(np.log(1e-12), np.log(1e3), nlog))
    uni = rng.uniform(0.0, 30.0, n - len(special) - nlog)
    x = np.concatenate([special, logu, uni])
    assert len(x) == n and x.max() <= 1.0e3 and x.min() == 0.0
    return rng.permutation(x)


def test_device_pow_against_host_libm(ctx, orc):
    """frzmlt_bottom_lateral with Tf = 0, no ice energy and frzmlt = -1e30: deltaT = sst exactly and rside is
    sst**1.36 times constants -- the device's pow against the checker's libm, on the boundaries of its log step"""
    ctx.thermo_init(); orc.init_thermo()
    ny, nx = 66, 130
    rng = np.random.default_rng(2026101904)
    sst = np.ones((ny, nx))
    sst[1:-1, 1:-1] = _pow_arguments((ny - 2) * (nx - 2)).reshape(ny - 2, nx - 2)
    sx = rng.uniform(2.5, 4.0, (ny, nx)); sy = rng.uniform(3.0, 5.0, (ny, nx))
    assert np.sqrt(np.sqrt(sx * sx + sy * sy) / synth.rhow).min() > 0.05         # ustar > ustar_min
    args = (2, nx - 1, 2, ny - 1, DT, np.full((ny, nx), 0.5), np.full((ny, nx), -1.0e30), np.zeros((20, ny, nx)),
            np.zeros((5, ny, nx)), sst, np.zeros((ny, nx)), sx, sy)
    got = ctx.frzmlt_bottom_lateral(*args); want = orc.frzmlt_bottom_lateral(*args)
    for g, w, nm in zip(got, want, ("Tbot", "fbot", "rside")):
        assert np.isfinite(w).all(), nm
        _close(g, w, TOL_POW, nm)
    r = want[2][1:-1, 1:-1]
    assert ((r > 0.0) & (r < 1.0)).mean() >= 0.95          # the clamp is not hiding pow
    assert len(np.unique(r)) > 7000
