"""The transport -> ridging hand-over on the device (cice_ridge_chain, cice_transport_download_state): cice_transport_remap
followed by cice_step_ridge with mode 1 (the download kept) and mode 2 (the download deferred) against the same calls with
mode 0 on a context of its own, np.array_equal on every array cice_step_ridge is given.  The two unchained entries are held
to the compiled reference by test_gpu_transport.py and test_gpu_ridge.py.  Global 24 x 20 cells, cyclic east-west, as one
block, as 2 x 2 blocks of 12 x 10 (the transport's level-major layout is not the batch's there) and as 3 x 2 blocks of
10 x 10 with a padded last column of blocks; ntrcr = 1 and ntrcr = 4 of max_ntrcr = 5 tracer planes.
The state is built as fresh() of test_gpu_transport.py builds it, on synth.evp_state(cover="full") so that every block holds
ice; rdg_conv up to 1e-6 1/s on half of the cells, rdg_shear up to 2e-6 1/s, as scripts/ridge_cost.py has them."""
import functools

import numpy as np
import pytest

from cice4_amd import lib, synth
from test_gpu_ridge import _one_call_arrays

pytestmark = pytest.mark.gpu
DT = 3600.0
NXG, NYG = 24, 20
DECOMP = {"1block": (24, 20), "2x2": (12, 10), "3x2pad": (10, 10)}
SEVEN = ("aice0", "aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon")
TRC = {
    "ntr1": dict(ntrcr=1, trcr_depend=(0,), nt_Tsfc=1),
    "ntr4": dict(ntrcr=4, trcr_depend=(0, 1, 0, 1), nt_Tsfc=1, nt_iage=2, nt_alvl=3, nt_vlvl=4, tr_iage=True, tr_lvl=True),
}
GRID_T = ("HTN", "HTE", "dxt", "dyt", "dxu", "dyu", "tarear", "hm")


def _context(decomp, trc, itd_trc=None, batch=True, evp=False):
    ctx = lib.Context()
    ctx.sync()
    dom = ctx.domain_create(NXG, NYG, *DECOMP[decomp], ew=1, ns=0)
    grid = synth.block_fields(synth.global_grid(NXG, NYG, perturb=0.1, land_frac=0.05), dom)
    if evp:
        ctx.evp_init(grid, ndte=120)
    ctx.transport_init({k: grid[k] for k in GRID_T}, ntrcr=TRC[trc]["ntrcr"], trcr_depend=TRC[trc]["trcr_depend"])
    ctx.itd_init(synth.hin_max(), **TRC[itd_trc or trc])
    ctx.ridge_init(krdg_partic=1, krdg_redist=1, mu_rdg=4.0)
    if batch:
        ctx.thermo_batch_alloc(ctx.nx, ctx.ny, ctx.nblocks)
    return ctx, dom, grid


def _physical(dom, grid):
    """the physical tmask cells, (nb, ny, nx) bool"""
    m = np.zeros(grid["tmask"].shape, bool)
    for b in range(dom["nblocks"]):
        m[b, dom["jlo"][b] - 1:dom["jhi"][b], dom["ilo"][b] - 1:dom["ihi"][b]] = True
    return m & (grid["tmask"] != 0)


def _inputs(dom, grid):
    """s: the arrays of evp(dt); ts: those of transport_remap (aicen, vicen, uvel, vvel are s's); a: those of step_ridge,
    the seven state arrays of ts among them -- the same objects, the hand-over goes by their addresses"""
    s = synth.evp_state(grid, dom, cover="full")
    nb, ncat, ny, nx = s["aicen"].shape
    an, vn = s["aicen"], s["vicen"]
    ts = dict(aicen=an, vicen=vn, uvel=s["uvel"], vvel=s["vvel"])
    ts["vsnon"] = np.ascontiguousarray(0.2 * an)
    tr = np.zeros((nb, ncat, 5, ny, nx))
    tr[:, :, 0] = -5.0 - 3.0 * np.arange(ncat)[None, :, None, None]
    tr[:, :, 1] = 10.0
    tr[:, :, 2] = 0.7
    tr[:, :, 3] = 0.6
    tr[:, :, 4] = 123.0                  # (never a tracer in use here)
    ts["trcrn"] = tr
    ts["eicen"] = np.ascontiguousarray(np.repeat(vn, 4, axis=1) * (-7.5e7) * (1.0 + 0.1 * np.arange(ncat * 4) % 4)[None, :, None, None])
    ts["esnon"] = np.ascontiguousarray(ts["vsnon"] * (-1.1e8))
    ts["aice0"] = np.ascontiguousarray(1.0 - an.sum(axis=1))
    rng = np.random.default_rng(107)
    shp = (nb, ny, nx)
    x = {k: ts[k] for k in SEVEN}
    x["tmask"] = np.ascontiguousarray(grid["tmask"], np.int32)
    x["rdg_conv"] = np.where(rng.random(shp) < 0.5, rng.uniform(0.0, 1.0e-6, shp), 0.0)
    x["rdg_shear"] = rng.uniform(0.0, 2.0e-6, shp)
    for k in ("dardg1dt", "dardg2dt", "dvirdgdt", "opening"):
        x[k] = np.zeros(shp)
    x["fresh"], x["fhocn"] = rng.uniform(0.0, 1.0e-5, shp), rng.uniform(-1.0, 0.0, shp)
    a = _one_call_arrays(x)
    for k in SEVEN:
        a[k] = ts[k]
    return s, ts, a


def _snap(d):
    return {k: v.copy() for k, v in d.items() if isinstance(v, np.ndarray)}


def _same(got, want, where, ntr=None):
    assert set(got) == set(want), where
    for k in want:
        g, w = got[k], want[k]
        if k == "trcr" and ntr is not None:
            g, w = g[:, :ntr], w[:, :ntr]
        assert np.array_equal(g, w, equal_nan=True), (where, k, int((g != w).sum()))


@functools.lru_cache(maxsize=None)
def _plain(decomp, trc, itd_trc=None, change=False):
    """mode 0 on a context of its own: the inputs, the seven arrays after the transport, everything after ridging.  With
    `change`, vsnon of one ice cell is half as much again between the two calls (what the flush tests do)."""
    ctx, dom, grid = _context(decomp, trc, itd_trc)
    try:
        s, ts, a = _inputs(dom, grid)
        before = _snap(a)
        ctx.ridge_chain(0)
        assert ctx.transport_remap(DT, ts) == (0, 0, 0)
        mid = _snap({k: ts[k] for k in SEVEN})
        assert not np.array_equal(mid["aicen"], before["aicen"])
        if change:
            _change(ts, _cell(dom, grid, mid))
        r = ctx.step_ridge(DT, a, bound=True)
        assert r["l_stop"] == 0 and r["stage"] == 0, r
        assert not np.array_equal(a["aicen"], mid["aicen"])
        phys = _physical(dom, grid)
        for b in range(dom["nblocks"]):
            if phys[b].any():
                assert (a["dardg1dt"][b][phys[b]] != 0.0).any(), ("no ridging in block", b)
        return before, mid, _snap(a)
    finally:
        ctx.close()


def _cell(dom, grid, mid):
    """(block, category, j, i) of the physical tmask cell with the most snow after the transport"""
    v = np.where(_physical(dom, grid)[:, None], mid["vsnon"], 0.0)
    assert v.max() > 0.0
    return np.unravel_index(np.argmax(v), v.shape)


def _change(ts, cell):
    ts["vsnon"][cell] *= 1.5


def _ntr(trc):
    return TRC[trc]["ntrcr"]


@pytest.mark.parametrize("trc", tuple(TRC))
@pytest.mark.parametrize("decomp", tuple(DECOMP))
@pytest.mark.parametrize("mode", (1, 2))
def test_one_step_chained_equals_unchained(mode, decomp, trc):
    before, mid, want = _plain(decomp, trc)
    ctx, dom, grid = _context(decomp, trc)
    try:
        s, ts, a = _inputs(dom, grid)
        ctx.ridge_chain(mode)
        assert ctx.transport_remap(DT, ts) == (0, 0, 0)
        _same({k: ts[k] for k in SEVEN}, {k: (mid if mode == 1 else before)[k] for k in SEVEN}, ("after the transport", mode))
        r = ctx.step_ridge(DT, a, bound=True)
        assert r["l_stop"] == 0 and r["stage"] == 0, r
        _same(a, want, (mode, decomp, trc), _ntr(trc))
    finally:
        ctx.close()


def test_two_steps_of_evp_transport_ridge_with_both_chains():
    """evp -> transport_remap -> step_ridge twice on 2 x 2 blocks: cice_transport_chain and cice_ridge_chain(2) together =
    the plain sequence"""
    def run(chained):
        ctx, dom, grid = _context("2x2", "ntr4", evp=True)
        try:
            s, ts, a = _inputs(dom, grid)
            if chained:
                ctx.transport_chain(ts)
                ctx.ridge_chain(2)
            for _ in range(2):
                ctx.evp(DT, s)
                assert ctx.transport_remap(DT, ts) == (0, 0, 0)
                assert ctx.step_ridge(DT, a, bound=True)["l_stop"] == 0
                for k in ("aice", "vice", "vsno", "aice0"):      # the aggregates the next evp reads
                    s[k][...] = a[k]
            return _snap(s), _snap(a)
        finally:
            ctx.close()

    s0, a0 = run(False)
    s1, a1 = run(True)
    assert np.abs(s0["uvel"]).max() > 0.01
    _same(a1, a0, "two steps, ridging", 4)
    _same(s1, s0, "two steps, dynamics")


def test_mode_1_reads_the_device_copy_not_the_host_arrays():
    before, mid, want = _plain("2x2", "ntr4")
    ctx, dom, grid = _context("2x2", "ntr4")
    try:
        s, ts, a = _inputs(dom, grid)
        ctx.ridge_chain(1)
        assert ctx.transport_remap(DT, ts) == (0, 0, 0)
        _same({k: ts[k] for k in SEVEN}, mid, "mode 1 downloads")
        ts["eicen"][...] = np.nan        # against the contract: nothing writes to the arrays between the two calls
        ts["vsnon"][...] = np.nan
        assert ctx.step_ridge(DT, a, bound=True)["l_stop"] == 0
        _same(a, want, "mode 1, host arrays spoilt", 4)
    finally:
        ctx.close()


def test_mode_2_downloads_once_at_the_end():
    before, mid, want = _plain("3x2pad", "ntr4")
    ctx, dom, grid = _context("3x2pad", "ntr4")
    try:
        s, ts, a = _inputs(dom, grid)
        ctx.ridge_chain(2)
        assert ctx.transport_remap(DT, ts) == (0, 0, 0)
        _same({k: ts[k] for k in SEVEN}, {k: before[k] for k in SEVEN}, "mode 2: no download by the transport")
        assert ctx.step_ridge(DT, a, bound=True)["l_stop"] == 0
        _same(a, want, "mode 2: the final state", 4)
    finally:
        ctx.close()


@pytest.mark.parametrize("flush", ("explicit", "halo", "sync"))
def test_a_deferred_state_is_flushed_and_the_next_step_ridge_uploads(flush):
    before, mid, clean = _plain("2x2", "ntr4")
    want = _plain("2x2", "ntr4", None, True)[2]
    ctx, dom, grid = _context("2x2", "ntr4")
    try:
        s, ts, a = _inputs(dom, grid)
        ctx.ridge_chain(2)
        assert ctx.transport_remap(DT, ts) == (0, 0, 0)
        assert np.array_equal(ts["aicen"], before["aicen"])
        if flush == "explicit":
            ctx.transport_download_state()
        elif flush == "halo":
            other = np.zeros((dom["nblocks"], 1, dom["ny"], dom["nx"]))
            ctx.halo_update_blocked(other)
        else:
            ctx.sync()
        _same({k: ts[k] for k in SEVEN}, mid, ("flushed", flush))
        cell = _cell(dom, grid, mid)
        _change(ts, cell)
        assert ctx.step_ridge(DT, a, bound=True)["l_stop"] == 0
        _same(a, want, ("uploaded after the flush", flush), 4)
        assert not np.array_equal(a["vsnon"], clean["vsnon"])
        ctx.transport_download_state()   # nothing pending: no effect
        _same(a, want, "second flush", 4)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", (1, 2))
def test_not_armed_another_pointer(mode):
    """the transport call arms, step_ridge is given a copy of aicen: it ends the hand-over (mode 2: the transport's result
    reaches the arrays that call was given) and uploads"""
    before, mid, want = _plain("2x2", "ntr1")
    ctx, dom, grid = _context("2x2", "ntr1")
    try:
        s, ts, a = _inputs(dom, grid)
        ctx.ridge_chain(mode)
        assert ctx.transport_remap(DT, ts) == (0, 0, 0)
        a["aicen"] = mid["aicen"].copy()   # what a caller who keeps a second array would hold
        assert ctx.step_ridge(DT, a, bound=True)["l_stop"] == 0
        assert np.array_equal(ts["aicen"], mid["aicen"])   # the transport's download, in the array it was given
        _same(a, want, ("other pointer", mode), 1)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", (1, 2))
def test_not_armed_no_batch_at_transport_time(mode):
    before, mid, want = _plain("2x2", "ntr1")
    ctx, dom, grid = _context("2x2", "ntr1", batch=False)
    try:
        s, ts, a = _inputs(dom, grid)
        ctx.ridge_chain(mode)
        assert ctx.transport_remap(DT, ts) == (0, 0, 0)
        _same({k: ts[k] for k in SEVEN}, mid, ("downloaded as always", mode))
        ctx.thermo_batch_alloc(ctx.nx, ctx.ny, ctx.nblocks)
        assert ctx.step_ridge(DT, a, bound=True)["l_stop"] == 0
        _same(a, want, ("no batch", mode), 1)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", (1, 2))
def test_not_armed_other_tracers_in_itd_init(mode):
    before, mid, want = _plain("2x2", "ntr1", "ntr4")
    ctx, dom, grid = _context("2x2", "ntr1", itd_trc="ntr4")
    try:
        s, ts, a = _inputs(dom, grid)
        ctx.ridge_chain(mode)
        assert ctx.transport_remap(DT, ts) == (0, 0, 0)
        _same({k: ts[k] for k in SEVEN}, mid, ("downloaded as always", mode))
        assert ctx.step_ridge(DT, a, bound=True)["l_stop"] == 0
        _same(a, want, ("other tracers", mode), 4)
    finally:
        ctx.close()


def test_not_armed_a_transport_call_that_stops():
    """departure points out of bounds: the call downloads in every mode and arms nothing; then a good step from fresh
    values in the same arrays"""
    before, mid, want = _plain("2x2", "ntr1")

    def run(mode):
        ctx, dom, grid = _context("2x2", "ntr1")
        try:
            s, ts, a = _inputs(dom, grid)
            ctx.ridge_chain(mode)
            jj, ii = np.nonzero(_physical(dom, grid)[1])
            ts["uvel"][1, jj[5], ii[5]] = 100.0
            stop = ctx.transport_remap(DT, ts)
            failed = _snap({k: ts[k] for k in SEVEN})
            ctx.transport_download_state()           # nothing is pending
            _same({k: ts[k] for k in SEVEN}, failed, ("nothing pending after a stop", mode))
            s2, ts2, a2 = _inputs(dom, grid)
            for k in ts:
                ts[k][...] = ts2[k]
            for k in a:
                a[k][...] = a2[k]
            assert ctx.transport_remap(DT, ts) == (0, 0, 0)
            assert ctx.step_ridge(DT, a, bound=True)["l_stop"] == 0
            _same(a, want, ("a good step after the stop", mode), 1)
            return stop, failed
        finally:
            ctx.close()

    stop0, failed0 = run(0)
    assert stop0[0] != 0, stop0
    for mode in (1, 2):
        stop, failed = run(mode)
        assert stop == stop0
        _same(failed, failed0, ("a stopped transport call downloads", mode))


def test_ridging_stop_in_block_2_of_4_in_mode_2():
    """rdg_conv < 0 in the two cells of the second block that the transport leaves with the least open water (as
    test_one_call_stop_in_block_2_of_4 of test_gpu_ridge.py has it; there the cells are given no open water, here the
    state comes out of the transport, so rdg_conv is -1e-3 1/s): the same report, and the host arrays of ALL four blocks as
    mode 0 leaves them -- the blocks behind the failing one hold the transport's result, which the host had not seen"""
    _, mid, _ = _plain("2x2", "ntr1")

    def run(mode):
        ctx, dom, grid = _context("2x2", "ntr1")
        try:
            s, ts, a = _inputs(dom, grid)
            open_water = np.where(_physical(dom, grid)[1], mid["aice0"][1], 2.0)
            flat = np.sort(np.argsort(open_water, axis=None)[:2])          # (list order: j, then i)
            cells = [tuple(int(x) for x in np.unravel_index(q, open_water.shape)) for q in flat]
            assert open_water[cells[0]] < 0.1 and open_water[cells[1]] < 0.1
            for j, i in cells:           # the new aice0 is far below -puny
                a["rdg_conv"][1, j, i], a["rdg_shear"][1, j, i] = -1.0e-3, 0.0
            ctx.ridge_chain(mode)
            assert ctx.transport_remap(DT, ts) == (0, 0, 0)
            r = ctx.step_ridge(DT, a, bound=True)
            return r, _snap(a), cells
        finally:
            ctx.close()

    r0, a0, cells = run(0)
    # (which of the two is named: a cell whose total area the transport left above 1 has its closing raised to make up for
    # that, ridge_prep, and does not fail)
    assert (r0["l_stop"], r0["stage"], r0["bstop"]) == (1, 1, 2), r0
    assert (r0["jstop"] - 1, r0["istop"] - 1) in cells, (r0, cells)
    assert np.array_equal(a0["aicen"][2:], mid["aicen"][2:]) and not np.array_equal(a0["aicen"][0], mid["aicen"][0])
    r2, a2, _ = run(2)
    assert r2 == r0
    _same(a2, a0, "a ridging stop in mode 2")
