"""The second half of step_therm2 on the device (cice_cleanup_itd, cice_aggregate, cice_step_therm2_cleanup) against what
the compiled reference recorded in tests/golden/cleanup_itd.npz: every block of every case, every output array, ghost
cells included, BIT FOR BIT -- there is no exp / pow on this path."""
import numpy as np
import pytest

import cleanup_itd_case as cc
import therm_itd_case as tc
from cice4_amd import lib, synth

pytestmark = pytest.mark.gpu
BOX = (cc.ILO, cc.IHI, cc.JLO, cc.JHI)
ONE_CALL_OUT = cc.STATE + cc.OUT_AGG + cc.FLUX + ("daidtt", "dvidtt")


@pytest.fixture(scope="module")
def gold():
    d = np.load(cc.FIXTURE)
    return {name: cc.load_case(d, name) for name in cc.ORDINARY}, d


@pytest.fixture(scope="module")
def dev():
    c = lib.Context()
    c.sync()
    yield c
    c.close()


def _bitwise(got, want, names, where):
    for k in names:
        g, w = cc.bits(got[k]), cc.bits(want[k])
        assert g.shape == w.shape and np.array_equal(g, w), (where, k, int((g != w).sum()))


def _block(s, b, names=None):
    """copies of block b of the named arrays (tc.block hands out views where it can)"""
    return {k: v.copy() for k, v in tc.block(s, b, names).items()}


def _agg_arrays(shape2, lead=()):
    z = lambda *s: np.zeros(lead + s + shape2)
    return dict(aice=z(), aice0=z(), vice=z(), vsno=z(), eice=z(), esno=z(), trcr=z(5))


def _clean_block(dev, blk, box=BOX):
    """cice_cleanup_itd on a block; aice, aice0 go in as a value the entry has to overwrite on every cell"""
    blk["aice"] = np.full(blk["fresh"].shape, -7.0)
    blk["aice0"] = np.full(blk["fresh"].shape, -7.0)
    return dev.cleanup_itd(*box, cc.DT, blk)


def _blockwise(dev, s, box=None):
    """the two block-wise entries on every block of s: (what cleanup_itd left, what aggregate made of it)"""
    nb, ny, nx = s["fresh"].shape
    box = box or (2, nx - 1, 2, ny - 1)
    out = {k: v.copy() for k, v in s.items()}
    out["aice"], out["aice0"] = np.zeros((nb, ny, nx)), np.zeros((nb, ny, nx))
    agg = _agg_arrays((ny, nx), (nb,))
    for b in range(nb):
        blk = _block(out, b)
        assert _clean_block(dev, blk, box) == (0, 0, 0), b
        for k in cc.OUT_CLEAN:
            out[k][b] = blk[k]
        ab = dict(_block(out, b, cc.STATE + ("tmask",)), **_block(agg, b))
        dev.aggregate(ab)
        for k in cc.OUT_AGG:
            agg[k][b] = ab[k]
    return out, agg


def _one_call_arrays(s):
    nb, ny, nx = s["fresh"].shape
    a = {k: v.copy() for k, v in s.items()}
    a.update({k: np.full(v.shape, -7.0) for k, v in _agg_arrays((ny, nx), (nb,)).items()})
    a["trcr"][:, 1:] = 0.0
    return a


def _expected(s, out, agg):
    e = {k: out[k] for k in cc.STATE + cc.FLUX}
    e.update(agg)
    e["daidtt"], e["dvidtt"] = cc.tendencies(s, agg)
    return e


def _trcr_planes(a, e, ntr):
    """trcr beyond the tracers in use is not written: compared on the planes in use only"""
    return dict(a, trcr=a["trcr"][:, :ntr]), dict(e, trcr=e["trcr"][:, :ntr])


@pytest.mark.parametrize("name", cc.ORDINARY)
def test_blockwise_entries_reproduce_the_reference(dev, gold, name):
    s, out, agg = gold[0][name]
    ntr = cc.ntrcr(name)
    quiet = [int(b) for b in gold[1][f"{name}_quiet"]]
    dev.itd_init(**cc.itd_kwargs(name))
    for b in range(cc.NB):
        blk = _block(s, b)
        assert _clean_block(dev, blk) == (0, 0, 0)
        _bitwise(blk, _block(out, b), cc.OUT_CLEAN, (name, "cleanup_itd", b))
        if b in quiet:
            assert tc.same(blk["trcrn"][:, :ntr], s["trcrn"][b][:, :ntr]), (name, "quiet block", b)
        ab = dict(_block(out, b, cc.STATE + ("tmask",)), **_agg_arrays((cc.NY, cc.NX)))
        keep = {k: ab[k].copy() for k in cc.STATE + ("tmask",)}
        dev.aggregate(ab)
        _bitwise(ab, _block(agg, b), cc.OUT_AGG, (name, "aggregate", b))
        _bitwise(ab, keep, cc.STATE, (name, "aggregate intent(in)", b))
        assert np.array_equal(ab["tmask"], keep["tmask"])
    assert quiet


def test_absent_fluxes_and_no_limit(dev, gold):
    """fresh / fsalt / fhocn absent: the state is the same and the arrays are not touched; limit_aice = F: no zap"""
    s, out, _ = gold[0]["ntr1"]
    dev.itd_init(**cc.itd_kwargs("ntr1"))
    blk = _block(s, 3)
    blk["aice"], blk["aice0"] = np.zeros((cc.NY, cc.NX)), np.zeros((cc.NY, cc.NX))
    assert dev.cleanup_itd(*BOX, cc.DT, blk, fluxes=()) == (0, 0, 0)
    _bitwise(blk, _block(out, 3), cc.STATE + ("aice", "aice0"), "no fluxes")
    _bitwise(blk, _block(s, 3), cc.FLUX, "no fluxes")
    blk = _block(s, 3)
    blk["aice"], blk["aice0"] = np.zeros((cc.NY, cc.NX)), np.zeros((cc.NY, cc.NX))
    assert dev.cleanup_itd(*BOX, cc.DT, blk, limit_aice=False) == (0, 0, 0)
    _bitwise(blk, _block(s, 3), ("aicen", "vicen", "eicen"), "limit_aice = F")     # block 4 has zaps only
    with pytest.raises(lib.CiceError):
        dev.cleanup_itd(*BOX, cc.DT, _block(out, 3), heat_capacity=False)


@pytest.mark.parametrize("which", cc.STOPS)
def test_stops(dev, gold, which):
    d = gold[1]
    dev.itd_init(**cc.itd_kwargs(which))
    blk, cell = cc.stop_inputs(which)
    assert cc.digest(blk) == str(d[f"{which}_sha256"])
    r = _clean_block(dev, blk)
    assert r == tuple(int(x) for x in d[f"{which}_stop"]) == (1,) + cell
    _bitwise(blk, {k: d[f"{which}_out_{k}"] for k in cc.OUT_CLEAN}, cc.OUT_CLEAN, which)


@pytest.mark.parametrize("name", cc.ORDINARY)
def test_one_call_from_host_state(dev, gold, name):
    """cice_step_therm2_cleanup, state_resident = 0, bound = 0, all four blocks: the fixture's final state"""
    s, out, agg = gold[0][name]
    dev.itd_init(**cc.itd_kwargs(name))
    dev.thermo_batch_alloc(cc.NX, cc.NY, cc.NB)
    a = _one_call_arrays(s)
    r = dev.step_therm2_cleanup(cc.DT, a)
    assert r["l_stop"] == 0 and r["stage"] == 0, r
    _bitwise(*_trcr_planes(a, _expected(s, out, agg), cc.ntrcr(name)), ONE_CALL_OUT, (name, "one call"))
    assert np.array_equal(a["tmask"], s["tmask"])


def test_one_call_stop_in_block_2_of_4(dev, gold):
    s, out, _ = gold[0]["ntr1"]
    dev.itd_init(**cc.itd_kwargs("ntr1"))
    dev.thermo_batch_alloc(cc.NX, cc.NY, cc.NB)
    s = {k: v.copy() for k, v in s.items()}
    jj, ii = np.nonzero(s["aicen"][1, 0, cc.JLO - 1:cc.JHI, cc.ILO - 1:cc.IHI] > 0.01)
    cells = [(int(jj[k]) + cc.JLO - 1, int(ii[k]) + cc.ILO - 1) for k in (0, len(jj) - 1)]
    for j, i in cells:
        s["aicen"][1, 0, j, i] += 1.1 - cc.cat_sum(s["aicen"][1][:, j:j + 1, i:i + 1])[0, 0]
    a = _one_call_arrays(s)
    a0 = {k: v.copy() for k, v in a.items()}
    r = dev.step_therm2_cleanup(cc.DT, a)
    assert (r["l_stop"], r["stage"], r["bstop"], r["istop"], r["jstop"]) == (1, 1, 2, cells[1][1] + 1, cells[1][0] + 1), r
    names = cc.STATE + cc.FLUX
    _bitwise({k: a[k][0] for k in names}, {k: out[k][0] for k in names}, names, "block 1: cleaned")
    blk = _block(s, 1)
    assert _clean_block(dev, blk) == (1, r["istop"], r["jstop"])
    _bitwise({k: a[k][1] for k in names}, blk, names, "block 2: as the block-wise entry leaves it")
    _bitwise({k: a[k][2:] for k in names}, {k: a0[k][2:] for k in names}, names, "blocks 3, 4: as they went in")
    _bitwise(a, a0, cc.OUT_AGG + ("daidtt", "dvidtt"), "outputs of stage 3")


def _capped(raw):
    """a synth.therm2_state with its areas brought to a sum <= 1 and the arrays of the one call"""
    s = {k: raw[k].copy() for k in cc.STATE + cc.FLUX + ("tmask",)}
    tot = cc.cat_sum(s["aicen"])
    f = np.where(tot > 1.0, 0.98 / np.where(tot > 1.0, tot, 1.0), 1.0)
    for k, per in (("aicen", 1), ("vicen", 1), ("vsnon", 1), ("eicen", cc.NILYR), ("esnon", cc.NSLYR)):
        s[k] = np.ascontiguousarray(s[k] * np.repeat(f[:, None], cc.NCAT * per, axis=1))
    rng = np.random.default_rng(5)
    s["daidtt"], s["dvidtt"] = rng.uniform(0, 1, tot.shape), rng.uniform(0, 3, tot.shape)
    return s


@pytest.mark.parametrize("shape", [(64, 5), (66, 5), (67, 4)])
def test_other_block_shapes_agree_with_blockwise(dev, shape):
    """a memory row of exactly one wavefront, one less and one more physical cell per row: the one call = the block-wise
    entries; the raw synthetic state holds categories that the column physics pushed out of their bounds"""
    nxb, nyb = shape
    dev.itd_init(**tc.itd_kwargs(tc.CASES["tracers"]))
    s = _capped(synth.therm2_state("mixed", nxb, nyb, 2, seed=177 + nxb, ntrcr=4))
    out, agg = _blockwise(dev, s)
    assert not tc.same(out["aicen"], s["aicen"])
    dev.thermo_batch_alloc(nxb, nyb, 2)
    a = _one_call_arrays(s)
    assert dev.step_therm2_cleanup(cc.DT, a)["l_stop"] == 0
    _bitwise(*_trcr_planes(a, _expected(s, out, agg), 4), ONE_CALL_OUT, shape)


def test_resident_chain_behind_step_therm1_and_the_first_half(dev):
    """cice_step_therm1 -> cice_step_therm2_itd(state_resident = 1) -> cice_step_therm2_cleanup(state_resident = 1) on one
    context = the block-wise entries applied to what the first call downloaded"""
    from test_gpu_thermo import _batch_inputs, DT
    from test_gpu_therm_itd import _blockwise as first_half_blockwise, _after_rain_and_aggregate
    assert DT == cc.DT
    ny, nx, nb = 12, 14, 2
    dev.thermo_init()
    dev.itd_init(**tc.itd_kwargs(tc.CASES["growth"]))
    batch, _ = _batch_inputs(ny, nx, nb, seed=35)
    for k in ("aicen", "vicen", "vsnon", "eicen", "esnon"):
        batch[k] *= 0.125                    # five independent areas of up to 0.95 each: a sum under 1, thicknesses as they were
    thick = (np.add.outer(np.arange(ny), np.arange(nx)) % 3 == 0)[None]     # category 2 at four times its thickness in a third of
    batch["vicen"][:, 1] *= np.where(thick, 4.0, 1.0)                          # the cells: linear_itd gives up on it, rebin moves it
    batch["eicen"][:, cc.NILYR:2 * cc.NILYR] *= np.where(thick, 4.0, 1.0)[:, None]
    rng = np.random.default_rng(6)
    U = lambda lo, hi: np.ascontiguousarray(rng.uniform(lo, hi, (nb, ny, nx)))
    aice = np.ascontiguousarray(batch["aicen"].sum(axis=1))
    fz = dict(aice=aice, frzmlt=U(-40, 60), Tf=np.full((nb, ny, nx), -1.8), strocnxT=U(-0.2, 0.2), strocnyT=U(-0.2, 0.2))
    fz["sst"] = fz["Tf"] + U(0, 0.5)
    pc = {k: np.ascontiguousarray(rng.uniform(-1, 1, batch["aicen"].shape)) for k in ("strairxn", "strairyn", "Trefn", "Qrefn")}
    acc = {k: U(-1, 1) for k in lib.MERGE_ORDER}
    st = {k: v.copy() for k, v in batch.items()}
    dev.thermo_batch_alloc(nx, ny, nb)
    tmask = np.ones((nb, ny, nx), np.int32)
    cl = dict(tmask=tmask, daidtt=U(0, 1), dvidtt=U(0, 3))
    with pytest.raises(lib.CiceError):       # nothing has left a full state on this batch yet
        dev.step_therm2_cleanup(cc.DT, _one_call_arrays(dict({k: st[k] for k in cc.STATE}, fresh=U(0, 1), fsalt=U(0, 1),
                                                               fhocn=U(0, 1), **cl)), state_resident=True)
    assert dev.step_therm1(DT, tc.YDAY, st, fz, pc, acc)["l_stop"] == 0
    ice = st["aicen"].sum(axis=1) > tc.PUNY
    rside = np.ascontiguousarray(np.where(ice & (fz["frzmlt"] < 0), U(0.005, 0.05), 0.0))
    a = dict({k: st[k].copy() for k in tc.STATE}, aicen_init=batch["aicen"].copy(), vicen_init=batch["vicen"].copy(),
             frain=U(0, 1e-5), frzmlt=fz["frzmlt"].copy(), Tf=fz["Tf"].copy(), rside=rside, tmask=tmask, aice=aice.copy(),
             aice0=np.maximum(1 - aice, 0), fresh=U(0, 1e-5), fsalt=U(0, 1e-7), fhocn=U(-5, 0), frazil=np.zeros((nb, ny, nx)),
             meltl=np.zeros((nb, ny, nx)), frz_onset=np.zeros((nb, ny, nx)))
    raw = {k: v.copy() for k, v in a.items()}
    res = {k: v for k, v in a.items() if k != "aicen_init"}
    assert dev.step_therm2_itd(tc.DT, tc.YDAY, res, state_resident=True)["l_stop"] == 0
    b = _one_call_arrays(dict({k: res[k] for k in cc.STATE + cc.FLUX}, **cl))
    assert dev.step_therm2_cleanup(cc.DT, b, state_resident=True)["l_stop"] == 0
    chain, _ = first_half_blockwise(dev, _after_rain_and_aggregate(raw))
    s = dict({k: chain[3][k] for k in cc.STATE + cc.FLUX}, **cl)
    out, agg = _blockwise(dev, s)
    _bitwise(*_trcr_planes(b, _expected(s, out, agg), 1), ONE_CALL_OUT, "resident chain")
    assert not tc.same(out["aicen"], s["aicen"])


@pytest.mark.parametrize("name", ("ntr1", "ntr4"))
def test_bound_state_on_the_contexts_domain(gold, name):
    """bound = 1 on 2 x 2 blocks, cyclic east-west = block-wise cleanup_itd, the context's host-array halo entries on the six
    arrays (tracer section 1:ntrcr), block-wise aggregate"""
    s, out, _ = gold[0][name]
    ntr = cc.ntrcr(name)
    c = lib.Context()
    try:
        c.domain_create(24, 20, 12, 10, ew=1, ns=0)
        assert (c.nx, c.ny, c.nblocks) == (cc.NX, cc.NY, cc.NB)
        c.itd_init(**cc.itd_kwargs(name))
        c.thermo_batch_alloc(cc.NX, cc.NY, cc.NB)
        a = _one_call_arrays(s)
        assert c.step_therm2_cleanup(cc.DT, a, bound=True)["l_stop"] == 0
        e = {k: out[k].copy() for k in cc.STATE + cc.FLUX + ("tmask",)}
        for k in ("aicen", "vicen", "vsnon", "eicen", "esnon"):
            c.halo_update_blocked(e[k])
        c.halo_update_strided(e["trcrn"][:, :, 0:ntr])
        assert not tc.same(e["aicen"], out["aicen"])
        agg = _agg_arrays((cc.NY, cc.NX), (cc.NB,))
        for b in range(cc.NB):
            ab = dict(_block(e, b, cc.STATE + ("tmask",)), **_block(agg, b))
            c.aggregate(ab)
            for k in cc.OUT_AGG:
                agg[k][b] = ab[k]
        _bitwise(*_trcr_planes(a, _expected(s, e, agg), ntr), ONE_CALL_OUT, (name, "bound = 1"))
    finally:
        c.close()


def test_bound_without_a_domain_is_refused(dev, gold):
    s, _, _ = gold[0]["ntr1"]
    dev.itd_init(**cc.itd_kwargs("ntr1"))
    dev.thermo_batch_alloc(cc.NX, cc.NY, cc.NB)
    with pytest.raises(lib.CiceError):
        dev.step_therm2_cleanup(cc.DT, _one_call_arrays(s), bound=True)
