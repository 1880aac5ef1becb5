"""Ridging on the device (cice_ridge_ice, cice_step_ridge) against what the compiled reference recorded in
tests/golden/ridge.npz: every block of every case, every output array, ghost and land cells included, BIT FOR BIT on a
host whose libm is the restated one (conftest.TOL_EXP = 0: ridge_itd and ridge_shift call exp), else to TOL_EXP."""
import numpy as np
import pytest

import cleanup_itd_case as cc
import ridge_case as rc
import therm_itd_case as tc
from conftest import relerr, TOL_EXP
from cice4_amd import lib

pytestmark = pytest.mark.gpu
BLOCK_IN = rc.STATE + ("aice0", "rdg_conv", "rdg_shear", "tmask") + rc.OPTIONAL
ONE_CALL_OUT = rc.STATE + rc.DIAG + cc.OUT_AGG + cc.FLUX + ("daidtd", "dvidtd")


@pytest.fixture(scope="module")
def gold():
    d = np.load(rc.FIXTURE)
    return {name: rc.load_case(d, name) for name in rc.ORDINARY}, d


@pytest.fixture(scope="module")
def dev():
    c = lib.Context()
    c.sync()
    yield c
    c.close()


def _init(dev, name):
    dev.itd_init(**rc.itd_kwargs(name))
    dev.ridge_init(**rc.ridge_kwargs(name))


def _agree(got, want, names, where):
    for k in names:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (where, k)
        if TOL_EXP == 0.0:
            ne = cc.bits(g) != cc.bits(w)
            assert not ne.any(), (where, k, int(ne.sum()))
        else:
            assert relerr(g, w) <= TOL_EXP, (where, k)


def _bitwise(got, want, names, where):
    for k in names:
        assert tc.same(got[k], want[k]), (where, k)


def _block(s, b, names=BLOCK_IN):
    return {k: v.copy() for k, v in tc.block(s, b, names).items()}


def _ridge_blocks(dev, s):
    """cice_ridge_ice on every block of s that has a tmask cell: what it left, the iterations"""
    out = {k: v.copy() for k, v in s.items()}
    nb = s["aice0"].shape[0]
    niter = np.zeros(nb, np.int32)
    for b in range(nb):
        lst = rc.tmask_list(s["tmask"][b])
        if lst[0] == 0:
            continue
        blk = _block(out, b)
        r = dev.ridge_ice(*lst, rc.DT, blk)
        assert r[:3] == (0, 0, 0), (b, r)
        niter[b] = r[3]
        for k in rc.OUT:
            out[k][b] = blk[k]
    return out, niter


@pytest.mark.parametrize("name", rc.ORDINARY)
def test_blockwise_entry_reproduces_the_reference(dev, gold, name):
    s, out, niter = gold[0][name]
    _init(dev, name)
    for b in range(rc.NB):
        lst = rc.tmask_list(s["tmask"][b])
        blk = _block(s, b)
        r = dev.ridge_ice(*lst, rc.DT, blk)
        assert r[:3] == (0, 0, 0), (name, b, r)
        _agree(blk, _block(out, b), rc.OUT, (name, b))
        if TOL_EXP == 0.0:
            assert r[3] == niter[b], (name, b, r[3], int(niter[b]))
        _bitwise(blk, _block(s, b), rc.IN_ONLY, (name, "intent(in)", b))
        assert np.array_equal(blk["tmask"], s["tmask"][b])
        if lst[0] == 0:                  # never called in the reference: nothing moves, the tracers of land stay
            _bitwise(blk, _block(s, b), rc.OUT, (name, "no list", b))
            assert r[3] == 0


def test_absent_optionals(dev, gold):
    """none of the six, and two of them: the state is the same, an absent array is not touched"""
    s, out, _ = gold[0]["ntr4"]
    _init(dev, "ntr4")
    b = 1
    lst = rc.tmask_list(s["tmask"][b])
    for given in ((), ("dardg2dt", "fhocn")):
        blk = _block(s, b)
        assert dev.ridge_ice(*lst, rc.DT, blk, optionals=given)[:3] == (0, 0, 0)
        _agree(blk, _block(out, b), rc.STATE + ("aice0",) + given, ("optionals", given))
        _bitwise(blk, _block(s, b), tuple(k for k in rc.OPTIONAL if k not in given), ("absent", given))


def test_stop_aice0_names_the_first_cell_and_leaves_the_second(dev, gold):
    d = gold[1]
    _init(dev, rc.STOP)
    blk, cells = rc.stop_inputs()
    assert rc.digest(blk) == str(d[f"{rc.STOP}_sha256"])
    before = {k: v.copy() for k, v in blk.items()}
    r = dev.ridge_ice(*rc.tmask_list(blk["tmask"]), rc.DT, blk)
    assert r[:3] == tuple(int(x) for x in d[f"{rc.STOP}_stop"]) == (1,) + cells[0]
    assert r[3] == int(d[f"{rc.STOP}_niter"])
    _agree(blk, {k: d[f"{rc.STOP}_out_{k}"] for k in rc.OUT}, rc.OUT, rc.STOP)
    (i1, j1), (i2, j2) = cells
    assert blk["aice0"][j1 - 1, i1 - 1] < -rc.PUNY
    assert tc.same(blk["aice0"][j2 - 1, i2 - 1], before["aice0"][j2 - 1, i2 - 1])
    _bitwise(blk, before, rc.OPTIONAL, "the diagnostics and fluxes of a stopped call")


def test_krdg_redist_0_is_unsupported(dev):
    dev.itd_init(**rc.itd_kwargs("ntr1"))
    with pytest.raises(lib.CiceError, match="error -4"):
        dev.ridge_init(krdg_partic=1, krdg_redist=0, mu_rdg=rc.MU_RDG)


@pytest.mark.parametrize("nxp", (63, 64, 65))
def test_a_block_padded_with_land_gives_the_same_bits(dev, gold, nxp):
    """blocks 3 (three iterations) and 4 (thin ice) of the tracer case inside blocks of 63, 64, 65 columns whose other
    cells are land: the same cells share a repeat flag, every cell comes out as in the fixture"""
    s, out, niter = gold[0]["ntr4"]
    _init(dev, "ntr4")
    for b, off in ((2, nxp - rc.NX), (3, 17)):
        icells, ii, jj = rc.tmask_list(s["tmask"][b])
        blk = {}
        for k in BLOCK_IN:
            src = s[k][b]
            big = np.zeros(src.shape[:-1] + (nxp,), src.dtype)
            if k == "trcrn":
                big[:, 0] = rc.TOCNFRZ
            big[..., off:off + rc.NX] = src
            blk[k] = np.ascontiguousarray(big)
        indxi = np.zeros(nxp * rc.NY, np.int32)
        indxj = np.zeros(nxp * rc.NY, np.int32)
        indxi[:icells], indxj[:icells] = ii[:icells] + off, jj[:icells]
        r = dev.ridge_ice(icells, indxi, indxj, rc.DT, blk)
        assert r[:3] == (0, 0, 0)
        if TOL_EXP == 0.0:
            assert r[3] == niter[b]
        _agree({k: blk[k][..., off:off + rc.NX] for k in rc.OUT}, _block(out, b, rc.OUT), rc.OUT, (nxp, b))
        pad = np.ones(nxp, bool)
        pad[off:off + rc.NX] = False
        assert (blk["trcrn"][:, :4][..., pad] == 0.0).all() and (blk["trcrn"][:, 4][..., pad] == 0.0).all()
        assert (blk["aicen"][..., pad] == 0.0).all() and (blk["aice0"][..., pad] == 0.0).all()


def _one_call_arrays(s, seed=11):
    nb, ny, nx = s["aice0"].shape
    rng = np.random.default_rng(seed)
    a = {k: s[k].copy() for k in BLOCK_IN}
    a["fsalt"] = rng.uniform(0.0, 1.0e-7, (nb, ny, nx))
    a["daidtd"], a["dvidtd"] = rng.uniform(0.0, 1.0, (nb, ny, nx)), rng.uniform(0.0, 3.0, (nb, ny, nx))
    for k in ("aice", "vice", "vsno", "eice", "esno"):
        a[k] = np.full((nb, ny, nx), -7.0)
    a["trcr"] = np.full((nb, 5, ny, nx), -7.0)
    a["trcr"][:, 1:] = 0.0
    return a


def _expected(dev, a, halo=None):
    """the block-wise entries one after the other: ridge_ice, cleanup_itd, [the halo update,] aggregate, the tendencies"""
    from test_gpu_cleanup_itd import _agg_arrays, _blockwise, _clean_block
    nb, ny, nx = a["aice0"].shape
    r, _ = _ridge_blocks(dev, {k: a[k] for k in BLOCK_IN})
    s2 = dict({k: r[k] for k in rc.STATE + ("fresh", "fhocn", "tmask")}, fsalt=a["fsalt"])
    if halo is None:
        out, agg = _blockwise(dev, s2)
    else:
        out = {k: v.copy() for k, v in s2.items()}
        for b in range(nb):
            blk = {k: v.copy() for k, v in tc.block(out, b).items()}
            assert _clean_block(dev, blk) == (0, 0, 0)
            for k in cc.STATE + cc.FLUX:
                out[k][b] = blk[k]
        halo(out)
        agg = _agg_arrays((ny, nx), (nb,))
        for b in range(nb):
            ab = {k: v.copy() for k, v in dict(tc.block(out, b, cc.STATE + ("tmask",)), **tc.block(agg, b)).items()}
            dev.aggregate(ab)
            for k in cc.OUT_AGG:
                agg[k][b] = ab[k]
    e = {k: out[k] for k in cc.STATE + cc.FLUX}
    e.update(agg)
    e.update({k: r[k] for k in rc.DIAG})
    e["daidtd"], e["dvidtd"] = (agg["aice"] - a["daidtd"]) / rc.DT, (agg["vice"] - a["dvidtd"]) / rc.DT
    return e


def _planes(a, e, ntr):
    return dict(a, trcr=a["trcr"][:, :ntr]), dict(e, trcr=e["trcr"][:, :ntr])


@pytest.mark.parametrize("name", ("ntr1", "ntr4"))
def test_one_call_equals_the_blockwise_entries(dev, gold, name):
    """cice_step_ridge, bound = 0, four blocks = cice_ridge_ice, cice_cleanup_itd, cice_aggregate block by block"""
    s = gold[0][name][0]
    _init(dev, name)
    dev.thermo_batch_alloc(rc.NX, rc.NY, rc.NB)
    a = _one_call_arrays(s)
    e = _expected(dev, a)
    r = dev.step_ridge(rc.DT, a)
    assert r["l_stop"] == 0 and r["stage"] == 0, r
    _bitwise(*_planes(a, e, rc.CASES[name]["ntrcr"]), ONE_CALL_OUT, (name, "one call"))
    _bitwise(a, s, rc.IN_ONLY, "intent(in)")
    assert not tc.same(a["aicen"], s["aicen"])


def test_one_call_with_bound_state_on_a_2_x_2_domain(gold):
    s = gold[0]["ntr4"][0]
    ntr = rc.CASES["ntr4"]["ntrcr"]
    c = lib.Context()
    try:
        c.domain_create(24, 20, 12, 10, ew=1, ns=0)
        assert (c.nx, c.ny, c.nblocks) == (rc.NX, rc.NY, rc.NB)
        _init(c, "ntr4")
        c.thermo_batch_alloc(rc.NX, rc.NY, rc.NB)
        a = _one_call_arrays(s)

        def halo(x):
            for k in ("aicen", "vicen", "vsnon", "eicen", "esnon"):
                c.halo_update_blocked(x[k])
            c.halo_update_strided(x["trcrn"][:, :, 0:ntr])

        e = _expected(c, a, halo)
        assert c.step_ridge(rc.DT, a, bound=True)["l_stop"] == 0
        _bitwise(*_planes(a, e, ntr), ONE_CALL_OUT, "bound = 1")
    finally:
        c.close()


def test_one_call_stop_in_block_2_of_4(dev, gold):
    s = gold[0]["ntr1"][0]
    _init(dev, "ntr1")
    dev.thermo_batch_alloc(rc.NX, rc.NY, rc.NB)
    s = {k: v.copy() for k, v in s.items()}
    lm = rc.listed_mask(s["tmask"])[1] & (s["aicen"][1] > 0.05).any(axis=0)
    jj, ii = np.nonzero(lm)
    cells = [(int(jj[k]), int(ii[k])) for k in (2, len(jj) - 3)]
    for j, i in cells:                   # full cover, no open water, rdg_conv < 0: the new aice0 is below -puny
        tot = cc.cat_sum(s["aicen"][1][:, j:j + 1, i:i + 1])[0, 0]
        for n in range(rc.NCAT):
            cc._scale(s, 1, n, j, i, 0.999 / tot)
        s["aice0"][1, j, i] = 0.0
        s["rdg_conv"][1, j, i], s["rdg_shear"][1, j, i] = -1.0e-5, 0.0
    a = _one_call_arrays(s)
    a0 = {k: v.copy() for k, v in a.items()}
    r = dev.step_ridge(rc.DT, a)
    assert (r["l_stop"], r["stage"], r["bstop"], r["istop"], r["jstop"]) == (1, 1, 2, cells[0][1] + 1, cells[0][0] + 1), r
    names = rc.OUT
    first = _block(s, 0)
    assert dev.ridge_ice(*rc.tmask_list(s["tmask"][0]), rc.DT, first)[:3] == (0, 0, 0)
    _bitwise({k: a[k][0] for k in names}, first, names, "block 1: ridged")
    blk = _block(s, 1)
    assert dev.ridge_ice(*rc.tmask_list(s["tmask"][1]), rc.DT, blk)[:3] == (1, r["istop"], r["jstop"])
    _bitwise({k: a[k][1] for k in names}, blk, names, "block 2: as the block-wise entry leaves it")
    _bitwise({k: a[k][2:] for k in names}, {k: a0[k][2:] for k in names}, names, "blocks 3, 4: as they went in")
    _bitwise(a, a0, ("aice", "vice", "vsno", "eice", "esno", "trcr", "fsalt", "daidtd", "dvidtd"), "later stages")
