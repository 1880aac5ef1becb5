"""compute_ponds and increment_age on the device -- cice_step_ponds, cice_compute_ponds, cice_increment_age -- against what
the compiled reference recorded in tests/golden/pond.npz, on all four blocks with no cell left out.  Every operation is one
correctly rounded fp64 operation or the restated exp, so the agreement is

  bit for bit, unconditionally: every word off the lists (it equals the input), every other tracer plane, the intent(in)
    arrays, iage, and apondn / hpondn / volpn on thin ice;
  bit for bit where conftest.TOL_EXP == 0 (the host libm that minted the fixture is the restated one), else to TOL_EXP of
    the field's magnitude: apondn, hpondn, volpn where the volume update ran.

Behind a real cice_step_therm1 the resident form is held to the uploading one and cice_step_therm2_itd to itself without
the stage in between; cice_pond_chain(1) into cice_step_radiation_dedd is held to the unchained call."""
import functools

import numpy as np
import pytest

import dedd_case as dc
import pond_case as pc
import therm_itd_case as tic
from conftest import TOL_EXP
from cice4_amd import lib

pytestmark = pytest.mark.gpu
NAMES = tuple(pc.CASES)


@functools.lru_cache(maxsize=None)
def _gold(name):
    return pc.load_case(np.load(pc.FIXTURE), name)


def _context(name, batch=True):
    c = pc.CASES[name]
    ctx = lib.Context()
    ctx.sync()
    ctx.thermo_init(tr_iage=c["tr_iage"], nt_Tsfc=c["nt_Tsfc"], nt_iage=c["nt_iage"] or pc.NTRCR)
    ctx.pond_init(c["nt_volpn"])
    if batch:
        ctx.thermo_batch_alloc(pc.NX, pc.NY, pc.NB)
    return ctx


def _got(name, a):
    """the members of pond_case.outputs_of from the arrays a call updated in place"""
    c = pc.CASES[name]
    src = dict(apondn=lambda: a["apondn"], hpondn=lambda: a["hpondn"], volpn=lambda: a["trcrn"][:, :, c["nt_volpn"] - 1],
               iage=lambda: a["trcrn"][:, :, c["nt_iage"] - 1])
    return {k: np.ascontiguousarray(src[k]()) for k in pc.outputs_of(name)}


def _check(name, s, a, want, where):
    """the arrays `a` after a call against the fixture by class of word, and against the inputs everywhere else"""
    c = pc.CASES[name]
    on = pc.listed(s)
    _, m = pc.restate(name, s)
    got = _got(name, a)
    for k, w in want.items():
        g = got[k]
        assert np.isfinite(g).all(), (where, k)
        exact = np.ones(on.shape, bool) if (k == "iage" or TOL_EXP == 0.0) else ~m["run"]
        assert tic.same(g[exact], w[exact]), (where, k, int((g[exact] != w[exact]).sum()))
        if not exact.all():
            assert np.abs(g - w).max() <= TOL_EXP * np.abs(w).max(), (where, k)
    owned = [c["nt_" + k] - 1 for k in want if k in ("volpn", "iage")]
    rest = [it for it in range(pc.NTRCR) if it not in owned]
    assert tic.same(a["trcrn"][:, :, rest], s["trcrn"][:, :, rest]), (where, "another tracer plane")
    for k in s:                              # intent(in), and what the flags leave alone
        if k != "trcrn" and k not in want:
            assert tic.same(a[k], s[k]), (where, k, "changed")
    return int(on.sum())


@pytest.mark.parametrize("name", NAMES)
def test_one_call_reproduces_the_reference(name):
    c = pc.CASES[name]
    s, want = _gold(name)
    a = {k: v.copy() for k, v in s.items()}
    ctx = _context(name)
    try:
        ctx.step_ponds(pc.DT, a, ponds=c["ponds"], age=c["age"])
    finally:
        ctx.close()
    assert _check(name, s, a, want, ("one call", name)) >= 1000


@pytest.mark.parametrize("name", ("freeze", "no_age"))
def test_blockwise_compute_ponds(name):
    c = pc.CASES[name]
    s, want = _gold(name)
    a = {k: v.copy() for k, v in s.items()}
    if c["age"]:                             # (as if increment_age had run: _check looks at every output of the case)
        a["trcrn"][:, :, c["nt_iage"] - 1] = want["iage"]
    blk = pc.block_table()
    ctx = _context(name, batch=False)
    try:
        for b in range(pc.NB):
            for n in range(pc.NCAT):
                one = dict(meltt=a["melttn"][b, n], melts=a["meltsn"][b, n], frain=a["frain"][b], aicen=a["aicen"][b, n],
                           vicen=a["vicen"][b, n], vsnon=a["vsnon"][b, n], trcrn=a["trcrn"][b, n], apondn=a["apondn"][b, n],
                           hpondn=a["hpondn"][b, n])         # views: updated in place
                ctx.compute_ponds(*[int(x) for x in blk[b]], pc.DT, one)
    finally:
        ctx.close()
    _check(name, s, a, want, ("block-wise", name))


def test_blockwise_increment_age_on_the_ice_list_and_on_another():
    s, want = _gold("age_only")
    it = pc.CASES["age_only"]["nt_iage"] - 1
    on = pc.listed(s)
    # another list: a checkerboard of the whole block, ghost and ice-free cells included
    jj, ii = np.indices((pc.NY, pc.NX))
    board = ((ii + jj) % 2 == 0)[None, None] & np.ones(on.shape, bool)
    assert (board & ~on).sum() >= 100 and (~board & on).sum() >= 100
    ctx = _context("age_only", batch=False)
    try:
        for lst, expect in ((on, want["iage"]), (board, pc.age_numpy("age_only", s, on=board))):
            a = {k: v.copy() for k, v in s.items()}
            for b in range(pc.NB):
                for n in range(pc.NCAT):
                    j, i = np.nonzero(lst[b, n])
                    indxi, indxj = np.zeros(pc.NX * pc.NY, np.int32), np.zeros(pc.NX * pc.NY, np.int32)
                    indxi[:len(i)], indxj[:len(i)] = i + 1, j + 1
                    ctx.increment_age(pc.DT, len(i), indxi, indxj, a["trcrn"][b, n, it])
            assert tic.same(a["trcrn"][:, :, it], expect), int((a["trcrn"][:, :, it] != expect).sum())
            rest = [k for k in range(pc.NTRCR) if k != it]
            assert tic.same(a["trcrn"][:, :, rest], s["trcrn"][:, :, rest])
    finally:
        ctx.close()


def _therm1(ctx, ny=12, nx=14, nb=2):
    """a real cice_step_therm1, set up as test_gpu_therm_itd.py::test_stage_on_resident_state_behind_step_therm1 sets it up;
    returns what it downloaded and the fields of the cice_step_therm2_itd behind it"""
    from test_gpu_thermo import DT, _batch_inputs
    assert DT == tic.DT == pc.DT
    batch, _ = _batch_inputs(ny, nx, nb, seed=35)
    rng = np.random.default_rng(6)
    U = lambda lo, hi: np.ascontiguousarray(rng.uniform(lo, hi, (nb, ny, nx)))  # noqa: E731
    aice = np.ascontiguousarray(batch["aicen"].sum(axis=1))
    fz = dict(aice=aice, frzmlt=U(-40, 60), Tf=np.full((nb, ny, nx), -1.8), strocnxT=U(-0.2, 0.2), strocnyT=U(-0.2, 0.2))
    fz["sst"] = fz["Tf"] + U(0, 0.5)
    percat = {k: np.ascontiguousarray(rng.uniform(-1, 1, batch["aicen"].shape)) for k in ("strairxn", "strairyn", "Trefn", "Qrefn")}
    acc = {k: U(-1, 1) for k in lib.MERGE_ORDER}
    st = {k: v.copy() for k, v in batch.items()}
    ctx.thermo_batch_alloc(nx, ny, nb)
    assert ctx.step_therm1(DT, tic.YDAY, st, fz, percat, acc)["l_stop"] == 0
    ice = st["aicen"].sum(axis=1) > tic.PUNY
    rside = np.ascontiguousarray(np.where(ice & (fz["frzmlt"] < 0), U(0.005, 0.05), 0.0))
    a2 = dict({k: st[k].copy() for k in tic.STATE}, vicen_init=batch["vicen"].copy(), frain=U(0, 1e-5),
              frzmlt=fz["frzmlt"].copy(), Tf=fz["Tf"].copy(), rside=rside, tmask=np.ones((nb, ny, nx), np.int32),
              aice=aice.copy(), aice0=np.maximum(1 - aice, 0), fresh=U(0, 1e-5), fsalt=U(0, 1e-7), fhocn=U(-5, 0),
              frazil=np.zeros((nb, ny, nx)), meltl=np.zeros((nb, ny, nx)), frz_onset=np.zeros((nb, ny, nx)))
    return st, a2


def _pond_arrays(st, seed=20261021):
    """the fields of cice_step_ponds around what cice_step_therm1 downloaded: tracers 2 (iage) and 3 (volpn), stale ponds"""
    rng = np.random.default_rng(seed)
    shp = st["aicen"].shape
    trcrn = st["trcrn"].copy()
    trcrn[:, :, 1] = rng.uniform(0.0, 1.0e7, shp)
    trcrn[:, :, 2] = np.where(rng.random(shp) < 0.3, 0.0, rng.uniform(0.0, 0.4, shp))
    trcrn[:, :, 3:] = rng.uniform(-5.0, 5.0, trcrn[:, :, 3:].shape)
    return dict(frain=rng.uniform(0.0, 1.0e-4, (shp[0],) + shp[2:]), trcrn=trcrn, apondn=rng.uniform(0.01, 0.5, shp),
                hpondn=rng.uniform(0.01, 0.4, shp), aicen=st["aicen"].copy(), vicen=st["vicen"].copy(), vsnon=st["vsnon"].copy(),
                melttn=st["meltt"].copy(), meltsn=st["melts"].copy())


def test_resident_state_behind_step_therm1():
    ctx = lib.Context()
    try:
        ctx.sync()
        ctx.thermo_init()                    # tr_iage, nt_Tsfc = 1, nt_iage = 2
        ctx.itd_init(**tic.itd_kwargs(tic.CASES["growth"]))
        ctx.pond_init(3)
        # without the stage: cice_step_therm1 -> cice_step_therm2_itd(state_resident = 1)
        st, a2 = _therm1(ctx)
        plain = {k: v.copy() for k, v in a2.items()}
        assert ctx.step_therm2_itd(tic.DT, tic.YDAY, plain, state_resident=True)["l_stop"] == 0
        with pytest.raises(lib.CiceError, match="error -1: cice_step_ponds: state_resident needs a cice_step_therm1"):
            ctx.step_ponds(pc.DT, _pond_arrays(st), state_resident=True)        # cice_step_therm2_itd ended the record
        # with it
        st_b, a2_b = _therm1(ctx)
        for k in st:
            assert tic.same(st[k], st_b[k]), k
        up = _pond_arrays(st_b)
        before = {k: v.copy() for k, v in up.items()}
        res = {k: (np.full_like(v, np.nan) if k in ("aicen", "vicen", "vsnon", "melttn", "meltsn") else v.copy())
               for k, v in up.items()}
        res["trcrn"][:, :, 0] = np.nan                                           # the state's pointers are not read
        ctx.step_ponds(pc.DT, res, state_resident=True)
        ctx.step_ponds(pc.DT, up, state_resident=False)                          # ... and the batch is left as it was
        again = {k: v.copy() for k, v in res.items()}
        for k in ("trcrn", "apondn", "hpondn"):
            again[k][...] = before[k]
        again["trcrn"][:, :, 0] = np.nan
        ctx.step_ponds(pc.DT, again, state_resident=True)                        # the record stands
        staged = {k: v.copy() for k, v in a2_b.items()}
        assert ctx.step_therm2_itd(tic.DT, tic.YDAY, staged, state_resident=True)["l_stop"] == 0
        fresh = lib.Context()
        try:
            fresh.sync()
            fresh.thermo_init()
            fresh.pond_init(3)
            fresh.thermo_batch_alloc(14, 12, 2)
            with pytest.raises(lib.CiceError, match="error -1: cice_step_ponds: state_resident needs a cice_step_therm1"):
                fresh.step_ponds(pc.DT, _pond_arrays(st), state_resident=True)   # no cice_step_therm1 in front
        finally:
            fresh.close()
    finally:
        ctx.close()
    on = (st_b["aicen"] > pc.PUNY)[:, :, 1:-1, 1:-1]
    assert on.sum() >= 100 and not tic.same(up["apondn"], before["apondn"]) and not tic.same(up["trcrn"], before["trcrn"])
    for k in ("apondn", "hpondn"):
        assert tic.same(res[k], up[k]) and tic.same(again[k], up[k]), k
    for it in (1, 2, 3, 4):
        assert tic.same(res["trcrn"][:, :, it], up["trcrn"][:, :, it]) and tic.same(again["trcrn"][:, :, it], up["trcrn"][:, :, it]), it
    for k in ("aicen", "vicen", "vsnon", "melttn", "meltsn", "frain"):
        assert tic.same(up[k], before[k]), ("intent(in)", k)
    for k in plain:
        assert tic.same(staged[k], plain[k]), ("cice_step_therm2_itd behind the stage", k)


def _dedd_call(ctx, s, apondn, hpondn):
    from test_gpu_dedd import IN_2D, _outputs
    a = {k: v for k, v in s.items() if k in dc.STATE + IN_2D}
    a.update(apondn=apondn, hpondn=hpondn)
    a.update(_outputs(s["aicen"].shape))
    ctx.step_radiation_dedd(a)
    return {k: a[k] for k in dc.OUT}


def test_pond_chain_into_step_radiation_dedd():
    s, _ = _gold("melt")
    rad = dc.case_inputs("tr_pond")
    ctx = _context("melt")
    try:
        ctx.shortwave_dedd_init(**dc.init_kwargs("tr_pond"))

        def ponds():
            a = {k: v.copy() for k, v in s.items()}
            ctx.step_ponds(pc.DT, a)
            kept = a["apondn"].copy(), a["hpondn"].copy()
            a["apondn"][...] = np.nan
            a["hpondn"][...] = np.nan
            return a, kept

        same = lambda x, y: all(tic.same(x[k], y[k]) for k in dc.OUT)  # noqa: E731
        ctx.pond_chain(1)
        a, kept = ponds()
        chained = _dedd_call(ctx, rad, a["apondn"], a["hpondn"])
        chained2 = _dedd_call(ctx, rad, a["apondn"], a["hpondn"])               # the record stays until the next cice_step_ponds
        other = _dedd_call(ctx, rad, a["apondn"].copy(), a["hpondn"])           # another pointer: the host arrays are read
        ctx.pond_chain(0)
        off = _dedd_call(ctx, rad, a["apondn"], a["hpondn"])
        want = _dedd_call(ctx, rad, *kept)
        ctx.pond_chain(1)
        b, _ = ponds()
        ctx.thermo_batch_alloc(pc.NX, pc.NY, pc.NB)
        realloc = _dedd_call(ctx, rad, b["apondn"], b["hpondn"])
        c, _ = ponds()
        d, kept_d = ponds()                                                     # the next cice_step_ponds takes the record over
        stale = _dedd_call(ctx, rad, c["apondn"], c["hpondn"])
        latest = _dedd_call(ctx, rad, d["apondn"], d["hpondn"])
    finally:
        ctx.close()
    assert (kept[0] > dc.PUNY).sum() >= 100 and want["albpndn"].max() > 0.0
    for k in dc.OUT:
        assert np.isfinite(want[k]).all(), k
        assert tic.same(chained[k], want[k]) and tic.same(chained2[k], want[k]) and tic.same(latest[k], want[k]), k
    for name, got in (("other pointers", other), ("mode 0", off), ("after cice_thermo_batch_alloc", realloc),
                      ("an older call's arrays", stale)):
        assert not same(got, want), (name, "the NaN in the host arrays does not show")


def test_pond_times():
    s, _ = _gold("melt")
    ctx = _context("melt")
    try:
        a = {k: v.copy() for k, v in s.items()}
        ctx.step_ponds(pc.DT, a)
        assert ctx.pond_times(True) == 0.0           # nothing was timed while it was off
        a = {k: v.copy() for k, v in s.items()}
        ctx.step_ponds(pc.DT, a)
        ms = ctx.pond_times(False)
        assert 0.0 < ms < 100.0, ms
        ctx.step_ponds(pc.DT, a)
        assert ctx.pond_times(False) == ms           # off again: the last timed call's
    finally:
        ctx.close()


def test_refusals_on_the_device():
    s, _ = _gold("age_only")
    ctx = _context("age_only")
    try:
        with pytest.raises(lib.CiceError, match="error -1: cice_step_ponds: ponds = 1"):
            ctx.step_ponds(pc.DT, {k: v.copy() for k, v in s.items()})
        with pytest.raises(lib.CiceError, match="error -1: cice_step_ponds: state_resident needs"):
            ctx.step_ponds(pc.DT, {k: v.copy() for k, v in s.items()}, ponds=False, state_resident=True)
    finally:
        ctx.close()
