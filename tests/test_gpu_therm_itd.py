"""The thickness-distribution stage on the device (cice_linear_itd, cice_add_new_ice, cice_lateral_melt, cice_shift_ice,
cice_step_therm2_itd) against what the compiled reference recorded in tests/golden/therm_itd.npz: every block of every
ordinary case, every output array, ghost cells included, BIT FOR BIT -- there is no exp / pow on this path."""
import numpy as np
import pytest

import therm_itd_case as tc
from cice4_amd import lib, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    d = np.load(tc.FIXTURE)
    return {name: tc.load_chain(d, name) for name in tc.ORDINARY}, d


@pytest.fixture(scope="module")
def dev():
    c = lib.Context()
    c.sync()
    yield c
    c.close()      # streams and device memory go back now, not when the collector gets to the object


def _init(dev, name):
    dev.itd_init(**tc.itd_kwargs(tc.CASES[name]))


def _bitwise(got, want, names, where, ntrcr=5):
    for k in names:
        g, w = got[k], want[k]
        if k == "trcrn":
            g, w = g[..., :ntrcr, :, :], w[..., :ntrcr, :, :]
        assert tc.same(g, w), (where, k, int((np.ascontiguousarray(g).view(np.uint64) != np.ascontiguousarray(w).view(np.uint64)).sum()))


def _blockwise(dev, s0, kitd=1, yday=tc.YDAY):
    """the three block-wise entries applied to every block of state s0 (after rain and aggregate_area): s1, s2, s3"""
    nb = s0["aice"].shape[0]
    chain = [s0]
    counts = 0
    for stage in (1, 2, 3):
        cur = {k: v.copy() for k, v in chain[-1].items()}
        for b in range(nb):
            blk = tc.block(cur, b)
            ny, nx = blk["aice"].shape
            if stage == 1:
                jj, ii = np.nonzero(blk["aice"][1:-1, 1:-1] > tc.PUNY)
                if len(ii) and kitd:
                    r = dev.linear_itd(len(ii), _pad(ii + 2, nx * ny), _pad(jj + 2, nx * ny), blk)
                    assert r[:3] == (0, 0, 0)
                    counts += r[3]
            elif stage == 2:
                jj, ii = np.nonzero(blk["tmask"])
                assert dev.add_new_ice(len(ii), _pad(ii + 1, nx * ny), _pad(jj + 1, nx * ny), tc.DT, yday, blk) == (0, 0, 0)
            else:
                dev.lateral_melt(2, nx - 1, 2, ny - 1, tc.DT, blk)
            for k in tc.CHAIN:
                cur[k][b] = blk[k]
        chain.append(cur)
    return chain, counts


def _pad(a, n):
    out = np.zeros(n, np.int32)
    out[:len(a)] = a
    return out


@pytest.mark.parametrize("name", tc.ORDINARY)
def test_blockwise_entries_reproduce_the_reference(dev, gold, name):
    """each entry on the recorded state in front of it gives the recorded state behind it; intent(in) arrays unchanged"""
    raw, chain = gold[0][name]
    ntr = tc.CASES[name]["ntrcr"]
    _init(dev, name)
    nn = 0
    for b in range(tc.NB):
        blk = tc.block(chain[0], b)
        keep = {k: blk[k].copy() for k in ("aicen_init", "vicen_init")}
        icells, ii, jj = tc.ice_list(blk["aice"])
        if icells:
            r = dev.linear_itd(icells, ii, jj, blk)
            assert r[:3] == (0, 0, 0)
            nn += r[3]
        _bitwise(blk, tc.block(chain[1], b), tc.OUT1, (name, "linear_itd", b), ntr)
        _bitwise(blk, keep, keep, (name, "linear_itd intent(in)", b))
        blk = tc.block(chain[1], b)
        keep = {k: blk[k].copy() for k in ("aice", "frzmlt", "Tf", "tmask")}
        icells, ii, jj = tc.ocean_list(blk["tmask"])
        assert dev.add_new_ice(icells, ii, jj, tc.DT, tc.YDAY, blk) == (0, 0, 0)
        _bitwise(blk, tc.block(chain[2], b), tc.OUT2, (name, "add_new_ice", b), ntr)
        for k in keep:
            assert np.array_equal(blk[k], keep[k]), (name, "add_new_ice intent(in)", k)
        blk = tc.block(chain[2], b)
        rs = blk["rside"].copy()
        dev.lateral_melt(tc.ILO, tc.IHI, tc.JLO, tc.JHI, tc.DT, blk)
        _bitwise(blk, tc.block(chain[3], b), tc.OUT3, (name, "lateral_melt", b))
        assert tc.same(blk["rside"], rs)
    assert nn == int(gold[1][f"{name}_not_remapped"])


def test_shift_ice_stop(dev, gold):
    """daice = 2 aicen(nd) in two cells of boundary 2: l_stop, the later cell, the state untouched"""
    _init(dev, "growth")
    s, icells, ii, jj, cell = tc.stop_shift_inputs()
    assert tc.digest(s) == str(gold[1]["stop_shift_sha256"])
    before = {k: v.copy() for k, v in s.items()}
    r = dev.shift_ice(icells, ii, jj, s)
    assert r == tuple(int(x) for x in gold[1]["stop_shift_stop"]) == (1,) + cell
    _bitwise(s, before, tc.STATE, "stop_shift")
    assert np.array_equal(s["donor"], before["donor"])


def test_add_new_ice_stop(dev, gold):
    _init(dev, "growth")
    s, cell = tc.stop_add_inputs()
    assert tc.digest(s) == str(gold[1]["stop_add_sha256"])
    icells, ii, jj = tc.ocean_list(s["tmask"])
    r = dev.add_new_ice(icells, ii, jj, tc.DT, tc.YDAY, s)
    assert r == tuple(int(x) for x in gold[1]["stop_add_stop"]) == (1,) + cell
    _bitwise(s, {k: gold[1][f"stop_add_out_{k}"] for k in tc.OUT2}, tc.OUT2, "stop_add")


@pytest.mark.parametrize("name", tc.ORDINARY)
def test_stage_from_host_state(dev, gold, name):
    """cice_step_therm2_itd, state_resident = 0, on the raw inputs: state3 of the case"""
    raw, chain = gold[0][name]
    _init(dev, name)
    dev.thermo_batch_alloc(tc.NX, tc.NY, tc.NB)
    a = {k: v.copy() for k, v in raw.items()}
    r = dev.step_therm2_itd(tc.DT, tc.YDAY, a)
    assert r["l_stop"] == 0 and r["stage"] == 0, r
    _bitwise(a, chain[3], tc.CHAIN, (name, "stage"), tc.CASES[name]["ntrcr"])
    for k in ("aicen_init", "vicen_init", "frain", "frzmlt", "Tf", "rside", "tmask"):
        assert np.array_equal(a[k], raw[k]), k


def _stop_stage2_inputs():
    raw, _ = tc.case_inputs("growth")
    a = {k: v.copy() for k, v in raw.items()}
    b, i, j = 1, 6, 5
    # with kitd = 0 the caller's aice and aice0 are what add_new_ice reads: half the cover and no open water in one cell
    a["aice"][b, j - 1, i - 1] = 0.5 * a["aicen"][b, :, j - 1, i - 1].sum()
    if a["aice"][b, j - 1, i - 1] <= 0.05:
        a["aicen"][b, 0, j - 1, i - 1] = 0.5; a["vicen"][b, 0, j - 1, i - 1] = 0.2; a["aice"][b, j - 1, i - 1] = 0.25
    a["aice0"][b, j - 1, i - 1] = 0.0
    a["frzmlt"][b, j - 1, i - 1] = 60.0
    a["tmask"][b, j - 1, i - 1] = 1
    return a, (b, i, j)


def test_stage_stop_in_add_new_ice(dev):
    """kitd = 0 with the caller's aice half the cover in one cell of block 2: stage = 2, that cell; block 2 has no
    lateral melt, block 1 has completed the stage, blocks 3 and 4 come back as they went in"""
    _init(dev, "growth")
    dev.thermo_batch_alloc(tc.NX, tc.NY, tc.NB)
    a, (b, i, j) = _stop_stage2_inputs()
    a["rside"][...] = np.where(a["aicen"].sum(axis=1) > 0, 0.02, 0.0)     # so that a lateral melt would show
    a0 = {k: v.copy() for k, v in a.items()}
    r = dev.step_therm2_itd(tc.DT, tc.YDAY, a, kitd=0)
    assert (r["l_stop"], r["stage"], r["bstop"], r["istop"], r["jstop"]) == (1, 2, b + 1, i, j), r
    assert tc.same(a["meltl"][b], a0["meltl"][b]) and tc.same(a["vsnon"][b], a0["vsnon"][b])   # stage 3 undone in block 2
    assert (a["meltl"][0] > 0).any()                                                         # block 1 completed
    for k in tc.STATE:
        assert tc.same(a[k][b + 1:], a0[k][b + 1:]), k                                      # blocks behind: untouched
    # block 2 is what the block-wise add_new_ice leaves (the stop is at its end)
    fresh0 = a0["fresh"] + a0["frain"] * a0["aice"]
    blk = tc.block(dict(a0, fresh=fresh0), b)
    jj, ii = np.nonzero(blk["tmask"])
    assert dev.add_new_ice(len(ii), _pad(ii + 1, tc.NX * tc.NY), _pad(jj + 1, tc.NX * tc.NY), tc.DT, tc.YDAY, blk) == (1, i, j)
    _bitwise({k: a[k][b] for k in tc.OUT2}, blk, tc.OUT2, "stage 2 stop, block 2")


@pytest.mark.parametrize("shape", [(64, 5), (66, 5), (67, 4)])
def test_other_block_shapes_agree_with_blockwise(dev, shape):
    """block shapes (nx_block, ny_block, ghost cells included) on one context, one after the other: a memory row of exactly
    one wavefront (64), and 64 / 65 physical cells per row (66 x 5 = a 64 x 3 block with its ghosts, 67 x 4 = 65 x 2):
    the stage call = the block-wise entries"""
    nxb, nyb = shape
    _init(dev, "tracers")
    raw = synth.therm2_state("mixed", nxb, nyb, 1, seed=77 + nxb, ntrcr=4)
    dev.thermo_batch_alloc(nxb, nyb, 1)
    a = {k: v.copy() for k, v in raw.items()}
    r = dev.step_therm2_itd(tc.DT, tc.YDAY, a)
    assert r["l_stop"] == 0
    chain, _ = _blockwise(dev, _after_rain_and_aggregate(raw))
    _bitwise(a, chain[3], tc.CHAIN, shape, 4)


def _after_rain_and_aggregate(raw):
    s0 = {k: v.copy() for k, v in raw.items()}
    s0["fresh"] = raw["fresh"] + raw["frain"] * raw["aice"]
    aice = np.zeros_like(raw["aice"])
    for n in range(5):
        aice = aice + raw["aicen"][:, n]
    s0["aice"] = aice
    s0["aice0"] = np.maximum(1.0 - aice, 0.0)
    return s0


def test_stage_on_resident_state_behind_step_therm1(dev):
    """state_resident = 1 behind a real cice_step_therm1 on the same context = the three block-wise entries applied to what
    that call downloaded: every array of the chain, frz_onset included (same dt, yday on both sides); frzmlt of both
    signs and rside > 0 under ice, so that all three routines work on the resident state"""
    from test_gpu_thermo import _batch_inputs, DT
    assert DT == tc.DT
    ny, nx, nb = 12, 14, 2
    dev.thermo_init()
    _init(dev, "growth")
    batch, percat = _batch_inputs(ny, nx, nb, seed=35)
    rng = np.random.default_rng(6)
    U = lambda lo, hi: np.ascontiguousarray(rng.uniform(lo, hi, (nb, ny, nx)))
    aice = np.ascontiguousarray(batch["aicen"].sum(axis=1))
    fz = dict(aice=aice, frzmlt=U(-40, 60), Tf=np.full((nb, ny, nx), -1.8), strocnxT=U(-0.2, 0.2), strocnyT=U(-0.2, 0.2))
    fz["sst"] = fz["Tf"] + U(0, 0.5)
    pc = {k: np.ascontiguousarray(rng.uniform(-1, 1, batch["aicen"].shape)) for k in ("strairxn", "strairyn", "Trefn", "Qrefn")}
    acc = {k: U(-1, 1) for k in lib.MERGE_ORDER}
    st = {k: v.copy() for k, v in batch.items()}
    dev.thermo_batch_alloc(nx, ny, nb)
    assert dev.step_therm1(DT, tc.YDAY, st, fz, pc, acc)["l_stop"] == 0
    ice = st["aicen"].sum(axis=1) > tc.PUNY
    rside = np.ascontiguousarray(np.where(ice & (fz["frzmlt"] < 0), U(0.005, 0.05), 0.0))
    assert (rside[:, 1:-1, 1:-1] > 0).sum() >= 8 and ((fz["frzmlt"] > 0) & ice).sum() >= 8
    a = dict({k: st[k].copy() for k in tc.STATE}, aicen_init=batch["aicen"].copy(),
             vicen_init=batch["vicen"].copy(), frain=U(0, 1e-5), frzmlt=fz["frzmlt"].copy(), Tf=fz["Tf"].copy(),
             rside=rside, tmask=np.ones((nb, ny, nx), np.int32), aice=aice.copy(), aice0=np.maximum(1 - aice, 0),
             fresh=U(0, 1e-5), fsalt=U(0, 1e-7), fhocn=U(-5, 0), frazil=np.zeros((nb, ny, nx)),
             meltl=np.zeros((nb, ny, nx)), frz_onset=np.zeros((nb, ny, nx)))
    raw = {k: v.copy() for k, v in a.items()}
    res = {k: v for k, v in a.items() if k != "aicen_init"}        # the batch kept the concentrations before the update
    r = dev.step_therm2_itd(tc.DT, tc.YDAY, res, state_resident=True)
    assert r["l_stop"] == 0, r
    chain, _ = _blockwise(dev, _after_rain_and_aggregate(raw))
    _bitwise(res, chain[3], tc.CHAIN, "resident", 1)
    assert not tc.same(chain[3]["meltl"], raw["meltl"]) and (chain[3]["frz_onset"] == tc.YDAY).any()
    # without a cice_step_therm1 call in front, the batch holds no concentrations to stand in for aicen_init
    dev.thermo_batch_alloc(nx, ny, nb)
    with pytest.raises(lib.CiceError):
        dev.step_therm2_itd(tc.DT, tc.YDAY, {k: v.copy() for k, v in res.items()}, state_resident=True)
