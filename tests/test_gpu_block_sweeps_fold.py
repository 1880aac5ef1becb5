"""K-subcycle sweeps on a ONE-TASK domain cut into several blocks under a tripole fold (option "skew_join_fold", off by
default): the sweep runs on the joined image as on an open north boundary, the fold is carried by a band of the top 2K + 1
rows that runs one subcycle at a time on the blocks of the top block row, and the blocks get the result back
(cice4_amd/csrc/join.hip; Evp::launch_subcycle_join_fold).

Every comparison is bit for bit.  WHOLE block arrays, ghost cells included, against one launch per subcycle plus the halo
update with the fold on the same blocks: that path is the one tests/test_gpu_evp.py pins to the compiled reference on
several blocks under a fold, so this is parity with the reference by one step of transitivity.  Physical cells against the
sweep of the same grid as one block under the fold."""
import numpy as np
import pytest

from cice4_amd import lib, synth
from test_gpu_evp import DT, NDTE, EVP_OUT_FIELDS
from test_gpu_block_sweeps import _case, _run, _global, SWEEP, SINGLES, JOIN_SPLIT

pytestmark = pytest.mark.gpu
KEYS = EVP_OUT_FIELDS + ("iceumask",)
# kernel launches a visit to the image adds under a fold: JOIN_SPLIT (the join, the split of the state, the split of the
# diagnostics) and one more that hands u, v of the top physical row and of the ghost row above it -- what the fold writes
# with or without ice -- from the band to the blocks.  (The band's own small launches are not counted, as in the one-block form.)
JOIN_SPLIT_FOLD = JOIN_SPLIT + 1
FOLD = dict(SWEEP, skew_fold=1, skew_join_fold=1)

# grids test_sweeps_on_a_tripole_grid proves the one-block fold sweep on, as 2 x 2, 4 x 1 and 1 x 4 blocks; 300 x 120 in
# blocks of 15 x 60; 96 x 70 in blocks of 40 x 30 (last blocks padded both ways, ten rows left for the top block row)
c = lambda a, b: -(-a // b)
LAYOUTS = [(nxg, nyg, bsx, bsy) for nxg, nyg in ((96, 70), (300, 120), (130, 48))
           for bsx, bsy in ((c(nxg, 2), c(nyg, 2)), (c(nxg, 4), nyg), (nxg, c(nyg, 4)))] + [(300, 120, 15, 60), (96, 70, 40, 30)]
RUNS = [(NDTE, False), (7, True), (13, False)]


def _fold_case(ctx, nxg, nyg, bsx, bsy, ns):
    return _case(ctx, nxg, nyg, 1, bsx, bsy, ns=ns, land_rows=0)


@pytest.mark.parametrize("ns", [3, 4], ids=["tripole", "tripoleT"])
@pytest.mark.parametrize("nxg,nyg,bsx,bsy", LAYOUTS)
def test_sweeps_on_the_joined_image_under_a_fold(ctx, nxg, nyg, bsx, bsy, ns):
    combos = [(K, graph, pairs) for K, graph, pairs in ((4, 1, 1), (4, 0, 1), (4, 1, 0), (3, 1, 1), (2, 0, 1)) if nyg >= 4 * K + 6]   # (as test_sweeps_on_a_tripole_grid skips K)
    # the same grid as ONE block under the fold: the physical cells, and its launches
    dom1, grid1, s1 = _fold_case(ctx, nxg, nyg, nxg, nyg, ns)
    one = {}
    for ndte, damping in RUNS:
        for K in sorted({K for K, _, _ in combos}):
            o, info, launches = _run(ctx, grid1, s1, ndte, damping, info=("skew_fold",), skew_levels=K, skew_fold=1, **SWEEP)
            assert info["skew_fold"] == 1
            one[ndte, damping, K] = ({k: _global(dom1, o, k, nxg, nyg) for k in KEYS}, launches)
    dom, grid, s = _fold_case(ctx, nxg, nyg, bsx, bsy, ns)
    assert dom["nblocks"] >= 4
    for ndte, damping in RUNS:
        ref, info, launches = _run(ctx, grid, s, ndte, damping, info=("skew", "skew_joined"), **SINGLES)
        assert info == dict(skew=0, skew_joined=0) and launches == ndte
        # a condition, not a measurement: the fold has to touch moving cells, or the comparison shows nothing
        assert np.abs(_global(dom, ref, "uvel", nxg, nyg)[-3:]).max() > 1e-4
        for K, graph, pairs in combos:
            got, info, launches = _run(ctx, grid, s, ndte, damping,
                                       info=("skew", "skew_joined", "skew_fold", "skew_levels", "skew_join_fold"),
                                       skew_levels=K, use_graph=graph, skew_pairs=pairs, **FOLD)
            assert info == dict(skew=1, skew_joined=1, skew_fold=1, skew_levels=K, skew_join_fold=1), info
            want1, launches1 = one[ndte, damping, K]
            print(f"launches {nxg}x{nyg} in {bsx}x{bsy} ns={ns} ndte={ndte} K={K}: {launches} (one block {launches1})")
            assert launches <= launches1 + JOIN_SPLIT_FOLD, (launches, launches1)
            if ndte == NDTE:
                assert launches < ndte and JOIN_SPLIT_FOLD < ndte
            for k in KEYS:
                assert np.array_equal(got[k], ref[k]), (ns, ndte, damping, K, graph, pairs, k, np.argwhere(got[k] != ref[k])[:6].tolist())
                assert np.array_equal(_global(dom, got, k, nxg, nyg), want1[k]), ("one block", ns, ndte, damping, K, k)
        # the switch off: today's path, today's bits
        got, info, launches = _run(ctx, grid, s, ndte, damping, info=("skew_joined", "skew_join_fold"), **dict(FOLD, skew_join_fold=0))
        assert info == dict(skew_joined=0, skew_join_fold=0) and launches == ndte
        for k in KEYS:
            assert np.array_equal(got[k], ref[k]), ("skew_join_fold = 0", ndte, damping, k)


@pytest.mark.parametrize("ns", [3, 4], ids=["tripole", "tripoleT"])
@pytest.mark.parametrize("nxg,nyg,bsx,bsy", [(96, 70, 48, 35), (300, 120, 15, 60), (96, 70, 40, 30)])
def test_ranges_and_a_second_step_under_a_fold(ctx, nxg, nyg, bsx, bsy, ns):
    """a loop cut into ranges (every range joins and splits; a single subcycle in between runs on the blocks, with its fold),
    then a second evp(dt) on the state the first one left"""
    dom, grid, s = _fold_case(ctx, nxg, nyg, bsx, bsy, ns)
    ref, _, _ = _run(ctx, grid, s, NDTE, False, **SINGLES)
    ref2 = {k: v.copy() for k, v in ref.items()}
    ctx.evp(DT, ref2)
    ctx.evp_init(grid, ndte=NDTE, krdg_partic=0, krdg_redist=0)
    for k, v in FOLD.items():
        ctx.evp_set_option(k, v)
    assert ctx.evp_get_info("skew_joined") == 1 and ctx.evp_get_info("skew_fold") == 1
    b = {k: v.copy() for k, v in s.items()}
    ctx.evp_upload(b); ctx.evp_prepare(DT)
    ctx.evp_subcycles(1, 8); ctx.evp_subcycles(9, 1); ctx.evp_subcycles(10, 3); ctx.evp_subcycles(13, NDTE - 12)
    ctx.evp_finish(); ctx.evp_download(b)
    for k in EVP_OUT_FIELDS:
        assert np.array_equal(b[k], ref[k]), ("ranges", k)
    got = {k: v.copy() for k, v in s.items()}
    ctx.evp(DT, got)
    for k in KEYS:
        assert np.array_equal(got[k], ref[k]), ("first evp(dt)", k)
    ctx.evp(DT, got)
    for k in KEYS:
        assert np.array_equal(got[k], ref2[k]), ("second evp(dt) on the state of the first", k)


@pytest.mark.parametrize("nxg,nyg,bsx,bsy", [(300, 120, 150, 60), (96, 70, 96, 18)])
def test_measured_balancing_under_a_fold(ctx, nxg, nyg, bsx, bsy):
    """the segment table of the sweep follows measured times (eager, measured sweeps; a new tuning phase every third loop);
    the band beside it does not care: the same bits every call"""
    dom, grid, s = _fold_case(ctx, nxg, nyg, bsx, bsy, 3)
    ref, _, _ = _run(ctx, grid, s, NDTE, False, **SINGLES)
    ctx.evp_init(grid, ndte=NDTE, krdg_partic=0, krdg_redist=0)
    for k, v in dict(FOLD, skew_balance=1, skew_balance_every=3).items():
        ctx.evp_set_option(k, v)
    assert ctx.evp_get_info("skew_joined") == 1 and ctx.evp_get_info("skew_fold") == 1 and ctx.evp_get_info("skew_balance") == 1
    for call in range(8):
        got = {k: v.copy() for k, v in s.items()}
        ctx.evp(DT, got)
        for k in KEYS:
            assert np.array_equal(got[k], ref[k]), (call, k)
    assert ctx.evp_get_info("skew_balanced") > 30


@pytest.mark.parametrize("nxg,nyg,bsx,bsy", [(300, 120, 15, 60), (96, 70, 48, 35)])
def test_fifty_replays_give_the_same_bits(ctx, nxg, nyg, bsx, bsy):
    """the sweep and the band run on two streams -- two branches of the captured graph: a missing edge between them shows
    up as a result that differs from call to call, or nowhere"""
    dom, grid, s = _fold_case(ctx, nxg, nyg, bsx, bsy, 3)
    ref, _, _ = _run(ctx, grid, s, NDTE, False, **SINGLES)
    ctx.evp_init(grid, ndte=NDTE, krdg_partic=0, krdg_redist=0)
    for k, v in dict(FOLD, use_graph=1).items():
        ctx.evp_set_option(k, v)
    assert ctx.evp_get_info("skew_joined") == 1
    for call in range(50):
        got = {k: v.copy() for k, v in s.items()}
        ctx.evp(DT, got)
        for k in KEYS:
            assert np.array_equal(got[k], ref[k]), (call, k)


def test_the_coupled_flavour_under_a_fold():
    """libcice4_amd_auscom.so (hemisphere-dependent turning angle, exp-free strength): against one launch per subcycle of
    the same library"""
    from test_oracle_auscom import NAMELISTS, two_hemispheres
    c = lib.Context(flavour="auscom")
    c.sync()
    nml = NAMELISTS[1]
    try:
        dom = c.domain_create(96, 70, 48, 35, ew=1, ns=3)
        gg = synth.global_grid(96, 70, perturb=0.15, land_frac=0.05, seed=3, land_rows=0)
        grid = two_hemispheres(synth.block_fields(gg, dom, ew_cyclic=True, north_ocean=True))
        s = synth.evp_state(grid, dom, seed=3, cover="patchy")
        rng = np.random.default_rng(3)
        s["ss_tltx"] = rng.uniform(-2e-5, 2e-5, s["ss_tltx"].shape); s["ss_tlty"] = rng.uniform(-2e-5, 2e-5, s["ss_tlty"].shape)
        c.set_auscom(**nml)
        for ndte, damping in ((NDTE, False), (7, True)):
            ref, info, launches = _run(c, grid, s, ndte, damping, info=("skew_joined",), **SINGLES)
            assert info["skew_joined"] == 0 and launches == ndte
            assert (ref["fm"] < 0).any() and (ref["fm"] > 0).any() and np.abs(ref["uvel"]).max() > 0.01
            for K in (4, 3):
                got, info, _ = _run(c, grid, s, ndte, damping, info=("skew", "skew_joined", "skew_fold"), skew_levels=K, **FOLD)
                assert info == dict(skew=1, skew_joined=1, skew_fold=1)
                for k in KEYS:
                    assert np.array_equal(got[k], ref[k]), (ndte, damping, K, k)
    finally:
        c.set_auscom()


def test_full_size_in_the_blocks_of_a_production_build_under_a_fold(ctx):
    """1440 x 1080 under a tripole fold in 192 blocks of 15 x 540, default options plus the switch"""
    nxg, nyg, ndte = 1440, 1080, 8
    dom1, grid1, s1 = _fold_case(ctx, nxg, nyg, nxg, nyg, 3)
    o1, info, launches1 = _run(ctx, grid1, s1, ndte, False, info=("skew", "skew_fold"))
    assert info == dict(skew=1, skew_fold=1)
    want = {k: _global(dom1, o1, k, nxg, nyg) for k in KEYS}
    del o1, grid1, s1
    dom, grid, s = _fold_case(ctx, nxg, nyg, 15, 540, 3)
    assert dom["nblocks"] == 192
    got, info, launches = _run(ctx, grid, s, ndte, False, info=("skew", "skew_joined", "skew_fold"), skew_join_fold=1)
    assert info == dict(skew=1, skew_joined=1, skew_fold=1) and launches <= launches1 + JOIN_SPLIT_FOLD
    for k in KEYS:
        assert np.array_equal(_global(dom, got, k, nxg, nyg), want[k]), k
