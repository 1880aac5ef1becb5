"""K-subcycle sweeps on a ONE-TASK domain cut into several blocks: the subcycle loop joins the blocks into one full-width
image, runs k_subcycle_skew on it and hands the result back (cice4_amd/csrc/join.hip, option "skew_join", info
"skew_joined").  Bit for bit -- every output field, whole block arrays, ghost cells included -- against one launch per
subcycle on the same blocks, and on the physical cells against the sweep on the same grid as one block."""
import numpy as np
import pytest

from cice4_amd import lib, synth
from test_gpu_evp import DT, NDTE, EVP_OUT_FIELDS
import ranks_case

pytestmark = pytest.mark.gpu
KEYS = EVP_OUT_FIELDS + ("iceumask",)
# kernel launches a visit to the image adds to the sweeps themselves: the join (state into both copies of the image), the
# split of the state and, behind the sweep that ends evp(dt), the split of the diagnostics it leaves
JOIN_SPLIT = 3


def _cuts(nxg, nyg):
    c = lambda a, b: -(-a // b)
    return [(c(nxg, 2), c(nyg, 2)), (c(nxg, 4), nyg), (nxg, c(nyg, 4))]


# grids whose widths the one-block sweep is proven on (test_k_subcycles_per_sweep), each as 2 x 2, 4 x 1 and 1 x 4 blocks;
# 200 x 50 in blocks of 64 x 16 (last blocks padded both ways), 300 x 120 in blocks of 15 x 60 (20 x 2 of them)
GRIDS = [(96, 70, 1), (200, 50, 1), (300, 120, 1), (111, 14, 1), (400, 30, 0), (130, 27, 2)]
LAYOUTS = [(nxg, nyg, ew, bsx, bsy) for nxg, nyg, ew in GRIDS for bsx, bsy in _cuts(nxg, nyg)] + \
          [(200, 50, 1, 64, 16), (300, 120, 1, 15, 60)]


def _case(c, nxg, nyg, ew, bsx, bsy, ns=0, cover="patchy", **grid_kw):
    dom = c.domain_create(nxg, nyg, bsx, bsy, ew=ew, ns=ns)
    gg = synth.global_grid(nxg, nyg, perturb=0.15, land_frac=0.05, seed=nxg + nyg, **grid_kw)
    grid = synth.block_fields(gg, dom, ew_cyclic=(ew == 1), north_ocean=ns in (3, 4))
    return dom, grid, synth.evp_state(grid, dom, seed=nxg, cover=cover)


def _run(c, grid, s, ndte, damping, info=(), **opts):
    sg = {k: v.copy() for k, v in s.items()}
    c.evp_init(grid, ndte=ndte, evp_damping=damping, krdg_partic=0, krdg_redist=0)
    for k, v in opts.items():
        c.evp_set_option(k, v)
    before = {k: c.evp_get_info(k) for k in info}
    c.evp(DT, sg)
    return sg, before, c.evp_get_info("last_launches")


SWEEP = dict(resident=0, skew=1, skew_min_cells=0)
SINGLES = dict(resident=0, skew=0, fuse=0)
RUNS = [(NDTE, False), (7, True), (13, False)]      # 13: three sweeps of four and a tail of one launch on the blocks


def _global(dom, s, k, nxg, nyg):
    return ranks_case.assemble_blocks([(dom, s)], k, nxg, nyg)


@pytest.mark.parametrize("nxg,nyg,ew,bsx,bsy", LAYOUTS)
def test_sweeps_on_the_joined_image(ctx, nxg, nyg, ew, bsx, bsy):
    """every K of the product build, graph and eager, both layouts of the image's state, subcycle counts that are no
    multiple of K, damping, ranges, carried state, and the switch"""
    # the same grid as ONE block: what the image has to reproduce on the physical cells, and its launches
    dom1, grid1, s1 = _case(ctx, nxg, nyg, ew, nxg, nyg)
    one = {}
    for ndte, damping in RUNS:
        for K in (4, 2, 3):
            if K != 4 and (ndte, damping) != (NDTE, False):
                continue
            o, info, launches = _run(ctx, grid1, s1, ndte, damping, info=("skew", "skew_pairs"), skew_levels=K, **SWEEP)
            assert info["skew"] == 1
            one[ndte, damping, K] = ({k: _global(dom1, o, k, nxg, nyg) for k in KEYS}, launches, info["skew_pairs"])
    dom, grid, s = _case(ctx, nxg, nyg, ew, bsx, bsy)
    assert dom["nblocks"] >= 4
    for ndte, damping in RUNS:
        ref, info, launches = _run(ctx, grid, s, ndte, damping, info=("skew", "skew_joined"), **SINGLES)
        assert info == dict(skew=0, skew_joined=0) and launches == ndte
        for K, graph, pairs in ((4, 1, 1), (4, 0, 1), (4, 1, 0), (2, 1, 1), (3, 0, 1)):
            if (ndte, damping, K) not in one:
                continue
            got, info, launches = _run(ctx, grid, s, ndte, damping, info=("skew", "skew_joined", "skew_levels", "skew_pairs"),
                                       skew_levels=K, use_graph=graph, skew_pairs=pairs, **SWEEP)
            want1, launches1, pairs1 = one[ndte, damping, K]
            assert info["skew"] == 1 and info["skew_joined"] == 1 and info["skew_levels"] == K
            assert info["skew_pairs"] == (pairs1 if pairs else 0)       # the layout the one-block sweep of this grid takes
            # (sweeps, a tail shorter than K on the blocks, one visit to the image: far below one launch per subcycle)
            assert launches <= launches1 + JOIN_SPLIT and launches <= ndte // K + K - 1 + JOIN_SPLIT, (launches, launches1, ndte)
            for k in KEYS:
                assert np.array_equal(got[k], ref[k]), (ndte, damping, K, graph, pairs, k, np.argwhere(got[k] != ref[k])[:6].tolist())
                assert np.array_equal(_global(dom, got, k, nxg, nyg), want1[k]), ("one block", ndte, damping, K, k)
        # the switch: today's path, same bits
        got, info, launches = _run(ctx, grid, s, ndte, damping, info=("skew", "skew_joined"), skew_join=0, **SWEEP)
        assert info == dict(skew=0, skew_joined=0) and launches == ndte
        for k in KEYS:
            assert np.array_equal(got[k], ref[k]), ("skew_join = 0", ndte, damping, k)
    # a loop cut into ranges (every range joins and splits; a single subcycle in between runs on the blocks), then a second
    # evp(dt) on the state the first one left
    ref, _, _ = _run(ctx, grid, s, NDTE, False, **SINGLES)
    ref2 = {k: v.copy() for k, v in ref.items()}
    ctx.evp(DT, ref2)
    ctx.evp_init(grid, ndte=NDTE, krdg_partic=0, krdg_redist=0)
    for k, v in SWEEP.items():
        ctx.evp_set_option(k, v)
    assert ctx.evp_get_info("skew_joined") == 1
    b = {k: v.copy() for k, v in s.items()}
    ctx.evp_upload(b); ctx.evp_prepare(DT)
    ctx.evp_subcycles(1, 8); ctx.evp_subcycles(9, 1); ctx.evp_subcycles(10, 3); ctx.evp_subcycles(13, NDTE - 12)
    ctx.evp_finish(); ctx.evp_download(b)
    for k in EVP_OUT_FIELDS:
        assert np.array_equal(b[k], ref[k]), ("ranges", k)
    got = {k: v.copy() for k, v in s.items()}
    ctx.evp(DT, got)
    ctx.evp(DT, got)
    for k in KEYS:
        assert np.array_equal(got[k], ref2[k]), ("second evp(dt) on the state of the first", k)


@pytest.mark.parametrize("nxg,nyg,ew,bsx,bsy", [(300, 120, 1, 150, 60), (96, 70, 1, 96, 18), (400, 30, 0, 100, 30)])
def test_measured_balancing_sees_the_image_as_one_block(ctx, nxg, nyg, ew, bsx, bsy):
    """the segment table follows the measured cost of its rows (eager, measured sweeps; a new tuning phase every third
    loop): any partition gives the same bits"""
    dom, grid, s = _case(ctx, nxg, nyg, ew, bsx, bsy)
    ref, _, _ = _run(ctx, grid, s, NDTE, False, **SINGLES)
    ctx.evp_init(grid, ndte=NDTE, krdg_partic=0, krdg_redist=0)
    for k, v in dict(SWEEP, skew_balance=1, skew_balance_every=3).items():
        ctx.evp_set_option(k, v)
    assert ctx.evp_get_info("skew_joined") == 1 and ctx.evp_get_info("skew_balance") == 1
    for call in range(8):
        got = {k: v.copy() for k, v in s.items()}
        ctx.evp(DT, got)
        for k in KEYS:
            assert np.array_equal(got[k], ref[k]), (call, k)
    assert ctx.evp_get_info("skew_balanced") > 30


@pytest.mark.parametrize("ns", [3, 4], ids=["tripole", "tripoleT"])
def test_a_fold_over_several_blocks_keeps_its_path(ctx, ns):
    nxg, nyg = 96, 70
    dom1, grid1, s1 = _case(ctx, nxg, nyg, 1, nxg, nyg, ns=ns, land_rows=0)
    o1, _, _ = _run(ctx, grid1, s1, NDTE, False, **SWEEP)
    want = {k: _global(dom1, o1, k, nxg, nyg) for k in KEYS}
    dom, grid, s = _case(ctx, nxg, nyg, 1, 48, 35, ns=ns, land_rows=0)
    got, info, launches = _run(ctx, grid, s, NDTE, False, info=("skew_joined",), **SWEEP)
    assert info["skew_joined"] == 0 and launches == NDTE
    for k in KEYS:
        assert np.array_equal(_global(dom, got, k, nxg, nyg), want[k]), (ns, k)


def test_the_coupled_flavour_on_the_joined_image(orc_aus):
    """libcice4_amd_auscom.so: the hemisphere-dependent turning angle travels with the cell; against the checker"""
    from test_oracle_auscom import NAMELISTS, two_hemispheres
    c = lib.Context(flavour="auscom")
    c.sync()
    nml = NAMELISTS[1]
    try:
        dom = c.domain_create(96, 70, 48, 35, ew=1, ns=0)
        grid = two_hemispheres(synth.block_fields(synth.global_grid(96, 70, perturb=0.15, land_frac=0.05, seed=3), dom))
        s = synth.evp_state(grid, dom, seed=3, cover="patchy")
        rng = np.random.default_rng(3)
        s["ss_tltx"] = rng.uniform(-2e-5, 2e-5, s["ss_tltx"].shape); s["ss_tlty"] = rng.uniform(-2e-5, 2e-5, s["ss_tlty"].shape)
        c.set_auscom(**nml); orc_aus.set_auscom(True, **nml)
        for ndte, damping in ((NDTE, False), (7, True)):
            orc_aus.set_evp_parameters(DT, ndte, damping); orc_aus.set_strength_parameters(1, 0, 0, 4.0)   # exp-free: bit for bit
            so = {k: v.copy() for k, v in s.items()}
            orc_aus.evp(orc_aus.make_domain(dom, grid), so)
            orc_aus.set_strength_parameters()
            assert (so["fm"] < 0).any() and (so["fm"] > 0).any() and np.abs(so["uvel"]).max() > 0.01
            for K in (4, 3):
                got, info, _ = _run(c, grid, s, ndte, damping, info=("skew", "skew_joined"), skew_levels=K, **SWEEP)
                assert info == dict(skew=1, skew_joined=1)
                for k in KEYS:
                    assert np.array_equal(got[k], so[k]), (ndte, damping, K, k)
    finally:
        c.set_auscom()


def test_full_size_in_the_blocks_of_a_production_build(ctx):
    """1440 x 1080 in 192 blocks of 15 x 540, default options: the sweeps take the image unasked"""
    nxg, nyg, ndte = 1440, 1080, 8
    dom1, grid1, s1 = _case(ctx, nxg, nyg, 1, nxg, nyg)
    o1, info, launches1 = _run(ctx, grid1, s1, ndte, False, info=("skew", "skew_joined"))
    assert info == dict(skew=1, skew_joined=0) 
    want = {k: _global(dom1, o1, k, nxg, nyg) for k in KEYS}
    del o1, grid1, s1
    dom, grid, s = _case(ctx, nxg, nyg, 1, 15, 540)
    assert dom["nblocks"] == 192
    got, info, launches = _run(ctx, grid, s, ndte, False, info=("skew", "skew_joined", "skew_pairs"))
    assert info == dict(skew=1, skew_joined=1, skew_pairs=1) and launches <= launches1 + JOIN_SPLIT
    for k in KEYS:
        assert np.array_equal(_global(dom, got, k, nxg, nyg), want[k]), k
