"""The granule loop of k_evp_resident after its hand-off chain was shortened: the momentum equation in two halves (the
half that needs no stress runs in front of the wait for the str row of the wavefront above), the read-only LDS inputs
read in front of the waits, lane 0's western / south-western velocities handed over by v_readlane from the lane that
lent its poll slot, shifts that leave the lane without a source zero, one priority schedule in the product build.

None of it changes a value: every case compares the one-launch loop (resident = 2, resident_granules = 1,
resident_dense = 0) with one launch per subcycle (resident = 0, fuse = 0) by np.array_equal on every output field of
evp(dt) plus iceumask -- strintx, strinty, strocnx, strocny, which the head / tail split produces, among them -- and
asserts afterwards that the loop ran (a fall-back cannot pass for it).

Grids: the smallest at which each changed piece can go wrong, all east-west cyclic, perturbed metrics, 5 % land."""
import numpy as np
import pytest

from cice4_amd import synth

pytestmark = pytest.mark.gpu

DT = 3600.0
EVP_OUT_FIELDS = ("uvel", "vvel", "strength", "divu", "shear", "rdg_conv", "rdg_shear", "prs_sig",
                  "strocnxT", "strocnyT", "strocnx", "strocny", "strintx", "strinty", "strairx",
                  "strairy", "fm", "strtltx", "strtlty") + synth.SIG_NAMES
KEYS = EVP_OUT_FIELDS + ("iceumask",)

GRIDS = [
    pytest.param(64, 9, 0, id="64x9-second-tile-column-owns-one-column"),   # the lanes that lend lane 0 their slot lie outside the block
    pytest.param(127, 7, 0, id="127x7-three-tile-columns"),
    pytest.param(7, 6, 0, id="7x6-narrower-than-a-tile"),
    pytest.param(63, 18, 0, id="63x18-full-row"),        # W = 4: lanes 1 .. 62 of wavefront 0 lend slot A, the other wavefronts slot B
    pytest.param(66, 10, 3, id="66x10-tripole"),         # the FOLD instantiation shares the loop
]


def _case(ctx, nxg, nyg, ns, cover):
    dom = ctx.domain_create(nxg, nyg, nxg, nyg, ew=1, ns=ns)
    fold = ns != 0
    gg = synth.global_grid(nxg, nyg, perturb=0.15, land_frac=0.05, seed=nxg + nyg, **({"land_rows": 0} if fold else {}))
    grid = synth.block_fields(gg, dom, ew_cyclic=True, north_ocean=fold)
    s = synth.evp_state(grid, dom, seed=nxg, cover=cover)
    return grid, s, fold


def _per_subcycle(ctx, grid, s, fold, ndte, damping, calls=2):
    """one launch per subcycle; `calls` evp(dt) in a row on the carried state, the outputs of each"""
    ctx.evp_init(grid, ndte=ndte, evp_damping=damping, krdg_partic=0, krdg_redist=0)
    ctx.evp_set_option("resident", 0); ctx.evp_set_option("fuse", 0)
    if fold:
        ctx.evp_set_option("resident_fold", 0)
    sg = {k: v.copy() for k, v in s.items()}
    outs = []
    for _ in range(calls):
        ctx.evp(DT, sg)
        outs.append({k: sg[k].copy() for k in KEYS})
    assert ctx.evp_get_info("resident") == 0
    return outs


def _one_launch(ctx, grid, s, fold, ndte, damping, W, ref, what, prio=None):
    ctx.evp_init(grid, ndte=ndte, evp_damping=damping, krdg_partic=0, krdg_redist=0)
    if fold:
        ctx.evp_set_option("resident_fold", 1)
    ctx.evp_set_option("resident_dense", 0); ctx.evp_set_option("resident", 2); ctx.evp_set_option("resident_waves", W)
    ctx.evp_set_option("resident_granules", 1)
    if prio is not None:
        ctx.evp_set_option("resident_prio", prio)
    try:
        assert ctx.evp_get_info("resident") == 1, ("not offered", what)
        assert ctx.evp_get_info("resident_granules") == 1 and ctx.evp_get_info("resident_dense") == 0, what
        sg = {k: v.copy() for k, v in s.items()}
        for call, want in enumerate(ref):       # the second call: the tags of the granules grow across launches
            ctx.evp(DT, sg)
            assert ctx.evp_get_info("resident") == 1, ("fell back", what, call)
            assert ctx.evp_get_info("last_launches") == 1, (what, call)
            for k in KEYS:
                assert np.array_equal(sg[k], want[k]), (what, call, k, np.argwhere(sg[k] != want[k])[:6].tolist())
    finally:
        ctx.evp_set_option("resident_waves", 0); ctx.evp_set_option("resident_dense", 1); ctx.evp_set_option("resident_prio", 2)


@pytest.mark.parametrize("cover", ["full", "patchy"])
@pytest.mark.parametrize("nxg,nyg,ns", GRIDS)
def test_granule_loop_bit_for_bit(ctx, nxg, nyg, ns, cover):
    """ndte 1 (no hand-off: only the last-subcycle path), 2 (one hand-off), 3; damping off and on; 4 and 11 wavefronts (11
    on these heights: one tile row, the upper wavefronts idle); a second evp(dt) on the carried state."""
    grid, s, fold = _case(ctx, nxg, nyg, ns, cover)
    for ndte in (1, 2, 3):
        for damping in (False, True):
            ref = _per_subcycle(ctx, grid, s, fold, ndte, damping)
            if cover == "full" and nyg >= 9 and ndte == 3:
                assert np.abs(ref[0]["uvel"]).max() > 0.0 and np.abs(ref[0]["strintx"]).max() > 0.0
            for W in (4, 11):
                _one_launch(ctx, grid, s, fold, ndte, damping, W, ref, (nxg, nyg, ns, cover, ndte, damping, W))


@pytest.mark.parametrize("prio", [3, 5])
def test_fenced_priority_schedules_are_accepted(ctx, prio):
    """resident_prio 3 and 5 measured slower and are compiled in experiment builds only: the option is still accepted,
    the product build runs its default schedule in their place, and the bits are the same."""
    grid, s, fold = _case(ctx, 127, 7, 0, "patchy")
    ref = _per_subcycle(ctx, grid, s, fold, 3, False, calls=1)
    for W in (4, 11):
        _one_launch(ctx, grid, s, fold, 3, False, W, ref, ("prio", prio, W), prio=prio)
