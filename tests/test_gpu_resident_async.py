"""One-launch EVP loops queued back to back (option "resident_async", the default): an untimed cice_evp_subcycles that takes
the one-launch loop of a one-rank domain returns with its launch pending, and the records of the pending launches are looked
at by the next entry that needs the outcome (Evp::retire_resident).  Everything here is compared, bit for bit, with the same
calls under resident_async = 0, which waits behind every launch as the library always did.

The late fall-back uses the library's own bounded time-out the way tests/test_gpu_evp.py::test_resident_loop_gives_up_cleanly
does: with resident_spin_us = 0 every wait of a tile fails at once, the launch raises its abort word and leaves the caller's
state as it was.  Under that setting every queued launch would give up by itself, so this cannot tell a launch that left at
once under another's abort word from one that gave up on its own: the bookkeeping for record sequences a device does not
produce on demand (clean, aborted, clean) is pinned host-side in tests/test_resident_async_plan.py.  One pass each; nothing
is run again after a failure."""
import numpy as np
import pytest

from cice4_amd import synth

pytestmark = pytest.mark.gpu

DT, NDTE = 3600.0, 120
RING = 16      # Evp::RES_RING
STATE = ("uvel", "vvel") + synth.SIG_NAMES


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _setup(ctx, nxg, nyg, ns, cover, ndte):
    dom = ctx.domain_create(nxg, nyg, nxg, nyg, ew=1, ns=ns)
    fold = ns in (3, 4)
    gg = synth.global_grid(nxg, nyg, perturb=0.15, land_frac=0.05, seed=5, land_rows=0 if fold else 2)
    grid = synth.block_fields(gg, dom, ew_cyclic=True, north_ocean=fold)
    s = synth.evp_state(grid, dom, seed=3, cover=cover)
    return dom, grid, s


def _steps(ctx, grid, s, ndte, ncalls, async_on, opts=(), watch=None):
    """ncalls untimed loops over the whole range behind one prepare; returns the downloaded state and what the library says"""
    ctx.evp_init(grid, ndte=ndte, krdg_partic=0, krdg_redist=0)
    ctx.evp_set_option("resident", 2)
    for k, v in opts:
        ctx.evp_set_option(k, v)
    ctx.evp_set_option("resident_async", async_on)
    sg = {k: v.copy() for k, v in s.items()}
    ctx.evp_upload(sg)
    ctx.evp_prepare(DT)
    depth = []
    for _ in range(ncalls):
        ctx.evp_subcycles(1, ndte)
        depth.append(ctx.evp_get_info("resident_pending"))
    if watch is not None:
        watch(depth)
    info = {k: ctx.evp_get_info(k) for k in ("resident", "resident_dense", "last_launches")}
    assert ctx.evp_get_info("resident_pending") == 0      # any other key looks at the records first
    ctx.evp_finish()
    ctx.evp_download(sg)
    return sg, info, depth


@pytest.mark.parametrize("nxg,nyg,ns,cover", [(320, 384, 0, "full"), (320, 384, 0, "caps"), (96, 70, 3, "full")],
                         ids=["gx1-full", "gx1-caps", "fold"])
def test_queued_loops_give_the_bits_of_waited_loops(ctx, nxg, nyg, ns, cover):
    """N = 6 consecutive untimed loops, open north at gx1 size (full cover, polar caps) and under a tripole fold"""
    dom, grid, s = _setup(ctx, nxg, nyg, ns, cover, NDTE)
    ref, iref, dref = _steps(ctx, grid, s, NDTE, 6, 0)
    assert dref == [0] * 6 and iref["resident"] == 1 and iref["last_launches"] == 1

    def watch(depth):
        assert depth == [1, 2, 3, 4, 5, 6], depth           # > 0 before the first query ...
        ctx.sync()
        assert ctx.evp_get_info("resident_pending") == 0    # ... and 0 after sync()

    got, info, _ = _steps(ctx, grid, s, NDTE, 6, 1, watch=watch)
    assert info["resident"] == 1 and info["last_launches"] == 1, info
    assert info == iref
    assert np.nanmax(np.abs(got["uvel"])) > 0.0
    for k in STATE:
        assert _same_bits(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:6].tolist())


@pytest.mark.parametrize("gran", [1, 0], ids=["granules", "progress-words"])
def test_a_late_fall_back_leaves_what_waited_loops_leave(ctx, capfd, gran):
    """Four loops queued, the first of which gives up: found out at the first query.  The launches behind it left at once;
    all four ranges run again as the calls they were.  The granule loop falls back for good (one message); the dense shape
    falls back to one workgroup per CU, which the second range then tries and, every wait failing, gives up as well (two
    messages, as with a wait behind every loop).  State, `resident`, `resident_dense`, `last_launches`: those of the waited run."""
    dom, grid, s = _setup(ctx, 320, 384, 0, "patchy", 12)
    opts = (("resident_spin_us", 0), ("resident_granules", gran))
    capfd.readouterr()
    ref, iref, _ = _steps(ctx, grid, s, 12, 4, 0, opts)
    msgs_ref = capfd.readouterr().err.count("resident EVP loop timed out")
    assert iref["resident"] == 0 and msgs_ref == (1 if gran else 2), (iref, msgs_ref)
    got, info, depth = _steps(ctx, grid, s, 12, 4, 1, opts)
    msgs = capfd.readouterr().err.count("resident EVP loop timed out")
    ctx.evp_set_option("resident_spin_us", 200000)
    assert depth == [1, 2, 3, 4], depth
    assert info == iref and info["resident"] == 0, (info, iref)
    assert msgs == msgs_ref, (msgs, msgs_ref)
    for k in STATE:
        assert _same_bits(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:6].tolist())
    # and against the loop that never was the one-launch loop
    ctx.evp_init(grid, ndte=12, krdg_partic=0, krdg_redist=0)
    ctx.evp_set_option("resident", 0)
    plain = {k: v.copy() for k, v in s.items()}
    ctx.evp_upload(plain); ctx.evp_prepare(DT)
    for _ in range(4):
        ctx.evp_subcycles(1, 12)
    assert ctx.evp_get_info("resident_pending") == 0
    ctx.evp_finish(); ctx.evp_download(plain)
    for k in STATE:
        assert _same_bits(got[k], plain[k]), k


def test_more_calls_than_records(ctx):
    """2 * RING + 3 calls: the depth never exceeds RING (a full ring is looked at before the next launch), same bits"""
    dom, grid, s = _setup(ctx, 320, 384, 0, "full", 12)
    n = 2 * RING + 3
    ref, iref, _ = _steps(ctx, grid, s, 12, n, 0)
    got, info, depth = _steps(ctx, grid, s, 12, n, 1)
    assert max(depth) == RING and min(depth) >= 1, depth
    assert depth == [(k % RING) + 1 for k in range(n)], depth
    assert info == iref and info["resident"] == 1 and info["last_launches"] == 1
    for k in STATE:
        assert _same_bits(got[k], ref[k]), k
