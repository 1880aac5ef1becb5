"""EVP subcycle rate of a ONE-RANK domain cut into several blocks: the one-launch loop (round 4) against one launch per
subcycle + on-rank halo copies (what such domains ran before), and the K-subcycle sweeps on a joined image of the blocks
(option "skew_join": larger grids; evp_subcycles(1, ndte) includes the join and the split).  With ns = 3 / 4 the grid has a
tripole fold ('tripole' / 'tripoleT', ocean up to it): the sweeps of several blocks then need option "skew_join_fold" (the
sweep on the image, a band of top rows on the blocks beside it), those of one block run as sweep + band (option "skew_fold").
usage: blocks_rate.py nxg nyg bsx bsy [ndte [repeats [ns]]]
Every form that applies to the layout is timed `repeats` times (default 3), alternating, in this one process."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (before the library: see bench.py)
torch.cuda.is_available()
from cice4_amd import lib, synth
nxg, nyg, bsx, bsy = (int(x) for x in sys.argv[1:5])
ndte = int(sys.argv[5]) if len(sys.argv) > 5 else 120
repeats = int(sys.argv[6]) if len(sys.argv) > 6 else 3
ns = int(sys.argv[7]) if len(sys.argv) > 7 else 0
ctx = lib.Context(device=0)
dom = ctx.domain_create(nxg, nyg, bsx, bsy, ew=1, ns=ns)
if ns:
    grid = synth.block_fields(synth.global_grid(nxg, nyg, land_rows=0), dom, ew_cyclic=True, north_ocean=True)
else:
    grid = synth.block_fields(synth.global_grid(nxg, nyg), dom)
state = synth.evp_state(grid, dom, cover="full")
FORMS = (("one launch per evp(dt) (k_evp_resident on %d blocks)" % dom["nblocks"], {"resident": 2}),
         ("one launch per subcycle (k_subcycle + on-rank halo)", {"resident": 0, "skew": 0, "fuse": 0}),
         ("K subcycles per sweep (k_subcycle_skew%s)" % (" on the joined image, join and split included" if dom["nblocks"] > 1 else ""),
          {"resident": 0, "skew": 1}))
if ns:
    fold = "ns = %d, " % ns
    FORMS = ((fold + "one launch per subcycle (k_subcycle + halo update with the fold; skew_join_fold = 0)", {"resident": 0, "skew": 0, "fuse": 0}),
             (fold + ("K subcycles per sweep (skew_join_fold = 1: k_subcycle_skew on the joined image + band on the blocks, join and split included)"
                      if dom["nblocks"] > 1 else "K subcycles per sweep (k_subcycle_skew + band of top rows)"),
              {"resident": 0, "skew": 1, "skew_fold": 1, "skew_join_fold": 1}))
for rep in range(repeats):
    for label, opts in FORMS:
        ctx.evp_init(grid, ndte=ndte)
        for k, v in opts.items():
            ctx.evp_set_option(k, v)
        if opts.get("resident") and not ctx.evp_get_info("resident") or opts.get("skew") and not ctx.evp_get_info("skew"):
            continue          # (the form does not apply to this layout: too large for the one-launch loop, too small for sweeps)
        ctx.evp_upload(state); ctx.evp_prepare(3600.0)
        for _ in range(5):
            ctx.evp_subcycles(1, ndte)
        ctx.sync()
        t0 = time.perf_counter(); n = 0
        while time.perf_counter() - t0 < 1.0:
            for _ in range(3 if nxg * nyg > 2000000 else 10):
                ctx.evp_subcycles(1, ndte)
                n += 1
            ctx.sync()
        dt = (time.perf_counter() - t0) / n
        print(f"{nxg}x{nyg} in {dom['nblocks']} blocks of {bsx}x{bsy}, run {rep + 1}: {label}: {dt / ndte * 1e6:.2f} us per subcycle "
              f"({ndte / dt:.0f} subcycles/s), launches per call {ctx.evp_get_info('last_launches')}, resident {ctx.evp_get_info('resident')}, "
              f"joined {ctx.evp_get_info('skew_joined')}" + (f", fold {ctx.evp_get_info('skew_fold')}" if ns else "")
              + (f", W = {ctx.evp_get_info('resident_waves')}, dense {ctx.evp_get_info('resident_dense')}" if ctx.evp_get_info('resident') else ""), flush=True)
