#!/usr/bin/env python3
"""Cost of the transport -> ridging hand-over (cice_ridge_chain) at gx1 size: 320 x 384 cells + ghosts, one block, on
synth.therm2_state "growth" made fit for ridging (scripts/ridge_cost.py: inputs), ice on the grid's ocean cells only,
velocities as bench.py makes them for its transport timing; host arrays page-locked.
One step = cice_transport_remap followed by cice_step_ridge (bound = 1) on the same seven state arrays.  The variants --
mode 0 (no hand-over: the yardstick), mode 1 (the download kept), mode 2 (the download deferred) -- take turns in ONE
process: ROUNDS rounds of 0, 1, 2, each STEPS timed steps after WARM untimed ones, every step from the same input.
Writes profiles/ridge_chain_cost.txt:
  * per variant the median of each round, the median of all timed steps and the extremes, for the pair and for either call;
  * whether the slowest round of a chained mode is below the fastest round of mode 0 ("faster in every round");
  * the device time of k_state_from_transport (HIP events, cice_ridge_chain_time; measured in steps of their own, a
    production call records none), the bytes it moves and the rate.
Run on a machine with a GPU:  python scripts/ridge_chain_cost.py"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from cice4_amd import lib, synth  # noqa: E402
from ridge_cost import inputs, NX, NY, DT  # noqa: E402

ROUNDS, STEPS, WARM = 4, 10, 2
SEVEN = ("aice0", "aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon")
PER_CELL = {"aice0": 1, "aicen": synth.NCAT, "vicen": synth.NCAT, "vsnon": synth.NCAT, "eicen": synth.NCAT * synth.NILYR,
            "esnon": synth.NCAT * synth.NSLYR}


def main():
    ctx = lib.Context()
    ctx.sync()
    dom = ctx.domain_create(NX - 2, NY - 2, NX - 2, NY - 2, ew=1, ns=0)
    grid = synth.block_fields(synth.global_grid(NX - 2, NY - 2), dom)
    ntrcr = 1
    ctx.transport_init({k: grid[k] for k in ("HTN", "HTE", "dxt", "dyt", "dxu", "dyu", "tarear", "hm")}, ntrcr=ntrcr,
                       trcr_depend=(0,))
    ctx.itd_init(synth.hin_max())
    ctx.ridge_init(krdg_partic=1, krdg_redist=1, mu_rdg=4.0)
    ctx.thermo_batch_alloc(NX, NY, 1)
    a = inputs("growth")
    ocean = grid["tmask"] != 0                       # ice where the transport's grid has ocean
    a["tmask"] = np.ascontiguousarray(grid["tmask"], np.int32)
    for k in ("aicen", "vicen", "vsnon", "eicen", "esnon"):
        a[k] = np.ascontiguousarray(np.where(ocean[:, None], a[k], 0.0))
    a["aice0"] = np.ascontiguousarray(np.where(ocean, a["aice0"], 1.0))
    jj, ii = np.meshgrid(np.arange(NY), np.arange(NX), indexing="ij")
    ts = {k: a[k] for k in SEVEN}
    ts["uvel"] = np.array(np.broadcast_to(0.2 * np.sin(2 * np.pi * ii / NX) * np.cos(np.pi * jj / NY), (1, NY, NX)))
    ts["vvel"] = np.array(np.broadcast_to(0.2 * np.cos(2 * np.pi * ii / NX) * np.sin(2 * np.pi * jj / NY), (1, NY, NX)))
    for d in (a, ts):
        for v in d.values():
            ctx.host_register(v)
    first = {k: v.copy() for k, v in dict(a, **ts).items()}

    def step():
        for k, v in first.items():
            (ts if k in ("uvel", "vvel") else a)[k][...] = v
        t0 = time.perf_counter()
        rc = ctx.transport_remap(DT, ts)
        t1 = time.perf_counter()
        r = ctx.step_ridge(DT, a, bound=True)
        t2 = time.perf_counter()
        assert rc == (0, 0, 0) and r["l_stop"] == 0, (rc, r)
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3

    want = None
    rounds = {m: [] for m in (0, 1, 2)}              # per mode: one list of (transport, ridge) per round
    for _ in range(ROUNDS):
        for mode in (0, 1, 2):
            ctx.ridge_chain(mode)
            got = [step() for _ in range(WARM + STEPS)][WARM:]
            rounds[mode].append(got)
            out = {k: a[k].copy() for k in SEVEN + ("aice", "vice", "dardg1dt")}
            if want is None:
                want = out
                assert np.abs(want["dardg1dt"]).max() > 0.0
            for k in want:
                assert np.array_equal(out[k], want[k]), ("mode", mode, k)
    ev = []
    ctx.ridge_chain(1)
    ctx.ridge_chain_time(True)
    for _ in range(WARM + STEPS):
        step()
        ev.append(ctx.ridge_chain_time(True))
    ctx.ridge_chain_time(False)
    ctx.ridge_chain(0)
    ctx.host_unregister_all()

    med = statistics.median
    lines = [f"cice_transport_remap + cice_step_ridge at gx1 size ({NX - 2} x {NY - 2} + ghosts, one block, bound = 1, ntrcr = "
             f"{ntrcr}), page-locked host arrays; {ROUNDS} rounds of mode 0, 1, 2 in turn, {STEPS} timed steps per round "
             f"after {WARM}; ms per step"]
    pair_rounds = {}
    for mode in (0, 1, 2):
        pr = [med(t + r for t, r in g) for g in rounds[mode]]
        pair_rounds[mode] = pr
        allp = [t + r for g in rounds[mode] for t, r in g]
        allt = [t for g in rounds[mode] for t, _ in g]
        allr = [r for g in rounds[mode] for _, r in g]
        lines.append(f"mode {mode}: pair median {med(allp):.2f} (min {min(allp):.2f}, max {max(allp):.2f}); round medians "
                     + " ".join(f"{x:.2f}" for x in pr) + f"; transport_remap {med(allt):.2f} ({min(allt):.2f} - {max(allt):.2f}), "
                     f"step_ridge {med(allr):.2f} ({min(allr):.2f} - {max(allr):.2f})")
    for mode in (1, 2):
        yes = max(pair_rounds[mode]) < min(pair_rounds[0])
        lines.append(f"mode {mode} against mode 0: slowest round {max(pair_rounds[mode]):.2f}, fastest round of mode 0 "
                     f"{min(pair_rounds[0]):.2f}: {'faster in every interleaved round' if yes else 'NOT faster in every interleaved round'}; "
                     f"median saving {med(pair_rounds[0]) - med(pair_rounds[mode]):.2f} ms")
    planes = sum(PER_CELL.values()) + synth.NCAT * ntrcr
    nbytes = planes * NX * NY * 8
    us = med(ev[WARM:]) * 1e3
    lines.append(f"k_state_from_transport: {planes} planes of {NX * NY} cells, {nbytes / 1e6:.1f} MB read and as much written; "
                 f"event time median {us:.1f} us (min {min(ev[WARM:]) * 1e3:.1f}, max {max(ev[WARM:]) * 1e3:.1f}), "
                 f"{2 * nbytes / (us * 1e-6) / 1e9:.0f} GB/s read + written")
    lines.append("all modes gave the same bits (seven state arrays, aice, vice, dardg1dt) in every round")
    out = os.path.join(ROOT, "profiles", "ridge_chain_cost.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
