#!/usr/bin/env python3
"""Cost of ridging at gx1 size: 320 x 384 cells + ghosts, one block, on synth.therm2_state "growth" and "melt" made fit for
ridging (areas brought to a sum <= 1 as for the cleanup; open water such that the total area is off 1 by up to 2e-3 either
way, as the transport leaves it; rdg_conv up to 1e-6 1/s on half of the cells, rdg_shear up to 2e-6 1/s).
Writes profiles/ridge_cost.txt:
  * device time per kernel and per iteration of cice_step_ridge's stage 1 (HIP events, cice_ridge_times; a production call
    records none), median of 20 calls after 3 warm-up calls, and how many iterations were queued;
  * the iterations the block took (cice_ridge_ice's niter);
  * wall time of the whole block-wise call cice_ridge_ice and of the whole cice_step_ridge (bound = 1) over PCIe;
  * the reference's time for ridge_ice is NOT measured here (the reference does not exist on a GPU box): run
    `python tests/golden/make_golden_ridge.py --time` on the build machine and add its lines to the file.
Run on a machine with a GPU:  python scripts/ridge_cost.py"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from cice4_amd import lib, synth  # noqa: E402
from therm2_cleanup_cost import capped  # noqa: E402

NX, NY, DT, REPS, WARM = 322, 386, 3600.0, 20, 3
STATE = ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon")
PUNY = 1.0e-11


def inputs(regime, nx=NX, ny=NY, nb=1, seed=7):
    """the arrays of cice_step_ridge (and with them those of cice_ridge_ice per block)"""
    s = capped(synth.therm2_state(regime, nx, ny, nb, seed=seed))
    rng = np.random.default_rng(seed + 100)
    shp = s["aice"].shape
    a = {k: np.ascontiguousarray(s[k]) for k in STATE + ("tmask", "fresh", "fsalt", "fhocn")}
    tot = np.zeros(shp)
    for n in range(synth.NCAT):
        tot = tot + a["aicen"][:, n]
    a["aice0"] = np.maximum(np.maximum(1.0 - tot, 0.0) + rng.uniform(-2.0e-3, 2.0e-3, shp), 0.0)
    nothing = ~((a["aice0"] > PUNY) | (a["aicen"] > PUNY).any(axis=1))
    a["aice0"][nothing] = 1.0
    a["rdg_conv"] = np.where(rng.random(shp) < 0.5, rng.uniform(0.0, 1.0e-6, shp), 0.0)
    a["rdg_shear"] = rng.uniform(0.0, 2.0e-6, shp)
    for k in ("dardg1dt", "dardg2dt", "dvirdgdt", "opening", "aice", "vice", "vsno", "eice", "esno"):
        a[k] = np.zeros(shp)
    a["trcr"] = np.zeros((shp[0], 5) + shp[1:])
    a["daidtd"], a["dvidtd"] = rng.uniform(0, 1, shp), rng.uniform(0, 3, shp)
    return a


def main():
    ctx = lib.Context()
    ctx.sync()
    ctx.domain_create(NX - 2, NY - 2, NX - 2, NY - 2, ew=1, ns=0)
    ctx.itd_init(synth.hin_max())
    ctx.ridge_init(krdg_partic=1, krdg_redist=1, mu_rdg=4.0)
    ctx.thermo_batch_alloc(NX, NY, 1)
    lines = [f"cice_step_ridge at gx1 size ({NX - 2} x {NY - 2} + ghosts, one block, bound = 1), median of {REPS} after {WARM}"]
    for regime in ("growth", "melt"):
        s = inputs(regime)
        jj, ii = np.nonzero(s["tmask"][0][1:-1, 1:-1])
        indxi, indxj = np.zeros(NX * NY, np.int32), np.zeros(NX * NY, np.int32)
        indxi[:len(ii)], indxj[:len(ii)] = ii + 2, jj + 2
        dev, wall, wall_b, niter = [], [], [], 0
        ctx.ridge_times(enable=True)
        for k in range(WARM + REPS):
            a = {key: v.copy() for key, v in s.items()}
            t0 = time.perf_counter()
            r = ctx.step_ridge(DT, a, bound=True)
            t1 = time.perf_counter()
            assert r["l_stop"] == 0, r
            blk = {key: np.ascontiguousarray(v[0]) for key, v in s.items() if key not in ("trcr",)}
            t2 = time.perf_counter()
            rb = ctx.ridge_ice(len(ii), indxi, indxj, DT, blk)
            t3 = time.perf_counter()
            assert rb[0] == 0, rb
            niter = rb[3]
            if k >= WARM:
                dev.append(ctx.ridge_times())
                wall_b.append((t3 - t2) * 1e3)
        ctx.ridge_times(enable=False)                 # a production call records no events
        for k in range(WARM + REPS):
            a = {key: v.copy() for key, v in s.items()}
            t0 = time.perf_counter()
            assert ctx.step_ridge(DT, a, bound=True)["l_stop"] == 0
            if k >= WARM:
                wall.append((time.perf_counter() - t0) * 1e3)
        med = {n: statistics.median(x[n] for x in dev) * 1e3 for n in lib.RIDGE_TIMES}
        queued = max(i for i in range(1, lib.RIDGE_NITERMAX + 1) if med[f"rates{i}"] > 0.0)
        per = ", ".join(f"{i}: rates {med[f'rates{i}']:.1f} + shift {med[f'shift{i}']:.1f}" for i in range(1, queued + 1))
        lines.append(f"{regime}: {len(ii)} listed cells, the block took {niter} iteration(s), {queued} queued; kernels (us) per "
                     f"iteration {per}; diagnostics {med['finish']:.1f}; ridging together {sum(med.values()):.1f} us")
        lines.append(f"{regime}: whole cice_ridge_ice (block-wise, host pointers) over PCIe: {statistics.median(wall_b):.2f} ms")
        lines.append(f"{regime}: whole cice_step_ridge (ridge_ice, cleanup_itd, bound_state, aggregate) over PCIe: "
                     f"{statistics.median(wall):.2f} ms")
    lines.append("reference on one core of the build machine: see `python tests/golden/make_golden_ridge.py --time`")
    out = os.path.join(ROOT, "profiles", "ridge_cost.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
