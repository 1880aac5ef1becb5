#!/usr/bin/env python3
"""Cost of the thickness-distribution stage (cice_step_therm2_itd) at gx1 size: 320 x 384 cells + ghosts, one block,
synth.therm2_state "growth" and "melt".  Writes profiles/therm2_itd_cost.txt:
  * device time of the kernels of the call (HIP events around each launch, cice_therm2_itd_times), median of 20 calls
    after 3 warm-up calls;
  * wall time of the whole call over PCIe with the state uploaded (state_resident = 0) and with the state left on the
    device by a preceding upload of the batch (state_resident = 1), median of 20;
  * the reference's time for the same three routines is NOT measured here (the reference does not exist on a GPU box):
    run `python tests/golden/make_golden_therm_itd.py --time` on the build machine and add its line to the file.
Run on a machine with a GPU:  python scripts/therm2_itd_cost.py"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cice4_amd import lib, synth  # noqa: E402

NX, NY, DT, YDAY, REPS, WARM = 322, 386, 3600.0, 100.5, 20, 3


def main():
    ctx = lib.Context()
    ctx.sync()
    ctx.thermo_init()
    ctx.itd_init(synth.hin_max())
    ctx.thermo_batch_alloc(NX, NY, 1)
    ctx.therm2_itd_times(enable=True)
    lines = [f"cice_step_therm2_itd at gx1 size ({NX - 2} x {NY - 2} + ghosts, one block), median of {REPS} after {WARM}"]
    for regime in ("growth", "melt"):
        raw = synth.therm2_state(regime, NX, NY, 1, seed=7)
        for resident in (0, 1):
            wall, dev = [], []
            for k in range(WARM + REPS):
                a = {key: v.copy() for key, v in raw.items()}
                if resident:     # what cice_step_therm1 leaves: the state and the old concentrations on the device
                    a2 = {key: v.copy() for key, v in raw.items()}
                    ctx.step_therm2_itd(DT, YDAY, a2, kitd=0)      # any call that uploads the state
                    ctx.lib.cice_device_sync(ctx.h)
                t0 = time.perf_counter()
                r = ctx.step_therm2_itd(DT, YDAY, a, state_resident=bool(resident))
                t1 = time.perf_counter()
                assert r["l_stop"] == 0
                if k >= WARM:
                    wall.append((t1 - t0) * 1e3)
                    dev.append(ctx.therm2_itd_times())
            med = [statistics.median(x[i] for x in dev) for i in range(4)]
            if not resident:
                lines.append(f"{regime}: kernels rain+aggregate {med[0] * 1e3:.1f} us, linear_itd {med[1] * 1e3:.1f} us, "
                             f"add_new_ice {med[2] * 1e3:.1f} us, lateral_melt {med[3] * 1e3:.1f} us")
            lines.append(f"{regime}: whole call over PCIe, state_resident = {resident}: {statistics.median(wall):.2f} ms")
    lines.append("reference on one core of the build machine: see `python tests/golden/make_golden_therm_itd.py --time`")
    out = os.path.join(ROOT, "profiles", "therm2_itd_cost.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
