#!/usr/bin/env python3
"""Cost of the second half of step_therm2 (cice_step_therm2_cleanup) at gx1 size: 320 x 384 cells + ghosts, one block, on
synth.therm2_state "growth" and "melt" (areas brought to a sum <= 1) pushed through the first half
(cice_step_therm2_itd).  Writes profiles/therm2_cleanup_cost.txt:
  * device time of the kernels of the call with bound = 1 (HIP events, cice_therm2_cleanup_times; a production call
    records none), median of 20 calls after 3 warm-up calls;
  * wall time of the whole call (bound = 1) with the state uploaded and with the state resident, median of 20;
  * the two halves back to back with the state resident in between, against the two halves with the state crossing
    PCIe in between, in alternating runs, median of 20 each;
  * the reference's time for cleanup_itd + aggregate is NOT measured here (the reference does not exist on a GPU box):
    run `python tests/golden/make_golden_cleanup_itd.py --time` on the build machine and add its lines to the file.
Run on a machine with a GPU:  python scripts/therm2_cleanup_cost.py"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cice4_amd import lib, synth  # noqa: E402

NX, NY, DT, YDAY, REPS, WARM = 322, 386, 3600.0, 100.5, 20, 3
STATE = ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon")


def capped(raw):
    """the synthetic state made fit for cleanup_itd: its "packed" cells sit at an area of 1 + 1e-9 and its thinnest melting
    categories end below zero volume, either of which stops the reference; areas are scaled to a sum of 0.98 there and
    no category is left thinner than 0.02 m (aicen_init / vicen_init alike)"""
    raw = {k: v.copy() for k, v in raw.items()}
    for a, v, e in (("aicen", "vicen", "eicen"), ("aicen_init", "vicen_init", None)):
        thin = raw[v] < 0.02 * raw[a]
        raw[v][thin] = 0.02 * raw[a][thin]
        if e:
            q = np.repeat(-3.0e8 * raw[v] / synth.NILYR, synth.NILYR, axis=1)
            raw[e] = np.where(np.repeat(thin, synth.NILYR, axis=1), q, raw[e])
    tot = np.zeros(raw["aice"].shape)
    for n in range(synth.NCAT):
        tot = tot + raw["aicen"][:, n]
    f = np.where(tot > 1.0, 0.98 / np.where(tot > 1.0, tot, 1.0), 1.0)
    s = {k: v.copy() for k, v in raw.items()}
    for k, per in (("aicen", 1), ("vicen", 1), ("vsnon", 1), ("aicen_init", 1), ("vicen_init", 1), ("eicen", synth.NILYR),
                   ("esnon", synth.NSLYR)):
        s[k] = np.ascontiguousarray(s[k] * np.repeat(f[:, None], synth.NCAT * per, axis=1))
    s["aice"] = np.minimum(s["aice"], 0.98)
    s["aice0"] = np.maximum(1.0 - s["aice"], 0.0)
    return s


def cleanup_arrays(a, rng):
    z = lambda: np.zeros(a["aice"].shape)
    c = {k: a[k] for k in STATE + ("tmask", "fresh", "fsalt", "fhocn")}
    c.update(aice=z(), aice0=z(), vice=z(), vsno=z(), eice=z(), esno=z(), trcr=np.zeros((a["aice"].shape[0], 5) + a["aice"].shape[1:]),
             daidtt=rng.uniform(0, 1, a["aice"].shape), dvidtt=rng.uniform(0, 3, a["aice"].shape))
    return c


def main():
    ctx = lib.Context()
    ctx.sync()
    ctx.domain_create(NX - 2, NY - 2, NX - 2, NY - 2, ew=1, ns=0)
    ctx.itd_init(synth.hin_max())
    ctx.thermo_batch_alloc(NX, NY, 1)
    rng = np.random.default_rng(3)
    lines = [f"cice_step_therm2_cleanup at gx1 size ({NX - 2} x {NY - 2} + ghosts, one block, bound = 1), median of {REPS} after {WARM}"]

    def halves(s, chained):
        a = {k: v.copy() for k, v in s.items()}
        t0 = time.perf_counter()
        assert ctx.step_therm2_itd(DT, YDAY, a)["l_stop"] == 0
        c = cleanup_arrays(a, rng)
        t1 = time.perf_counter()
        r = ctx.step_therm2_cleanup(DT, c, state_resident=chained, bound=True)
        t2 = time.perf_counter()
        assert r["l_stop"] == 0, r
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3

    for regime in ("growth", "melt"):
        s = capped(synth.therm2_state(regime, NX, NY, 1, seed=7))
        ctx.therm2_cleanup_times(enable=True)
        dev, wall = [], {0: [], 1: []}
        for k in range(WARM + REPS):
            for resident in (0, 1):
                w = halves(s, bool(resident))[1]
                if k >= WARM:
                    wall[resident].append(w)
                    if not resident:
                        dev.append(ctx.therm2_cleanup_times())
        med = {n: statistics.median(x[n] for x in dev) * 1e3 for n in lib.CLEANUP_TIMES}
        passes = sum(med[f"pass{p}"] for p in range(1, 9))
        lines.append(f"{regime}: kernels head {med['head']:.1f} us, rebin passes " +
                     " ".join(f"{med[f'pass{p}']:.1f}" for p in range(1, 9)) + f" = {passes:.1f} us, zap {med['zap']:.1f} us, "
                     f"bound_state {med['bound_state']:.1f} us, aggregate + tendencies {med['aggregate']:.1f} us, together "
                     f"{sum(med.values()):.1f} us")
        for resident in (0, 1):
            lines.append(f"{regime}: whole call over PCIe, state_resident = {resident}: {statistics.median(wall[resident]):.2f} ms")
        ctx.therm2_cleanup_times(enable=False)        # a production call records no events
        pair = {True: [], False: []}
        for k in range(WARM + REPS):
            for chained in (True, False):             # alternating runs on the same box
                t = sum(halves(s, chained))
                if k >= WARM:
                    pair[chained].append(t)
        lines.append(f"{regime}: both halves, state resident in between {statistics.median(pair[True]):.2f} ms, state over PCIe "
                     f"in between {statistics.median(pair[False]):.2f} ms (alternating runs)")
    lines.append("reference on one core of the build machine: see `python tests/golden/make_golden_cleanup_itd.py --time`")
    out = os.path.join(ROOT, "profiles", "therm2_cleanup_cost.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
