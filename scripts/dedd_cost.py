#!/usr/bin/env python3
"""Cost of the delta-Eddington shortwave stage (cice_step_radiation_dedd) at gx1 size: 320 x 384 cells + ghosts, one block,
ncat = 5, on synth.therm2_state "mixed" with seeded shortwave forcing and a coszen field that holds both day and night
(inputs); host arrays page-locked.  Writes profiles/dedd_cost.txt:
  * the device time of k_shortwave_dedd (HIP events, cice_dedd_times; measured in calls of their own) and what that makes
    per (cell, category) pair the scheme runs on;
  * the whole call over PCIe with the state uploaded, and with the state resident (behind a cice_step_therm2_cleanup on
    the same batch) where that stage accepts these inputs.
Medians of ten after two, with min - max.  The reference's figure for the same inputs comes from
`python tests/golden/make_golden_dedd.py --time` (no GPU).
Run on a machine with a GPU:  python scripts/dedd_cost.py"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import radiation_cost as rc  # noqa: E402
from cice4_amd import lib, synth  # noqa: E402

NX, NY, DT = rc.NX, rc.NY, rc.DT
STEPS, WARM = 10, 2


def inputs(nx=NX, ny=NY, nb=1, seed=2026102026):
    """state and forcing of one cice_step_radiation_dedd (also what make_golden_dedd.py --time runs the reference on): the
    state of radiation_cost.inputs, surfaces warmed on a third of the pairs so that ponds form, and a coszen that runs from
    night (a quarter of the cells at or below 0) through the horizon to the zenith"""
    s = rc.inputs(nx, ny, nb, seed=seed)
    rng = np.random.default_rng(seed + 2)
    T = s["trcrn"][:, :, 0]
    warm = rng.random(T.shape) < 0.33
    T[warm] = -rng.uniform(0.0, 1.0, int(warm.sum()))
    s["coszen"] = np.ascontiguousarray(rng.uniform(-0.33, 1.0, (nb, ny, nx)))
    return s


def outputs(shape):
    o = rc.outputs(shape)
    o["albpndn"] = np.zeros(shape)
    return o


def main():
    import dedd_case as dc           # (tests/: on the path)
    lines = []
    ctx = lib.Context()
    ctx.sync()
    ctx.thermo_init()
    ctx.shortwave_dedd_init(**dc.init_kwargs("default"))
    ctx.itd_init(synth.hin_max())
    ctx.thermo_batch_alloc(NX, NY, 1)
    s = inputs()
    raw = s.pop("_raw")
    a = dict(s, **outputs(s["aicen"].shape))
    for v in a.values():
        ctx.host_register(v)
    ncol = NX * NY * synth.NCAT
    on = dc.listed(s, dc.block_table(1, NY, NX))
    lit = int((on & (s["coszen"] > dc.PUNY)[:, None]).sum())
    ctx.dedd_times(True)
    ev = []
    for _ in range(WARM + STEPS):
        ctx.step_radiation_dedd(a)
        ev.append(ctx.dedd_times(True))
    ctx.dedd_times(False)
    ev = ev[WARM:]
    ms = statistics.median(ev)
    lines.append(f"gx1 size: one block of {NX - 2} x {NY - 2} cells + ghosts, ncat = {synth.NCAT}: {ncol} (cell, category) pairs, "
                 f"{int(on.sum())} of them listed, {lit} with the sun up; page-locked host arrays; medians of {STEPS} after {WARM}")
    lines.append(f"k_shortwave_dedd: event time median {ms:.3f} ms (min {min(ev):.3f}, max {max(ev):.3f}): "
                 f"{ms * 1e6 / max(lit, 1):.1f} ns per pair with the sun up")
    lines.append("cice_step_radiation_dedd, state uploaded: " + rc.fmt(rc.timed(lambda: ctx.step_radiation_dedd(a), STEPS, WARM)))
    want = {k: a[k].copy() for k in dc.OUT}
    c = {k: raw[k].copy() for k in ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon", "tmask", "aice", "aice0", "fresh", "fsalt",
                                    "fhocn")}
    c["trcrn"][:, :, 0] = s["trcrn"][:, :, 0]
    shp = raw["aice"].shape
    c.update(vice=np.zeros(shp), vsno=np.zeros(shp), eice=np.zeros(shp), esno=np.zeros(shp), trcr=np.zeros((1, 5, NY, NX)),
             daidtt=np.zeros(shp), dvidtt=np.zeros(shp))
    r = ctx.step_therm2_cleanup(DT, c, state_resident=False, bound=False)
    if r["l_stop"] == 0:
        a2 = dict(a, **{k: c[k] for k in rc.STATE})
        lines.append("cice_step_radiation_dedd, state resident (behind cice_step_therm2_cleanup): "
                     + rc.fmt(rc.timed(lambda: ctx.step_radiation_dedd(a2, state_resident=True), STEPS, WARM)))
    else:
        lines.append(f"cice_step_radiation_dedd, state resident: not measured (cice_step_therm2_cleanup stopped on these inputs: {r})")
    ctx.step_radiation_dedd(a)
    for k in dc.OUT:
        assert np.array_equal(a[k], want[k]), k
    ctx.host_unregister_all()
    ctx.close()
    out = os.path.join(ROOT, "profiles", "dedd_cost.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
