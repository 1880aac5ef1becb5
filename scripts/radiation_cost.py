#!/usr/bin/env python3
"""Cost of the shortwave stage (cice_step_radiation, cice_prep_radiation, cice_radiation_chain) at gx1 size: 320 x 384 cells
+ ghosts, one block, ncat = 5, on synth.therm2_state "mixed" with seeded shortwave forcing (inputs); host arrays
page-locked.  Writes profiles/radiation_cost.txt:
  * the device times of k_shortwave_ccsm3 and k_prep_radiation (HIP events, cice_radiation_times; measured in calls of their
    own, a production call records none), the algorithmic traffic of k_shortwave_ccsm3 -- 9 words in and 14 out per
    (cell, category) = 184 B -- and the rate that makes, next to the copy rate of k_state_from_transport in
    profiles/ridge_chain_cost.txt;
  * the whole calls over PCIe: cice_step_radiation with the state uploaded and with the state resident (behind a
    cice_step_therm2_cleanup on the same batch), cice_prep_radiation with the shortwave arrays uploaded and resident;
  * cice_step_radiation + cice_prep_radiation + cice_step_therm1 per step on thermo_case.therm1_inputs at the same size,
    mode 0 and mode 1 of cice_radiation_chain taking turns in ONE process: ROUNDS rounds, each STEPS timed steps after WARM
    untimed ones, every step from the same input; a saving is claimed only if the slowest chained round beats the fastest
    unchained round.
The reference's figure for the same inputs comes from `python tests/golden/make_golden_shortwave.py --time` (no GPU).
Run on a machine with a GPU:  python scripts/radiation_cost.py"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cice4_amd import lib, synth  # noqa: E402

NX, NY, DT, YDAY = 322, 386, 3600.0, 150.0
ROUNDS, STEPS, WARM = 4, 10, 2
SW = ("swvdr", "swvdf", "swidr", "swidf")
STATE = ("aicen", "trcrn", "vicen", "vsnon")
WORDS_IN, WORDS_OUT = 9, 14          # aicen vicen vsnon Tsfc 4 x sw ocn | 6 albedos 3 fluxes 4 Iswabs 1 Sswabs


def inputs(nx=NX, ny=NY, nb=1, seed=2026102015, sw_max=120.0):
    """state and forcing of one cice_step_radiation (also what make_golden_shortwave.py --time runs the reference on)"""
    raw = synth.therm2_state("mixed", nx, ny, nb, seed=seed, ntrcr=1)
    s = {k: raw[k] for k in STATE}
    rng = np.random.default_rng(seed + 1)
    for k in SW:
        s[k] = np.ascontiguousarray(rng.uniform(0.0, sw_max, (nb, ny, nx)))
    s["_raw"] = raw
    return s


def outputs(shape):
    nb, ncat, ny, nx = shape
    o = {k: np.zeros(shape) for k in ("alvdrn", "alidrn", "alvdfn", "alidfn", "albicen", "albsnon", "fswsfcn", "fswintn",
                                      "fswthrun")}
    o["Sswabsn"] = np.zeros((nb, ncat, synth.NSLYR, ny, nx))
    o["Iswabsn"] = np.zeros((nb, ncat, synth.NILYR, ny, nx))
    return o


def timed(fn, n=STEPS, warm=WARM):
    t = []
    for _ in range(warm + n):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return t[warm:]


def fmt(t):
    return f"{statistics.median(t):.2f} ms (min {min(t):.2f}, max {max(t):.2f})"


def chain(sc, tcase):
    """step_radiation + prep_radiation + step_therm1, mode 0 and 1 of cice_radiation_chain in turn: the report's lines"""
    lines = []
    ctx = lib.Context()
    ctx.sync()
    ctx.thermo_init()
    ctx.shortwave_init(**sc.init_kwargs("default"))
    ctx.thermo_batch_alloc(NX, NY, 1)
    batch, _, fz, pc, acc = tcase.therm1_inputs(NY, NX, 1, seed=35)
    shp = (1, NY, NX)
    rng = np.random.default_rng(2026102016)
    sw = {k: rng.uniform(0.0, 15.0, shp) for k in SW}
    gbm = {k: rng.uniform(0.05, 0.9, shp) for k in ("alvdr_gbm", "alvdf_gbm", "alidr_gbm", "alidf_gbm")}
    extra = dict(scale_factor=rng.uniform(10.0, 40.0, shp), fswfac=np.zeros(shp))
    alb = {k: np.zeros(batch["aicen"].shape) for k in ("alvdrn", "alidrn", "alvdfn", "alidfn", "albicen", "albsnon")}
    five = dict(fswsfcn=batch["fswsfc"], fswintn=batch["fswint"], fswthrun=batch["fswthrun"], Sswabsn=batch["Sswabs"],
                Iswabsn=batch["Iswabs"])
    fzb = dict(fz, Tbot=np.zeros(shp), fbot=np.zeros(shp), rside=np.zeros(shp))
    groups = (batch, sw, gbm, extra, alb, fzb, pc, acc)
    for d in groups:
        for v in d.values():
            if isinstance(v, np.ndarray):
                ctx.host_register(v)
    first = [{k: v.copy() for k, v in d.items() if isinstance(v, np.ndarray)} for d in groups]

    def step():
        for d, f in zip(groups, first):
            for k, v in f.items():
                d[k][...] = v
        t0 = time.perf_counter()
        ctx.step_radiation(dict({k: batch[k] for k in STATE}, **sw, **alb, **five))
        ctx.prep_radiation(dict(sw, **gbm, **extra, **five, aice=fz["aice"], aicen=batch["aicen"]), sw_resident=True)
        r = ctx.step_therm1(DT, YDAY, batch, fzb, pc, acc)
        t = (time.perf_counter() - t0) * 1e3
        assert r["l_stop"] == 0, r
        return t

    rounds = {0: [], 1: []}
    ref = None
    for _ in range(ROUNDS):
        for mode in (0, 1):
            ctx.radiation_chain(mode)
            rounds[mode].append([step() for _ in range(WARM + STEPS)][WARM:])
            out = {k: batch[k].copy() for k in ("aicen", "vicen", "trcrn", "fswsfc", "Iswabs", "meltt")}
            ref = ref or out
            for k in ref:
                assert np.array_equal(out[k], ref[k]), ("mode", mode, k)
    ctx.radiation_chain(0)
    ctx.host_unregister_all()
    ctx.close()
    med = statistics.median
    lines.append(f"cice_step_radiation + cice_prep_radiation (resident) + cice_step_therm1 per step, {ROUNDS} rounds of mode 0, 1 in "
                 f"turn, {STEPS} timed steps per round after {WARM}; ms per step")
    rm = {}
    for mode in (0, 1):
        rm[mode] = [med(g) for g in rounds[mode]]
        allt = [t for g in rounds[mode] for t in g]
        lines.append(f"mode {mode}: median {med(allt):.2f} (min {min(allt):.2f}, max {max(allt):.2f}); round medians "
                     + " ".join(f"{x:.2f}" for x in rm[mode]))
    yes = max(rm[1]) < min(rm[0])
    lines.append(f"mode 1 against mode 0: slowest round {max(rm[1]):.2f}, fastest round of mode 0 {min(rm[0]):.2f}: "
                 f"{'faster in every interleaved round' if yes else 'NOT faster in every interleaved round'}; median saving "
                 f"{med(rm[0]) - med(rm[1]):.2f} ms")
    lines.append("both modes gave the same bits (aicen, vicen, trcrn, fswsfc, Iswabs, meltt) in every round")
    return lines


def main():
    import shortwave_case as sc      # (tests/: on the path)
    import thermo_case as tcase
    lines = []
    ctx = lib.Context()
    ctx.sync()
    ctx.thermo_init()
    ctx.shortwave_init(**sc.init_kwargs("default"))
    ctx.itd_init(synth.hin_max())
    ctx.thermo_batch_alloc(NX, NY, 1)
    s = inputs()
    raw = s.pop("_raw")
    a = dict(s, **outputs(s["aicen"].shape))
    for v in a.values():
        ctx.host_register(v)
    ncol = NX * NY * synth.NCAT
    listed = int(sc.listed(s, sc.block_table(1, NY, NX)).sum())
    # the kernels by themselves
    ctx.radiation_times(True)
    ev_sw, ev_prep = [], []
    p = sc.prep_inputs(1, NY, NX, sw_arrays={k: a[k] for k in sc.PREP_SW}, aicen=s["aicen"])
    for k in ("swvdr", "swvdf", "swidr", "swidf", "alvdr_gbm", "alvdf_gbm", "alidr_gbm", "alidf_gbm", "aice", "scale_factor",
              "fswfac"):
        ctx.host_register(p[k])
    sf0 = p["scale_factor"].copy()
    for _ in range(WARM + STEPS):
        ctx.step_radiation(a)
        p["scale_factor"][...] = sf0
        ctx.prep_radiation(p, sw_resident=True)
        ms = ctx.radiation_times(True)
        ev_sw.append(ms[0]); ev_prep.append(ms[1])
    ctx.radiation_times(False)
    ev_sw, ev_prep = ev_sw[WARM:], ev_prep[WARM:]
    nbytes = (WORDS_IN + WORDS_OUT) * 8 * ncol
    us = statistics.median(ev_sw) * 1e3
    lines.append(f"gx1 size: one block of {NX - 2} x {NY - 2} cells + ghosts, ncat = {synth.NCAT}: {ncol} (cell, category) pairs, "
                 f"{listed} of them listed; page-locked host arrays; medians of {STEPS} after {WARM}")
    lines.append(f"k_shortwave_ccsm3: event time median {us:.1f} us (min {min(ev_sw) * 1e3:.1f}, max {max(ev_sw) * 1e3:.1f}); "
                 f"algorithmic traffic {WORDS_IN} words in + {WORDS_OUT} out per pair = {nbytes / 1e6:.1f} MB: "
                 f"{nbytes / (us * 1e-6) / 1e9:.0f} GB/s")
    lines.append(f"k_prep_radiation: event time median {statistics.median(ev_prep) * 1e3:.1f} us (min {min(ev_prep) * 1e3:.1f}, "
                 f"max {max(ev_prep) * 1e3:.1f})")
    # the whole calls
    lines.append("cice_step_radiation, state uploaded: " + fmt(timed(lambda: ctx.step_radiation(a))))
    want = {k: a[k].copy() for k in sc.OUT}
    c = {k: raw[k].copy() for k in ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon", "tmask", "aice", "aice0", "fresh", "fsalt", "fhocn")}
    shp = raw["aice"].shape
    c.update(vice=np.zeros(shp), vsno=np.zeros(shp), eice=np.zeros(shp), esno=np.zeros(shp), trcr=np.zeros((1, 5, NY, NX)),
             daidtt=np.zeros(shp), dvidtt=np.zeros(shp))
    r = ctx.step_therm2_cleanup(DT, c, state_resident=False, bound=False)
    if r["l_stop"] == 0:
        a2 = dict(a, **{k: c[k] for k in STATE})
        lines.append("cice_step_radiation, state resident (behind cice_step_therm2_cleanup): "
                     + fmt(timed(lambda: ctx.step_radiation(a2, state_resident=True))))
    else:
        lines.append(f"cice_step_radiation, state resident: not measured (cice_step_therm2_cleanup stopped on these inputs: {r})")
    ctx.step_radiation(a)
    for k in sc.OUT:
        assert np.array_equal(a[k], want[k]), k

    def prep(resident):
        p["scale_factor"][...] = sf0
        ctx.prep_radiation(p, sw_resident=resident)

    lines.append("cice_prep_radiation, shortwave arrays uploaded: " + fmt(timed(lambda: prep(False))))
    lines.append("cice_prep_radiation, shortwave arrays resident: " + fmt(timed(lambda: prep(True))))
    ctx.host_unregister_all()
    ctx.close()

    try:
        lines += chain(sc, tcase)
    except AssertionError as e:
        lines.append(f"cice_radiation_chain: not measured ({e})")
    out = os.path.join(ROOT, "profiles", "radiation_cost.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
