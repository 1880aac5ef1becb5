#!/usr/bin/env python3
"""Cost of the coupling stage (cice_coupling_prep) at gx1 size: 320 x 384 cells + ghosts, one block, ncat = 5, on the seeded
fields of tests/coupling_case.py (inputs); host arrays page-locked; medians of STEPS after WARM.  Writes
profiles/coupling_cost.txt:
  * the device times of k_ocean_mixed_layer and k_coupling_prep (HIP events, cice_coupling_times; measured in calls of their
    own, a production call records none) and the algorithmic traffic they move;
  * the whole call over PCIe with everything uploaded;
  * the call with alb_resident = 1 (behind a cice_step_radiation on the same batch) and, where the state can be made resident
    on these inputs (behind a cice_step_therm2_cleanup), state_resident = 1 -- uploaded and resident calls taking turns in
    ONE process: ROUNDS rounds, each STEPS timed calls after WARM untimed ones.  The resident form is called faster only if
    its slowest round beats the fastest uploaded round.
Each GPU step is a process of its own under its own `timeout`; after a step that fails nothing more is started.
The reference's figure for the same inputs comes from `python tests/golden/make_golden_coupling.py --time` (no GPU).
Run on a machine with a GPU:  python scripts/coupling_cost.py"""
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NX, NY, DT = 322, 386, 3600.0
ROUNDS, STEPS, WARM = 4, 10, 2
STEP_LIMIT = 300                       # seconds per GPU step
# words per cell: k_coupling_prep reads 8 per-category arrays x 5, tmask (half a word), 9 + 13 fields, writes 13 + 16;
# k_ocean_mixed_layer reads tmask, 8 + 2 + 9 fields, writes 2 + 13 + 4
WORDS_PREP, WORDS_MIX = 8 * 5 + 0.5 + 9 + 13 + 13 + 16, 0.5 + 8 + 2 + 9 + 2 + 13 + 4


def inputs(nx=NX, ny=NY, nb=1, seed=2026102204):
    """the fields of one cice_coupling_prep (also what make_golden_coupling.py --time runs the reference on)"""
    import coupling_case as cc
    return cc.make_inputs("standalone", nb, ny, nx, seed=seed)


def timed(fn, n=STEPS, warm=WARM):
    t = []
    for _ in range(warm + n):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return t[warm:]


def fmt(t):
    return f"{statistics.median(t):.2f} ms (min {min(t):.2f}, max {max(t):.2f})"


def arrays(s):
    """the dict of a call: the inputs themselves, copies of the in / out fields, zeroed outputs"""
    import coupling_case as cc
    a = {k: v for k, v in s.items() if k != "albcnt"}
    for k in cc.FLUXES + cc.MIX_IO:
        a[k] = s[k].copy()
    for k in cc.OUT + cc.MIX_OUT:
        a[k] = np.zeros(s["coszen"].shape)
    a["albcnt"] = s["albcnt"][:1].copy()
    return a


def context():
    from cice4_amd import lib
    ctx = lib.Context()
    ctx.sync()
    ctx.thermo_init()
    ctx.coupling_init()
    ctx.thermo_batch_alloc(NX, NY, 1)
    return ctx


def restore(a, s):
    import coupling_case as cc
    for k in cc.FLUXES + cc.MIX_IO:
        a[k][...] = s[k]


def step_kernels():
    s = inputs()
    ctx = context()
    a = arrays(s)
    for v in a.values():
        ctx.host_register(v)
    ctx.coupling_times(True)
    ev = []
    for _ in range(WARM + STEPS):
        restore(a, s)
        ctx.coupling_prep(DT, a, nstreams=1)
        ev.append(ctx.coupling_times(True))
    ctx.coupling_times(False)
    ev = ev[WARM:]
    ncell = NX * NY
    ocean = int((s["tmask"] != 0).sum())
    print(f"gx1 size: one block of {NX - 2} x {NY - 2} cells + ghosts = {ncell} cells, {ocean} of them ocean, ncat = 5; page-locked "
          f"host arrays; medians of {STEPS} after {WARM}")
    for k, (name, words) in enumerate((("k_ocean_mixed_layer", WORDS_MIX), ("k_coupling_prep", WORDS_PREP))):
        t = [e[k] * 1e3 for e in ev]
        us = statistics.median(t)
        nbytes = words * 8 * ncell
        print(f"{name}: event time median {us:.1f} us (min {min(t):.1f}, max {max(t):.1f}); algorithmic traffic {words:g} words "
              f"per cell = {nbytes / 1e6:.1f} MB: {nbytes / (us * 1e-6) / 1e9:.0f} GB/s")
    restore(a, s)
    t = timed(lambda: ctx.coupling_prep(DT, a, nstreams=1))
    import coupling_case as cc
    up = sum(a[k].nbytes for k in ("tmask", "aicen", "albcnt") + cc.CAT_ALB + cc.IN2 + cc.FLUXES + cc.MIX_IN + cc.MIX_IO if k in a)
    down = sum(a[k].nbytes for k in ("albcnt",) + cc.FLUXES + cc.OUT + cc.MIX_IO + cc.MIX_OUT)
    print(f"cice_coupling_prep, everything uploaded ({up / (ncell * 8):g} planes of {ncell * 8 / 1e6:.2f} MB up, "
          f"{down / (ncell * 8):g} down): " + fmt(t))
    ctx.host_unregister_all()
    ctx.close()


def step_resident():
    import coupling_case as cc
    import shortwave_case as sc
    from cice4_amd import synth
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import radiation_cost as rc
    ctx = context()
    ctx.shortwave_init(**sc.init_kwargs("default"))
    ctx.itd_init(synth.hin_max())
    r = rc.inputs()
    raw = r.pop("_raw")
    rad = dict(r, **rc.outputs(r["aicen"].shape))
    # the state: resident behind cice_step_therm2_cleanup where that accepts these inputs
    c = {k: raw[k].copy() for k in ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon", "tmask", "aice", "aice0", "fresh",
                                    "fsalt", "fhocn")}
    shp = raw["aice"].shape
    c.update(vice=np.zeros(shp), vsno=np.zeros(shp), eice=np.zeros(shp), esno=np.zeros(shp), trcr=np.zeros((1, 5, NY, NX)),
             daidtt=np.zeros(shp), dvidtt=np.zeros(shp))
    stop = ctx.step_therm2_cleanup(DT, c, state_resident=False, bound=False)
    st_res = stop["l_stop"] == 0
    if st_res:
        rad.update({k: c[k] for k in rc.STATE})
    ctx.step_radiation(rad, state_resident=st_res)          # leaves the per-category albedos (and their record) on the device
    s = inputs()
    s = {k: v for k, v in s.items() if k not in cc.CAT_ALB + ("aicen",)}
    s["aicen"] = rad["aicen"]
    s.update({k: rad[k] for k in cc.CAT_ALB[:6]})
    a = arrays(s)
    for v in a.values():
        ctx.host_register(v)
    rounds = {False: [], True: []}
    first = None
    for _ in range(ROUNDS):
        for resident in (False, True):
            def call():
                restore(a, s)
                ctx.coupling_prep(DT, a, nstreams=1, alb_resident=resident, state_resident=resident and st_res)
            rounds[resident].append(timed(call))
            out = {k: a[k].copy() for k in cc.OUT + cc.FLUXES + cc.MIX_IO + cc.MIX_OUT}
            first = first or out
            for k in first:
                assert np.array_equal(out[k], first[k]), ("resident", resident, k)
    ctx.host_unregister_all()
    ctx.close()
    med = statistics.median
    what = "alb_resident = 1 and state_resident = 1 (behind cice_step_therm2_cleanup and cice_step_radiation)" if st_res else \
        f"alb_resident = 1 (behind cice_step_radiation); state_resident = 1 not measured: cice_step_therm2_cleanup stopped on " \
        f"these inputs ({stop}), so aicen is uploaded in both forms"
    print(f"cice_coupling_prep uploaded against {what}: {ROUNDS} rounds of the two in turn, {STEPS} timed calls per round after "
          f"{WARM}; ms per call (the refill of the 15 in / out planes on the host included in both)")
    rm = {}
    for resident in (False, True):
        rm[resident] = [med(g) for g in rounds[resident]]
        allt = [t for g in rounds[resident] for t in g]
        print(f"{'resident' if resident else 'uploaded'}: median {med(allt):.2f} (min {min(allt):.2f}, max {max(allt):.2f}); round "
              "medians " + " ".join(f"{x:.2f}" for x in rm[resident]))
    yes = max(rm[True]) < min(rm[False])
    print(f"resident against uploaded: slowest resident round {max(rm[True]):.2f}, fastest uploaded round {min(rm[False]):.2f}: "
          f"{'faster in every interleaved round' if yes else 'NOT faster in every interleaved round'}; median saving "
          f"{med(rm[False]) - med(rm[True]):.2f} ms")
    print("both forms gave the same bits in every round")


STEPS_GPU = {"kernels": step_kernels, "resident": step_resident}


def main():
    lines = []
    for name in STEPS_GPU:
        p = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--step", name],
                           stdout=subprocess.PIPE, text=True)
        lines += p.stdout.splitlines()
        if p.returncode != 0:
            lines.append(f"step {name}: ended with status {p.returncode}; nothing further was started")
            break
    out = os.path.join(ROOT, "profiles", "coupling_cost.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if lines and "ended with status" not in lines[-1] else 1


if __name__ == "__main__":
    if "--step" in sys.argv:
        STEPS_GPU[sys.argv[sys.argv.index("--step") + 1]]()
    else:
        sys.exit(main())
