#!/usr/bin/env python3
"""Mint tests/golden/therm_itd.npz FROM THE COMPILED REFERENCE: linear_itd, add_new_ice, lateral_melt of its
source/ice_therm_itd.F90 and shift_ice of ice_itd, for the cases of tests/therm_itd_case.py.

The reference's ice_therm_itd.F90 is compiled where it lies, with the capture wrapper tests/golden/therm_itd_capture.F90,
into a temporary directory that is deleted again: against the module files of oracle/_ref/obj_small, linked to
oracle/_ref/libcice_ref_small.so, with the flags of oracle/build_ref.sh.  Nothing compiled is kept.  The fixture holds
seeds, input hashes, recorded outputs and `meta`.  The script asserts on what the reference DID (tests/therm_itd_case.py
branch_counts, at least 8 cells per branch over the ordinary cases; the cells its nu_diag lines name as not remapped, above
0 in some case; the two stops) and writes nothing otherwise.

Run from the repo root where oracle/_ref is built:  python tests/golden/make_golden_therm_itd.py [--time]
--time: instead of minting, time the three routines of the reference on one core of this host on ONE block of gx1
size (320 x 384 cells + ghosts; the wrapper is then built against oracle/_ref/obj_gx1 and libcice_ref_gx1.so) and print
the host's name with the figures."""
import ctypes as C
import os
import platform
import shutil
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)

import therm_itd_case as tc  # noqa: E402
from cice4_amd import synth  # noqa: E402

REF = os.environ.get("CICE_REFERENCE_ROOT", "/root/reference")
FC = os.environ.get("FC", "/opt/rocm/bin/amdflang")
BASE = "-O2 -fPIC -w -cpp -fdefault-real-8 -fconvert=big-endian -ffp-contract=off -DLINUX"
SMALL = "-DNXGLOB=24 -DNYGLOB=20 -DBLCKX=12 -DBLCKY=10 -DMXBLCKS=4"
FLAGS = (BASE + " " + SMALL).split()


def build(tmp, cfg="small", dims=SMALL):
    obj, flags = os.path.join(ROOT, "oracle", "_ref", "obj_" + cfg), (BASE + " " + dims).split()
    objs = []
    for src in (os.path.join(REF, "source", "ice_therm_itd.F90"), os.path.join(HERE, "therm_itd_capture.F90")):
        o = os.path.join(tmp, os.path.basename(src)[:-4] + ".o")
        subprocess.check_call([FC, *flags, "-J", tmp, "-I", tmp, "-I", obj, "-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtherm_itd_capture.so")
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call([FC, "-shared", "-o", so, *objs, "-L", refdir, "-lcice_ref_" + cfg, "-Wl,-rpath," + refdir])
    L = C.CDLL(so)
    L.diag = os.path.join(tmp, "nu_diag.txt")      # what the reference writes to nu_diag (cap_set opens it)
    L.diag_at = 0
    return L


def diag_cells(L):
    """the distinct (i, j) the reference named in the `ITD:` lines it wrote to nu_diag since the last call
    (ice_therm_itd.F90:328-378: `my_task, ':', i, j, 'ITD: ...'` for every check a cell fails)"""
    with open(L.diag) as f:
        f.seek(L.diag_at)
        text = f.read()
        L.diag_at = f.tell()
    cells = set()
    for line in text.splitlines():
        if "ITD" in line and ":" in line:
            w = line.split(":", 1)[1].split()
            cells.add((int(w[0]), int(w[1])))
    return cells


def f8(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def i4(a):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def cap_set(L, kw):
    dep = np.zeros(5, np.int32)
    dep[:kw["ntrcr"]] = kw["trcr_depend"]
    hm = np.ascontiguousarray(kw["hin_max"], np.float64)
    L.cap_set(kw["ntrcr"], i4(dep), kw["nt_Tsfc"], kw["nt_iage"], kw["nt_alvl"], kw["nt_vlvl"], int(kw["tr_iage"]),
              int(kw["tr_lvl"]), int(kw["update_ocn_f"]), f8(hm), C.c_double(kw["hi_min"]), L.diag.encode(), len(L.diag))


def ref_linear(L, icells, ii, jj, b):
    st = [C.c_int(0) for _ in range(3)]
    L.cap_linear_itd(icells, i4(ii), i4(jj), *[f8(b[k]) for k in ("aicen_init", "vicen_init", "aicen", "trcrn", "vicen",
                     "vsnon", "eicen", "esnon", "aice", "aice0")], *[C.byref(x) for x in st])
    return tuple(x.value for x in st)


def ref_add(L, icells, ii, jj, b):
    st = [C.c_int(0) for _ in range(3)]
    L.cap_add_new_ice(icells, i4(ii), i4(jj), i4(b["tmask"]), C.c_double(tc.DT),
                      *[f8(b[k]) for k in ("aicen", "trcrn", "vicen", "eicen", "aice0", "aice", "frzmlt", "frazil",
                                           "frz_onset")], C.c_double(tc.YDAY), f8(b["fresh"]), f8(b["fsalt"]), f8(b["Tf"]),
                      *[C.byref(x) for x in st])
    return tuple(x.value for x in st)


def ref_melt(L, b):
    L.cap_lateral_melt(tc.ILO, tc.IHI, tc.JLO, tc.JHI, C.c_double(tc.DT),
                       *[f8(b[k]) for k in ("fresh", "fsalt", "fhocn", "rside", "meltl", "aicen", "vicen", "vsnon", "eicen",
                                            "esnon")])


def not_remapped_restated(s0):
    """CROSS-CHECK ONLY (the recorded count is what the reference itself reported, diag_cells): the cells of the lists whose
    remap_flag a restatement of ice_therm_itd.F90:294-383 finds false."""
    hm = synth.hin_max().copy()
    hm[synth.NCAT] = 999.9
    n_no = 0
    for b in range(tc.NB):
        icells, ii, jj = tc.ice_list(s0["aice"][b])
        for k in range(icells):
            i, j = ii[k] - 1, jj[k] - 1
            a = s0["aicen"][b, :, j, i]; v = s0["vicen"][b, :, j, i]
            ai = s0["aicen_init"][b, :, j, i]; vi = s0["vicen_init"][b, :, j, i]
            hinit = np.array([vi[n] / ai[n] if ai[n] > tc.PUNY else 0.0 for n in range(5)])
            h = np.array([v[n] / a[n] if a[n] > tc.PUNY else 0.0 for n in range(5)])
            dh = np.where(a > tc.PUNY, h - hinit, 0.0)
            flag = True
            for n in range(1, 5):
                if hinit[n - 1] > tc.PUNY and hinit[n] > tc.PUNY:
                    slope = (dh[n] - dh[n - 1]) / (hinit[n] - hinit[n - 1])
                    hb = hm[n] + dh[n - 1] + slope * (hm[n] - hinit[n - 1])
                elif hinit[n - 1] > tc.PUNY:
                    hb = hm[n] + dh[n - 1]
                elif hinit[n] > tc.PUNY:
                    hb = hm[n] + dh[n]
                else:
                    hb = hm[n]
                if a[n - 1] > tc.PUNY and h[n - 1] >= hb:
                    flag = False
                elif a[n] > tc.PUNY and h[n] <= hb:
                    flag = False
                if hb > hm[n + 1] or hb < hm[n - 1]:
                    flag = False
            n_no += not flag
    return n_no


def run_case(L, name):
    c = tc.CASES[name]
    cap_set(L, tc.itd_kwargs(c))
    raw, s0 = tc.case_inputs(name)
    chain = [s0]
    n_named = 0
    for stage in (1, 2, 3):
        cur = {k: v.copy() for k, v in chain[-1].items()}
        for b in range(tc.NB):
            blk = tc.block(cur, b)
            if stage == 1:
                icells, ii, jj = tc.ice_list(blk["aice"])
                if icells > 0:
                    diag_cells(L)
                    assert ref_linear(L, icells, ii, jj, blk) == (0, 0, 0), name
                    named = diag_cells(L)
                    assert named <= set(zip(ii[:icells].tolist(), jj[:icells].tolist())), (name, b, named)
                    n_named += len(named)
            elif stage == 2:
                icells, ii, jj = tc.ocean_list(blk["tmask"])
                assert ref_add(L, icells, ii, jj, blk) == (0, 0, 0), name
            else:
                ref_melt(L, blk)
            for k in tc.CHAIN:
                cur[k][b] = blk[k]
        chain.append(cur)
    return raw, chain, n_named


def mint(L):
    d = {}
    total = {k: 0 for k in tc.BRANCHES}
    any_noremap = 0
    for name in tc.ORDINARY:
        raw, chain, nn = run_case(L, name)                 # nn: cells the reference's own diagnosis named
        counts = tc.branch_counts(chain, tc.CASES[name]["ntrcr"])
        assert nn == not_remapped_restated(chain[0]), (name, nn, not_remapped_restated(chain[0]))
        print(name, counts, "not remapped:", nn)
        for k, v in counts.items():
            total[k] += v
        any_noremap = max(any_noremap, nn)
        for s in (1, 2, 3):
            for k in tc.CHAIN:
                d[f"{name}_s{s}_{k}"] = tc.xor(chain[s][k], chain[s - 1][k])
        d[f"{name}_seed"] = np.array(tc.CASES[name]["seed"])
        d[f"{name}_sha256"] = np.array(tc.digest(raw))
        d[f"{name}_not_remapped"] = np.array(nn)
    print("total", total)
    short = {k: v for k, v in total.items() if v < 8}
    assert not short, ("branches the reference took in fewer than 8 cells", short)
    assert any_noremap > 0, "no case with a cell that was not remapped"
    # stops
    cap_set(L, tc.itd_kwargs(tc.CASES["growth"]))
    s, cell = tc.stop_add_inputs()
    d["stop_add_sha256"] = np.array(tc.digest(s))
    icells, ii, jj = tc.ocean_list(s["tmask"])
    r = ref_add(L, icells, ii, jj, s)
    assert r == (1,) + cell, ("stop_add: the reference reports", r, "expected", cell)
    d["stop_add_stop"] = np.array(r)
    for k in tc.OUT2:
        d[f"stop_add_out_{k}"] = s[k]
    s, icells, ii, jj, cell = tc.stop_shift_inputs()
    d["stop_shift_sha256"] = np.array(tc.digest(s))
    before = {k: v.copy() for k, v in s.items()}
    st = [C.c_int(0) for _ in range(3)]
    L.cap_shift_ice(icells, i4(ii), i4(jj), *[f8(s[k]) for k in ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon",
                    "hicen")], i4(s["donor"]), f8(s["daice"]), f8(s["dvice"]), *[C.byref(x) for x in st])
    r = tuple(x.value for x in st)
    assert r == (1,) + cell, ("stop_shift: the reference reports", r, "expected", cell)
    for k in tc.STATE:
        assert tc.same(s[k], before[k]), ("stop_shift: the reference changed", k)
    d["stop_shift_stop"] = np.array(r)
    return d


def timing(L):
    """the three routines on ONE block of gx1 size (the capture library built against oracle/_ref/obj_gx1), one core"""
    nx, ny, reps = 322, 386, 10
    cap_set(L, tc.itd_kwargs(tc.CASES["growth"]))

    def lst(mask, i0, j0):
        jj, ii = np.nonzero(mask)
        out = [np.zeros(nx * ny, np.int32), np.zeros(nx * ny, np.int32)]
        out[0][:len(ii)] = ii + i0
        out[1][:len(ii)] = jj + j0
        return len(ii), out[0], out[1]

    for regime in ("growth", "melt"):
        raw = synth.therm2_state(regime, nx, ny, 1, seed=7)
        t = np.zeros((reps, 3))
        for r in range(reps):
            blk = tc.block(raw, 0)
            icells, ii, jj = lst(blk["aice"][1:-1, 1:-1] > tc.PUNY, 2, 2)
            oc, oi, oj = lst(blk["tmask"] != 0, 1, 1)
            st = [C.c_int(0) for _ in range(3)]
            t0 = time.perf_counter()
            ref_linear(L, icells, ii, jj, blk)
            t1 = time.perf_counter()
            ref_add(L, oc, oi, oj, blk)
            t2 = time.perf_counter()
            L.cap_lateral_melt(2, nx - 1, 2, ny - 1, C.c_double(tc.DT), *[f8(blk[k]) for k in (
                "fresh", "fsalt", "fhocn", "rside", "meltl", "aicen", "vicen", "vsnon", "eicen", "esnon")])
            t3 = time.perf_counter()
            t[r] = (t1 - t0, t2 - t1, t3 - t2)
        m = np.median(t, axis=0) * 1e3
        print(f"{regime}: reference (amdflang -O2) on host {platform.node()} ({platform.machine()}), one core, one block of "
              f"320 x 384 cells + ghosts, median of {reps}: linear_itd {m[0]:.2f} ms, add_new_ice {m[1]:.2f} ms, "
              f"lateral_melt {m[2]:.2f} ms, together {m.sum():.2f} ms")


if __name__ == "__main__":
    tmp = tempfile.mkdtemp(prefix="therm_itd_")
    try:
        if "--time" in sys.argv:
            L = build(tmp, "gx1", "-DNXGLOB=320 -DNYGLOB=384 -DBLCKX=320 -DBLCKY=384 -DMXBLCKS=1")
            threading.stack_size(1 << 30)      # the reference's automatic arrays of a gx1-size list live on the stack
            th = threading.Thread(target=timing, args=(L,))
            th.start()
            th.join()
        else:
            d = mint(build(tmp))
            d["meta"] = np.array(["reference: COSIMA/cice4 source/ice_therm_itd.F90, source/ice_itd.F90; compiler: " + FC.split("/")[-1] +
                                  " (flang) " + " ".join(FLAGS) + "; configuration small; generator: "
                                  "tests/golden/make_golden_therm_itd.py"])
            np.savez_compressed(tc.FIXTURE, **d)
            print("written", tc.FIXTURE, os.path.getsize(tc.FIXTURE), "bytes")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
