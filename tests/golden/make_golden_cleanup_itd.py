#!/usr/bin/env python3
"""Mint tests/golden/cleanup_itd.npz FROM THE COMPILED REFERENCE: cleanup_itd and aggregate of its source/ice_itd.F90 for
the cases of tests/cleanup_itd_case.py.

The capture wrapper tests/golden/cleanup_itd_capture.F90 is compiled into a temporary directory that is deleted again:
against the module files of oracle/_ref/obj_small, linked to oracle/_ref/libcice_ref_small.so, with the flags of
oracle/build_ref.sh.  Nothing compiled is kept.  The fixture holds seeds, input hashes, recorded outputs, the branch
counts and `meta`.  The script asserts on what the reference DID (cleanup_itd_case.branch_counts against
cleanup_itd_case.NEED over the ordinary cases; the two stops) and writes nothing otherwise.

Run from the repo root where oracle/_ref is built:  python tests/golden/make_golden_cleanup_itd.py [--time]
--time: instead of minting, time cleanup_itd + aggregate of the reference on one core of this host on ONE block of gx1
size (320 x 384 cells + ghosts; the wrapper is then built against oracle/_ref/obj_gx1 and libcice_ref_gx1.so) on
synth.therm2_state "growth" and "melt" pushed through the first half by the reference's own routines, and print the host's
name with the figures."""
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
sys.path.insert(0, HERE)

import cleanup_itd_case as cc  # noqa: E402
import therm_itd_case as tc  # noqa: E402
from cice4_amd import synth  # noqa: E402

FC = os.environ.get("FC", "/opt/rocm/bin/amdflang")
BASE = "-O2 -fPIC -w -cpp -fdefault-real-8 -fconvert=big-endian -ffp-contract=off -DLINUX"
SMALL = "-DNXGLOB=24 -DNYGLOB=20 -DBLCKX=12 -DBLCKY=10 -DMXBLCKS=4"
GX1 = "-DNXGLOB=320 -DNYGLOB=384 -DBLCKX=320 -DBLCKY=384 -DMXBLCKS=1"


def build(tmp, cfg="small", dims=SMALL):
    obj, flags = os.path.join(ROOT, "oracle", "_ref", "obj_" + cfg), (BASE + " " + dims).split()
    src = os.path.join(HERE, "cleanup_itd_capture.F90")
    o = os.path.join(tmp, "cleanup_itd_capture.o")
    subprocess.check_call([FC, *flags, "-J", tmp, "-I", tmp, "-I", obj, "-c", src, "-o", o])
    so = os.path.join(tmp, "libcleanup_itd_capture.so")
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call([FC, "-shared", "-o", so, o, "-L", refdir, "-lcice_ref_" + cfg, "-Wl,-rpath," + refdir])
    L = C.CDLL(so)
    L.diag = os.path.join(tmp, "nu_diag.txt")
    return L


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
    L.ccap_set(kw["ntrcr"], i4(dep), kw["nt_Tsfc"], f8(hm), L.diag.encode(), len(L.diag))


def ref_cleanup(L, b, box=(cc.ILO, cc.IHI, cc.JLO, cc.JHI), with_flux=1, limit=1):
    st = [C.c_int(0) for _ in range(3)]
    L.ccap_cleanup_itd(*box, C.c_double(cc.DT), *[f8(b[k]) for k in ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon",
                       "aice0", "aice", "fresh", "fsalt", "fhocn")], with_flux, limit, *[C.byref(x) for x in st])
    return tuple(x.value for x in st)


def ref_aggregate(L, b):
    L.ccap_aggregate(*[f8(b[k]) for k in ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon", "aice", "trcr", "vice", "vsno",
                                          "eice", "esno", "aice0")], i4(b["tmask"]))


def agg_arrays(shape2, lead=()):
    z = lambda *s: np.zeros(lead + s + shape2)
    return dict(aice=z(), aice0=z(), vice=z(), vsno=z(), eice=z(), esno=z(), trcr=z(5))


def run_case(L, name):
    cap_set(L, cc.itd_kwargs(name))
    s = cc.case_inputs(name)
    out = {k: v.copy() for k, v in s.items()}
    out["aice"] = np.full(s["fresh"].shape, -7.0)          # cleanup_itd writes both on every cell
    out["aice0"] = np.full(s["fresh"].shape, -7.0)
    agg = agg_arrays((cc.NY, cc.NX), (cc.NB,))
    for b in range(cc.NB):
        blk = tc.block(out, b)
        assert ref_cleanup(L, blk) == (0, 0, 0), (name, b)
        for k in cc.OUT_CLEAN:
            out[k][b] = blk[k]
        ab = dict(tc.block(out, b, cc.STATE + ("tmask",)), **tc.block(agg, b))
        ref_aggregate(L, ab)
        for k in cc.OUT_AGG:
            agg[k][b] = ab[k]
    return s, out, agg


def mint(L):
    d = {}
    total = {k: 0 for k in cc.BRANCHES}
    for name in cc.ORDINARY:
        s, out, agg = run_case(L, name)
        counts, quiet = cc.branch_counts(name, s, out)
        print(name, counts, "quiet blocks:", quiet)
        for k, v in counts.items():
            total[k] += v
        for k in cc.OUT_CLEAN:
            d[f"{name}_clean_{k}"] = out[k] if k in ("aice", "aice0") else tc.xor(out[k], s[k])
        for k in cc.OUT_AGG:
            d[f"{name}_agg_{k}"] = agg[k]
        d[f"{name}_seed"] = np.array(cc.CASES[name]["seed"])
        d[f"{name}_sha256"] = np.array(cc.digest(s))
        d[f"{name}_quiet"] = np.array(quiet, np.int32)
        d[f"{name}_counts"] = np.array([counts[k] for k in cc.BRANCHES], np.int64)
    print("total", total)
    short = {k: v for k, v in total.items() if v < cc.NEED[k]}
    assert not short, ("branches the reference took in too few cells", short)
    assert total["floor_cat1"] == int(d["floor_counts"][cc.BRANCHES.index("floor_cat1")]), "floor_cat1 outside its case"
    cap_set(L, cc.itd_kwargs("stop_area"))
    for which in cc.STOPS:
        blk, cell = cc.stop_inputs(which)
        d[f"{which}_sha256"] = np.array(cc.digest(blk))
        before = {k: v.copy() for k, v in blk.items()}
        blk["aice"] = np.full((cc.NY, cc.NX), -7.0)
        blk["aice0"] = np.full((cc.NY, cc.NX), -7.0)
        r = ref_cleanup(L, blk)
        assert r == (1,) + cell, (which, "the reference reports", r, "expected", cell)
        for k in cc.FLUX:
            assert tc.same(blk[k], before[k]), (which, "the reference changed", k)
        if which == "stop_area":
            for k in cc.STATE:
                assert tc.same(blk[k], before[k]), (which, "the reference changed", k)
        else:
            a0, a1 = before["aicen"], blk["aicen"]
            tiny = (a0 != 0) & (np.abs(a0) <= cc.PUNY)
            assert (a1[:2][tiny[:2]] == 0).all() and tiny[:2].sum() >= 2 and tc.same(a1[2:], a0[2:]) and tiny[3].sum() >= 1
        d[f"{which}_stop"] = np.array(r)
        for k in cc.OUT_CLEAN:
            d[f"{which}_out_{k}"] = blk[k]
    return d


def timing(L):
    """cleanup_itd + aggregate on ONE block of gx1 size, one core; inputs: therm2_state through the reference's first half"""
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import make_golden_therm_itd as g1
    import therm2_cleanup_cost as cost
    nx, ny, reps = 322, 386, 10
    tmp = tempfile.mkdtemp(prefix="therm_itd_t_")
    try:
        L1 = g1.build(tmp, "gx1", GX1)
        for regime in ("growth", "melt"):
            g1.cap_set(L1, tc.itd_kwargs(tc.CASES["growth"]))
            cap_set(L, dict(tc.itd_kwargs(tc.CASES["growth"])))
            raw = cost.capped(synth.therm2_state(regime, nx, ny, 1, seed=7))     # the inputs of the device measurement
            blk = tc.block(raw, 0)
            blk["fresh"] = blk["fresh"] + blk["frain"] * blk["aice"]

            def lst(mask, i0, j0):
                jj, ii = np.nonzero(mask)
                out = [np.zeros(nx * ny, np.int32), np.zeros(nx * ny, np.int32)]
                out[0][:len(ii)] = ii + i0
                out[1][:len(ii)] = jj + j0
                return len(ii), out[0], out[1]

            ic, ii, jj = lst(blk["aice"][1:-1, 1:-1] > tc.PUNY, 2, 2)
            g1.ref_linear(L1, ic, ii, jj, blk)
            oc, oi, oj = lst(blk["tmask"] != 0, 1, 1)
            g1.ref_add(L1, oc, oi, oj, blk)
            L1.cap_lateral_melt(2, nx - 1, 2, ny - 1, C.c_double(tc.DT), *[g1.f8(blk[k]) for k in (
                "fresh", "fsalt", "fhocn", "rside", "meltl", "aicen", "vicen", "vsnon", "eicen", "esnon")])
            t = np.zeros((reps, 2))
            for r in range(reps):
                w = {k: v.copy() for k, v in blk.items()}
                w.update(agg_arrays((ny, nx)))
                t0 = time.perf_counter()
                st = ref_cleanup(L, w, box=(2, nx - 1, 2, ny - 1))
                t1 = time.perf_counter()
                ref_aggregate(L, w)
                t2 = time.perf_counter()
                assert st == (0, 0, 0), st
                t[r] = (t1 - t0, t2 - t1)
            m = np.median(t, axis=0) * 1e3
            print(f"{regime}: reference (amdflang -O2) on host {platform.node()} ({platform.machine()}), one core, one block "
                  f"of 320 x 384 cells + ghosts, median of {reps}: cleanup_itd {m[0]:.2f} ms, aggregate {m[1]:.2f} ms, "
                  f"together {m.sum():.2f} ms")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    tmp = tempfile.mkdtemp(prefix="cleanup_itd_")
    try:
        if "--time" in sys.argv:
            L = build(tmp, "gx1", GX1)
            threading.stack_size(1 << 30)      # the reference's automatic arrays of a gx1-size block live on the stack
            th = threading.Thread(target=timing, args=(L,))
            th.start()
            th.join()
        else:
            d = mint(build(tmp))
            d["meta"] = np.array(["reference: COSIMA/cice4 source/ice_itd.F90 (cleanup_itd, aggregate); compiler: " +
                                  FC.split("/")[-1] + " (flang) " + BASE + " " + SMALL + "; configuration small; generator: "
                                  "tests/golden/make_golden_cleanup_itd.py"])
            np.savez_compressed(cc.FIXTURE, **d)
            print("written", cc.FIXTURE, os.path.getsize(cc.FIXTURE), "bytes")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
