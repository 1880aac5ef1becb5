#!/usr/bin/env python3
"""Mint tests/golden/pond.npz FROM THE COMPILED REFERENCE: compute_ponds of its source/ice_meltpond.F90 and increment_age of
its source/ice_age.F90 for the cases of tests/pond_case.py, per (block, category), increment_age on the list step_therm1
builds (aicen > puny on the physical cells).

ice_meltpond.F90 is not in the closure of oracle/build_ref.sh (ice_age is).  It is compiled unmodified, from where it lies,
with the flags of oracle/build_ref.sh, into a temporary directory that is deleted again, against the module files of
oracle/_ref/obj_small, and linked to oracle/_ref/libcice_ref_small.so together with the capture wrapper
tests/golden/pond_capture.F90, which sets ice_calendar's dt and ice_state's nt_Tsfc and nt_volpn.  Nothing compiled is kept.

The script asserts, and writes nothing otherwise:
  the numpy restatement (pond_case.pond_numpy, age_numpy) equals the reference IN EVERY WORD, off the lists included;
  every array that is intent(in) in the reference, and every tracer plane the routines do not own, came back as it went in;
  every branch of pond_case.BRANCHES occurs in at least NEED (cell, category) pairs over the cases;
  |hi - hicemin|, |hs - puny|, |sqrt(volpn/dpthfrac) - 1| and |hpondn - 0.9 hi| are at least 1e-9 at their comparisons
    (hs: on the columns with snow; vsnon = 0 gives hs = 0 with no rounding anywhere).
The fixture holds seeds, input hashes, the recorded outputs on the pairs where the list ran, branch counts and `meta`.

Run from the repo root where oracle/_ref is built:  python tests/golden/make_golden_pond.py [--time]
--time: instead of minting, time the reference's two routines on one core of this host for the five categories of ONE block
of gx1 size (320 x 384 cells + ghosts; built against oracle/_ref/obj_gx1) on the inputs of scripts/pond_cost.py, median of
five."""
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

import make_golden_shortwave as mgs  # noqa: E402
import pond_case as pc  # noqa: E402
import therm_itd_case as tc  # noqa: E402
from make_golden_shortwave import f8, i4, ice_list  # noqa: E402


def build(tmp, cfg="small", dims=mgs.SMALL):
    refdir = os.path.join(ROOT, "oracle", "_ref")
    obj = os.path.join(refdir, "obj_" + cfg)
    flags = (mgs.BASE + " " + dims).split()
    objs = []
    for src in (os.path.join(mgs.REF, "source", "ice_meltpond.F90"), os.path.join(HERE, "pond_capture.F90")):
        o = os.path.join(tmp, os.path.basename(src)[:-4] + ".o")
        subprocess.check_call([mgs.FC, *flags, "-J", tmp, "-I", tmp, "-I", obj, "-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libpond_capture.so")
    subprocess.check_call([mgs.FC, "-shared", "-o", so, *objs, "-L", refdir, "-lcice_ref_" + cfg, "-Wl,-rpath," + refdir])
    return C.CDLL(so)


def ref_case(L, name, s):
    """the reference on every (block, category) of a copy of s; returns the copy"""
    c = pc.CASES[name]
    r = {k: v.copy() for k, v in s.items()}
    nb, ncat, ny, nx = r["aicen"].shape
    blk = pc.block_table(nb, ny, nx)
    L.pdcap_set(C.c_double(pc.DT), c["nt_Tsfc"], max(c["nt_volpn"], 1))
    for b in range(nb):
        for n in range(ncat):
            cat = lambda k: f8(r[k][b, n])  # noqa: E731  (views into r: updated in place)
            if c["age"]:                     # in front of thermo_vertical in the reference; the order does not matter here
                icells, indxi, indxj = ice_list(r["aicen"][b, n], blk[b], nx * ny)
                L.pdcap_age(C.c_double(pc.DT), icells, i4(indxi), i4(indxj), f8(r["trcrn"][b, n, c["nt_iage"] - 1]))
            if c["ponds"]:
                L.pdcap_ponds(*[int(x) for x in blk[b]], cat("melttn"), cat("meltsn"), f8(r["frain"][b]), cat("aicen"),
                              cat("vicen"), cat("vsnon"), f8(r["trcrn"][b, n]), cat("apondn"), cat("hpondn"))
    return r


def outputs(name, r):
    c = pc.CASES[name]
    o = {}
    if c["ponds"]:
        o.update(apondn=r["apondn"], hpondn=r["hpondn"], volpn=np.ascontiguousarray(r["trcrn"][:, :, c["nt_volpn"] - 1]))
    if c["age"]:
        o["iage"] = np.ascontiguousarray(r["trcrn"][:, :, c["nt_iage"] - 1])
    return o


def mint():
    d = {}
    total = {k: 0 for k in pc.BRANCHES}
    margins = {}
    tmp = tempfile.mkdtemp(prefix="pond_")
    try:
        L = build(tmp)
        for name, c in pc.CASES.items():
            s = pc.case_inputs(name)
            r = ref_case(L, name, s)
            out = outputs(name, r)
            ours, m = pc.restate(name, s)
            for k in pc.outputs_of(name):
                assert np.isfinite(out[k]).all(), (name, k, "not finite")
                assert tc.same(ours[k], out[k]), (name, k, "the restatement is not the reference",
                                                  int((ours[k].view(np.uint64) != out[k].view(np.uint64)).sum()))
            owned = [c[k] - 1 for k, flag in (("nt_volpn", c["ponds"]), ("nt_iage", c["age"])) if flag]
            for k in s:                      # intent(in), and what the flags leave alone
                if k == "trcrn":
                    rest = [it for it in range(pc.NTRCR) if it not in owned]
                    assert tc.same(r[k][:, :, rest], s[k][:, :, rest]), (name, "a tracer plane the routines do not own changed")
                elif not (c["ponds"] and k in ("apondn", "hpondn")):
                    assert tc.same(r[k], s[k]), (name, k, "changed")
            counts = pc.branch_counts(name, s, out)
            print(name, counts, "listed", int(pc.listed(s).sum()))
            for k, v in counts.items():
                total[k] += v
            if m is not None:
                for k, v in m["cond"].items():
                    margins[k] = min(margins.get(k, np.inf), float(v.min()))
            d.update(pc.pack(name, s, out))
            d[f"{name}_seed"] = np.array(c["seed"])
            d[f"{name}_sha256"] = np.array(pc.digest(s))
            d[f"{name}_counts"] = np.array([counts[k] for k in pc.BRANCHES], np.int64)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("total", total)
    print("smallest margins at the four comparisons", margins)
    short = {k: v for k, v in total.items() if v < pc.NEED[k]}
    assert not short, ("branches the reference took in too few (cell, category) pairs", short)
    assert all(v >= pc.MARGIN for v in margins.values()), ("a comparison is closer than 1e-9", margins)
    return d


def timing(L):
    nx, ny, reps = 322, 386, 5
    s = pc.make_inputs("melt", 1, ny, nx)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ref_case(L, "melt", s)
        t.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    {k: v.copy() for k, v in s.items()}
    copy = time.perf_counter() - t0
    print(f"reference (amdflang -O2) on host {platform.node()} ({platform.machine()}), one core, one block of 320 x 384 "
          f"cells + ghosts, {pc.NCAT} categories, {int(pc.listed(s).sum())} listed (cell, category) pairs, median of {reps}: "
          f"increment_age + compute_ponds x {pc.NCAT} {np.median(t) * 1e3:.2f} ms (min {min(t) * 1e3:.2f}, max "
          f"{max(t) * 1e3:.2f}; the lists of the wrapper and a copy of the inputs, {copy * 1e3:.2f} ms, included)")


if __name__ == "__main__":
    if "--time" in sys.argv:
        tmp = tempfile.mkdtemp(prefix="pond_")
        try:
            L = build(tmp, "gx1", mgs.GX1)
            threading.stack_size(1 << 30)      # the reference's automatic arrays of a gx1-size block live on the stack
            th = threading.Thread(target=timing, args=(L,))
            th.start()
            th.join()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    else:
        d = mint()
        d["meta"] = np.array(["reference: COSIMA/cice4 source/ice_meltpond.F90 (compute_ponds), source/ice_age.F90 "
                              "(increment_age); compiler: " + mgs.FC.split("/")[-1] + " (flang) " + mgs.BASE + " " + mgs.SMALL +
                              "; configuration small; generator: tests/golden/make_golden_pond.py"])
        d["branches"] = np.array(pc.BRANCHES)
        np.savez_compressed(pc.FIXTURE, **d)
        print("written", pc.FIXTURE, os.path.getsize(pc.FIXTURE), "bytes")
