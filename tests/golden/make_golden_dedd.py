#!/usr/bin/env python3
"""Mint tests/golden/dedd.npz FROM THE COMPILED REFERENCE: the delta-Eddington shortwave of its source/ice_shortwave.F90 for
the cases of tests/dedd_case.py -- for the driver cases shortwave_dEdd_set_snow, shortwave_dEdd_set_pond and shortwave_dEdd
per (block, category) on the lists step_radiation builds, for the block-wise case shortwave_dEdd alone.

ice_shortwave.F90 and the four modules it uses are compiled unmodified, from where they lie, exactly as
make_golden_shortwave.py does it (its compile_five, its flags: those of oracle/build_ref.sh), into a temporary directory
that is deleted again, against the module files of oracle/_ref/obj_small, and linked to oracle/_ref/libcice_ref_small.so
together with the capture wrapper tests/golden/dedd_capture.F90.  Nothing compiled is kept.

The fixture holds seeds, input hashes, the recorded outputs on the pairs where the scheme ran (the minter checks that every
other word is +0), branch counts, the pairs per interval of the snow grain radius table, and `meta`.  The script asserts on
what the reference DID (dedd_case.branch_counts against dedd_case.NEED over the cases, every interval of the radius table
used) and that every output is finite, and writes nothing otherwise.

Run from the repo root where oracle/_ref is built:  python tests/golden/make_golden_dedd.py [--time]
--time: instead of minting, time the reference's dEdd branch of step_radiation on one core of this host for the five
categories of ONE block of gx1 size (320 x 384 cells + ghosts; built against oracle/_ref/obj_gx1) on the inputs of
scripts/dedd_cost.py."""
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

import dedd_case as dc  # noqa: E402
import make_golden_shortwave as mgs  # noqa: E402
from make_golden_shortwave import f8, i4, ice_list  # noqa: E402


def build(tmp, cfg="small", dims=mgs.SMALL):
    refdir = os.path.join(ROOT, "oracle", "_ref")
    obj = os.path.join(refdir, "obj_" + cfg)
    flags = (mgs.BASE + " " + dims).split()
    objs = mgs.compile_five(tmp, obj, flags)
    o = os.path.join(tmp, "dedd_capture.o")
    subprocess.check_call([mgs.FC, *flags, "-J", tmp, "-I", tmp, "-I", obj, "-c", os.path.join(HERE, "dedd_capture.F90"), "-o", o])
    so = os.path.join(tmp, "libdedd_capture.so")
    subprocess.check_call([mgs.FC, "-shared", "-o", so, o, *objs, "-L", refdir, "-lcice_ref_" + cfg, "-Wl,-rpath," + refdir])
    L = C.CDLL(so)
    L.ddcap_exp_min.restype = C.c_double
    return L


def cap_set(L, name):
    c = dc.CASES[name]
    L.ddcap_set(C.c_double(c["R_ice"]), C.c_double(c["R_pnd"]), C.c_double(c["R_snw"]))
    got, want = L.ddcap_exp_min(), dc._libm.exp(-10.0)
    assert got == want, ("the reference's exp_min is not the host libm's exp(-10)", got.hex(), want.hex())


def ref_pair(L, name, s, b, n, blk_b, poison=np.nan):
    """the reference on (block b, category n); every output starts as `poison` (intent(out))"""
    c = dc.CASES[name]
    ny, nx = s["aicen"].shape[2:]
    icells, indxi, indxj = ice_list(s["aicen"][b, n], blk_b, nx * ny)
    o = {k: np.full((dc.LAYERS[k], ny, nx) if k in dc.LAYERS else (ny, nx), poison) for k in dc.OUT}
    cat = lambda k: f8(np.ascontiguousarray(s[k][b, n]))  # noqa: E731
    cell = lambda k: f8(np.ascontiguousarray(s[k][b]))  # noqa: E731
    outs = [f8(o[k]) for k in ("alvdrn", "alvdfn", "alidrn", "alidfn", "fswsfcn", "fswintn", "fswthrun", "Sswabsn", "Iswabsn",
                               "albicen", "albsnon", "albpndn")]
    if c["blockwise"]:
        L.ddcap_dedd(icells, i4(indxi), i4(indxj), cell("coszen"), cat("aicen"), cat("vicen"), cat("vsnon"), cat("fs"),
                     cat("rhosnw"), cat("rsnw"), cat("fp"), cat("hp"), *[cell(k) for k in dc.SW], *outs)
    else:
        zero = np.zeros((ny, nx))
        pond = [cat("apondn"), cat("hpondn")] if c["tr_pond"] else [f8(zero), f8(zero)]
        L.ddcap_step(icells, i4(indxi), i4(indxj), int(c["tr_pond"]), cell("coszen"), cat("aicen"), cat("vicen"), cat("vsnon"),
                     f8(np.ascontiguousarray(s["trcrn"][b, n, 0])), *pond, *[cell(k) for k in dc.SW], *outs)
    return o


def run_case(L, name, s=None):
    cap_set(L, name)
    s = dc.case_inputs(name) if s is None else s
    nb, ncat, ny, nx = s["aicen"].shape
    blk = dc.block_table(nb, ny, nx)
    out = {k: np.zeros((nb, ncat) + ((dc.LAYERS[k],) if k in dc.LAYERS else ()) + (ny, nx)) for k in dc.OUT}
    for b in range(nb):
        for n in range(ncat):
            o = ref_pair(L, name, s, b, n, blk[b])
            for k in dc.OUT:
                assert np.isfinite(o[k]).all(), (name, b, n, k, "not finite")
                out[k][b, n] = o[k]
    return s, out


def mint():
    d = {}
    total = {k: 0 for k in dc.BRANCHES}
    intervals = np.zeros(31, np.int64)
    tmp = tempfile.mkdtemp(prefix="dedd_")
    try:
        L = build(tmp)
        for name in dc.CASES:
            s, out = run_case(L, name)
            counts, iv = dc.branch_counts(name, s, out)
            print(name, counts, "intervals", iv.tolist())
            for k, v in counts.items():
                total[k] += v
            if dc.CASES[name]["blockwise"]:
                intervals += iv
            d.update(dc.pack(name, s, out))
            d[f"{name}_seed"] = np.array(dc.CASES[name]["seed"])
            d[f"{name}_sha256"] = np.array(dc.digest(s))
            d[f"{name}_counts"] = np.array([counts[k] for k in dc.BRANCHES], np.int64)
            d[f"{name}_intervals"] = iv
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("total", total, "intervals of the radius table (tables)", intervals.tolist())
    short = {k: v for k, v in total.items() if v < dc.NEED[k]}
    assert not short, ("branches the reference took in too few (cell, category) pairs", short)
    assert (intervals >= dc.NEED_INTERVALS).all(), ("intervals of the radius table no pair used", intervals.tolist())
    return d


def timing(L):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import dedd_cost as cost
    nx, ny, reps = 322, 386, 3
    cap_set(L, "default")
    s = cost.inputs(nx, ny, 1)
    blk = dc.block_table(1, ny, nx)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for n in range(dc.NCAT):
            ref_pair(L, "default", s, 0, n, blk[0], poison=0.0)
        t.append(time.perf_counter() - t0)
    on = dc.listed(s, blk)
    lit = int((on & (s["coszen"] > dc.PUNY)[:, None]).sum())
    print(f"reference (amdflang -O2) on host {platform.node()} ({platform.machine()}), one core, one block of 320 x 384 "
          f"cells + ghosts, {dc.NCAT} categories, {int(on.sum())} listed (cell, category) pairs, {lit} of them with the sun up, "
          f"median of {reps}: set_snow + set_pond + shortwave_dEdd x {dc.NCAT} {np.median(t) * 1e3:.1f} ms "
          f"(min {min(t) * 1e3:.1f}, max {max(t) * 1e3:.1f}; the lists and the copies of the wrapper included)")


if __name__ == "__main__":
    if "--time" in sys.argv:
        tmp = tempfile.mkdtemp(prefix="dedd_")
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
        d["meta"] = np.array(["reference: COSIMA/cice4 source/ice_shortwave.F90 (shortwave_dEdd, shortwave_dEdd_set_snow, "
                              "shortwave_dEdd_set_pond); compiler: " + mgs.FC.split("/")[-1] + " (flang) " + mgs.BASE + " " +
                              mgs.SMALL + "; configuration small; generator: tests/golden/make_golden_dedd.py"])
        d["branches"] = np.array(dc.BRANCHES)
        np.savez_compressed(dc.FIXTURE, **d)
        print("written", dc.FIXTURE, os.path.getsize(dc.FIXTURE), "bytes")
