#!/usr/bin/env python3
"""Mint tests/golden/shortwave.npz FROM THE COMPILED REFERENCE: shortwave_ccsm3 of its source/ice_shortwave.F90 for the
cases of tests/shortwave_case.py, per (block, category) on the lists step_radiation builds.

ice_shortwave.F90 is not in the closure of oracle/build_ref.sh.  It and the four modules it uses (csm_share/shr_orb_mod,
source/ice_diagnostics, ice_orbital, ice_meltpond) are compiled unmodified, from where they lie, with the flags of
oracle/build_ref.sh, into a temporary directory that is deleted again, against the module files of oracle/_ref/obj_small
and linked to oracle/_ref/libcice_ref_small.so together with the capture wrapper tests/golden/shortwave_capture.F90.  The
case "auscom" is minted from the -DAusCOM compile of ice_shortwave.F90 (and of the wrapper) against obj_small_aus, which
`AUS=1 oracle/build_ref.sh small ...` builds first where it is missing.  Nothing compiled is kept.

The fixture holds seeds, input hashes, recorded outputs, branch counts and `meta`.  The script asserts on what the
reference DID (shortwave_case.branch_counts against shortwave_case.NEED over the cases) and that every output is finite,
and writes nothing otherwise.

Run from the repo root where oracle/_ref is built:  python tests/golden/make_golden_shortwave.py [--time]
--time: instead of minting, time shortwave_ccsm3 of the reference on one core of this host for the five categories of ONE
block of gx1 size (320 x 384 cells + ghosts; built against oracle/_ref/obj_gx1) on the inputs of scripts/radiation_cost.py."""
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

import shortwave_case as sc  # noqa: E402
import therm_itd_case as tc  # noqa: E402

FC = os.environ.get("FC", "/opt/rocm/bin/amdflang")
REF = os.environ.get("CICE_REFERENCE_ROOT", "/root/reference")
BASE = "-O2 -fPIC -w -cpp -fdefault-real-8 -fconvert=big-endian -ffp-contract=off -DLINUX"
SMALL = "-DNXGLOB=24 -DNYGLOB=20 -DBLCKX=12 -DBLCKY=10 -DMXBLCKS=4"
GX1 = "-DNXGLOB=320 -DNYGLOB=384 -DBLCKX=320 -DBLCKY=384 -DMXBLCKS=1"
# ice_shortwave.F90 and what it uses beyond the closure of build_ref.sh, in dependency order
FIVE = ("csm_share/shr_orb_mod.F90", "source/ice_diagnostics.F90", "source/ice_orbital.F90", "source/ice_meltpond.F90",
        "source/ice_shortwave.F90")


def compile_five(tmp, obj, flags, auscom=False):
    """the five files into tmp; returns the object files"""
    objs = []
    for f in FIVE:
        o = os.path.join(tmp, os.path.basename(f)[:-4] + ".o")
        extra = ["-DAusCOM"] if auscom and f.endswith("ice_shortwave.F90") else []
        subprocess.check_call([FC, *flags, *extra, "-J", tmp, "-I", tmp, "-I", obj, "-c", os.path.join(REF, f), "-o", o])
        objs.append(o)
    return objs


def build(tmp, cfg="small", dims=SMALL, auscom=False):
    refdir = os.path.join(ROOT, "oracle", "_ref")
    obj = os.path.join(refdir, "obj_" + cfg + ("_aus" if auscom else ""))
    libname = "cice_ref" + ("aus" if auscom else "") + "_" + cfg
    if auscom and not os.path.exists(os.path.join(refdir, "lib" + libname + ".so")):
        n = [x[2:].split("=")[1] for x in dims.split()]
        subprocess.check_call(["bash", os.path.join(ROOT, "oracle", "build_ref.sh"), cfg, *n],
                              env=dict(os.environ, AUS="1"), stdout=subprocess.DEVNULL)
    flags = (BASE + " " + dims).split()
    objs = compile_five(tmp, obj, flags, auscom)
    o = os.path.join(tmp, "shortwave_capture.o")
    subprocess.check_call([FC, *flags, *(["-DAusCOM"] if auscom else []), "-J", tmp, "-I", tmp, "-I", obj, "-c",
                           os.path.join(HERE, "shortwave_capture.F90"), "-o", o])
    so = os.path.join(tmp, "libshortwave_capture.so")
    subprocess.check_call([FC, "-shared", "-o", so, o, *objs, "-L", refdir, "-l" + libname, "-Wl,-rpath," + refdir])
    return C.CDLL(so)


def f8(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def i4(a):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def cap_set(L, name):
    c = sc.CASES[name]
    nl = sc.NAMELIST
    L.swcap_set(int(c["albedo_type"] == "constant"), *[C.c_double(nl[k]) for k in ("albicev", "albicei", "albsnowv",
                                                                                  "albsnowi", "ahmax")],
                C.c_double(c["snowpatch"]), C.c_double(c["dT_mlt"]), C.c_double(c["dalb_mlt"]),
                *[C.c_double(c.get("awt", sc.AWT)[k]) for k in ("awtvdr", "awtidr", "awtvdf", "awtidf")])


def ice_list(aicen_bn, blk_b, pad):
    """step_radiation's list of a (block, category): aicen > puny on the physical cells, j then i, 1-based"""
    ilo, ihi, jlo, jhi = (int(x) for x in blk_b)
    jj, ii = np.nonzero(aicen_bn[jlo - 1:jhi, ilo - 1:ihi] > sc.PUNY)
    indxi, indxj = np.zeros(pad, np.int32), np.zeros(pad, np.int32)
    indxi[:len(ii)] = ii + ilo
    indxj[:len(ii)] = jj + jlo
    return len(ii), indxi, indxj


def ref_ccsm3(L, s, b, n, blk_b, poison=np.nan):
    """shortwave_ccsm3 of the reference on (block b, category n); every output starts as `poison` (intent(out))"""
    ny, nx = s["aicen"].shape[2:]
    icells, indxi, indxj = ice_list(s["aicen"][b, n], blk_b, nx * ny)
    o = {k: np.full((ny, nx), poison) for k in ("alvdrn", "alidrn", "alvdfn", "alidfn", "fswsfcn", "fswintn", "fswthrun")}
    o["Iswabsn"] = np.full((sc.NILYR, ny, nx), poison)
    o["albicen"], o["albsnon"] = np.full((ny, nx), poison), np.full((ny, nx), poison)
    ocn = np.ascontiguousarray(s["ocn_albedo"][b]) if "ocn_albedo" in s else np.zeros((ny, nx))
    tsf = np.ascontiguousarray(s["trcrn"][b, n, 0])
    L.swcap_ccsm3(icells, i4(indxi), i4(indxj), *[f8(np.ascontiguousarray(s[k][b, n])) for k in ("aicen", "vicen", "vsnon")],
                  f8(tsf), *[f8(np.ascontiguousarray(s[k][b])) for k in sc.SW],
                  *[f8(o[k]) for k in ("alvdrn", "alidrn", "alvdfn", "alidfn", "fswsfcn", "fswintn", "fswthrun", "Iswabsn",
                                       "albicen", "albsnon")], f8(ocn))
    return o


def run_case(L, name):
    cap_set(L, name)
    s = sc.case_inputs(name)
    nb, ncat, ny, nx = s["aicen"].shape
    blk = sc.block_table(nb, ny, nx)
    out = {k: np.zeros((nb, ncat) + ((sc.NILYR,) if k == "Iswabsn" else ()) + (ny, nx)) for k in sc.OUT}
    for b in range(nb):
        for n in range(ncat):
            o = ref_ccsm3(L, s, b, n, blk[b])
            for k in sc.OUT:
                assert np.isfinite(o[k]).all(), (name, b, n, k, "not finite")
                out[k][b, n] = o[k]
    return s, out


def mint():
    d = {}
    total = {k: 0 for k in sc.BRANCHES}
    for name in sc.CASES:
        tmp = tempfile.mkdtemp(prefix="shortwave_")
        try:
            L = build(tmp, auscom=sc.CASES[name]["flavour"] == "auscom")
            s, out = run_case(L, name)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        counts = sc.branch_counts(name, s, out)
        print(name, counts)
        for k, v in counts.items():
            total[k] += v
        for k in sc.OUT:
            if k in ("alvdrn", "alidrn"):
                continue
            d[f"{name}_{k}"] = np.ascontiguousarray(out[k]).view(np.uint64)
        for dr, df in (("alvdrn", "alvdfn"), ("alidrn", "alidfn")):
            d[f"{name}_{dr}_xor"] = tc.xor(out[dr], out[df])
            assert not d[f"{name}_{dr}_xor"].any(), (name, dr, "direct differs from diffuse")
        d[f"{name}_seed"] = np.array(sc.CASES[name]["seed"])
        d[f"{name}_sha256"] = np.array(sc.digest(s))
        d[f"{name}_counts"] = np.array([counts[k] for k in sc.BRANCHES], np.int64)
    print("total", total)
    short = {k: v for k, v in total.items() if v < sc.NEED[k]}
    assert not short, ("branches the reference took in too few (cell, category) pairs", short)
    return d


def timing(L):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import radiation_cost as cost
    nx, ny, reps = 322, 386, 5
    cap_set(L, "default")
    s = cost.inputs(nx, ny, 1)
    blk = sc.block_table(1, ny, nx)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for n in range(sc.NCAT):
            ref_ccsm3(L, s, 0, n, blk[0], poison=0.0)
        t.append(time.perf_counter() - t0)
    listed = int(sc.listed(s, blk).sum())
    print(f"reference (amdflang -O2) on host {platform.node()} ({platform.machine()}), one core, one block of 320 x 384 "
          f"cells + ghosts, {sc.NCAT} categories, {listed} listed (cell, category) pairs, median of {reps}: shortwave_ccsm3 "
          f"x {sc.NCAT} {np.median(t) * 1e3:.2f} ms (the lists and the copies of the wrapper included)")


if __name__ == "__main__":
    if "--time" in sys.argv:
        tmp = tempfile.mkdtemp(prefix="shortwave_")
        try:
            L = build(tmp, "gx1", GX1)
            threading.stack_size(1 << 30)      # the reference's automatic arrays of a gx1-size block live on the stack
            th = threading.Thread(target=timing, args=(L,))
            th.start()
            th.join()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    else:
        d = mint()
        d["meta"] = np.array(["reference: COSIMA/cice4 source/ice_shortwave.F90 (shortwave_ccsm3; case auscom: -DAusCOM); "
                              "compiler: " + FC.split("/")[-1] + " (flang) " + BASE + " " + SMALL + "; configuration small; "
                              "generator: tests/golden/make_golden_shortwave.py"])
        np.savez_compressed(sc.FIXTURE, **d)
        print("written", sc.FIXTURE, os.path.getsize(sc.FIXTURE), "bytes")
