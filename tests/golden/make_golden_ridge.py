#!/usr/bin/env python3
"""Mint tests/golden/ridge.npz FROM THE COMPILED REFERENCE: ridge_ice of its source/ice_mechred.F90 for the cases of
tests/ridge_case.py.

The capture wrapper tests/golden/ridge_capture.F90 is compiled into a temporary directory that is deleted again: against
the module files of oracle/_ref/obj_small, linked to oracle/_ref/libcice_ref_small.so, with the flags of
oracle/build_ref.sh.  Nothing compiled is kept.  The fixture holds seeds, input hashes, recorded outputs, the iterations
per block (counted from the "Repeat ridging" lines the reference writes to nu_diag), the branch counts and `meta`.  The
script asserts on what the reference DID (ridge_case.branch_counts against ridge_case.NEED over the ordinary cases; the
stop) and that every output is finite, and writes nothing otherwise.

Run from the repo root where oracle/_ref is built:  python tests/golden/make_golden_ridge.py [--time | --search N]
--time: instead of minting, time ridge_ice of the reference on one core of this host on ONE block of gx1 size (320 x 384
cells + ghosts; the wrapper is then built against oracle/_ref/obj_gx1 and libcice_ref_gx1.so) on the inputs of
scripts/ridge_cost.py, and print the host's name with the figures.
--search N: N seeded variations of the first case's inputs with stronger forcing; prints the largest number of iterations a
block took (the niter == nitermax stop is pinned only if one reaches 20)."""
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

import ridge_case as rc  # noqa: E402
import therm_itd_case as tc  # noqa: E402

FC = os.environ.get("FC", "/opt/rocm/bin/amdflang")
BASE = "-O2 -fPIC -w -cpp -fdefault-real-8 -fconvert=big-endian -ffp-contract=off -DLINUX"
SMALL = "-DNXGLOB=24 -DNYGLOB=20 -DBLCKX=12 -DBLCKY=10 -DMXBLCKS=4"
GX1 = "-DNXGLOB=320 -DNYGLOB=384 -DBLCKX=320 -DBLCKY=384 -DMXBLCKS=1"


def build(tmp, cfg="small", dims=SMALL):
    obj, flags = os.path.join(ROOT, "oracle", "_ref", "obj_" + cfg), (BASE + " " + dims).split()
    src = os.path.join(HERE, "ridge_capture.F90")
    o = os.path.join(tmp, "ridge_capture.o")
    subprocess.check_call([FC, *flags, "-J", tmp, "-I", tmp, "-I", obj, "-c", src, "-o", o])
    so = os.path.join(tmp, "libridge_capture.so")
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


def cap_set(L, kw, rk):
    dep = np.zeros(5, np.int32)
    dep[:kw["ntrcr"]] = kw["trcr_depend"]
    hm = np.ascontiguousarray(kw["hin_max"], np.float64)
    L.rcap_set(kw["ntrcr"], i4(dep), kw["nt_Tsfc"], kw["nt_alvl"], kw["nt_vlvl"], int(kw["tr_lvl"]), f8(hm),
               rk["krdg_partic"], rk["krdg_redist"], C.c_double(rk["mu_rdg"]), L.diag.encode(), len(L.diag))


def repeats(L):
    """"Repeat ridging" lines in nu_diag so far"""
    if not os.path.exists(L.diag):
        return 0
    with open(L.diag, errors="replace") as f:
        return sum(1 for line in f if "Repeat ridging" in line)


def ref_ridge(L, blk, lst, with_opt=1, dt=rc.DT):
    """ridge_ice on one block; returns (l_stop, istop, jstop, niter)"""
    icells, indxi, indxj = lst
    st = [C.c_int(0) for _ in range(3)]
    before = repeats(L)
    L.rcap_ridge_ice(C.c_double(dt), icells, i4(indxi), i4(indxj),
                     *[f8(blk[k]) for k in ("rdg_conv", "rdg_shear", "aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon",
                                            "aice0")], *[C.byref(x) for x in st],
                     *[f8(blk[k]) for k in rc.OPTIONAL], with_opt)
    return tuple(x.value for x in st) + (repeats(L) - before + 1,)


def run_case(L, name):
    cap_set(L, rc.itd_kwargs(name), rc.ridge_kwargs(name))
    s = rc.case_inputs(name)
    out = {k: v.copy() for k, v in s.items()}
    niter = np.zeros(rc.NB, np.int32)
    for b in range(rc.NB):
        lst = rc.tmask_list(s["tmask"][b])
        if lst[0] == 0:                  # `if (icells > 0)` of the caller
            continue
        blk = tc.block(out, b)
        r = ref_ridge(L, blk, lst)
        assert r[:3] == (0, 0, 0), (name, b, r)
        niter[b] = r[3]
        for k in rc.OUT:
            out[k][b] = blk[k]
            assert np.isfinite(blk[k]).all(), (name, b, k, "not finite")
    return s, out, niter


def mint(L):
    d = {}
    total = {k: 0 for k in rc.BRANCHES}
    for name in rc.ORDINARY:
        s, out, niter = run_case(L, name)
        counts = rc.branch_counts(name, s, out, niter)
        print(name, "niter", niter.tolist(), counts)
        for k, v in counts.items():
            total[k] += v
        for k in rc.OUT:
            d[f"{name}_out_{k}"] = tc.xor(out[k], s[k])
        d[f"{name}_niter"] = niter
        d[f"{name}_seed"] = np.array(rc.CASES[name]["seed"])
        d[f"{name}_sha256"] = np.array(rc.digest(s))
        d[f"{name}_counts"] = np.array([counts[k] for k in rc.BRANCHES], np.int64)
    print("total", total)
    short = {k: v for k, v in total.items() if v < rc.NEED[k]}
    assert not short, ("branches the reference took in too few cells", short)
    # the stop: rdg_conv < 0 in two cells; the first is named, the second untouched
    cap_set(L, rc.itd_kwargs(rc.STOP), rc.ridge_kwargs(rc.STOP))
    blk, cells = rc.stop_inputs()
    d[f"{rc.STOP}_sha256"] = np.array(rc.digest(blk))
    before = {k: v.copy() for k, v in blk.items()}
    r = ref_ridge(L, blk, rc.tmask_list(blk["tmask"]))
    assert r[:3] == (1,) + cells[0], ("the reference reports", r, "expected", cells[0])
    (i1, j1), (i2, j2) = cells
    assert blk["aice0"][j1 - 1, i1 - 1] < -rc.PUNY
    assert tc.same(blk["aice0"][j2 - 1, i2 - 1], before["aice0"][j2 - 1, i2 - 1])
    for k in rc.STATE + rc.OPTIONAL:
        assert tc.same(blk[k], before[k]), ("the reference changed", k, "in the iteration that stopped")
    assert not tc.same(blk["aice0"], before["aice0"])
    d[f"{rc.STOP}_stop"] = np.array(r[:3])
    d[f"{rc.STOP}_niter"] = np.array(r[3])
    d[f"{rc.STOP}_cells"] = np.array(cells)
    for k in rc.OUT:
        d[f"{rc.STOP}_out_{k}"] = blk[k]
    return d


def search(L, n):
    """seeded variations with forcing up to 1e-4 1/s: the most iterations any block took"""
    most, stops = 0, 0
    cap_set(L, rc.itd_kwargs("ntr4"), rc.ridge_kwargs("ntr4"))
    s0 = rc.case_inputs("ntr4")
    for k in range(n):
        rng = np.random.default_rng(2026102100 + k)
        s = {key: v.copy() for key, v in s0.items()}
        s["rdg_conv"] = np.where(rng.random(s["aice0"].shape) < 0.5, 10.0 ** rng.uniform(-7.0, -4.0, s["aice0"].shape), 0.0)
        s["aice0"] = s["aice0"] * rng.uniform(0.0, 1.0, s["aice0"].shape)
        for b in range(rc.NB):
            lst = rc.tmask_list(s["tmask"][b])
            if lst[0]:
                r = ref_ridge(L, tc.block(s, b), lst)
                most = max(most, r[3])
                stops += r[0]
    print(f"search over {n} x {rc.NB} blocks: at most {most} iterations, {stops} stops")


def timing(L):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import ridge_cost as cost
    nx, ny, reps = 322, 386, 5
    cap_set(L, rc.itd_kwargs("ntr1"), rc.ridge_kwargs("ntr1"))
    for regime in ("growth", "melt"):
        raw = cost.inputs(regime, nx, ny, 1)
        blk0 = tc.block(raw, 0)
        jj, ii = np.nonzero(blk0["tmask"][1:-1, 1:-1])
        lst = [len(ii), np.zeros(nx * ny, np.int32), np.zeros(nx * ny, np.int32)]
        lst[1][:len(ii)] = ii + 2
        lst[2][:len(ii)] = jj + 2
        t, nit = [], 0
        for _ in range(reps):
            w = {k: v.copy() for k, v in blk0.items()}
            t0 = time.perf_counter()
            r = ref_ridge(L, w, lst)
            t.append(time.perf_counter() - t0)
            assert r[0] == 0, r
            nit = r[3]
        print(f"{regime}: reference (amdflang -O2) on host {platform.node()} ({platform.machine()}), one core, one block of "
              f"320 x 384 cells + ghosts, {lst[0]} listed cells, {nit} iterations, median of {reps}: ridge_ice "
              f"{np.median(t) * 1e3:.2f} ms")


if __name__ == "__main__":
    tmp = tempfile.mkdtemp(prefix="ridge_")
    try:
        if "--time" in sys.argv:
            L = build(tmp, "gx1", GX1)
            threading.stack_size(1 << 30)      # the reference's automatic arrays of a gx1-size block live on the stack
            th = threading.Thread(target=timing, args=(L,))
            th.start()
            th.join()
        elif "--search" in sys.argv:
            search(build(tmp), int(sys.argv[sys.argv.index("--search") + 1]))
        else:
            d = mint(build(tmp))
            d["meta"] = np.array(["reference: COSIMA/cice4 source/ice_mechred.F90 (ridge_ice); compiler: " +
                                  FC.split("/")[-1] + " (flang) " + BASE + " " + SMALL + "; configuration small; generator: "
                                  "tests/golden/make_golden_ridge.py"])
            np.savez_compressed(rc.FIXTURE, **d)
            print("written", rc.FIXTURE, os.path.getsize(rc.FIXTURE), "bytes")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
