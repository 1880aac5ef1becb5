#!/usr/bin/env python3
"""Mint tests/golden/coupling.npz FROM THE COMPILED REFERENCE for the cases of tests/coupling_case.py: its scale_fluxes
(source/ice_flux.F90) on the 13 fluxes and the merged albedos of every block, its ocean_mixed_layer (source/ice_ocean.F90)
called through the module arrays of ice_flux, ice_state, ice_grid and ice_domain with atmbndy = 'default', and its
atmo_boundary_layer('ocn') for the four arrays ocean_mixed_layer keeps local.

All three routines are in the closure of oracle/build_ref.sh: the capture wrapper tests/golden/coupling_capture.F90 is
compiled with that script's flags into a temporary directory that is deleted again, against the module files of
oracle/_ref/obj_small, and linked to oracle/_ref/libcice_ref_small.so.  Nothing compiled is kept.  The loops of
coupling_prep itself live in the driver file, which cannot be compiled here; coupling_case.merge_numpy restates them.

The fixture holds seeds, input hashes, the recorded outputs, branch counts and `meta`.  The script asserts on what the
reference DID -- every branch of coupling_case.BRANCHES in at least coupling_case.NEED cells over the cases, on a physical
and on a ghost cell --, on the conditioning of the mixed layer's cells (coupling_case.ill_conditioned: none), that the
restatements of scale_fluxes and of the mixed layer's tail give the reference's bits, that every output is finite, and
writes nothing otherwise.

Run from the repo root where oracle/_ref is built:  python tests/golden/make_golden_coupling.py [--time]
--time: instead of minting, time the reference's scale_fluxes + ocean_mixed_layer on one core of this host for ONE block of
gx1 size (320 x 384 cells + ghosts; built against oracle/_ref/obj_gx1) on the inputs of scripts/coupling_cost.py."""
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

import atmo_case as ac  # noqa: E402
import coupling_case as cc  # noqa: E402
import make_golden_shortwave as mgs  # noqa: E402
from make_golden_shortwave import f8, i4  # noqa: E402


def build(tmp, cfg="small", dims=mgs.SMALL):
    refdir = os.path.join(ROOT, "oracle", "_ref")
    obj = os.path.join(refdir, "obj_" + cfg)
    flags = (mgs.BASE + " " + dims).split()
    o = os.path.join(tmp, "coupling_capture.o")
    subprocess.check_call([mgs.FC, *flags, "-J", tmp, "-I", tmp, "-I", obj, "-c", os.path.join(HERE, "coupling_capture.F90"),
                           "-o", o])
    so = os.path.join(tmp, "libcoupling_capture.so")
    subprocess.check_call([mgs.FC, "-shared", "-o", so, o, "-L", refdir, "-lcice_ref_" + cfg, "-Wl,-rpath," + refdir])
    return C.CDLL(so)


def ref_scale(L, s, alb):
    """scale_fluxes of the reference block by block on copies: the 17 arrays of coupling_case.SCALED"""
    out = {k: np.array(s[k] if k in cc.FLUXES else alb[k]) for k in cc.SCALED}
    for b in range(s["aice"].shape[0]):
        blk = {k: np.ascontiguousarray(out[k][b]) for k in cc.SCALED}
        L.cpcap_scale(i4(np.ascontiguousarray(s["tmask"][b])), *[f8(np.ascontiguousarray(s[k][b])) for k in ("aice", "Tf", "Tair", "Qa")],
                      *[f8(blk[k]) for k in cc.SCALED])
        for k in cc.SCALED:
            out[k][b] = blk[k]
    return out


def ref_mixed(L, s, poison=np.nan):
    """ocean_mixed_layer of the reference on all blocks, and atmo_boundary_layer('ocn') per block for the four locals"""
    nb, ny, nx = s["sst"].shape
    a_in = np.ascontiguousarray(np.stack([s[k] for k in cc.MIX_CAPTURE_IN]))
    a_io = np.ascontiguousarray(np.stack([s[k] for k in cc.MIX_IO]))
    a_out = np.full((len(cc.MIX_OUT), nb, ny, nx), poison)
    L.cpcap_mixed(nb, C.c_double(cc.DT), i4(s["tmask"]), f8(a_in), f8(a_io), f8(a_out))
    o = dict(zip(cc.MIX_IO, a_io))
    o.update(zip(cc.MIX_OUT, a_out))
    for k in cc.MIX_OPT:
        o[k] = np.full((nb, ny, nx), poison)
    for b in range(nb):
        loc = {k: np.full((ny, nx), poison) for k in cc.MIX_OPT}
        L.cpcap_atmo(i4(np.ascontiguousarray(s["tmask"][b])),
                     *[f8(np.ascontiguousarray(s[k][b])) for k in ("sst", "potT", "uatm", "vatm", "wind", "zlvl", "Qa", "rhoa")],
                     *[f8(loc[k]) for k in ("delt", "delq", "lhcoef", "shcoef")])
        for k in cc.MIX_OPT:
            o[k][b] = loc[k]
    return {k: np.ascontiguousarray(v) for k, v in o.items()}


def same_bits(got, want, what):
    for k in want:
        bad = cc.u64(got[k]) != cc.u64(want[k])
        assert not bad.any(), (what, k, int(bad.sum()), "words differ from the compiled reference", np.argwhere(bad)[:4].tolist())


def mint():
    d = {}
    total = {k: (0, 0) for k in cc.BRANCHES}
    tmp = tempfile.mkdtemp(prefix="coupling_")
    try:
        L = build(tmp)
        for name, c in cc.CASES.items():
            s = cc.case_inputs(name)
            merged = cc.merge_numpy(s)
            scaled = mixed = None
            if c["scale_fluxes"]:
                scaled = ref_scale(L, s, merged)
                same_bits(cc.scale_fluxes_numpy(s, merged), scaled, (name, "scale_fluxes"))
                for k in cc.SCALED:
                    assert np.isfinite(scaled[k]).all(), (name, k, "not finite")
                    d[f"{name}_sf_{k}"] = cc.u64(scaled[k])
            if c["oceanmixed_ice"]:
                mixed = ref_mixed(L, s)
                for k, v in mixed.items():
                    assert np.isfinite(v).all(), (name, k, "not finite")
                    d[f"{name}_ml_{k}"] = cc.u64(v)
                want, m, cond = cc.mixed_tail_numpy(s, mixed)
                same_bits(want, {k: mixed[k] for k in cc.MIX_TAIL}, (name, "mixed layer :190-231"))
                assert all((mixed[k] == cc.ALBOCN).all() for k in cc.MIX_OUT[-4:]), "the ocean albedos are not albocn"
                ocean = s["tmask"] != 0
                for k in cc.MIX_OUT[5:9] + cc.MIX_OPT:
                    assert not cc.u64(mixed[k])[~ocean].any(), (k, "not +0 on land")
                _, hol = cc.atmo_all(s, ac.atmo_numpy)
                bad = {k: int(v.sum()) for k, v in cc.ill_conditioned(s, cond, m, hol).items() if v.any()}
                assert not bad, ("ill-conditioned ocean cells", bad)
            counts = cc.branch_counts(name, s, scaled, mixed)
            print(name, counts)
            total = {k: (total[k][0] + v[0], total[k][1] + v[1]) for k, v in counts.items()}
            d[f"{name}_seed"] = np.array(c["seed"])
            d[f"{name}_sha256"] = np.array(cc.digest(s))
            d[f"{name}_counts"] = np.array([counts[k] for k in cc.BRANCHES], np.int64)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("total", total)
    short = cc.short_of(total)
    assert not short, ("branches the reference took in too few cells (physical, ghost)", short)
    return d


def timing(L):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import coupling_cost as cost
    reps = 5
    s = cost.inputs()
    merged = cc.merge_numpy(s)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ref_mixed(L, s, poison=0.0)
        t1 = time.perf_counter()
        ref_scale(L, s, merged)
        t.append((t1 - t0, time.perf_counter() - t1))
    ml, sf = np.median([x[0] for x in t]), np.median([x[1] for x in t])
    print(f"reference (amdflang -O2) on host {platform.node()} ({platform.machine()}), one core, one block of 320 x 384 "
          f"cells + ghosts, median of {reps}: ocean_mixed_layer {ml * 1e3:.2f} ms (with a second atmo_boundary_layer call for "
          f"the four local arrays), scale_fluxes {sf * 1e3:.2f} ms (the copies of the wrapper included)")


if __name__ == "__main__":
    if "--time" in sys.argv:
        tmp = tempfile.mkdtemp(prefix="coupling_")
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
        d["meta"] = np.array(["reference: COSIMA/cice4 source/ice_flux.F90 (scale_fluxes), source/ice_ocean.F90 "
                              "(ocean_mixed_layer), source/ice_atmo.F90 (atmo_boundary_layer 'ocn'); compiler: " +
                              mgs.FC.split("/")[-1] + " (flang) " + mgs.BASE + " " + mgs.SMALL + "; configuration small; "
                              "generator: tests/golden/make_golden_coupling.py"])
        d["branches"] = np.array(cc.BRANCHES)
        np.savez_compressed(cc.FIXTURE, **d)
        print("written", cc.FIXTURE, os.path.getsize(cc.FIXTURE), "bytes")
