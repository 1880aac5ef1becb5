#!/usr/bin/env python3
"""Mint tests/golden/atmo.npz FROM THE COMPILED REFERENCE: atmo_boundary_layer of its source/ice_atmo.F90 (through
oracle/refapi.py, Ref.atmo_boundary_layer of oracle/_ref/libcice_ref_gx3.so) on the cases of tests/atmo_case.py.

Per case the fixture holds the eight input fields, the list, the eight outputs on the listed cells of the run with
calc_strair = T (the minter checks that every other word is +0), the cells of the constructed part per class of
atmo_case.BRANCHES, the seed and a checksum of the inputs; for the case atmo_case.LIST_CASE also the run with calc_strair = F
(the caller's stresses and the outputs) and the run on the full interior; and `meta`.  Data only.

The script asserts on what the reference DID -- every output finite, zeros off the list, the caller's stresses untouched
under calc_strair = F, delq exactly 0 on the `neutral` cells, every class in at least atmo_case.NEED cells of the constructed
part, the conditioning rule of atmo_case on every listed cell -- and writes nothing otherwise.

Run from the repo root where oracle/_ref is built:  python tests/golden/make_golden_atmo.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)

import atmo_case as ac  # noqa: E402

FC = os.environ.get("FC", "/opt/rocm/bin/amdflang")
FLAGS = "-O2 -fPIC -w -cpp -fdefault-real-8 -fconvert=big-endian -ffp-contract=off -DLINUX"     # oracle/build_ref.sh


def run(ref, sfctype, mask, a, calc_strair=True, sx=None, sy=None):
    """the reference on the list of `mask`, checked: finite, +0 off the list"""
    icells, indxi, indxj = ac.make_list(mask)
    o = ref.atmo_boundary_layer(sfctype, icells, indxi, indxj, a, calc_strair=calc_strair, strx=sx, stry=sy)
    for k in ac.OUT:
        assert np.isfinite(o[k]).all(), (sfctype, k, "not finite")
        if calc_strair or k not in ("strx", "stry"):
            assert not o[k][~mask].view(np.uint64).any(), (sfctype, k, "a word off the list is not +0")
    return o


def mint(ref=None):
    if ref is None:
        from oracle import refapi
        ref = refapi.Ref("gx3")
    d = {}
    for name, c in ac.CASES.items():
        sfc = c["sfctype"]
        a, mask, sx, sy = ac.make_inputs(name)
        before = ac.digest(a)
        out = run(ref, sfc, mask, a)
        ours = ac.atmo_numpy(sfc, *ac.make_list(mask), a)
        bad = ac.ill_conditioned(ours[1], mask)
        assert not bad.any(), (name, "0 < |hol| < HOL_MIN on listed cells", np.argwhere(bad).tolist())
        neutral = ac.class_masks(sfc, a, ours[1], mask)["neutral"] & ac.constructed_mask(sfc)
        assert neutral.sum() >= ac.NEED and not out["delq"][neutral].view(np.uint64).any() \
            and not out["delt"][neutral].view(np.uint64).any(), (name, "the reference's delt, delq on the neutral cells are not +0")
        counts = ac.branch_counts(sfc, a, mask, out, ours)
        print(name, int(mask.sum()), "listed cells;", counts)
        short = {k: v for k, v in counts.items() if v < ac.needed(sfc)[k]}
        assert not short, (name, "classes the reference took in too few cells of the constructed part", short)
        icells, indxi, indxj = ac.make_list(mask)
        for k in ac.INS:
            d[f"{name}_{k}"] = a[k]
        d[f"{name}_icells"] = np.array(icells)
        d[f"{name}_indxi"], d[f"{name}_indxj"] = indxi[:icells].copy(), indxj[:icells].copy()
        for k, v in ac.pack(mask, out).items():
            d[f"{name}_{k}"] = v
        if name == ac.LIST_CASE:
            o = run(ref, sfc, mask, a, calc_strair=False, sx=sx, sy=sy)
            assert np.array_equal(o["strx"], sx) and np.array_equal(o["stry"], sy), "calc_strair = F: the stresses changed"
            for k in ac.OUT:
                if k not in ("strx", "stry"):
                    assert np.array_equal(o[k].view(np.uint64), out[k].view(np.uint64)), (k, "depends on calc_strair")
            d[f"{name}_F_strx_in"], d[f"{name}_F_stry_in"] = sx, sy
            for k, v in ac.pack(mask, o).items():
                d[f"{name}_F_{k}"] = v
            for k, v in ac.pack(ac.interior(), run(ref, sfc, ac.interior(), a)).items():
                d[f"{name}_interior_{k}"] = v
            d[f"{name}_sublists"] = np.array(ac.SUBLISTS)
        assert ac.digest(a) == before, (name, "the reference changed an input")
        d[f"{name}_seed"] = np.array(c["seed"])
        d[f"{name}_sha256"] = np.array(before)
        d[f"{name}_counts"] = np.array([counts[k] for k in ac.BRANCHES], np.int64)
    d["branches"] = np.array(ac.BRANCHES)
    d["meta"] = np.array(["reference: COSIMA/cice4 source/ice_atmo.F90 (atmo_boundary_layer) through oracle/ref_capi.F90 "
                          "(ref_atmo_boundary_layer); compiler: " + FC.split("/")[-1] + " (flang) " + FLAGS +
                          "; configuration gx3; generator: tests/golden/make_golden_atmo.py"])
    return d


if __name__ == "__main__":
    d = mint()
    np.savez_compressed(ac.FIXTURE, **d)
    print("written", ac.FIXTURE, os.path.getsize(ac.FIXTURE), "bytes")
