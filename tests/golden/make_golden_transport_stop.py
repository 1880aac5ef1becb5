#!/usr/bin/env python3
"""Mint tests/golden/transport_stop.npz FROM THE COMPILED REFERENCE ITSELF (oracle/_ref/libcice_ref_small.so): the
cell `call transport_remap(dt)` names before it ends through abort_ice, for the failing cases of
tests/transport_stop_case.py.  No GPU and no GPU library: every case runs in a child process with the reference
alone, which prints its diagnosis (ice_transport_remap.F90:1660-1669, 3779-3783; :655-662, 841-875) and stops.

Only recorded numbers are stored, per case: the failure kind (1 departure points, 2 negative area), the local i, j
the reference printed, the printed displacement or new mass, the local block and category of the abort message, the
seed, and the SHA-256 of the inputs.  The script fails if a case's inputs do not meet their conditions (checked in the
children: tests/transport_stop_case.py check_inputs and the `probe` run) or if the reference names another cell
than the case was built to discriminate.

Run from the repo root where oracle/_ref is built:  python tests/golden/make_golden_transport_stop.py
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)

import transport_stop_case as sc  # noqa: E402


def child(mode, name):
    p = subprocess.run([sys.executable, os.path.join(TESTS, "transport_stop_case.py"), mode, name],
                       capture_output=True, text=True, timeout=600)
    return p.returncode, p.stdout, p.stderr


def mint():
    data = {}
    for name, c in sc.CASES.items():
        rc, out, err = child("probe", name)
        assert rc == 0 and "STOP-PROBE-OK" in out, (name, "probe", out[-2000:], err[-2000:])
        rc, out, err = child("mint", name)
        # abort_ice of the serial build is `stop`: a clean exit, after the diagnosis
        assert rc == 0 and "STOP-NOT-REACHED" not in out and "STOP-INPUTS" in out, (name, rc, out[-2000:], err[-2000:])
        r = sc.parse_reference_output(out)
        digest = [ln.split()[2] for ln in out.splitlines() if ln.startswith("STOP-INPUTS")][0]
        assert r["kind"] in (1, 2), (name, out[-2000:])
        # margins of the cell the reference printed: 2 % beyond the edge / below -1e-3
        if r["kind"] == 1:
            assert r["value"] > 0.0
        else:
            assert r["value"] < -1e-3, (name, r)
        assert (r["kind"], r["i"], r["j"]) == c["expect"], (name, "the reference names", r, "expected", c["expect"])
        for k, v in r.items():
            data[f"{name}_{k}"] = np.array(v)
        data[f"{name}_seed"] = np.array(c["seed"])
        data[f"{name}_sha256"] = np.array(digest)
    return data


if __name__ == "__main__":
    d = mint()
    d["meta"] = np.array(["reference: COSIMA/cice4, -O2 -fdefault-real-8 -ffp-contract=off (oracle/build_ref.sh), configuration "
                          "small cyclic open; generator: tests/golden/make_golden_transport_stop.py"])
    np.savez_compressed(sc.FIXTURE, **d)
    for name in sc.CASES:
        print(name, {k: d[f"{name}_{k}"].item() for k in ("kind", "i", "j", "value", "iblk", "cat")})
    print("written", sc.FIXTURE)
