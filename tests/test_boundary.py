"""Boundary module (ice_HaloCreate / ice_HaloUpdate / ice_HaloExtrapolate) against the compiled
reference, one process per boundary combination (tests/boundary_case.py)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Rectangular grid.  'closed' edges cannot be initialised with any grid the reference ships
# (rectgrid aborts for closed E-W, ice_grid.F90:1124; the gx3 land mask has ocean on the northern
# edge, ice_domain.F90:313-347); for ghost copies the reference treats 'closed' exactly like 'open'
# (no neighbour: ice_blocks.F90:455-458,482-485,504-507,522-525), which is what 'open' covers here.
CASES = [("gx3b4", "cyclic", "open"), ("pad", "cyclic", "open"), ("pad", "open", "open"),
         ("pad", "open", "cyclic"), ("pad", "cyclic", "cyclic"), ("padx", "cyclic", "open"),   # padx: max_blocks > blocks
         # tripole (U-fold) north boundary, serial/ice_boundary.F90:705-869: every field location x kind x type
         ("small", "cyclic", "tripole"), ("pad", "cyclic", "tripole"),
         # the fold through T points (serial/ice_boundary.F90:725-776: three buffer rows, other offsets and symmetric pairs)
         # (2 x 2 blocks, and 10 x 12 blocks with a padded last column and six rows in the top block row; the 'pad'
         #  configurations have two rows there: the reference itself stops, "not enough points in block for tripole")
         ("small", "cyclic", "tripoleT"), ("gx3b4", "cyclic", "tripoleT"),
         # land-block elimination on the reference's own gx3 grid and land mask: 10 x 12 blocks, the 4 all-land ones dropped by
         # create_distribution; ghost cells facing them take the fill value (mpi/ice_boundary.F90:5108-5111)
         ("gx3e", "cyclic", "open", "gx3"),
         # ... and the same block distribution under either fold
         ("gx3e", "cyclic", "tripole", "gx3"), ("gx3e", "cyclic", "tripoleT", "gx3")]


# test_boundary_module_dropin once more with the host arrays of these cases updated ON THE DEVICE: every fold, the
# eliminated land blocks, and padded blocks without either
ON_DEVICE = [c for c in CASES if c[2].startswith("tripole") or c[0] == "gx3e" or c == ("pad", "cyclic", "open")]
HOST_ON_DEVICE = "CICE4_AMD_HALO_HOST_ON_DEVICE"
# lists only: the gx3 land mask with one block of the top block row made land, so that the reference eliminates a top-row
# block as well -- under a fold its cells are missing from the tripole buffer, which keeps fillValue there
LISTS_ONLY = [("gx3e", "cyclic", "tripole", "gx3-landtop"), ("gx3e", "cyclic", "tripoleT", "gx3-landtop")]


def run_case(mode, cfg, ew, ns, *extra, on_device=False):
    from oracle import refapi
    need = [("ref", cfg)] + ([("dropin", cfg)] if mode == "gpu" else [])
    for kind, c in need:
        if not refapi.available(c, kind):
            pytest.skip(f"oracle/_ref/libcice_{kind}_{c}.so not built")
    env = {k: v for k, v in os.environ.items() if k != HOST_ON_DEVICE}
    if on_device:
        env[HOST_ON_DEVICE] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "boundary_case.py"), mode, cfg, ew, ns, *extra],
                       capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0 and "BOUNDARY-OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


@pytest.mark.parametrize("case", CASES + LISTS_ONLY, ids=lambda c: "-".join(c))
def test_halo_lists_equal_reference_update(case):
    """Host topology (cice4_amd/csrc/domain.cpp) == serial/ice_boundary.F90 for padded blocks and
    every boundary type the path supports."""
    run_case("lists", *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case,on_device", [pytest.param(c, False, id="-".join(c)) for c in CASES] +
                         [pytest.param(c, True, id="-".join(c) + "-on-device") for c in ON_DEVICE])
def test_boundary_module_dropin(case, on_device):
    """The reference's callers (ice_domain, ice_grid, ice_state) linked with our ice_boundary
    module: same grid, same updates, bit for bit.  These domains have one rank, so the module's
    host arrays are updated on the HOST from the domain's lists (halo_host_lists); only evp(dt),
    whose fields are resident, fills ghost cells on the MI355X.  on_device: the same run with
    CICE4_AMD_HALO_HOST_ON_DEVICE=1 in the child's environment -- every ice_HaloUpdate of a host
    array then runs on the MI355X, on the gathered frame of the blocks or on the whole field."""
    run_case("gpu", *case, on_device=on_device)
