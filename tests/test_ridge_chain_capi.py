"""The transport -> ridging hand-over without a device: both builds of the library export cice_ridge_chain and
cice_transport_download_state, the header declares them, the argument check and the behaviour on a host without a GPU, and
the Fortran side (interface blocks in cice4_amd_c.F90, the CICE4_AMD_CHAIN_RIDGE switch of the drop-in
ice_transport_driver.F90, step_ridge_gpu of ice_ridge_gpu.F90) compiles against the drop-in build's module files, with a
caller written like the part of step_dynamics behind evp (source/ice_step_mod.F90:581-745)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from cice4_amd import lib
from test_ridge_fortran import FC, FDIR, FLAGS, SHIM, _ref_modules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cice_ridge_chain", "cice_transport_download_state")
CALLER = """
      subroutine dynamics_behind_evp (dt)
      use ice_kinds_mod
      use ice_transport_driver, only: transport_remap
      use ice_ridge_gpu, only: step_ridge_gpu
      use ice_exit, only: abort_ice
      real (kind=dbl_kind) :: dt
      integer (kind=int_kind) :: istop, jstop, bstop, stage
      logical (kind=log_kind) :: l_stop
      call transport_remap (dt)
      call step_ridge_gpu (dt, l_stop, istop, jstop, bstop, stage)
      if (l_stop .and. stage == 1) call abort_ice ('ice: Ridging error')
      if (l_stop) call abort_ice ('ice: ITD cleanup error')
      end subroutine dynamics_behind_evp
"""


@pytest.mark.parametrize("flavour", ["standalone", "auscom"])
def test_both_libraries_export_the_entries(flavour):
    l = lib.load(flavour)
    for n in ENTRIES:
        assert hasattr(l, n), n


def test_header_declares_the_entries():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cice4_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+cice_ridge_chain\s*\(\s*cice_ctx\s*\*\s*ctx\s*,\s*int\s+mode\s*\)\s*;", src)
    assert re.search(r"\bint\s+cice_transport_download_state\s*\(\s*cice_ctx\s*\*\s*ctx\s*\)\s*;", src)


def test_mode_outside_0_to_2_is_einval():
    c = lib.Context()
    for mode in (0, 1, 2, 0):
        c.ridge_chain(mode)
    for bad in (-1, 3, 7):
        with pytest.raises(lib.CiceError, match="error -1: cice_ridge_chain"):
            c.ridge_chain(bad)
    assert c.lib.cice_ridge_chain(None, 1) == -1 and c.lib.cice_transport_download_state(None) == -1


def test_without_a_gpu_nothing_is_pending_and_device_entries_fail_loudly():
    """neither entry needs a device by itself: the mode is a flag, and nothing can be pending before a transport call --
    which needs the device and says so (CICE_EDEVICE), in every mode"""
    import numpy as np
    import torch
    c = lib.Context()
    c.transport_download_state()
    c.ridge_chain(2)
    c.transport_download_state()
    if torch.cuda.is_available():
        return
    c.domain_create(16, 12, 8, 6)
    g = {k: np.ones((c.nblocks, c.ny, c.nx)) for k in ("HTN", "HTE", "dxt", "dyt", "dxu", "dyu", "tarear", "hm")}
    with pytest.raises(lib.CiceError, match="error -2"):
        c.transport_init(g, ntrcr=1, trcr_depend=(0,))
    c.transport_download_state()
    c.ridge_chain(0)


@pytest.mark.skipif(not os.path.exists(FC), reason="no Fortran compiler")
def test_shim_carries_the_interface_blocks():
    shim = open(SHIM).read()
    for n in ENTRIES:
        assert re.search(r"function %s\(.*bind\(C, name='%s'\)" % (n, n), shim), n
    tmp = tempfile.mkdtemp(prefix="ridge_chain_f90_")
    try:
        subprocess.check_call([FC, "-cpp", "-fPIC", "-w", "-J", tmp, "-c", SHIM, "-o", os.path.join(tmp, "shim.o")])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_fortran_sources_name_the_switch_and_the_one_call_form():
    drv = open(os.path.join(FDIR, "ice_transport_driver.F90")).read()
    assert "CICE4_AMD_CHAIN_RIDGE" in drv and "cice_ridge_chain(cice_gpu_ctx" in drv
    mod = open(os.path.join(FDIR, "ice_ridge_gpu.F90")).read()
    assert re.search(r"public :: .*\bstep_ridge_gpu\b", mod)
    assert re.search(r"subroutine step_ridge_gpu \(dt, l_stop, istop, jstop, bstop, stage\)", mod)
    assert "cice_step_ridge(cice_gpu_ctx" in mod


@pytest.mark.skipif(not os.path.exists(FC) or _ref_modules() is None, reason="no Fortran compiler or no compiled reference")
def test_fortran_side_compiles_against_the_reference_and_a_chained_caller_against_it():
    tmp = tempfile.mkdtemp(prefix="ridge_chain_f90_")
    try:
        ref = _ref_modules()
        inc = ["-J", tmp, "-I", tmp, "-I", ref]
        subprocess.check_call([FC, *FLAGS, *inc, "-c", SHIM, "-o", os.path.join(tmp, "shim.o")])
        for name in ("ice_ridge_gpu", "ice_transport_driver"):
            subprocess.check_call([FC, *FLAGS, *inc, "-c", os.path.join(FDIR, name + ".F90"), "-o", os.path.join(tmp, name + ".o")])
        src = os.path.join(tmp, "caller.F90")
        with open(src, "w") as f:
            f.write(CALLER)
        subprocess.check_call([FC, *FLAGS, *inc, "-c", src, "-o", os.path.join(tmp, "c.o")])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
