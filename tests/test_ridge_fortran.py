"""cice4_amd/fortran/cice4_amd_c.F90 carries interface blocks for cice_ridge_init, cice_ridge_ice and cice_step_ridge, and
cice4_amd/fortran/ice_ridge_gpu.F90 offers ridge_ice with the reference's interface on top of them: the shim compiles, the
derived type has the members of the C struct in its order, and -- where the compiled reference's module files are there
(oracle/_ref, made by build()) -- the module compiles against them and a caller written like step_dynamics
(source/ice_step_mod.F90:641-659) compiles against the module."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FC = os.environ.get("FC", "/opt/rocm/bin/amdflang")
FDIR = os.path.join(ROOT, "cice4_amd", "fortran")
SHIM = os.path.join(FDIR, "cice4_amd_c.F90")
FLAGS = ("-O2 -fPIC -w -cpp -fdefault-real-8 -fconvert=big-endian -ffp-contract=off -DLINUX "
         "-DNXGLOB=24 -DNYGLOB=20 -DBLCKX=12 -DBLCKY=10 -DMXBLCKS=4").split()
CALLER = """
      subroutine column_half (dt, iblk, icells, indxi, indxj)
      use ice_kinds_mod
      use ice_blocks, only: nx_block, ny_block
      use ice_state
      use ice_flux
      use ice_ridge_gpu, only: ridge_ice
      real (kind=dbl_kind) :: dt
      integer (kind=int_kind) :: iblk, icells, indxi(nx_block*ny_block), indxj(nx_block*ny_block), istop, jstop
      logical (kind=log_kind) :: l_stop
      call ridge_ice (nx_block, ny_block, dt, ntrcr, icells, indxi, indxj, rdg_conv(:,:,iblk), rdg_shear(:,:,iblk), &
                      aicen(:,:,:,iblk), trcrn(:,:,1:ntrcr,:,iblk), vicen(:,:,:,iblk), vsnon(:,:,:,iblk), &
                      eicen(:,:,:,iblk), esnon(:,:,:,iblk), aice0(:,:,iblk), trcr_depend(1:ntrcr), l_stop, istop, jstop, &
                      dardg1dt(:,:,iblk), dardg2dt(:,:,iblk), dvirdgdt(:,:,iblk), opening(:,:,iblk), fresh(:,:,iblk), &
                      fhocn(:,:,iblk))
      call ridge_ice (nx_block, ny_block, dt, ntrcr, icells, indxi, indxj, rdg_conv(:,:,iblk), rdg_shear(:,:,iblk), &
                      aicen(:,:,:,iblk), trcrn(:,:,1:ntrcr,:,iblk), vicen(:,:,:,iblk), vsnon(:,:,:,iblk), &
                      eicen(:,:,:,iblk), esnon(:,:,:,iblk), aice0(:,:,iblk), trcr_depend(1:ntrcr), l_stop, istop, jstop)
      end subroutine column_half
"""


def _ref_modules():
    for name in ("obj_small_dropin", "obj_small"):
        p = os.path.join(ROOT, "oracle", "_ref", name)
        if os.path.exists(os.path.join(p, "ice_mechred.mod")):
            return p
    return None


@pytest.mark.skipif(not os.path.exists(FC), reason="no Fortran compiler")
def test_shim_compiles():
    tmp = tempfile.mkdtemp(prefix="ridge_f90_")
    try:
        subprocess.check_call([FC, "-cpp", "-fPIC", "-w", "-J", tmp, "-c", SHIM, "-o", os.path.join(tmp, "shim.o")])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


@pytest.mark.skipif(not os.path.exists(FC) or _ref_modules() is None, reason="no Fortran compiler or no compiled reference")
def test_module_compiles_against_the_reference_and_a_caller_against_it():
    tmp = tempfile.mkdtemp(prefix="ridge_f90_")
    try:
        ref = _ref_modules()
        inc = ["-J", tmp, "-I", tmp, "-I", ref]
        subprocess.check_call([FC, *FLAGS, *inc, "-c", SHIM, "-o", os.path.join(tmp, "shim.o")])
        subprocess.check_call([FC, *FLAGS, *inc, "-c", os.path.join(FDIR, "ice_ridge_gpu.F90"), "-o", os.path.join(tmp, "m.o")])
        src = os.path.join(tmp, "caller.F90")
        with open(src, "w") as f:
            f.write(CALLER)
        subprocess.check_call([FC, *FLAGS, *inc, "-c", src, "-o", os.path.join(tmp, "c.o")])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_module_keeps_to_its_own_name_and_copies_nothing():
    text = open(os.path.join(FDIR, "ice_ridge_gpu.F90")).read()
    assert re.search(r"^\s*module ice_ridge_gpu\s*$", text, re.M) and "module ice_mechred" not in text
    assert "public :: ridge_ice" in text and "cice_ridge_ice(" in text
    assert "subroutine ice_strength" not in text and "subroutine ridge_shift" not in text


def test_derived_type_mirrors_the_c_struct():
    head = open(os.path.join(ROOT, "include", "cice4_amd.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} cice_ridge_fields;", head)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    c_members = re.findall(r"\*?(\w+)\s*[,;]", body)
    shim = open(SHIM).read()
    t = re.search(r"type, bind\(C\) :: cice_ridge_fields(.*?)end type", shim, re.S).group(1)
    f_members = [w.strip() for line in t.strip().splitlines() for w in line.split("::")[1].split(",")]
    assert c_members == f_members and len(f_members) == 27
