"""cice4_amd/fortran/cice4_amd_c.F90 carries interface blocks for cice_cleanup_itd, cice_aggregate and
cice_step_therm2_cleanup: the module compiles, a caller written against the argument lists of include/cice4_amd.h
compiles against it, and the derived type has the members of the C struct in its order."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FC = os.environ.get("FC", "/opt/rocm/bin/amdflang")
SHIM = os.path.join(ROOT, "cice4_amd", "fortran", "cice4_amd_c.F90")
CALLER = """
      subroutine second_half (ctx, nx, ny, nb, dt, aicen, trcrn, vicen, vsnon, eicen, esnon, tmask, a2, trcr, fl, dep)
      use iso_c_binding
      use cice4_amd_c
      type(c_ptr) :: ctx
      integer(c_int) :: nx, ny, nb, rc, l_stop, istop, jstop, bstop, stage
      real(c_double) :: dt
      real(c_double), target :: aicen(nx,ny,5,nb), trcrn(nx,ny,5,5,nb), vicen(nx,ny,5,nb), vsnon(nx,ny,5,nb), &
         eicen(nx,ny,20,nb), esnon(nx,ny,5,nb), a2(nx,ny,nb,6), trcr(nx,ny,5,nb), fl(nx,ny,nb,5)
      integer(c_int), target :: tmask(nx,ny,nb), dep(5)
      type(cice_therm2_cleanup_fields) :: f
      rc = cice_cleanup_itd(ctx, nx, ny, 2, nx-1, 2, ny-1, dt, 1, aicen, trcrn, vicen, vsnon, eicen, esnon, a2(:,:,1,2), &
                            a2(:,:,1,1), dep, c_loc(fl(1,1,1,1)), c_null_ptr, c_loc(fl(1,1,1,3)), 1, l_stop, istop, jstop, 1)
      rc = cice_aggregate(ctx, nx, ny, aicen, trcrn, vicen, vsnon, eicen, esnon, a2(:,:,1,1), trcr, a2(:,:,1,3), &
                          a2(:,:,1,4), a2(:,:,1,5), a2(:,:,1,6), a2(:,:,1,2), tmask, 1, dep)
      f%ncat = 5; f%state_resident = 1; f%bound = 1
      f%aicen = c_loc(aicen); f%trcrn = c_loc(trcrn); f%vicen = c_loc(vicen); f%vsnon = c_loc(vsnon)
      f%eicen = c_loc(eicen); f%esnon = c_loc(esnon); f%tmask = c_loc(tmask)
      f%aice = c_loc(a2(1,1,1,1)); f%aice0 = c_loc(a2(1,1,1,2)); f%vice = c_loc(a2(1,1,1,3)); f%vsno = c_loc(a2(1,1,1,4))
      f%eice = c_loc(a2(1,1,1,5)); f%esno = c_loc(a2(1,1,1,6)); f%trcr = c_loc(trcr)
      f%fresh = c_loc(fl(1,1,1,1)); f%fsalt = c_loc(fl(1,1,1,2)); f%fhocn = c_loc(fl(1,1,1,3))
      f%daidtt = c_loc(fl(1,1,1,4)); f%dvidtt = c_loc(fl(1,1,1,5))
      rc = cice_step_therm2_cleanup(ctx, dt, f, l_stop, istop, jstop, bstop, stage)
      end subroutine second_half
"""


@pytest.mark.skipif(not os.path.exists(FC), reason="no Fortran compiler")
def test_interfaces_compile_and_a_caller_compiles_against_them():
    tmp = tempfile.mkdtemp(prefix="cleanup_f90_")
    try:
        subprocess.check_call([FC, "-cpp", "-fPIC", "-w", "-J", tmp, "-c", SHIM, "-o", os.path.join(tmp, "shim.o")])
        src = os.path.join(tmp, "caller.f90")
        with open(src, "w") as f:
            f.write(CALLER)
        subprocess.check_call([FC, "-ffree-form", "-fPIC", "-w", "-I", tmp, "-J", tmp, "-c", src, "-o", os.path.join(tmp, "c.o")])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_derived_type_mirrors_the_c_struct():
    head = open(os.path.join(ROOT, "include", "cice4_amd.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} cice_therm2_cleanup_fields;", head)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    c_members = re.findall(r"\*?(\w+)\s*[,;]", body)
    shim = open(SHIM).read()
    t = re.search(r"type, bind\(C\) :: cice_therm2_cleanup_fields(.*?)end type", shim, re.S).group(1)
    f_members = [w.strip() for line in t.strip().splitlines() for w in line.split("::")[1].split(",")]
    assert c_members == f_members and len(f_members) == 22
