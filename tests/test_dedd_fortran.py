"""cice4_amd/fortran/cice4_amd_c.F90 carries interface blocks and bind(C) types for the delta-Eddington entries, and the new
module cice4_amd/fortran/ice_radiation_dedd_gpu.F90 offers shortwave_dEdd with the reference's interface plus
step_radiation_dedd_gpu on top of them: the shim compiles, the derived types have the members of the C structs in their
order, and -- where the compiled reference's module files are there (oracle/_ref, made by build()) -- the module compiles
against them and a caller written like the dEdd branch of step_radiation (source/ice_step_mod.F90:899-916) compiles against
the module.  ice_shortwave is not in the closure of oracle/build_ref.sh: the test compiles it and the four modules it uses
from the reference's tree into its temporary directory first, as test_shortwave_fortran.py does.  The module holds no
arithmetic of the scheme, and ice_radiation_gpu.F90 holds no shortwave_dEdd."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from test_shortwave_fortran import FC, FDIR, FIVE, FLAGS, REF, ROOT, SHIM, _ref_modules

MODULE = os.path.join(FDIR, "ice_radiation_dedd_gpu.F90")
CALLER = """
      subroutine dedd_of_a_block (dt, iblk, n, icells, indxi, indxj, fsn, rhosnwn, rsnwn, fpn, hpn)
      use ice_kinds_mod
      use ice_domain_size, only: nslyr
      use ice_blocks, only: nx_block, ny_block
      use ice_state
      use ice_flux
      use ice_itd, only: ilyr1, ilyrn, slyr1, slyrn
      use ice_shortwave, only: alvdrn, alidrn, alvdfn, alidfn, fswsfcn, fswintn, fswthrun, Sswabsn, Iswabsn, albicen, &
                               albsnon, albpndn
      use ice_radiation_dedd_gpu, only: shortwave_dEdd, step_radiation_dedd_gpu
      real (kind=dbl_kind) :: dt
      integer (kind=int_kind) :: iblk, n, icells, indxi(nx_block*ny_block), indxj(nx_block*ny_block), il1, il2, sl1, sl2
      real (kind=dbl_kind), dimension (nx_block,ny_block) :: fsn, fpn, hpn
      real (kind=dbl_kind), dimension (nx_block,ny_block,nslyr) :: rhosnwn, rsnwn
      il1 = ilyr1(n)
      il2 = ilyrn(n)
      sl1 = slyr1(n)
      sl2 = slyrn(n)
      call shortwave_dEdd(nx_block,     ny_block,            &
                     icells,                                 &
                     indxi,             indxj,               &
                     coszen(:,:, iblk),                      &
                     aicen(:,:,n,iblk), vicen(:,:,n,iblk),   &
                     vsnon(:,:,n,iblk), fsn,                 &
                     rhosnwn,           rsnwn,               &
                     fpn,               hpn,                 &
                     swvdr(:,:,  iblk), swvdf(:,:,  iblk),   &
                     swidr(:,:,  iblk), swidf(:,:,  iblk),   &
                     alvdrn(:,:,n,iblk),alvdfn(:,:,n,iblk),  &
                     alidrn(:,:,n,iblk),alidfn(:,:,n,iblk),  &
                     fswsfcn(:,:,n,iblk),fswintn(:,:,n,iblk),&
                     fswthrun(:,:,n,iblk),                   &
                     Sswabsn(:,:,sl1:sl2,iblk),              &
                     Iswabsn(:,:,il1:il2,iblk),              &
                     albicen(:,:,n,iblk),                    &
                     albsnon(:,:,n,iblk),albpndn(:,:,n,iblk))
      call step_radiation_dedd_gpu (dt)
      call step_radiation_dedd_gpu (dt, state_resident=.true.)
      end subroutine dedd_of_a_block
"""
STRUCTS = {"cice_dedd_config": 8, "cice_radiation_dedd_fields": 25}


@pytest.mark.skipif(not os.path.exists(FC), reason="no Fortran compiler")
def test_shim_compiles_and_carries_the_interface_blocks():
    shim = open(SHIM).read()
    for n in ("cice_shortwave_dedd_init", "cice_shortwave_dEdd", "cice_step_radiation_dedd"):
        assert re.search(r"function %s\(.*?bind\(C, name='%s'\)" % (n, n), shim, re.S), n
    tmp = tempfile.mkdtemp(prefix="dedd_f90_")
    try:
        subprocess.check_call([FC, "-cpp", "-fPIC", "-w", "-J", tmp, "-c", SHIM, "-o", os.path.join(tmp, "shim.o")])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


@pytest.mark.skipif(not os.path.exists(FC) or _ref_modules() is None, reason="no Fortran compiler or no compiled reference")
def test_module_compiles_against_the_reference_and_a_caller_against_it():
    tmp = tempfile.mkdtemp(prefix="dedd_f90_")
    try:
        ref = _ref_modules()
        inc = ["-J", tmp, "-I", tmp, "-I", ref]
        if not os.path.exists(os.path.join(ref, "ice_shortwave.mod")):
            if not os.path.isdir(os.path.join(REF, "source")):
                pytest.skip("ice_shortwave.mod is not built and the reference's tree is not here")
            for f in FIVE:
                subprocess.check_call([FC, *FLAGS, *inc, "-c", os.path.join(REF, f), "-o",
                                       os.path.join(tmp, os.path.basename(f)[:-4] + ".o")])
        subprocess.check_call([FC, *FLAGS, *inc, "-c", SHIM, "-o", os.path.join(tmp, "shim.o")])
        subprocess.check_call([FC, *FLAGS, *inc, "-c", MODULE, "-o", os.path.join(tmp, "m.o")])
        src = os.path.join(tmp, "caller.F90")
        with open(src, "w") as f:
            f.write(CALLER)
        subprocess.check_call([FC, *FLAGS, *inc, "-c", src, "-o", os.path.join(tmp, "c.o")])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_module_keeps_to_its_own_name_and_holds_no_arithmetic_of_the_scheme():
    text = open(MODULE).read()
    assert re.search(r"^\s*module ice_radiation_dedd_gpu\s*$", text, re.M) and "module ice_shortwave" not in text
    assert "public :: shortwave_dEdd, step_radiation_dedd_gpu" in text
    for entry in ("cice_shortwave_dEdd(", "cice_step_radiation_dedd(", "cice_shortwave_dedd_init(", "call compute_coszen"):
        assert entry in text, entry
    for routine in ("compute_dEdd", "solution_dEdd", "shortwave_dEdd_set_snow", "shortwave_dEdd_set_pond", "compute_coszen"):
        assert "subroutine " + routine not in text, routine
    assert "exp(" not in text and "sqrt(" not in text and "exp (" not in text and "sqrt (" not in text
    assert "subroutine shortwave_dEdd" not in open(os.path.join(FDIR, "ice_radiation_gpu.F90")).read()


@pytest.mark.parametrize("struct", tuple(STRUCTS))
def test_derived_types_mirror_the_c_structs(struct):
    head = open(os.path.join(ROOT, "include", "cice4_amd.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", head)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    c_members = re.findall(r"\*?(\w+)\s*[,;]", body)
    shim = open(SHIM).read()
    t = re.search(r"type, bind\(C\) :: " + struct + r"\b(.*?)end type", shim, re.S).group(1)
    f_members = [w.strip() for line in t.strip().splitlines() for w in line.split("::")[1].split(",")]
    assert c_members == f_members and len(f_members) == STRUCTS[struct]
