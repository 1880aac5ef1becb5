"""cice4_amd/fortran/cice4_amd_c.F90 carries interface blocks and bind(C) types for the shortwave entries, and
cice4_amd/fortran/ice_radiation_gpu.F90 offers shortwave_ccsm3 with the reference's interface plus step_radiation_gpu and
prep_radiation_gpu on top of them: the shim compiles, the derived types have the members of the C structs in their order,
and -- where the compiled reference's module files are there (oracle/_ref, made by build()) -- the module compiles against
them and a caller written like step_radiation (source/ice_step_mod.F90:920-940) compiles against the module.
ice_shortwave is not in the closure of oracle/build_ref.sh: where its module file is absent, the test first compiles it and
the four modules it uses from the reference's tree into its temporary directory, as tests/golden/make_golden_shortwave.py
does."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FC = os.environ.get("FC", "/opt/rocm/bin/amdflang")
REF = os.environ.get("CICE_REFERENCE_ROOT", "/root/reference")
FDIR = os.path.join(ROOT, "cice4_amd", "fortran")
SHIM = os.path.join(FDIR, "cice4_amd_c.F90")
MODULE = os.path.join(FDIR, "ice_radiation_gpu.F90")
FLAGS = ("-O2 -fPIC -w -cpp -fdefault-real-8 -fconvert=big-endian -ffp-contract=off -DLINUX "
         "-DNXGLOB=24 -DNYGLOB=20 -DBLCKX=12 -DBLCKY=10 -DMXBLCKS=4").split()
FIVE = ("csm_share/shr_orb_mod.F90", "source/ice_diagnostics.F90", "source/ice_orbital.F90", "source/ice_meltpond.F90",
        "source/ice_shortwave.F90")
CALLER = """
      subroutine radiation_of_a_block (dt, iblk, n, icells, indxi, indxj)
      use ice_kinds_mod
      use ice_constants
      use ice_blocks, only: nx_block, ny_block
      use ice_state
      use ice_flux
      use ice_itd, only: ilyr1, ilyrn, slyr1, slyrn
      use ice_shortwave, only: alvdrn, alidrn, alvdfn, alidfn, fswsfcn, fswintn, fswthrun, Sswabsn, Iswabsn, albicen, &
                               albsnon
      use ice_radiation_gpu, only: shortwave_ccsm3, step_radiation_gpu, prep_radiation_gpu
      real (kind=dbl_kind) :: dt
      integer (kind=int_kind) :: iblk, n, icells, indxi(nx_block*ny_block), indxj(nx_block*ny_block), il1, il2, sl1, sl2
      il1 = ilyr1(n)
      il2 = ilyrn(n)
      sl1 = slyr1(n)
      sl2 = slyrn(n)
      Sswabsn(:,:,sl1:sl2,iblk) = c0
      call shortwave_ccsm3(nx_block,     ny_block,           &
                     icells,                                 &
                     indxi,             indxj,               &
                     aicen(:,:,n,iblk), vicen(:,:,n,iblk),   &
                     vsnon(:,:,n,iblk),                      &
                     trcrn(:,:,nt_Tsfc,n,iblk),              &
                     swvdr(:,:,  iblk), swvdf(:,:,  iblk),   &
                     swidr(:,:,  iblk), swidf(:,:,  iblk),   &
                     alvdrn(:,:,n,iblk),alidrn(:,:,n,iblk),  &
                     alvdfn(:,:,n,iblk),alidfn(:,:,n,iblk),  &
                     fswsfcn(:,:,n,iblk),fswintn(:,:,n,iblk),&
                     fswthrun(:,:,n,iblk),                   &
                     Iswabsn(:,:,il1:il2,iblk),              &
                     albicen(:,:,n,iblk),albsnon(:,:,n,iblk))
      call prep_radiation_gpu (dt)
      call step_radiation_gpu (dt)
      call step_radiation_gpu (dt, state_resident=.true.)
      end subroutine radiation_of_a_block
"""
STRUCTS = {"cice_shortwave_config": 15, "cice_radiation_fields": 23, "cice_prep_radiation_fields": 19}


def _ref_modules():
    p = os.path.join(ROOT, "oracle", "_ref", "obj_small")
    return p if os.path.exists(os.path.join(p, "ice_therm_vertical.mod")) else None


@pytest.mark.skipif(not os.path.exists(FC), reason="no Fortran compiler")
def test_shim_compiles():
    tmp = tempfile.mkdtemp(prefix="shortwave_f90_")
    try:
        subprocess.check_call([FC, "-cpp", "-fPIC", "-w", "-J", tmp, "-c", SHIM, "-o", os.path.join(tmp, "shim.o")])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


@pytest.mark.skipif(not os.path.exists(FC) or _ref_modules() is None, reason="no Fortran compiler or no compiled reference")
def test_module_compiles_against_the_reference_and_a_caller_against_it():
    tmp = tempfile.mkdtemp(prefix="shortwave_f90_")
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


def test_module_keeps_to_its_own_name_and_copies_nothing():
    text = open(MODULE).read()
    assert re.search(r"^\s*module ice_radiation_gpu\s*$", text, re.M) and "module ice_shortwave" not in text
    assert "public :: shortwave_ccsm3, step_radiation_gpu, prep_radiation_gpu" in text
    for entry in ("cice_shortwave_ccsm3(", "cice_step_radiation(", "cice_prep_radiation(", "cice_shortwave_init(",
                  "cice_radiation_chain("):
        assert entry in text, entry
    assert "CICE4_AMD_CHAIN_RADIATION" in text and "ocn_albedo2Da" in text
    for routine in ("compute_albedos", "constant_albedos", "absorbed_solar", "shortwave_dEdd", "init_shortwave"):
        assert "subroutine " + routine not in text, routine
    assert "atan" not in text and "exp (" not in text and "exp(" not in text      # no arithmetic of the scheme


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
