"""cice4_amd/fortran/cice4_amd_c.F90 carries interface blocks and the bind(C) type for the pond entries, and
cice4_amd/fortran/ice_pond_gpu.F90 offers step_ponds_gpu on top of them: the shim compiles, the derived type has the members
of the C struct in their order, and -- where the compiled reference's module files are there (oracle/_ref, made by build())
-- the module compiles against them and a caller written like the reference's driver compiles against the module.
ice_meltpond (tr_pond) and ice_shortwave (the namelist's `shortwave`) are not in the closure of oracle/build_ref.sh: where
their module files are absent, the test first compiles them and the three modules they use from the reference's tree into its
temporary directory, as tests/test_coupling_fortran.py does."""
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
MODULE = os.path.join(FDIR, "ice_pond_gpu.F90")
FLAGS = ("-O2 -fPIC -w -cpp -fdefault-real-8 -fconvert=big-endian -ffp-contract=off -DLINUX "
         "-DNXGLOB=24 -DNYGLOB=20 -DBLCKX=12 -DBLCKY=10 -DMXBLCKS=4").split()
FIVE = ("csm_share/shr_orb_mod.F90", "source/ice_diagnostics.F90", "source/ice_orbital.F90", "source/ice_meltpond.F90",
        "source/ice_shortwave.F90")
CALLER = """
      subroutine ponds_of_a_step (dt, melttn, meltsn)
      use ice_kinds_mod
      use ice_domain_size, only: ncat, max_blocks
      use ice_blocks, only: nx_block, ny_block
      use ice_pond_gpu, only: step_ponds_gpu
      real (kind=dbl_kind) :: dt
      real (kind=dbl_kind), dimension(nx_block,ny_block,ncat,max_blocks) :: melttn, meltsn
      call step_ponds_gpu (dt)
      call step_ponds_gpu (dt, state_resident=.true.)
      call step_ponds_gpu (dt, .false., melttn, meltsn)
      end subroutine ponds_of_a_step
"""


def _ref_modules():
    p = os.path.join(ROOT, "oracle", "_ref", "obj_small")
    return p if os.path.exists(os.path.join(p, "ice_age.mod")) else None


@pytest.mark.skipif(not os.path.exists(FC), reason="no Fortran compiler")
def test_shim_compiles():
    tmp = tempfile.mkdtemp(prefix="pond_f90_")
    try:
        subprocess.check_call([FC, "-cpp", "-fPIC", "-w", "-J", tmp, "-c", SHIM, "-o", os.path.join(tmp, "shim.o")])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


@pytest.mark.skipif(not os.path.exists(FC) or _ref_modules() is None, reason="no Fortran compiler or no compiled reference")
def test_module_compiles_against_the_reference_and_a_caller_against_it():
    tmp = tempfile.mkdtemp(prefix="pond_f90_")
    try:
        ref = _ref_modules()
        inc = ["-J", tmp, "-I", tmp, "-I", ref]
        if not (os.path.exists(os.path.join(ref, "ice_meltpond.mod")) and os.path.exists(os.path.join(ref, "ice_shortwave.mod"))):
            if not os.path.isdir(os.path.join(REF, "source")):
                pytest.skip("ice_meltpond.mod is not built and the reference's tree is not here")
            for f in FIVE:                   # ice_meltpond.F90 first of the two: it is not in oracle/_ref/obj_small
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
    assert re.search(r"^\s*module ice_pond_gpu\s*$", text, re.M)
    assert "public :: step_ponds_gpu" in text
    for entry in ("cice_step_ponds(", "cice_pond_init(", "cice_thermo_batch_alloc("):
        assert entry in text, entry
    for routine in ("compute_ponds", "increment_age", "init_meltponds"):
        assert "subroutine " + routine not in text, routine
    assert "dpthfrac" not in text and "rhofresh" not in text and "sqrt" not in text    # no arithmetic of the routines


def test_derived_type_mirrors_the_c_struct():
    head = open(os.path.join(ROOT, "include", "cice4_amd.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} cice_pond_fields;", head)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    c_members = re.findall(r"\*?(\w+)\s*[,;]", body)
    shim = open(SHIM).read()
    t = re.search(r"type, bind\(C\) :: cice_pond_fields\b(.*?)end type", shim, re.S).group(1)
    f_members = [w.strip() for line in t.strip().splitlines() for w in line.split("::")[1].split(",")]
    assert c_members == f_members and len(f_members) == 13
    for entry in ("cice_pond_init", "cice_compute_ponds", "cice_increment_age", "cice_step_ponds", "cice_pond_times",
                  "cice_pond_chain"):
        assert f"bind(C, name='{entry}')" in shim, entry
