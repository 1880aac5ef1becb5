"""The coupling entries without a device: both builds of the library export them, the ctypes struct has the members of the C
struct in their order, and the argument checks that need no device fire with texts that name the entry --
cice_coupling_init wants cice_thermo_init first and answers atmbndy = 'constant' with CICE_EUNSUPPORTED, cice_coupling_prep
wants the library's ncat, the init and a batch."""
import ctypes as C
import re
import os

import pytest

from cice4_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cice_coupling_init", "cice_coupling_prep", "cice_coupling_times")


@pytest.mark.parametrize("flavour", ["standalone", "auscom"])
def test_both_libraries_export_the_entries(flavour):
    l = lib.load(flavour)
    for n in ENTRIES:
        assert hasattr(l, n), n


def _c_members(struct):
    head = open(os.path.join(ROOT, "include", "cice4_amd.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", head)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return re.findall(r"\*?(\w+)\s*[,;]", body)


def test_struct_layout():
    assert _c_members("cice_coupling_fields") == [n for n, _t in lib.CouplingFields._fields_]
    assert _c_members("cice_coupling_config") == [n for n, _t in lib.CouplingConfig._fields_]
    assert len(lib.CouplingFields._fields_) == 5 + 1 + len(lib.COUPLING_PTRS) == 80
    assert C.sizeof(lib.CouplingFields) == 24 + 8 * 75 and C.sizeof(lib.CouplingConfig) == 24
    assert lib.CouplingFields.tmask.offset == 24 and lib.CouplingConfig.albocn.offset == 16


@pytest.mark.parametrize("flavour", ["standalone", "auscom"])
def test_init_needs_thermo_init_and_refuses_atmbndy_constant(flavour):
    c = lib.Context(flavour=flavour)
    with pytest.raises(lib.CiceError, match="error -1: cice_coupling_init: cice_thermo_init has not been called"):
        c.coupling_init()
    c.thermo_init()
    assert c.lib.cice_coupling_init(c.h, None) == -1 and b"cice_coupling_init" in c.lib.cice_last_error(c.h)
    assert c.lib.cice_coupling_init(None, None) == -1
    with pytest.raises(lib.CiceError, match=r"error -4: cice_coupling_init: atmbndy = 'constant'.*delt and delq"):
        c.coupling_init(atmbndy="constant")
    for bad in (dict(scale_fluxes=2), dict(oceanmixed_ice=-1)):
        with pytest.raises(lib.CiceError, match="error -1: cice_coupling_init: "):
            c.coupling_init(**bad)
    cfg = lib.CouplingConfig(1, 1, 2, 0.06)
    assert c.lib.cice_coupling_init(c.h, C.byref(cfg)) == -1 and b"atmbndy" in c.lib.cice_last_error(c.h)
    c.coupling_init()
    c.coupling_init(scale_fluxes=False, oceanmixed_ice=False)


def test_prep_checks_its_arguments_before_the_device():
    c = lib.Context()
    f = lib.CouplingFields()
    f.ncat = lib.NCAT
    assert c.lib.cice_coupling_prep(c.h, C.c_double(3600.0), None) == -1
    assert b"cice_coupling_prep" in c.lib.cice_last_error(c.h)
    assert c.lib.cice_coupling_prep(None, C.c_double(3600.0), C.byref(f)) == -1
    f.ncat = lib.NCAT + 1
    assert c.lib.cice_coupling_prep(c.h, C.c_double(3600.0), C.byref(f)) == -1
    assert c.lib.cice_last_error(c.h) == b"cice_coupling_prep: ncat is not the library's"
    f.ncat = lib.NCAT
    assert c.lib.cice_coupling_prep(c.h, C.c_double(3600.0), C.byref(f)) == -1
    assert c.lib.cice_last_error(c.h) == b"cice_coupling_prep: cice_coupling_init has not been called"
    c.thermo_init()
    c.coupling_init()
    assert c.lib.cice_coupling_prep(c.h, C.c_double(3600.0), C.byref(f)) == -1
    assert c.lib.cice_last_error(c.h) == b"cice_coupling_prep: cice_thermo_batch_alloc has not been called"
    assert c.coupling_times(False) == (0.0, 0.0)
