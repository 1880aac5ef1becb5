"""The pond entries without a device: both builds of the library export them, the ctypes struct has the members of the C
struct in their order, and the argument checks that need no device fire with texts that name the entry -- cice_pond_init
wants cice_thermo_init first and a slot in range that is neither nt_Tsfc nor nt_iage; cice_step_ponds wants the library's
ncat, the init, flags that the tracers allow, every array its flags require and a batch; cice_pond_chain wants 0 or 1."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cice4_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cice_pond_init", "cice_compute_ponds", "cice_increment_age", "cice_step_ponds", "cice_pond_times",
           "cice_pond_chain")
DT = C.c_double(3600.0)


@pytest.mark.parametrize("flavour", ["standalone", "auscom"])
def test_both_libraries_export_the_entries(flavour):
    l = lib.load(flavour)
    for n in ENTRIES:
        assert hasattr(l, n), n


def test_struct_layout():
    head = open(os.path.join(ROOT, "include", "cice4_amd.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} cice_pond_fields;", head)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"\*?(\w+)\s*[,;]", body) == [n for n, _t in lib.PondFields._fields_]
    assert len(lib.PondFields._fields_) == 4 + len(lib.POND_PTRS) == 13
    assert C.sizeof(lib.PondFields) == 16 + 8 * 9 and lib.PondFields.frain.offset == 16 and lib.PondFields.meltsn.offset == 80


@pytest.mark.parametrize("flavour", ["standalone", "auscom"])
def test_init_refusals(flavour):
    c = lib.Context(flavour=flavour)
    with pytest.raises(lib.CiceError, match="error -1: cice_pond_init: cice_thermo_init has not been called"):
        c.pond_init(3)
    assert c.lib.cice_pond_init(None, 3) == -1
    c.thermo_init(tr_iage=True, nt_Tsfc=1, nt_iage=2)
    for bad in (-1, lib.MAX_NTRCR + 1):
        with pytest.raises(lib.CiceError, match="error -1: cice_pond_init: nt_volpn out of range"):
            c.pond_init(bad)
    with pytest.raises(lib.CiceError, match="error -1: cice_pond_init: nt_volpn is nt_Tsfc"):
        c.pond_init(1)
    with pytest.raises(lib.CiceError, match="error -1: cice_pond_init: nt_volpn is nt_iage"):
        c.pond_init(2)
    for ok in (0, 3, lib.MAX_NTRCR):
        c.pond_init(ok)
    c.thermo_init(tr_iage=False, nt_Tsfc=1, nt_iage=2)    # without tr_iage the age slot is free
    c.pond_init(2)


def _fields(arrays, **flags):
    f = lib.PondFields()
    f.ncat, f.state_resident, f.ponds, f.age = lib.NCAT, 0, 1, 1
    for k, v in flags.items():
        setattr(f, k, v)
    for n in lib.POND_PTRS:
        setattr(f, n, arrays[n].ctypes.data_as(C.c_void_p) if n in arrays else None)
    return f


def test_step_checks_its_arguments_before_the_device():
    c = lib.Context()
    call = lambda f: c.lib.cice_step_ponds(c.h, DT, C.byref(f) if f is not None else None)  # noqa: E731
    err = lambda: c.lib.cice_last_error(c.h)  # noqa: E731
    arrays = {n: np.zeros(8) for n in lib.POND_PTRS}
    assert call(None) == -1 and err() == b"cice_step_ponds: NULL argument"
    assert c.lib.cice_step_ponds(None, DT, C.byref(_fields(arrays))) == -1
    assert call(_fields(arrays, ncat=lib.NCAT + 1)) == -1 and err() == b"cice_step_ponds: ncat is not the library's"
    assert call(_fields(arrays)) == -1 and err() == b"cice_step_ponds: cice_pond_init has not been called"
    c.thermo_init(tr_iage=True, nt_Tsfc=1, nt_iage=2)
    assert call(_fields(arrays)) == -1 and err() == b"cice_step_ponds: cice_pond_init has not been called"
    c.pond_init(0)
    assert call(_fields(arrays)) == -1 and err().startswith(b"cice_step_ponds: ponds = 1, but cice_pond_init was given no pond")
    c.pond_init(3)
    for bad in (dict(state_resident=2), dict(ponds=2), dict(age=-1), dict(ponds=0, age=0)):
        assert call(_fields(arrays, **bad)) == -1 and err().startswith(b"cice_step_ponds: "), bad
    # each array the flags require
    for n in lib.POND_PTRS:
        assert call(_fields({k: v for k, v in arrays.items() if k != n})) == -1 and err() == b"cice_step_ponds: NULL field", n
    for n in ("trcrn", "aicen"):                     # age alone: the tracers and the list
        f = _fields({k: v for k, v in arrays.items() if k != n}, ponds=0)
        assert call(f) == -1 and err() == b"cice_step_ponds: NULL field", n
    for n in ("frain", "trcrn", "apondn", "hpondn"):  # a resident state: the four that still travel
        f = _fields({k: v for k, v in arrays.items() if k != n}, state_resident=1)
        assert call(f) == -1 and err() == b"cice_step_ponds: NULL field", n
    # all there: the batch is missing (age alone needs fewer arrays, a resident state none of the state's)
    for f in (_fields(arrays), _fields({"trcrn": arrays["trcrn"], "aicen": arrays["aicen"]}, ponds=0),
              _fields({n: arrays[n] for n in ("frain", "trcrn", "apondn", "hpondn")}, state_resident=1)):
        assert call(f) == -1 and err() == b"cice_step_ponds: cice_thermo_batch_alloc has not been called"
    c.thermo_init(tr_iage=False, nt_Tsfc=1, nt_iage=2)
    assert call(_fields(arrays)) == -1 and err().startswith(b"cice_step_ponds: age = 1, but cice_thermo_init was given tr_iage")
    c.thermo_init(tr_iage=True, nt_Tsfc=3, nt_iage=2)   # a later cice_thermo_init that takes the pond slot
    assert call(_fields(arrays)) == -1 and err() == b"cice_step_ponds: nt_volpn is nt_Tsfc"
    assert c.pond_times(False) == 0.0


def test_blockwise_entries_check_their_arguments_before_the_device():
    c = lib.Context()
    a = {k: np.zeros((4, 6)) for k in ("meltt", "melts", "frain", "aicen", "vicen", "vsnon", "apondn", "hpondn")}
    a["trcrn"] = np.zeros((lib.MAX_NTRCR, 4, 6))
    with pytest.raises(lib.CiceError, match="error -1: cice_compute_ponds: cice_pond_init has not been called"):
        c.compute_ponds(2, 5, 2, 3, 3600.0, a)
    c.thermo_init()
    c.pond_init(0)
    with pytest.raises(lib.CiceError, match="error -1: cice_compute_ponds: cice_pond_init was given no pond tracer"):
        c.compute_ponds(2, 5, 2, 3, 3600.0, a)
    c.pond_init(3)
    for box in ((0, 5, 2, 3), (2, 7, 2, 3), (2, 5, 0, 3), (2, 5, 2, 5)):
        with pytest.raises(lib.CiceError, match="error -1: cice_compute_ponds: bad dimensions"):
            c.compute_ponds(*box, 3600.0, a)
    assert c.lib.cice_compute_ponds(c.h, 6, 4, 2, 5, 2, 3, DT, *([None] * 9)) == -1
    assert c.lib.cice_last_error(c.h) == b"cice_compute_ponds: NULL argument"
    ii, jj = np.array([7, 1], np.int32), np.array([1, 1], np.int32)
    with pytest.raises(lib.CiceError, match="error -1: index list outside the block"):
        c.increment_age(3600.0, 2, ii, jj, np.zeros((4, 6)))
    assert c.lib.cice_increment_age(c.h, 6, 4, DT, 0, None, None, None) == -1
    assert c.lib.cice_last_error(c.h) == b"cice_increment_age: NULL argument"


def test_chain_refuses_other_modes():
    c = lib.Context()
    for bad in (-1, 2, 7):
        with pytest.raises(lib.CiceError, match="error -1: cice_pond_chain: mode must be 0 or 1"):
            c.pond_chain(bad)
    c.pond_chain(1)
    c.pond_chain(0)
