"""The delta-Eddington entries without a device: both builds of the library export them, and the argument checks fire before
any device call -- cice_shortwave_dedd_init wants cice_thermo_init first, cice_shortwave_dEdd refuses NULL arguments and
index lists that leave the block, cice_step_radiation_dedd wants the init, a batch and the library's ncat -- while
cice_shortwave_init(shortwave = 1) keeps answering CICE_EUNSUPPORTED and now names the new entry."""
import ctypes as C

import numpy as np
import pytest

import dedd_case as dc
import shortwave_case as sc
from cice4_amd import lib

ENTRIES = ("cice_shortwave_dedd_init", "cice_shortwave_dEdd", "cice_step_radiation_dedd", "cice_dedd_times")
NY, NX = 6, 8


@pytest.mark.parametrize("flavour", ["standalone", "auscom"])
def test_both_libraries_export_the_entries(flavour):
    l = lib.load(flavour)
    for n in ENTRIES:
        assert hasattr(l, n), n


def _arrays():
    a = {k: np.zeros((NY, NX)) for k in lib.Context.DEDD_IN + lib.Context.DEDD_OUT}
    for k in ("rhosnw", "rsnw", "Sswabs"):
        a[k] = np.zeros((dc.NSLYR, NY, NX))
    a["Iswabs"] = np.zeros((dc.NILYR, NY, NX))
    return a


def test_init_needs_thermo_init_and_null_is_einval():
    c = lib.Context()
    with pytest.raises(lib.CiceError, match="error -1: cice_shortwave_dedd_init: cice_thermo_init has not been called"):
        c.shortwave_dedd_init()
    c.thermo_init()
    assert c.lib.cice_shortwave_dedd_init(c.h, None) == -1
    assert c.lib.cice_shortwave_dedd_init(None, None) == -1
    with pytest.raises(lib.CiceError, match="error -1: cice_shortwave_dedd_init: tr_pond"):
        c.shortwave_dedd_init(tr_pond=2)
    with pytest.raises(lib.CiceError, match="error -1: cice_shortwave_dedd_init: R_ice"):
        c.shortwave_dedd_init(R_ice=float("nan"))
    c.shortwave_dedd_init(**dc.init_kwargs("tuned_neg"))
    c.shortwave_dedd_init()


def _raw(c, icells, ii, jj, a, null=None):
    """the entry through ctypes, one array argument NULL; returns the code and the message"""
    ptr = lambda k: None if k == null else lib._f8(a[k])  # noqa: E731
    rc = c.lib.cice_shortwave_dEdd(c.h, NX, NY, icells, lib._i4(ii), lib._i4(jj), *[ptr(k) for k in lib.Context.DEDD_IN],
                                   *[ptr(k) for k in lib.Context.DEDD_OUT])
    return rc, c.lib.cice_last_error(c.h).decode()


def test_blockwise_entry_checks_its_arguments_before_the_device():
    c = lib.Context()
    c.thermo_init()
    a = _arrays()
    ii, jj = np.array([1, NX], np.int32), np.array([1, NY], np.int32)
    with pytest.raises(lib.CiceError, match="error -1: cice_shortwave_dedd_init has not been called"):
        c.shortwave_dEdd(2, ii, jj, a)
    c.shortwave_dedd_init()
    for k in lib.Context.DEDD_IN + lib.Context.DEDD_OUT:
        assert _raw(c, 2, ii, jj, a, null=k) == (-1, "shortwave_dEdd: NULL argument"), k
    assert _raw(c, 2, None, jj, a) == (-1, "bad dimensions or NULL index list")
    assert _raw(c, 2, ii, None, a) == (-1, "bad dimensions or NULL index list")
    assert _raw(c, NX * NY + 1, ii, jj, a) == (-1, "bad dimensions or NULL index list")
    assert _raw(c, -1, ii, jj, a) == (-1, "bad dimensions or NULL index list")
    for bad_i, bad_j in ((0, 1), (NX + 1, 1), (1, 0), (1, NY + 1)):
        with pytest.raises(lib.CiceError, match="error -1: index list outside the block"):
            c.shortwave_dEdd(2, np.array([1, bad_i], np.int32), np.array([1, bad_j], np.int32), a)


def test_one_call_entry_checks_its_arguments_before_the_device():
    c = lib.Context()
    f = lib.RadiationDeddFields()
    f.ncat = lib.NCAT
    assert c.lib.cice_step_radiation_dedd(c.h, None) == -1 and c.lib.cice_step_radiation_dedd(None, C.byref(f)) == -1
    f.ncat = lib.NCAT + 1
    assert c.lib.cice_step_radiation_dedd(c.h, C.byref(f)) == -1
    assert b"ncat" in c.lib.cice_last_error(c.h)
    f.ncat = lib.NCAT
    assert c.lib.cice_step_radiation_dedd(c.h, C.byref(f)) == -1
    assert b"cice_thermo_batch_alloc has not been called" in c.lib.cice_last_error(c.h)
    assert c.dedd_times(False) == 0.0


def test_the_old_refusal_stays_and_names_the_new_entry():
    c = lib.Context()
    c.thermo_init()
    with pytest.raises(lib.CiceError, match="error -4: .*cice_shortwave_dedd_init"):
        c.shortwave_init(**dict(sc.init_kwargs("default"), shortwave="dEdd"))
    c.shortwave_dedd_init()                                        # the two schemes side by side
    c.shortwave_init(**sc.init_kwargs("default"))
    with pytest.raises(lib.CiceError, match="error -4"):
        c.shortwave_init(**dict(sc.init_kwargs("default"), shortwave="dEdd"))
