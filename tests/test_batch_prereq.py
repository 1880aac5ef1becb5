"""What the entries of the column batch (cice_thermo_batch_*, cice_step_therm1, cice_step_therm2_itd) and their neighbours
answer on a fresh context, before any allocation: return codes, messages and the order of the checks.  Host code only -- the
device is not asked for before the arguments have been looked at."""
import re

import numpy as np
import pytest

from cice4_amd import lib

NO_BATCH = "cice_thermo_batch_alloc has not been called"


@pytest.fixture()
def fresh():
    c = lib.Context()
    yield c
    c.close()


def _refused(call, code, text):
    with pytest.raises(lib.CiceError) as e:
        call()
    m = re.match(r"cice4_amd error (-?\d+): (.*)", str(e.value), re.S)
    assert m and int(m.group(1)) == code and text in m.group(2), str(e.value)


def _merge_args():
    z = np.zeros((1, lib.NCAT, 3, 3))
    percat = {k: z.copy() for k in ("aicen_init", "strairxn", "strairyn", "Trefn", "Qrefn")}
    acc = {k: np.zeros((1, 3, 3)) for k in lib.MERGE_ORDER}
    return percat, acc


def test_batch_entries_before_alloc(fresh):
    c = fresh
    percat, acc = _merge_args()
    _refused(lambda: c.thermo_batch_upload({}), -1, NO_BATCH)
    _refused(lambda: c.thermo_batch_step(3600.0), -1, NO_BATCH)
    _refused(lambda: c.thermo_batch_download({}), -1, NO_BATCH)
    _refused(lambda: c.thermo_batch_merge(percat, acc), -1, NO_BATCH)
    _refused(lambda: c.step_therm1(3600.0, 1.0, {}, {}, percat, acc), -1, NO_BATCH)
    _refused(lambda: c.step_therm1(3600.0, 1.0, {}, {}, percat, acc, atm={}), -1, NO_BATCH)
    _refused(lambda: c.step_therm2_itd(3600.0, 1.0, {}), -1, NO_BATCH)
    _refused(lambda: c.step_therm2_itd(3600.0, 1.0, {}, state_resident=True), -1, NO_BATCH)
    _refused(c.evp_adopt_thermo_state, -1, "cice_evp_init has not been called")


def test_settings_and_debug_reads_work_before_alloc(fresh):
    c = fresh
    assert len(c.therm2_itd_times(True)) == 4
    # the six stage clocks: no device, no batch, nothing timed yet -- zeros, with the flag set and with it cleared again
    for read, n in ((c.therm2_itd_times, 4), (c.therm2_cleanup_times, 12), (c.ridge_times, 41), (c.radiation_times, 2),
                    (c.dedd_times, 1), (c.ridge_chain_time, 1)):
        for enable in (True, False):
            t = read(enable)
            t = list(t.values()) if isinstance(t, dict) else list(t) if isinstance(t, tuple) else [t]
            assert t == [0.0] * n, (read.__name__, enable, t)
    c.thermo_set_option("sort_chunk", 256)
    c.thermo_set_option("sort_group", 8)
    _refused(lambda: c.thermo_set_option("sort_chunk", 100), -1, "sort_chunk must be 0 or 256 .. 2048 in steps of 256")
    assert c.evp_debug("thermo_niter").size == 0
    assert c.evp_debug("thermo_perm").size == 0


def test_alloc_checks_its_arguments_before_asking_for_the_device(fresh):
    c = fresh
    _refused(lambda: c.thermo_batch_alloc(2, 4, 1), -1, "bad dimensions")
    if c.lib.cice_device_count() == 0:
        _refused(lambda: c.thermo_batch_alloc(4, 4, 1), -2, "")
        _refused(lambda: c.thermo_batch_upload({}), -1, NO_BATCH)      # a failed allocation leaves no batch
    else:
        c.thermo_batch_alloc(4, 4, 1)


def test_blockwise_thermo_asks_for_its_own_init(fresh):
    z = np.zeros((3, 3))
    a = {k: z for k in lib.THERMO_ARGS}
    ii = np.zeros(9, np.int32)
    _refused(lambda: fresh.thermo_vertical(3600.0, 0, ii, ii, a), -1, "cice_thermo_init has not been called")
