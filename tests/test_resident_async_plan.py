"""Host only, no device: the bookkeeping of Evp::retire_resident on synthetic sequences of pending records
(cice_debug_resident_plan).  The GPU test of the late fall-back (tests/test_gpu_resident_async.py) provokes its time-out with
resident_spin_us = 0, under which every launch gives up by itself: it cannot tell a launch that left at once under another's
abort word from one that gave up on its own.  Here the records say what they like -- in particular a CLEAN word behind an
aborted one, which has to be run again all the same: that launch began from the state the aborted loop never produced."""
import ctypes as C

import numpy as np

from cice4_amd import lib


def _plan(word0, cur, flips, ident, now):
    L = lib.load()
    n = len(word0)
    w = np.asarray(word0, dtype=np.uint32); c = np.asarray(cur, dtype=np.int32)
    f = np.asarray(flips, dtype=np.int32); i = np.asarray(ident, dtype=np.int32)
    out = (C.c_int32 * 5)()
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    assert L.cice_debug_resident_plan(n, p(w, C.c_uint32), p(c, C.c_int32), p(f, C.c_int32), p(i, C.c_int32), *now, out) == 0
    return list(out)


def _log(n, cur0=0, flips0=5, ident0=1):
    """what n queued launches log: every launch flips the copies, and after the first they are no longer identical"""
    cur = [(cur0 + k) & 1 for k in range(n)]
    flips = [flips0 + k for k in range(n)]
    ident = [ident0 if k == 0 else 0 for k in range(n)]
    return cur, flips, ident, ((cur0 + n) & 1, flips0 + n, 0 if n else ident0)


def test_all_clean_keeps_the_state_and_counts_every_cover():
    cur, flips, ident, now = _log(4)
    assert _plan([0, 0, 0, 0], cur, flips, ident, now) == [4, 0, now[0], now[1], now[2]]
    assert _plan([], [], [], [], (1, 7, 0)) == [0, 0, 1, 7, 0]


def test_clean_aborted_clean():
    """the third record reads clean, yet its launch began from the copy the second never wrote: both run again, and the
    state goes back to what the SECOND launch found (cur flipped once, one more flip, copies no longer identical)"""
    cur, flips, ident, now = _log(3)
    assert _plan([0, 1, 0], cur, flips, ident, now) == [1, 2, 1, 6, 0]


def test_first_aborted_restores_the_very_first_state():
    cur, flips, ident, now = _log(16, cur0=1, flips0=0, ident0=1)
    assert _plan([1] * 16, cur, flips, ident, now) == [0, 16, 1, 0, 1]
    assert _plan([1] + [0] * 15, cur, flips, ident, now) == [0, 16, 1, 0, 1]


def test_last_aborted():
    cur, flips, ident, now = _log(5)
    assert _plan([0, 0, 0, 0, 3], cur, flips, ident, now) == [4, 1, cur[4], flips[4], 0]


def test_bad_arguments():
    L = lib.load()
    out = (C.c_int32 * 5)()
    assert L.cice_debug_resident_plan(-1, None, None, None, None, 0, 0, 0, out) != 0
    assert L.cice_debug_resident_plan(2, None, None, None, None, 0, 0, 0, out) != 0
    assert L.cice_debug_resident_plan(0, None, None, None, None, 0, 0, 0, None) != 0
