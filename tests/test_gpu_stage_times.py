"""The device times of the column stages (cice_therm2_itd_times, cice_therm2_cleanup_times, cice_ridge_times,
cice_radiation_times, cice_dedd_times), one test per stage on that stage's fixture and smallest case:

  zeros before any timed call -- a call with timing off leaves the accessor at zeros;
  a timed call gives the bits of the untimed call; afterwards every slot around a kernel that ran is > 0, every other >= 0;
  the values survive switching off and a further untimed call -- except ridging, whose slots every cice_step_ridge zeroes;
  cice_step_radiation fills slot 0 of the radiation times only, cice_prep_radiation slot 1 only.

Every accessor reads the stored times and then sets the flag, so `x_times(True)` on a context whose timing is off answers
with what was stored while it was off."""
import numpy as np
import pytest

import cleanup_itd_case as cc
import dedd_case as dc
import ridge_case as rc
import shortwave_case as sc
import therm_itd_case as tc
from cice4_amd import lib

pytestmark = pytest.mark.gpu
RIDGE_QUEUE = 3                          # iterations queued between two looks at the block words (ridge.h)


@pytest.fixture()
def ctx():
    c = lib.Context()
    c.sync()
    yield c
    c.close()


def _same(got, want, where):
    assert set(got) == set(want), where
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), (where, k, int((got[k] != want[k]).sum()))


def _three_calls(call, times, zero):
    """call() with timing off, on, off; returns (the timed call's times, the times after the third call).  call() gives
    its outputs; times(enable) gives the accessor's answer."""
    assert times(False) == zero
    off = call()
    assert times(True) == zero, "a call with timing off left times behind"
    on = call()
    _same(on, off, "timed against untimed")
    t = times(False)
    third = call()
    _same(third, off, "untimed again")
    return t, times(False)


def test_therm2_itd_times(ctx):
    name = tc.ORDINARY[0]
    raw, _ = tc.load_chain(np.load(tc.FIXTURE), name)
    ctx.itd_init(**tc.itd_kwargs(tc.CASES[name]))
    ctx.thermo_batch_alloc(tc.NX, tc.NY, tc.NB)

    def call():
        a = {k: v.copy() for k, v in raw.items()}
        r = ctx.step_therm2_itd(tc.DT, tc.YDAY, a)
        assert r["l_stop"] == 0, r
        return a

    t, after = _three_calls(call, ctx.therm2_itd_times, (0.0,) * 4)
    assert len(t) == 4 and all(x > 0.0 for x in t), t      # rain + aggregate, linear_itd (kitd = 1), add_new_ice, lateral_melt
    assert after == t


def test_therm2_cleanup_times(ctx):
    from test_gpu_cleanup_itd import _one_call_arrays
    name = cc.ORDINARY[0]
    s, _, _ = cc.load_case(np.load(cc.FIXTURE), name)
    ctx.itd_init(**cc.itd_kwargs(name))
    ctx.thermo_batch_alloc(cc.NX, cc.NY, cc.NB)

    def call():
        a = _one_call_arrays(s)
        r = ctx.step_therm2_cleanup(cc.DT, a)
        assert r["l_stop"] == 0, r
        return a

    zero = dict.fromkeys(lib.CLEANUP_TIMES, 0.0)
    t, after = _three_calls(call, ctx.therm2_cleanup_times, zero)
    assert len(t) == 12
    for k, x in t.items():               # bound = 0: nothing runs between the zap and aggregate
        assert x >= 0.0 if k == "bound_state" else x > 0.0, t
    assert after == t


def test_ridge_times(ctx):
    from test_gpu_ridge import _one_call_arrays
    s, _, niter = rc.load_case(np.load(rc.FIXTURE), "ntr1")
    ctx.itd_init(**rc.itd_kwargs("ntr1"))
    ctx.ridge_init(**rc.ridge_kwargs("ntr1"))
    ctx.thermo_batch_alloc(rc.NX, rc.NY, rc.NB)

    def call():
        a = _one_call_arrays(s)
        r = ctx.step_ridge(rc.DT, a)
        assert r["l_stop"] == 0, r
        return a

    zero = dict.fromkeys(lib.RIDGE_TIMES, 0.0)
    t, after = _three_calls(call, ctx.ridge_times, zero)
    v = [t[k] for k in lib.RIDGE_TIMES]
    assert len(v) == 41
    ran = max(k for k in range(40) if v[k] > 0.0) // 2 + 1     # iterations whose two kernels were launched
    assert ran >= int(max(niter)) and (ran % RIDGE_QUEUE == 0 or ran == 20), (ran, niter)
    assert all(x > 0.0 for x in v[:2 * ran]) and all(x == 0.0 for x in v[2 * ran:40]), v
    assert v[40] > 0.0                   # the finish
    assert after == zero                 # every cice_step_ridge zeroes them, timed or not


def test_radiation_times(ctx):
    from test_gpu_shortwave import ALL_OUT, _outputs
    s, _ = sc.load_case(np.load(sc.FIXTURE), "default")
    ctx.thermo_init()
    ctx.shortwave_init(**sc.init_kwargs("default"))
    ctx.thermo_batch_alloc(sc.NX, sc.NY, sc.NB)

    def step():
        a = dict(s)
        a.update(_outputs(s["aicen"].shape))
        ctx.step_radiation(a)
        return {k: a[k] for k in ALL_OUT}

    def prep():
        p = sc.prep_inputs()
        ctx.prep_radiation(p)
        return {k: p[k] for k in ("scale_factor", "fswfac") + sc.PREP_SW}

    assert ctx.radiation_times(False) == (0.0, 0.0)
    off = step(), prep()
    assert ctx.radiation_times(True) == (0.0, 0.0)
    on_step = step()
    t1 = ctx.radiation_times(True)
    assert t1[0] > 0.0 and t1[1] == 0.0, t1                # k_shortwave_ccsm3 fills slot 0 only
    on_prep = prep()
    t2 = ctx.radiation_times(True)
    assert t2[0] == t1[0] and t2[1] > 0.0, (t1, t2)        # k_prep_radiation fills slot 1 only
    _same(on_step, off[0], "step_radiation, timed against untimed")
    _same(on_prep, off[1], "prep_radiation, timed against untimed")
    assert ctx.radiation_times(False) == t2
    _same(step(), off[0], "step_radiation, untimed again")
    _same(prep(), off[1], "prep_radiation, untimed again")
    assert ctx.radiation_times(False) == t2


def test_dedd_times(ctx):
    from test_gpu_dedd import IN_2D, _outputs
    s, _ = dc.load_case(np.load(dc.FIXTURE), dc.DRIVER_CASES[0])
    ctx.thermo_init()
    ctx.shortwave_dedd_init(**dc.init_kwargs(dc.DRIVER_CASES[0]))
    ctx.thermo_batch_alloc(dc.NX, dc.NY, dc.NB)

    def call():
        a = {k: v for k, v in s.items() if k in dc.STATE + IN_2D + ("apondn", "hpondn")}
        a.update(_outputs(s["aicen"].shape))
        ctx.step_radiation_dedd(a)
        return {k: a[k] for k in dc.OUT}

    t, after = _three_calls(call, ctx.dedd_times, 0.0)
    assert t > 0.0
    assert after == t

