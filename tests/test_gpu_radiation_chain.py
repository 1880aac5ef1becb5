"""radiation -> step_therm1 without the upload of the five shortwave arrays (cice_radiation_chain): two steps of
cice_step_radiation -> cice_prep_radiation -> cice_step_therm1 with mode 1 against the same calls with mode 0 on a context
of its own, np.array_equal on everything cice_step_therm1 downloads.  The unchained entries are held to the reference by
test_gpu_shortwave.py and test_gpu_thermo.py.  The state is thermo_case.therm1_inputs' (2 blocks of 22 x 14 with ghosts);
the shortwave arrays of cice_thermo_fields are the arrays the two radiation calls write -- the same objects, the chain goes
by their addresses."""
import functools

import numpy as np
import pytest

import shortwave_case as sc
import thermo_case as tcase
from cice4_amd import lib

pytestmark = pytest.mark.gpu
DT, YDAY = tcase.DT, 150.0
NY, NX, NB = 14, 22, 2
FIVE = ("fswsfc", "fswint", "fswthrun", "Sswabs", "Iswabs")


def _snap(d):
    return {k: v.copy() for k, v in d.items() if isinstance(v, np.ndarray)}


def _run(mode, spoil=False, change=None, steps=2):
    """change: None, "other_pointers" (step_therm1 is given copies of the five arrays, fswsfc halved) or "upload_between" (a
    cice_thermo_batch_upload behind prep_radiation, then fswsfc halved in place).  spoil: the contents of the five host arrays
    are NaN when step_therm1 is called (against the contract: they are what the device holds)."""
    ctx = lib.Context()
    try:
        ctx.sync()
        ctx.thermo_init()
        ctx.shortwave_init(**sc.init_kwargs("default"))
        ctx.thermo_batch_alloc(NX, NY, NB)
        ctx.radiation_chain(mode)
        batch, _, fz, pc, acc = tcase.therm1_inputs(NY, NX, NB, seed=35)
        rng = np.random.default_rng(20261021)
        shp = (NB, NY, NX)
        sw = {k: rng.uniform(0.0, 15.0, shp) for k in sc.SW}   # (what the cold columns of the state can take)
        gbm = {k: rng.uniform(0.05, 0.9, shp) for k in ("alvdr_gbm", "alvdf_gbm", "alidr_gbm", "alidf_gbm")}
        extra = dict(scale_factor=rng.uniform(10.0, 40.0, shp), fswfac=np.zeros(shp))
        alb = {k: np.zeros(batch["aicen"].shape) for k in ("alvdrn", "alidrn", "alvdfn", "alidfn", "albicen", "albsnon")}
        five = dict(fswsfcn=batch["fswsfc"], fswintn=batch["fswint"], fswthrun=batch["fswthrun"], Sswabsn=batch["Sswabs"],
                    Iswabsn=batch["Iswabs"])
        fzb = dict(fz, Tbot=np.zeros(shp), fbot=np.zeros(shp), rside=np.zeros(shp))
        for _ in range(steps):
            ctx.step_radiation(dict({k: batch[k] for k in sc.STATE}, **sw, **alb, **five))
            assert batch["fswsfc"].max() > 0.0
            ctx.prep_radiation(dict(sw, **gbm, **extra, **five, aice=fz["aice"], aicen=batch["aicen"]), sw_resident=True)
            st = batch
            if change == "upload_between":
                ctx.thermo_batch_upload(batch)
                batch["fswsfc"] *= 0.5
            elif change == "other_pointers":
                st = dict(batch, **{k: batch[k].copy() for k in FIVE})
                st["fswsfc"] *= 0.5
            if spoil:
                for k in FIVE:
                    batch[k][...] = np.nan
            r = ctx.step_therm1(DT, YDAY, st, fzb, pc, acc)
            assert r["l_stop"] == 0 and r["n_updates"] > 0, r
            if st is not batch:
                for k in FIVE:
                    batch[k][...] = st[k]
        return _snap(batch), _snap(acc), _snap(fzb), _snap(extra)
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def _plain(change=None):
    return _run(0, change=change)


def _same(got, want, where, skip=()):
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for k in w:
            if k not in skip:
                assert np.array_equal(g[k], w[k], equal_nan=True), (where, k, int((g[k] != w[k]).sum()))


def test_two_steps_chained_equal_unchained():
    want = _plain()
    assert np.isfinite(want[0]["fswsfc"]).all() and want[0]["fswsfc"].max() > 0.0 and np.abs(want[1]["fswabs"]).max() > 0.0
    _same(_run(1), want, "mode 1")


def test_the_device_copies_are_what_is_read():
    """mode 1 with the five host arrays NaN at the time of cice_step_therm1: mode 0's result (fswthrun is not among what
    cice_step_therm1 downloads, so the host array keeps the NaN)"""
    got = _run(1, spoil=True)
    assert np.isnan(got[0]["fswthrun"]).all()
    _same(got, _plain(), "mode 1, host arrays spoilt", skip=("fswthrun",))


def test_other_pointers_upload_as_always():
    want = _plain("other_pointers")
    assert not np.array_equal(want[0]["vicen"], _plain()[0]["vicen"])      # (halving fswsfc changes the step)
    _same(_run(1, change="other_pointers"), want, "mode 1, other pointers")


def test_a_batch_upload_in_between_disarms_the_chain():
    _same(_run(1, change="upload_between"), _plain("upload_between"), "mode 1, cice_thermo_batch_upload in between")
