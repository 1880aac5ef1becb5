"""Cases, inputs and bookkeeping shared by tests/golden/make_golden_cleanup_itd.py (which runs the compiled reference) and
the tests of the second half of step_therm2 (test_cleanup_itd_golden.py, test_gpu_cleanup_itd.py).  No GPU here.

A case starts from the state s3 of a case of tests/golden/therm_itd.npz (what lateral_melt leaves on 4 blocks of 14 x 12)
and applies seeded edits: blocks 1 and 2 get categories that are out of their thickness bounds, block 3 is put in
bounds and cleared of tiny areas (the quiet one), block 4 is put in bounds and gets tiny, negative-tiny and excess areas.
The fixture stores what cleanup_itd left as the XOR of its bit patterns with the inputs, and what aggregate made of that."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import therm_itd_case as tc  # noqa: E402
from cice4_amd import synth  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "cleanup_itd.npz")
NX, NY, NB, DT, PUNY = tc.NX, tc.NY, tc.NB, tc.DT, tc.PUNY
ILO, IHI, JLO, JHI = tc.ILO, tc.IHI, tc.JLO, tc.JHI
NCAT, NILYR, NSLYR = synth.NCAT, synth.NILYR, synth.NSLYR
TOCNFRZ = synth.Tocnfrz

CASES = {
    "ntr1": dict(base="growth", seed=2026101901, hin0=0.0),
    "ntr4": dict(base="tracers", seed=2026101902, hin0=0.0),
    "floor": dict(base="growth", seed=2026101903, hin0=0.05),
}
ORDINARY = tuple(CASES)
STOPS = ("stop_area", "stop_zap")
STATE = tc.STATE
FLUX = ("fresh", "fsalt", "fhocn")
OUT_CLEAN = STATE + ("aice", "aice0") + FLUX          # what cleanup_itd writes
OUT_AGG = ("aice", "aice0", "vice", "vsno", "eice", "esno", "trcr")
BRANCHES = ("up_one", "up_cascade", "down_one", "floor_cat1", "bystander_roundtrip", "bystander_zeroed", "quiet_block",
            "two_passes_one_block", "zap_pos", "zap_neg", "zap_all", "zap_excess", "neg_zero_flux")
NEED = dict({k: 8 for k in BRANCHES}, quiet_block=1, two_passes_one_block=1)


def ntrcr(name):
    return tc.CASES[CASES[name]["base"] if name in CASES else "growth"]["ntrcr"]


def hin_max(name):
    hm = synth.hin_max().copy()
    hm[0] = CASES[name]["hin0"] if name in CASES else 0.0
    return hm


def itd_kwargs(name):
    kw = tc.itd_kwargs(tc.CASES[CASES[name]["base"] if name in CASES else "growth"])
    kw["hin_max"] = hin_max(name)
    return kw


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def cat_sum(aicen):
    """sum over categories in category order; aicen (..., ncat, ny, nx) -> (..., ny, nx)"""
    s = np.zeros(aicen.shape[:-3] + aicen.shape[-2:])
    for n in range(NCAT):
        s = s + aicen[..., n, :, :]
    return s


def _scale(s, b, n, j, i, r):
    """category n of cell (j, i) of block b times r: area, volumes, energies"""
    for k in ("aicen", "vicen", "vsnon"):
        s[k][b, n, j, i] *= r
    s["eicen"][b, n * NILYR:(n + 1) * NILYR, j, i] *= r
    s["esnon"][b, n * NSLYR:(n + 1) * NSLYR, j, i] *= r


def _empty(s, b, n, j, i):
    _scale(s, b, n, j, i, 0.0)
    s["trcrn"][b, n, :, j, i] = 0.0
    s["trcrn"][b, n, 0, j, i] = TOCNFRZ


def _set_h(s, b, n, j, i, h):
    """thickness of category n: the volume and with it the layer energies"""
    v = s["vicen"][b, n, j, i]
    new = s["aicen"][b, n, j, i] * h
    s["eicen"][b, n * NILYR:(n + 1) * NILYR, j, i] *= (new / v) if v != 0.0 else 0.0
    s["vicen"][b, n, j, i] = new


def _in_bounds(s, b, hm, clear_tiny):
    top = np.append(hm[:NCAT], hm[NCAT - 1] + 2.0)
    for j in range(NY):
        for i in range(NX):
            for n in range(NCAT):
                a, v = s["aicen"][b, n, j, i], s["vicen"][b, n, j, i]
                if clear_tiny and a != 0.0 and abs(a) <= PUNY:
                    _empty(s, b, n, j, i)
                elif a > PUNY and not (top[n] < v / a <= top[n + 1] or (n == NCAT - 1 and v / a > top[n])):
                    _set_h(s, b, n, j, i, 0.5 * (top[n] + top[n + 1]))


def _cells(rng, s, b, cond, count):
    """`count` physical cells of block b where cond (ny, nx) holds, no cell twice over the calls of a case"""
    ok = cond.copy()
    ok[:JLO - 1] = ok[JHI:] = False
    ok[:, :ILO - 1] = ok[:, IHI:] = False
    ok &= ~s["_used"][b]
    jj, ii = np.nonzero(ok)
    assert len(jj) >= count, (b, len(jj), count)
    pick = rng.choice(len(jj), size=count, replace=False)
    out = [(int(jj[k]), int(ii[k])) for k in sorted(pick)]
    for j, i in out:
        s["_used"][b, j, i] = True
    return out


def base_state(name):
    """s3 of the base case with its tmask, areas brought to a sum <= 1, empty categories at Tocnfrz, daidtt / dvidtt"""
    c = CASES[name] if name in CASES else dict(base="growth", seed=2026101904)
    raw, chain = tc.load_chain(np.load(tc.FIXTURE), c["base"])
    s = {k: chain[3][k].copy() for k in STATE + FLUX}
    s["tmask"] = raw["tmask"].copy()
    tot = cat_sum(s["aicen"])
    f = np.where(tot > 1.0, 0.98 / np.where(tot > 1.0, tot, 1.0), 1.0)
    for k, per in (("aicen", 1), ("vicen", 1), ("vsnon", 1), ("eicen", NILYR), ("esnon", NSLYR)):
        s[k] = s[k] * np.repeat(f[:, None], NCAT * per, axis=1)
    none = s["aicen"] == 0.0
    s["trcrn"][:, :, 1:][np.broadcast_to(none[:, :, None], s["trcrn"][:, :, 1:].shape)] = 0.0
    s["trcrn"][:, :, 0][none] = TOCNFRZ
    rng = np.random.default_rng(c["seed"])
    s["daidtt"] = rng.uniform(0.0, 1.0, s["fresh"].shape)
    s["dvidtt"] = rng.uniform(0.0, 3.0, s["fresh"].shape)
    return s, rng


def case_inputs(name):
    """the edited state of an ordinary case, all blocks"""
    s, rng = base_state(name)
    hm = hin_max(name)
    top = np.append(hm[:NCAT], hm[NCAT - 1] + 2.0)
    s["_used"] = np.zeros((NB, NY, NX), bool)
    a = s["aicen"]
    _in_bounds(s, 2, hm, True)
    _in_bounds(s, 3, hm, False)
    # blocks 1 and 2: out of bounds.  Block 1 upward (one boundary, then a cascade over two), block 2 downward and upward
    for b, plan in ((0, ("up", "cascade")), (1, ("down", "up"))):
        for what in plan:
            if what == "up":
                n = int(rng.integers(0, NCAT - 1))
                for j, i in _cells(rng, s, b, a[b, n] > 0.01, 9):
                    _set_h(s, b, n, j, i, 0.5 * (top[n + 1] + top[n + 2]))
            elif what == "cascade":
                n = int(rng.integers(0, NCAT - 2))
                for j, i in _cells(rng, s, b, a[b, n] > 0.01, 9):
                    _empty(s, b, n + 1, j, i)
                    _set_h(s, b, n, j, i, 0.5 * (top[n + 2] + top[n + 3]))
            else:
                n = int(rng.integers(1, NCAT))
                for j, i in _cells(rng, s, b, a[b, n] > 0.01, 9):
                    _set_h(s, b, n, j, i, 0.5 * (top[n - 1] + top[n]) if n > 1 else 0.5 * (max(hm[0], 0.06) + top[1]))
    if hm[0] > 0.0:        # category 1 thinner than hin_max(0): lifted, in a block with shifts and in one without
        for b in (0, 3):
            for j, i in _cells(rng, s, b, a[b, 0] > 0.01, 6):
                _set_h(s, b, 0, j, i, float(rng.uniform(0.01, 0.04)))
    # block 4: zaps only
    b = 3
    any_ice = (a[b] > 0.01).any(axis=0)
    for j, i in _cells(rng, s, b, any_ice, 10):           # 0 < aicen <= puny
        n = int(np.nonzero(a[b, :, j, i] > 0.01)[0][0])
        _scale(s, b, n, j, i, rng.uniform(1e-12, 9e-12) / a[b, n, j, i])
    for j, i in _cells(rng, s, b, any_ice, 10):           # -puny <= aicen < 0
        n = int(np.nonzero(a[b, :, j, i] > 0.01)[0][-1])
        _scale(s, b, n, j, i, -rng.uniform(1e-12, 9e-12) / a[b, n, j, i])
    for j, i in _cells(rng, s, b, any_ice, 9):            # every category tiny
        for n in range(NCAT):
            if a[b, n, j, i] > 0.0:
                _scale(s, b, n, j, i, rng.uniform(1e-12, 9e-12) / a[b, n, j, i])
            else:
                a[b, n, j, i] = rng.uniform(1e-12, 9e-12)
                s["vicen"][b, n, j, i] = a[b, n, j, i] * 0.5 * (top[n] + top[n + 1])
                s["eicen"][b, n * NILYR:(n + 1) * NILYR, j, i] = -3.0e8 * s["vicen"][b, n, j, i] / NILYR
                s["trcrn"][b, n, 0, j, i] = -5.0
    for j, i in _cells(rng, s, b, any_ice, 10):           # areas summing to a value in (1, 1 + puny)
        r = (1.0 + 3.0e-12) / cat_sum(a[b][:, j:j + 1, i:i + 1])[0, 0]
        for n in range(NCAT):
            _scale(s, b, n, j, i, r)
        last = int(np.nonzero(a[b, :, j, i] > 0.01)[0][-1])
        for _ in range(60):
            tot = cat_sum(a[b][:, j:j + 1, i:i + 1])[0, 0]
            if 1.0 + 1.0e-12 < tot < 1.0 + 6.0e-12:
                break
            a[b, last, j, i] += (1.0 + 3.0e-12) - tot
        assert 1.0 < cat_sum(a[b][:, j:j + 1, i:i + 1])[0, 0] < 1.0 + PUNY
    # -0.0 going in where no zap can reach: the ghost cells of every block
    ghost = np.ones((NB, NY, NX), bool)
    ghost[:, JLO - 1:JHI, ILO - 1:IHI] = False
    s["fresh"][ghost & (rng.random((NB, NY, NX)) < 0.5)] = -0.0
    del s["_used"]
    return {k: np.ascontiguousarray(v) for k, v in s.items()}


def stop_inputs(which):
    """one block (block 4 of the base state, in bounds) and the cell the reference is expected to name.
    stop_area: aice = 1.1 in two cells -- the LAST is named.  stop_zap: aicen(3) = -1e-6 in two cells -- the FIRST is named;
    tiny areas in categories 1, 2 (zapped) and 4 (not reached) of other cells."""
    s, rng = base_state(which)
    hm = synth.hin_max().copy()
    s["_used"] = np.zeros((NB, NY, NX), bool)
    _in_bounds(s, 3, hm, True)
    a = s["aicen"]
    b = 3
    cells = _cells(rng, s, b, a[b, 0] > 0.01, 2)
    if which == "stop_area":
        for j, i in cells:
            a[b, 0, j, i] += 1.1 - cat_sum(a[b][:, j:j + 1, i:i + 1])[0, 0]
        expect = cells[-1]
    else:
        for j, i in cells:
            a[b, 2, j, i] = -1.0e-6
        for n in (0, 1, 3):
            for j, i in _cells(rng, s, b, a[b, n] > 0.01, 3):
                _scale(s, b, n, j, i, 5.0e-12 / a[b, n, j, i])
        expect = cells[0]
    del s["_used"]
    blk = {k: np.ascontiguousarray(v[b]) for k, v in s.items()}
    return blk, (expect[1] + 1, expect[0] + 1)


def digest(s):
    return tc.digest(s)


def head_aice(s):
    return cat_sum(s["aicen"])


def branch_counts(name, s, out):
    """cells (or blocks) per branch of BRANCHES from the inputs s and what cleanup_itd left, all blocks of one case"""
    ntr = ntrcr(name)
    a0, a1 = s["aicen"], out["aicen"]
    inner = np.zeros((NB, NY, NX), bool)
    inner[:, JLO - 1:JHI, ILO - 1:IHI] = True
    aice = head_aice(s)
    listed = inner & (aice > PUNY)
    gone = (a0 > PUNY) & (a1 == 0.0)                       # a whole category moved away
    up = np.zeros((NB, NCAT, NY, NX), bool)
    down = np.zeros_like(up)
    up[:, :-1] = gone[:, :-1] & ((a1[:, 1:] > a0[:, 1:]) | gone[:, 1:])
    down[:, 1:] = gone[:, 1:] & (a1[:, :-1] > a0[:, :-1])
    casc = np.zeros((NB, NY, NX), bool)
    for n in range(NCAT - 2):
        casc |= gone[:, n] & (a1[:, n + 1] == 0.0) & (a1[:, n + 2] > a0[:, n + 2]) & ~(a0[:, n + 1] > PUNY)
    shifted = listed & (up.any(axis=1) | down.any(axis=1) | casc)
    passes = [set() for _ in range(NB)]
    for b in range(NB):
        for n in range(NCAT):
            if (listed[b] & up[b, n]).any():
                passes[b].add(("up", n))
            if (listed[b] & casc[b]).any():
                passes[b].add(("up", "second"))
            if (listed[b] & down[b, n]).any():
                passes[b].add(("down", n))
    fired = np.array([len(p) > 0 for p in passes])
    t0, t1 = bits(s["trcrn"][:, :, :ntr]), bits(out["trcrn"][:, :, :ntr])
    tchg = (t0 != t1).reshape(NB, -1, NY, NX).any(axis=1)
    tiny = (a0 != 0.0) & (np.abs(a0) <= PUNY)
    zapped = tiny & (a1 == 0.0)
    thin = (a0[:, 0] > PUNY) & (s["vicen"][:, 0] / np.where(a0[:, 0] > PUNY, a0[:, 0], 1.0) <= hin_max(name)[0])
    c = dict(
        up_one=int((listed & up.any(axis=1) & ~casc).sum()),
        up_cascade=int((listed & casc).sum()),
        down_one=int((listed & down.any(axis=1)).sum()),
        floor_cat1=int((listed & thin & (hin_max(name)[0] > 0.0) & (bits(a1[:, 0]) != bits(a0[:, 0]))).sum()),
        bystander_roundtrip=int((listed & ~shifted & fired[:, None, None] & tchg & ~zapped.any(axis=1)).sum()),
        bystander_zeroed=int((~listed & fired[:, None, None] & ((s["trcrn"][:, :, 0] == TOCNFRZ) &
                                                                  (bits(out["trcrn"][:, :, 0]) == 0)).any(axis=1)).sum()),
        quiet_block=int(sum(1 for b in range(NB) if listed[b].any() and not fired[b] and not tchg[b].any())),
        two_passes_one_block=int(sum(1 for p in passes if len(p) >= 2)),
        zap_pos=int((inner & (zapped & (a0 > 0.0)).any(axis=1)).sum()),
        zap_neg=int((inner & (zapped & (a0 < 0.0)).any(axis=1)).sum()),
        zap_all=int((inner & zapped.all(axis=1)).sum()),
        zap_excess=int((inner & (aice > 1.0) & (aice < 1.0 + PUNY) & (out["aice"] == 1.0) & (out["aice0"] == 0.0)).sum()),
        neg_zero_flux=int(((bits(s["fresh"]) == bits(np.array(-0.0))) & (bits(out["fresh"]) == 0)).sum()),
    )
    return c, [b for b in range(NB) if listed[b].any() and not fired[b] and not tchg[b].any()]


def load_case(d, name):
    """inputs, what cleanup_itd left, what aggregate made of it -- from the fixture d (np.load) and the case module"""
    s = case_inputs(name)
    out = {k: v.copy() for k, v in s.items()}              # tmask, daidtt, dvidtt: cleanup_itd does not see them
    for k in OUT_CLEAN:
        out[k] = d[f"{name}_clean_{k}"] if k in ("aice", "aice0") else tc.unxor(d[f"{name}_clean_{k}"], s[k]).reshape(s[k].shape)
    agg = {k: d[f"{name}_agg_{k}"] for k in OUT_AGG}
    return s, out, agg


def tendencies(s, agg):
    """ice_step_mod.F90:504-509"""
    return (agg["aice"] - s["daidtt"]) / DT, (agg["vice"] - s["dvidtt"]) / DT
