"""One horizontal-transport comparison in its own process (the compiled reference allows ONE init_domain and ONE tracer
set per process and library).  Started by tests/test_gpu_transport.py:

    python tests/transport_case.py <cfg> <ew> <ns> [gx3|-] [upwind|-] [trc=0,1,2]

`call transport_remap(dt)` of the compiled reference (source/ice_transport_driver.F90:179; oracle/_ref) on its own
module arrays, block distribution and boundary types, against cice_transport_remap on the MI355X with the same
inputs: every state array, ghost cells included, bit for bit.  With `upwind`: `call transport_upwind(dt)` (:672) against
cice_transport_upwind.  `trc=` is trcr_depend(1:ntrcr) (0 ice area, 1 ice volume, 2 snow volume; default 0,1 = Tsfc, iage).
The planes ntrcr+1 .. max_ntrcr of trcrn carry a sentinel pattern that both sides must leave alone, and every trial is
stepped a SECOND time from the state the first step produced (areas at or below puny, cells just entered, tracers
zeroed by the update).  Prints 'TRANSPORT-OK <n checks>'.

tests/transport_stop_case.py uses the pieces (setup, synth_state, load, fetch) for the failure reports.
"""
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BND = {"open": 0, "cyclic": 1, "closed": 2, "tripole": 3, "tripoleT": 4}
NC, NI, NS, NT = 5, 4, 1, 5
DT = 3600.0
TRIALS = ((0.35, "patchy"), (0.9, "full"), (0.15, "edge"))
STATE = ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon")


def setup(cfg, ew, ns, gx3=False, upwind=False, trc=(0, 1), device=True):
    """The reference initialised for one configuration and tracer set and -- with `device` -- the library on the
    reference's block -> task map with the reference's grid arrays."""
    gridkw = {}
    if gx3:   # the reference's own gx3 grid + land mask, written from the committed fixture
        d = tempfile.mkdtemp()
        z = np.load(os.path.join(ROOT, "tests", "golden", "gx3_grid_kmt.npz"))
        with open(os.path.join(d, "global_gx3.grid"), "wb") as f:
            for k in ("ULAT", "ULON", "HTN", "HTE", "HUS", "HUW", "ANGLE"):
                f.write(z[k].astype(">f8").tobytes())
        with open(os.path.join(d, "global_gx3.kmt"), "wb") as f:
            f.write(z["kmt"].astype(">i4").tobytes())
        gridkw = dict(grid="displaced_pole", grid_file=os.path.join(d, "global_gx3.grid"),
                      kmt_file=os.path.join(d, "global_gx3.kmt"))
    from __graft_entry__ import REF_CONFIGS
    from oracle import refapi
    e = types.SimpleNamespace(cfg=cfg, ew=ew, ns=ns, upwind=upwind, trc=tuple(trc), ntrcr=len(trc))
    e.nxg, e.nyg, bsx, bsy, _mxb = REF_CONFIGS[cfg]
    ref = e.ref = refapi.Ref(cfg)
    ref.init_domain(tempfile.mkdtemp(), dt=DT, ndte=4, ew=ew, ns=ns, **gridkw)
    ref.init_transport(e.ntrcr, e.trc)
    e.nbm, e.ny, e.nx, e.nbl = ref.max_blocks, ref.ny_block, ref.nx_block, ref.nblocks
    nbl, nx, ny = e.nbl, e.nx, e.ny
    e.info = [ref.block_info(l + 1) for l in range(nbl)]
    e.grid = {k: np.ascontiguousarray(ref.get(k)[:nbl]) for k in ("HTN", "HTE", "dxt", "dyt", "dxu", "dyu", "tarear", "hm")}
    e.ctx = e.dom = None
    if device:
        from cice4_amd import lib
        # device topology = the reference's block -> task map
        nbx, nby = (e.nxg - 1) // bsx + 1, (e.nyg - 1) // bsy + 1
        owner = -np.ones(nbx * nby, np.int32); lid = -np.ones(nbx * nby, np.int32)
        for l in range(nbl):
            g = e.info[l]["block_id"] - 1
            owner[g] = 0; lid[g] = l
        ctx = e.ctx = lib.Context(); ctx.sync()
        e.dom = ctx.domain_create_map(e.nxg, e.nyg, bsx, bsy, owner, ew=BND[ew], ns=BND[ns], local_id=lid)
        assert e.dom["nblocks"] == nbl
        if upwind:
            ctx.transport_upwind_init(e.grid["HTE"], e.grid["HTN"], np.ascontiguousarray(ref.get("tarea")[:nbl]),
                                      ntrcr=e.ntrcr, trcr_depend=e.trc, nt_Tsfc=1)
        else:
            ctx.transport_init(e.grid, ntrcr=e.ntrcr, trcr_depend=e.trc)
    # largest displacement that stays inside the neighbouring cells (departure_points :1611-1620), per U point
    HTN, HTE = e.grid["HTN"], e.grid["HTE"]
    dloc = np.zeros_like(HTN)
    dloc[:, :-1, :-1] = np.minimum(np.minimum(HTN[:, :-1, :-1], HTN[:, :-1, 1:]), np.minimum(HTE[:, :-1, :-1], HTE[:, 1:, :-1]))
    e.dloc = np.maximum(dloc, 0.0)
    # global coordinates of every local cell (ghost cells through the block offsets) for smooth fields
    e.gi = np.zeros((nbl, ny, nx)); e.gj = np.zeros((nbl, ny, nx))
    for b in range(nbl):
        i = e.info[b]
        ii = (np.arange(nx) - (i["ilo"] - 1) + (int(i["i_glob"][i["ilo"] - 1]) - 1)) % e.nxg
        jj = np.arange(ny) - (i["jlo"] - 1) + (int(i["j_glob"][i["jlo"] - 1]) - 1)
        e.gi[b], e.gj[b] = np.meshgrid(ii, jj, indexing="xy")
    return e


def sentinel(e):
    """trcrn planes ntrcr+1 .. max_ntrcr: a value no kernel produces, different per block, category, plane and cell"""
    s = np.zeros((e.nbm, NC, NT, e.ny, e.nx))
    cell = np.arange(e.ny * e.nx, dtype=float).reshape(e.ny, e.nx)
    for b in range(e.nbm):
        for n in range(NC):
            for it in range(e.ntrcr, NT):
                s[b, n, it] = -(7.0e6 + 1.0e5 * it + 1.0e4 * n + 1.0e3 * b) - cell
    return s


def synth_state(e, rng, speed, cover):
    """A state on the physical cells and velocities at the U points, displacements up to `speed` of the smallest cell
    edge: the six state arrays (STATE order), aice0, uvel, vvel as (max_blocks, ...) host arrays without ghost cells."""
    nbl, ny, nx, nxg, nyg, gi, gj = e.nbl, e.ny, e.nx, e.nxg, e.nyg, e.gi, e.gj
    hm = e.grid["hm"]
    sm = lambda k: 0.5 + 0.5 * np.sin(2 * np.pi * (k + 1) * gi / nxg + k) * np.cos(np.pi * (k + 2) * gj / nyg + 0.3 * k)
    conc = 0.2 + 0.75 * sm(0)
    if cover == "patchy":
        conc = np.where(sm(1) < 0.35, 0.0, conc)
    elif cover == "edge":
        conc = np.where(gj < nyg / 2, 0.0, conc) * (rng.uniform(0, 1, conc.shape) < 0.8)
    conc = conc * (hm > 0)
    w = np.array([0.1, 0.2, 0.3, 0.25, 0.15])
    aicen = np.zeros((nbl, NC, ny, nx)); vicen = np.zeros_like(aicen); vsnon = np.zeros_like(aicen)
    trcrn = np.zeros((nbl, NC, NT, ny, nx)); eicen = np.zeros((nbl, NC * NI, ny, nx)); esnon = np.zeros((nbl, NC * NS, ny, nx))
    for n in range(NC):
        aicen[:, n] = conc * w[n] * (0.7 + 0.6 * sm(n + 2)) * (rng.uniform(0, 1, conc.shape) < 0.9)
        h = 0.3 + n * 0.8 + 0.5 * sm(n + 7) + 0.05 * rng.uniform(0, 1, conc.shape)
        vicen[:, n] = aicen[:, n] * h
        hs = np.where(sm(n + 11) > 0.4, 0.25 * sm(n + 12), 0.0)          # snow-free patches
        vsnon[:, n] = aicen[:, n] * hs
        ice = aicen[:, n] > 0
        for it, dep in enumerate(e.trc):      # a field of its own per tracer: swapped planes cannot compare equal
            if it == 0:
                assert dep == 0
                trcrn[:, n, 0] = np.where(ice, -1.8 - 15.0 * sm(n + 13), 0.0)           # Tsfc (nt_Tsfc = 1)
            elif it == 1 and dep == 1:
                trcrn[:, n, 1] = np.where(ice, 1.0e5 * (1 + n) * sm(n + 14), 0.0)        # iage (nt_iage = 2)
            else:
                amp = (2.0, 3.0e4, 40.0)[dep] * (1.0 + n + 0.37 * it)
                # a snow-volume tracer (dep 2) has values in snow-free cells too: the reference carries them in and the
                # update decides what comes out; some ice cells hold no tracer at all
                trcrn[:, n, it] = np.where(ice & (sm(n + it + 46) > 0.15), amp * (0.1 + sm(n + 21 + 5 * it)), 0.0)
        for l in range(NI):
            eicen[:, n * NI + l] = -vicen[:, n] / NI * 3.0e8 * (0.8 + 0.2 * sm(n + l + 15))
        esnon[:, n] = -vsnon[:, n] * 1.1e8 * (0.9 + 0.1 * sm(n + 20))
    tot = aicen.sum(axis=1)
    scale = np.where(tot > 0.98, 0.98 / np.maximum(tot, 1e-30), 1.0)[:, None]
    aicen *= scale; vicen *= scale; vsnon *= scale; eicen *= scale; esnon *= scale
    aice0 = 1.0 - aicen.sum(axis=1)
    # velocities at U points: displacements up to `speed` of the smallest cell edge, some cells at rest
    umax = speed * e.dloc / DT
    uvel = umax * (np.sin(2 * np.pi * gi / nxg * 2 + 0.5) * np.cos(np.pi * gj / nyg) + 0.4 * rng.uniform(-1, 1, gi.shape))
    vvel = umax * (np.cos(2 * np.pi * gi / nxg) * np.sin(np.pi * gj / nyg * 2) + 0.4 * rng.uniform(-1, 1, gi.shape))
    rest = rng.uniform(0, 1, gi.shape) < 0.1
    uvel = np.where(rest, 0.0, uvel) / 1.4; vvel = np.where(rest, 0.0, vvel) / 1.4
    return dict(aicen=aicen, trcrn=trcrn, vicen=vicen, vsnon=vsnon, eicen=eicen, esnon=esnon, aice0=aice0, uvel=uvel, vvel=vvel)


def with_ghosts(e, s):
    """(max_blocks, ...) arrays with consistent ghost cells, the way the model keeps its state (the reference's own
    bound_state and ice_HaloUpdate), and the sentinel planes of trcrn: STATE + aice0, uvel, vvel."""
    def full(a):       # host arrays of the reference carry max_blocks blocks
        out = np.zeros((e.nbm,) + a.shape[1:], a.dtype); out[:e.nbl] = a
        return out
    f = {k: full(v) for k, v in s.items()}
    e.ref.bound_state(*[f[k] for k in STATE])
    e.ref.halo_nd(f["aice0"], 1, 1)
    e.ref.halo_nd(f["uvel"], 2, 2); e.ref.halo_nd(f["vvel"], 2, 2)
    f["trcrn"][:, :, e.ntrcr:] = sentinel(e)[:, :, e.ntrcr:]
    return f


def load(e, f):
    """f into the reference's module arrays; returns the library's copies (local blocks)"""
    ny, nx = e.ny, e.nx
    for k in STATE:
        e.ref.set(k, f[k].reshape(-1, ny, nx))
    for k in ("aice0", "uvel", "vvel"):
        e.ref.set(k, f[k])
    return {k: v[:e.nbl].copy() for k, v in f.items()}


def fetch(e):
    nbm, ny, nx, ref = e.nbm, e.ny, e.nx, e.ref
    return dict(aicen=ref.get("aicen", nbm * NC).reshape(nbm, NC, ny, nx), trcrn=ref.get("trcrn", nbm * NC * NT).reshape(nbm, NC, NT, ny, nx),
                vicen=ref.get("vicen", nbm * NC).reshape(nbm, NC, ny, nx), vsnon=ref.get("vsnon", nbm * NC).reshape(nbm, NC, ny, nx),
                eicen=ref.get("eicen", nbm * NC * NI).reshape(nbm, NC * NI, ny, nx),
                esnon=ref.get("esnon", nbm * NC * NS).reshape(nbm, NC * NS, ny, nx), aice0=ref.get("aice0"))


def step_and_compare(e, dev, tag):
    """One step on both sides from what each holds; every state array bit for bit, the sentinel planes as they were.
    Returns the number of arrays compared and of arrays the step changed."""
    before = {k: v.copy() for k, v in dev.items()}
    if e.upwind:
        e.ref.transport_upwind(DT)
        e.ctx.transport_upwind(DT, dev)
    else:
        e.ref.transport_remap(DT)
        assert e.ctx.transport_remap(DT, dev) == (0, 0, 0)
    want = fetch(e)
    sent = sentinel(e)[:e.nbl, :, e.ntrcr:]
    if e.ntrcr < NT:    # the reference leaves the planes beyond ntrcr alone (bound_state: trcrn(:,:,1:ntrcr,:,:)); so must we
        assert np.array_equal(want["trcrn"][:e.nbl, :, e.ntrcr:], sent), (tag, "reference touched the planes beyond ntrcr")
        assert np.array_equal(dev["trcrn"][:, :, e.ntrcr:], sent), (tag, "planes beyond ntrcr touched")
    moved = nchk = 0
    for k, wv in want.items():
        wv = wv[:e.nbl]
        if not np.array_equal(dev[k], wv):
            bad = np.argwhere(dev[k] != wv)
            raise AssertionError((e.cfg, e.ew, e.ns, e.trc, tag, k, len(bad), bad[:6].tolist(),
                                  float(np.abs(dev[k] - wv).max()), float(np.abs(wv).max())))
        moved += int(not np.array_equal(wv, before[k]))
        nchk += 1
    return nchk, moved, not np.array_equal(dev["aicen"], before["aicen"])


def main():
    cfg, ew, ns = sys.argv[1:4]
    rest = sys.argv[4:]
    trc = (0, 1)
    for a in rest:
        if a.startswith("trc="):
            trc = tuple(int(x) for x in a[4:].split(","))
    e = setup(cfg, ew, ns, gx3="gx3" in rest, upwind="upwind" in rest, trc=trc)
    rng = np.random.default_rng(20261004)
    nchk = 0
    for trial, (speed, cover) in enumerate(TRIALS):
        dev = load(e, with_ghosts(e, synth_state(e, rng, speed, cover)))
        n, moved, _ = step_and_compare(e, dev, (trial, "step 1"))
        nchk += n
        # the step really changed the state (a tracer set without a used plane still moves the other six arrays)
        assert moved >= 6, (trial, moved)
        # ... and once more from the state just produced (bit-equal on both sides), same velocities
        n, _, area_moved = step_and_compare(e, dev, (trial, "step 2"))
        nchk += n
        assert area_moved, (trial, "second step left aicen as it was")
    print("TRANSPORT-OK", nchk)


if __name__ == "__main__":
    main()
