"""The failure reports of the horizontal transport: (l_stop, istop, jstop) of cice_transport_remap against the cell the
compiled reference names before it ends through abort_ice.  One process per call (the reference allows one init_domain
per process, and a failing transport_remap of the reference ends its process):

    python tests/transport_stop_case.py mint  <case>   reference alone: prints the inputs' checksum and the margins, then
                                                        `call transport_remap(dt)`: the reference prints its diagnosis and stops
    python tests/transport_stop_case.py probe <case>   reference alone, the intended cells repaired: the call completes; checks
                                                        that no OTHER cell is anywhere near a threshold
    python tests/transport_stop_case.py gpu             every case on ONE library context against tests/golden/
                                                        transport_stop.npz, then a good call against the reference, bit for bit

All cases on `small cyclic open` (24 x 20 cells, 2 x 2 blocks of 12 x 10; local blocks 0..3, local 1-based (i, j) with one
ghost cell: physical cells 2..13 x 2..11).  The reference's rule (source/ice_transport_remap.F90): departure_points
(:1640-1655) and update_fields (:3756-3772) overwrite istop, jstop at every failing cell, so the LAST failing cell in
j-then-i order is named; the departure checks of all blocks (:560-665) come before any area check (:701-879); the first
failing block ends the run; within a block open water (:830-848) comes before the categories in order (:855-875).

Inputs are made of uniform random numbers and + - * / only (bit-reproducible on any host, no libm), from the case's seed.

How an area fails here.  With l_dp_midpt = T (ice_transport_driver.F90:60) a departure point is taken with the velocity
interpolated at the midpoint of the back trajectory, inside the cell between the moving corners: for corners that move
apart by d and w cells the corrected displacements add up to (d + w) - (d + w)^2 / 2 <= 1/2 per axis, so no velocity
field that passes the departure check turns a cell's departure region inside out, and the limited reconstruction is not
negative: a divergent flow alone cannot push a new area below -puny by a margin.  What does reach update_fields' check is
a state that comes in wrong: an over-full cell (sum of aicen > 1, aice0 < 0: convergence before ridging) for open
water, a negative category area for a category.  The four U points around every such cell are at rest, so its four
edge fluxes are exactly zero and its new mass IS its old mass (-0.05): the margin is exact, not a matter of rounding.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import transport_case as tc  # noqa: E402

CFG = ("small", "cyclic", "open")
FIXTURE = os.path.join(HERE, "golden", "transport_stop.npz")
NC, NI, NT, DT = tc.NC, tc.NI, tc.NT, tc.DT
DEFICIT = -0.05          # new (= old) mass of an intended area failure: far below -1e-3
OVER = 1.05              # displacement of an intended departure failure, in units of the edge it must stay within

# case -> seed, intended failures.  dep: (block, i, j) of U points; open: (block, i, j) of cells; cat: (block, category, i, j)
# of 3 x 3 patches' centres, every U point of a patch physical (aice0 exactly 0 on the patch, the category alone covers it with area 1, the centre is negative).
#
# What each wrong ordering would return -- every one differs from the expected report:
#   dep        expected (1, 9, 7): last failing U point of block 1, the first failing block.
#              first instead of last: (1, 4, 3).  a later block: (1, 6, 5).
#   area-open  expected (2, 10, 8): open water, last failing cell of block 1.
#              first instead of last: (2, 5, 4).  a later block: (2, 7, 6).
#   area-cat   expected (2, 11, 4): category 1 (patches B1, B2) is the first failing category of block 1, B2's centre its last
#              failing cell; patch A (category 3) lies behind both in j-then-i order.
#              first instead of last: (2, 4, 4) (B1).  cell before category: (2, 7, 9) (A) with the last cell, (2, 4, 4) with
#              the first.  a later block: (2, 7, 6).  block and category fields swapped in the key: the over-full cell of
#              block 3 (category 0) then comes before block 1 / category 1: (2, 7, 6).
#   dep+area   expected (1, 9, 7): the departure report wins although the area failure lies in an EARLIER block (0).
#              code 2 over code 1, or block before code: (2, 8, 9).
CASES = {
    "dep": dict(seed=71001, dep=[(1, 4, 3), (1, 9, 7), (3, 6, 5)], expect=(1, 9, 7)),
    "area-open": dict(seed=71002, open=[(1, 5, 4), (1, 10, 8), (3, 7, 6)], expect=(2, 10, 8)),
    "area-cat": dict(seed=71003, cat=[(1, 1, 4, 4), (1, 1, 11, 4), (1, 3, 7, 9)], open=[(3, 7, 6)], expect=(2, 11, 4)),
    "dep+area": dict(seed=71004, dep=[(1, 4, 3), (1, 9, 7), (3, 6, 5)], open=[(0, 8, 9)], expect=(1, 9, 7)),
}


def physical(e):
    m = np.zeros((e.nbl, e.ny, e.nx), bool)
    for b, i in enumerate(e.info):
        m[b, i["jlo"] - 1:i["jhi"], i["ilo"] - 1:i["ihi"]] = True
    return m


def build(e, name, repaired=False):
    """The (max_blocks, ...) input arrays of a case, ghost cells filled by the reference's halo routines (the transport of
    the reference never sees them here), and their checksum."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    sh = (e.nbl, e.ny, e.nx)
    U = lambda: rng.uniform(0.0, 1.0, sh)
    ocean = (e.grid["hm"] > 0) * 1.0
    w = np.array([0.1, 0.2, 0.3, 0.25, 0.15])
    aicen = np.zeros((e.nbl, NC) + sh[1:]); vicen = np.zeros_like(aicen); vsnon = np.zeros_like(aicen)
    trcrn = np.zeros((e.nbl, NC, NT) + sh[1:]); eicen = np.zeros((e.nbl, NC * NI) + sh[1:]); esnon = np.zeros((e.nbl, NC) + sh[1:])
    for n in range(NC):
        aicen[:, n] = ocean * w[n] * (0.55 + 0.25 * U())           # full cover, sum <= 0.8
        vicen[:, n] = aicen[:, n] * (0.5 + 0.7 * n + 0.2 * U())
        vsnon[:, n] = aicen[:, n] * 0.1 * U()
        trcrn[:, n, 0] = ocean * (-5.0 - 3.0 * U())
        trcrn[:, n, 1] = ocean * 1.0e4 * U()
        for l in range(NI):
            eicen[:, n * NI + l] = -vicen[:, n] / NI * 3.0e8 * (0.8 + 0.2 * U())
        esnon[:, n] = -vsnon[:, n] * 1.1e8
    uvel = 0.3 * e.dloc / DT * (2.0 * U() - 1.0)                   # |displacement| <= 0.3 of the smallest edge
    vvel = 0.3 * e.dloc / DT * (2.0 * U() - 1.0)
    HTN, HTE = e.grid["HTN"], e.grid["HTE"]
    # U points that touch a land cell are at rest (the model's umask): no ice trickles into a land cell, where a new area
    # of 1e-8 would sit closer to update_fields' threshold than the conditions on the inputs allow
    umask = np.zeros(sh)
    umask[:, :-1, :-1] = ocean[:, :-1, :-1] * ocean[:, :-1, 1:] * ocean[:, 1:, :-1] * ocean[:, 1:, 1:]
    uvel *= umask; vvel *= umask

    def at_rest(b, i0, i1, j0, j1):     # U points (1-based, inclusive) around cells
        uvel[b, j0 - 1:j1, i0 - 1:i1] = 0.0; vvel[b, j0 - 1:j1, i0 - 1:i1] = 0.0

    for (b, i, j) in c.get("open", ()):             # over-full cell: the categories scaled to a sum of 1.05
        at_rest(b, i - 1, i, j - 1, j)
        if not repaired:
            s = (1.0 - DEFICIT) / aicen[b, :, j - 1, i - 1].sum()
            for a in (aicen, vicen, vsnon):
                a[b, :, j - 1, i - 1] *= s
            eicen[b, :, j - 1, i - 1] *= s; esnon[b, :, j - 1, i - 1] *= s
    for (b, n, i, j) in c.get("cat", ()):           # 3 x 3 patch, category n alone, every U point of it at rest
        at_rest(b, i - 2, i + 1, j - 2, j + 1)
        J, I = slice(j - 2, j + 1), slice(i - 2, i + 1)
        for a in (aicen, vicen, vsnon, eicen, esnon):
            a[b, :, J, I] = 0.0
        trcrn[b, :, :, J, I] = 0.0
        aicen[b, n - 1, J, I] = 1.0; vicen[b, n - 1, J, I] = 2.0
        trcrn[b, n - 1, 0, J, I] = -6.0
        eicen[b, (n - 1) * NI:n * NI, J, I] = -1.4e8
        if not repaired:
            aicen[b, n - 1, j - 1, i - 1] = DEFICIT; vicen[b, n - 1, j - 1, i - 1] = 0.0
            trcrn[b, n - 1, 0, j - 1, i - 1] = 0.0; eicen[b, (n - 1) * NI:n * NI, j - 1, i - 1] = 0.0
    aice0 = 1.0 - aicen.sum(axis=1)
    for (b, n, i, j) in c.get("cat", ()):
        aice0[b, j - 2:j + 1, i - 2:i + 1] = 0.0    # exactly 0 on the patch (the centre's category area is what is wrong)
    for (b, i, j) in c.get("dep", ()):              # 5 % beyond the east neighbour's north edge: dpx > HTN(i+1,j) (:1647)
        if not repaired:
            uvel[b, j - 1, i - 1] = -OVER * HTN[b, j - 1, i] / DT
    f = tc.with_ghosts(e, dict(aicen=aicen, trcrn=trcrn, vicen=vicen, vsnon=vsnon, eicen=eicen, esnon=esnon, aice0=aice0,
                               uvel=uvel, vvel=vvel))
    h = hashlib.sha256()
    for k in sorted(f):
        h.update(np.ascontiguousarray(f[k]).tobytes())
    return f, h.hexdigest()


def departure_failures(e, f):
    """The four inequalities of departure_points :1647-1648 at every physical U point: one fp64 multiply and a compare
    each, as in the reference.  Returns the failing (block, i, j), in the reference's loop order, and for every physical
    point the largest displacement in units of the edge it is checked against."""
    HTN, HTE = e.grid["HTN"], e.grid["HTE"]
    u, v = f["uvel"][:e.nbl], f["vvel"][:e.nbl]
    dpx, dpy = -DT * u, -DT * v
    bad = np.zeros(u.shape, bool); ratio = np.zeros(u.shape)
    C = (slice(None), slice(0, -1), slice(0, -1))
    E = (slice(None), slice(0, -1), slice(1, None)); N = (slice(None), slice(1, None), slice(0, -1))
    bad[C] = (dpx[C] < -HTN[C]) | (dpx[C] > HTN[E]) | (dpy[C] < -HTE[C]) | (dpy[C] > HTE[N])
    ratio[C] = np.maximum(np.maximum(-dpx[C] / HTN[C], dpx[C] / HTN[E]), np.maximum(-dpy[C] / HTE[C], dpy[C] / HTE[N]))
    phys = physical(e)
    bad &= phys
    return [(int(b), int(i) + 1, int(j) + 1) for b, j, i in np.argwhere(bad)], np.where(phys, ratio, 0.0)


def check_inputs(e, name, f):
    """The conditions on a case's inputs that can be read off the inputs; raises if one does not hold."""
    c = CASES[name]
    fails, ratio = departure_failures(e, f)
    assert sorted(fails) == sorted(c.get("dep", ())), (name, fails)
    for (b, i, j) in c.get("dep", ()):
        assert ratio[b, j - 1, i - 1] >= 1.02, (name, b, i, j, ratio[b, j - 1, i - 1])       # at least 2 % beyond the edge
    rest = ratio.copy()
    for (b, i, j) in c.get("dep", ()):
        rest[b, j - 1, i - 1] = 0.0
    assert rest.max() < 0.9, (name, rest.max())                                             # all other points below 0.9
    # intended area failures: the four U points around the cell at rest => all four edge fluxes are exactly 0 and
    # update_fields' new mass is the old one, bit for bit: DEFICIT < -1e-3
    for (b, i, j) in c.get("open", ()):
        assert not f["uvel"][b, j - 2:j, i - 2:i].any() and not f["vvel"][b, j - 2:j, i - 2:i].any()
        assert f["aice0"][b, j - 1, i - 1] < -1e-3 and abs(f["aice0"][b, j - 1, i - 1] - DEFICIT) < 1e-12
    for (b, n, i, j) in c.get("cat", ()):
        assert not f["uvel"][b, j - 3:j + 1, i - 3:i + 1].any() and not f["vvel"][b, j - 3:j + 1, i - 3:i + 1].any()
        assert f["aicen"][b, n - 1, j - 1, i - 1] == DEFICIT and not f["aice0"][b, j - 2:j + 1, i - 2:i + 1].any()
    # nothing else is negative on input
    neg = int((f["aice0"][:e.nbl] < 0).sum() + (f["aicen"][:e.nbl] < 0).sum())
    assert neg == len(c.get("open", ())) + len(c.get("cat", ())), (name, neg)
    return ratio


def parse_reference_output(text):
    """What the reference printed before it stopped -> dict(kind, i, j, value, iblk, cat)"""
    lines = text.splitlines()
    r = dict(kind=0, i=0, j=0, value=0.0, iblk=0, cat=-1)
    num = lambda s: [float(x) for x in s.replace("'", " ").split()]
    for ln in lines:
        if "my_task, i, j =" in ln:
            _t, r["i"], r["j"] = (int(x) for x in num(ln.split("=", 1)[1]))
        elif "dpx, dpy =" in ln:
            r["value"] = max(abs(x) for x in num(ln.split("=", 1)[1]))
        elif "New mass < 0, i, j =" in ln:
            r["i"], r["j"] = (int(x) for x in num(ln.split("=", 1)[1]))
        elif "New mass =" in ln:
            r["value"] = num(ln.split("=", 1)[1])[0]
        elif "istep1, my_task, iblk, cat =" in ln:
            v = num(ln.split("=", 1)[1])
            r["iblk"], r["cat"] = int(v[2]), int(v[3])
        elif "istep1, my_task, iblk =" in ln:
            r["iblk"] = int(num(ln.split("=", 1)[1])[2])
        elif "bad departure points" in ln:
            r["kind"] = 1
        elif "negative area (open water)" in ln:
            r["kind"] = 2; assert r["cat"] == 0
        elif "negative area (ice)" in ln:
            r["kind"] = 2; assert r["cat"] >= 1
    return r


def mint(name, probe):
    e = tc.setup(*CFG, device=False)
    f, digest = build(e, name)
    check_inputs(e, name, f)
    print("STOP-INPUTS", name, digest, flush=True)
    if probe:
        # the same inputs with the intended cells repaired: the call completes, and every cell whose mass the call changed
        # ends far from update_fields' threshold -puny (a cell the call leaves as it is cannot be moved across it by
        # rounding); no departure point beyond 0.9 was checked above.  The repaired cells' neighbours see another value
        # in their gradient stencil than in the failing call, but no flux through the shared edges in either (the
        # corners are at rest): with areas >= 0.05 there and displacements <= 0.3 they stay far above 1e-6 in both.
        g, _ = build(e, name, repaired=True)
        old = tc.load(e, g)
        e.ref.transport_remap(DT)
        new = tc.fetch(e)
        worst = np.inf
        for k, o, w in (("aice0", old["aice0"], new["aice0"][:e.nbl]), ("aicen", old["aicen"], new["aicen"][:e.nbl])):
            ph = physical(e) if k == "aice0" else np.broadcast_to(physical(e)[:, None], w.shape)
            ch = (w != o) & ph
            assert (w[ph] >= 0).all()
            if ch.any():
                worst = min(worst, float(w[ch].min()))
        assert worst > 1e-6, (name, worst)
        print("STOP-PROBE-OK", name, worst, flush=True)
        return
    tc.load(e, f)
    sys.stdout.flush()
    e.ref.transport_remap(DT)          # the reference prints its diagnosis and ends the process (abort_ice: stop)
    print("STOP-NOT-REACHED", name, flush=True)


def gpu():
    """Every case on one context: the report equals the fixture's; then one good call equals the reference bit for bit."""
    fx = np.load(FIXTURE)
    e = tc.setup(*CFG)
    n = 0
    for name, c in CASES.items():
        f, digest = build(e, name)
        assert digest == str(fx[name + "_sha256"]), (name, "inputs differ from the ones the fixture was minted from")
        dev = {k: v[:e.nbl].copy() for k, v in f.items()}
        got = e.ctx.transport_remap(DT, dev)
        want = (int(fx[name + "_kind"]), int(fx[name + "_i"]), int(fx[name + "_j"]))
        print("STOP-REPORT", name, "library", got, "reference", want, flush=True)
        assert got == want == c["expect"], (name, got, want, c["expect"])
        if "dep" in c:     # the fixture's cell is the last failing one of the first failing block
            fails, _ = departure_failures(e, f)
            b0 = min(b for b, _i, _j in fails)
            last = [(i, j) for b, i, j in fails if b == b0][-1]
            assert last == want[1:] and b0 + 1 == int(fx[name + "_iblk"]), (name, fails, want)
        n += 1
    # the key is reset and nothing is left behind: the first trial of the bit-exact case on the SAME context
    rng = np.random.default_rng(20261004)
    dev = tc.load(e, tc.with_ghosts(e, tc.synth_state(e, rng, *tc.TRIALS[0])))
    nchk, moved, _ = tc.step_and_compare(e, dev, "good call after the failed ones")
    assert moved >= 6
    print("TRANSPORT-STOP-OK", n, nchk)


if __name__ == "__main__":
    if sys.argv[1] == "gpu":
        gpu()
    else:
        mint(sys.argv[2], sys.argv[1] == "probe")
