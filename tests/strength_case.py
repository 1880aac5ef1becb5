"""Inputs and bookkeeping shared by the tests of the strength stage that opens every evp(dt) (test_strength_case.py on the
CPU, test_gpu_strength.py on the device): ice_strength with asum_ridging and ridge_itd (ice_mechred.F90:1869-2036, :573,
:773-1098).  No GPU here.

synth.evp_state fills all five categories of every ice cell, mid-bin, with aice0 >= 0.01, so none of the routine's guards
ever sees an input.  CATALOGUE is a list of single-cell thickness distributions that sit ON those guards; seed_state
scatters it over the ocean cells of an evp_state; branch_counts restates, in numpy and from the inputs alone, which branch
each (cell, category) takes, so that a test can require every branch to be taken."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from cice4_amd import synth  # noqa: E402

NCAT = synth.NCAT
PUNY = 1.0e-11
GSTAR, MAXRAFT, HSTAR = 0.15, 1.0, 25.0
# (kstrength, krdg_partic, krdg_redist, mu_rdg): the five meaningful configurations, and mu_rdg away from its default
CONFIGS = ((1, 1, 1, 4.0), (1, 0, 0, 4.0), (1, 0, 1, 3.0), (1, 1, 0, 4.0), (0, 1, 1, 4.0), (1, 1, 1, 5.0), (1, 0, 1, 5.0))
EXP_FREE = ((1, 0, 0), (1, 0, 1))     # no exp() in ice_strength: bit for bit on any host
NXG, NYG = 24, 20                     # the grid of every seeded case


def cfg_id(c):
    return "k%d_p%d_r%d_mu%g" % c


def mid():
    """mid-bin thickness per category, the last bin capped at + 2 m"""
    top = synth.hin_max().copy()
    top[NCAT] = top[NCAT - 1] + 2.0
    return 0.5 * (top[:-1] + top[1:])


def _catalogue():
    m = mid()
    out = []

    def add(kind, a, h=None, aice0=None, v=None):
        a = np.array(a, np.float64)
        v = a * (m if h is None else np.array(h, np.float64)) if v is None else np.array(v, np.float64)
        out.append((kind, a, v, float(1.0 - a.sum() if aice0 is None else aice0)))

    add("open", [0.0] * NCAT, aice0=1.0)          # in the list only through its neighbours
    for n in range(NCAT):
        add(f"alone{n}", [0.93 if k == n else 0.0 for k in range(NCAT)])
    for n in range(NCAT):
        for kind, x in (("empty", 0.0), ("at_puny", PUNY), ("below_puny", 0.5 * PUNY), ("above_puny", 2.0 * PUNY)):
            add(f"{kind}{n}", [x if k == n else 0.23 for k in range(NCAT)])
    w = [[.1, .2, .3, .25, .15], [.15, .25, .3, .2, .1], [.02, .03, .05, .4, .5], [.5, .4, .05, .03, .02]]
    for a0 in (0.0, 0.5 * PUNY, PUNY):
        add("packed", w[0], aice0=a0)
    for a0 in (0.0, .02, .06, .149, .15, .151, .4, .8, .95):
        for k, wk in enumerate(w):
            add(f"gstar{k}", np.array(wk) * (1.0 - a0), aice0=a0)
    add("gstar4", [.01, .02, .03, .04, .9], aice0=0.0)
    add("raft", [0.18] * NCAT, h=[1.0, 1.0, 1.0 - 1e-12, 1.0 + 1e-12, 3.0])
    add("slab", [.1, .1, .1, .1, .5], h=[m[0], m[1], m[2], m[3], 120.0])      # hrmax = hrmin + puny
    add("film", [.3, .1, .1, .1, .1], h=[1e-13, m[1], m[2], m[3], m[4]])      # hi < puny
    add("trace", [1e-9, 1e-10, 3e-11, 0.0, 0.0])
    for kind, a, v, a0 in out:     # the reference divides by zero where nothing is above puny
        assert (a > PUNY).any() or a0 > PUNY, kind
    return out


CATALOGUE = _catalogue()


def catalogue_arrays():
    """(aicen, vicen, aice0) of the whole catalogue: (ncells, NCAT), (ncells, NCAT), (ncells,)"""
    return (np.array([c[1] for c in CATALOGUE]), np.array([c[2] for c in CATALOGUE]), np.array([c[3] for c in CATALOGUE]))


def as_row():
    """the bare catalogue as one row of physical cells inside a ring of empty ghost cells: the arguments of ice_strength
    (ilo, ihi, jlo, jhi, icells, indxi, indxj, aice, vice, aice0, aicen, vicen) on an (nx, 3) block"""
    a, v, a0 = catalogue_arrays()
    nc = len(a0)
    nx, ny = nc + 2, 3
    aicen = np.zeros((NCAT, ny, nx)); vicen = np.zeros((NCAT, ny, nx)); aice0 = np.ones((ny, nx))
    aicen[:, 1, 1:-1] = a.T
    vicen[:, 1, 1:-1] = v.T
    aice0[1, 1:-1] = a0
    aice, vice = aggregate(aicen, vicen)
    li = np.zeros(nx * ny, np.int32); lj = np.zeros(nx * ny, np.int32)
    li[:nc] = np.arange(nc) + 2
    lj[:nc] = 2
    return (2, nx - 1, 2, 2, nc, li, lj, aice, vice, aice0, aicen, vicen)


def aggregate(aicen, vicen):
    """aice, vice as aggregate_area sums them: in category order (category axis: -3)"""
    aice = np.zeros(aicen.shape[:-3] + aicen.shape[-2:]); vice = np.zeros_like(aice)
    for n in range(NCAT):
        aice = aice + aicen[..., n, :, :]
        vice = vice + vicen[..., n, :, :]
    return aice, vice


def global_coords(dom, b):
    """global (row, column) of every cell of block b, ghost cells included; columns wrap (the grids here are cyclic
    east-west), rows beyond the closed north and south boundaries are -1"""
    ii = (np.arange(dom["nx"]) - (dom["ilo"][b] - 1) + dom["i0"][b]) % dom["nxg"]
    jj = np.arange(dom["ny"]) - (dom["jlo"][b] - 1) + dom["j0"][b]
    jj = np.where((jj >= 0) & (jj < dom["nyg"]), jj, -1)
    return jj, ii


def seed_state(grid, dom, s, seed=2026101901):
    """Overwrite aicen, vicen, aice0, aice, vice of s (a synth.evp_state(..., cover="patchy") on the blocks of dom) with
    catalogue cells, in randomly chosen ocean cells of the GLOBAL grid: every catalogue cell at least 4 times, and at
    least one in the first and in the last physical row and column of every block.  Every copy of a global cell -- its
    owner's and the ghost cells of the neighbours -- gets the same values.  Returns which[nyg, nxg]: the catalogue index
    placed in a global cell, -1 where the state is left as it was."""
    rng = np.random.default_rng(seed)
    nxg, nyg, nb = dom["nxg"], dom["nyg"], dom["nblocks"]
    ocean = np.zeros((nyg, nxg), bool)
    edges = []
    for b in range(nb):
        jj, ii = global_coords(dom, b)
        js, is_ = slice(dom["jlo"][b] - 1, dom["jhi"][b]), slice(dom["ilo"][b] - 1, dom["ihi"][b])
        ocean[np.ix_(jj[js], ii[is_])] = grid["tmask"][b][js, is_] != 0
        edges += [(jj[js][:1], ii[is_]), (jj[js][-1:], ii[is_]), (jj[js], ii[is_][:1]), (jj[js], ii[is_][-1:])]
    which = np.full((nyg, nxg), -1, np.int64)
    places = []
    for rows, cols in edges:                  # one ocean cell on every edge of every block ...
        cand = [(j, i) for j in rows for i in cols if ocean[j, i] and (j, i) not in places]
        assert cand, "a block edge without a free ocean cell"
        places.append(cand[rng.integers(len(cand))])
    rest = [(j, i) for j, i in zip(*np.nonzero(ocean)) if (j, i) not in places]
    need = 4 * len(CATALOGUE)
    assert len(places) + len(rest) >= need, "the grid has too few ocean cells for four copies of the catalogue"
    places += [rest[k] for k in rng.permutation(len(rest))[:need - len(places)]]
    order = rng.permutation(len(CATALOGUE))   # ... and the catalogue dealt round and round over the places
    for k, (j, i) in enumerate(places):
        which[j, i] = order[k % len(CATALOGUE)]
    ca, cv, c0 = catalogue_arrays()
    for b in range(nb):
        jj, ii = global_coords(dom, b)
        w = np.where(jj[:, None] >= 0, which[np.ix_(np.maximum(jj, 0), ii)], -1)
        m = w >= 0
        for n in range(NCAT):
            s["aicen"][b, n][m] = ca[w[m], n]
            s["vicen"][b, n][m] = cv[w[m], n]
        s["aice0"][b][m] = c0[w[m]]
    s["aice"][...], s["vice"][...] = aggregate(s["aicen"], s["vicen"])
    return which


def seeded_case(ctx, bsx, bsy, nxg=NXG, nyg=NYG, seed=2026101901):
    """(dom, grid, s, which): an nxg x nyg grid (cyclic east-west, ocean up to its closed north and south boundaries,
    islands) cut into blocks of bsx x bsy, with a seeded patchy state"""
    dom = ctx.domain_create(nxg, nyg, bsx, bsy, ew=1, ns=0)
    grid = synth.block_fields(synth.global_grid(nxg, nyg, perturb=0.15, land_frac=0.05, land_rows=0), dom)
    s = synth.evp_state(grid, dom, cover="patchy")
    which = seed_state(grid, dom, s, seed)
    return dom, grid, s, which


def reachable(cfg):
    """the entries of branch_counts that a configuration can reach"""
    ks, kp, kr, _ = cfg
    if ks != 1:
        return ()                              # Hibler 79: none of the routine's guards
    r = ["open_le_puny", "cat_zero", "cat_le_puny", "raft_2hi", "raft_hi_plus_1", "raft_tie", "hi_below_puny"]
    if kp == 0:
        r += ["thorndike_below", "thorndike_straddle", "thorndike_above", "ice_with_zero_strength"]
    if kr == 0:
        r += ["hrmax_clamped"]
    return tuple(r)


def branch_counts(aicen, vicen, aice0, cfg):
    """(cell, n) pairs per branch of ice_strength under cfg, from the inputs alone; aicen, vicen (ncells, NCAT), aice0
    (ncells,).  thorndike_* restate asum_ridging's Gsum normalisation (:631-667) and count n = 0..NCAT (0: open water);
    thorndike_straddle is a list indexed by n.  ice_with_zero_strength counts cells: ice, and no category above puny
    that takes part in ridging (Thorndike's participation function gives open water all of it once aice0 >= Gstar)."""
    kp, kr = cfg[1], cfg[2]
    a, v = np.asarray(aicen, np.float64), np.asarray(vicen, np.float64)
    a0 = np.asarray(aice0, np.float64)
    nc = len(a0)
    G = np.zeros((nc, NCAT + 2))
    G[:, 1] = np.where(a0 > PUNY, a0, G[:, 0])
    for n in range(1, NCAT + 1):
        G[:, n + 1] = np.where(a[:, n - 1] > PUNY, G[:, n] + a[:, n - 1], G[:, n])
    work = 1.0 / G[:, NCAT + 1]
    for n in range(NCAT + 1):
        G[:, n + 1] = G[:, n + 1] * work
    g, gm = G[:, 1:], G[:, :-1]                # Gsum(n), Gsum(n-1) for n = 0..NCAT
    below, straddle, above = g < GSTAR, (g >= GSTAR) & (gm < GSTAR), gm >= GSTAR
    has = a > PUNY
    with np.errstate(divide="ignore", invalid="ignore"):
        hi = np.where(has, v / np.where(has, a, 1.0), 0.0)
    tiny = has & (hi < PUNY)
    if kr == 1:
        hi = np.where(has, np.maximum(hi, PUNY), hi)
    h2, h1 = 2.0 * hi, hi + MAXRAFT
    hrmin = np.minimum(h2, h1)
    clamped = has & (2.0 * np.sqrt(HSTAR * hi) < hrmin + PUNY)
    if kp == 0:     # apartic(n) > 0 for an ice category: some of [Gsum(n-1), Gsum(n)) lies below Gstar
        takes_part = has & (gm[:, 1:] < GSTAR) & (g[:, 1:] > gm[:, 1:])
    else:
        takes_part = has
    return dict(
        open_le_puny=int((a0 <= PUNY).sum()), cat_zero=int((a == 0.0).sum()), cat_le_puny=int(((a > 0.0) & ~has).sum()),
        thorndike_below=int(below.sum()), thorndike_straddle=[int(straddle[:, n].sum()) for n in range(NCAT + 1)],
        thorndike_above=int(above.sum()),
        raft_2hi=int((has & (h2 < h1)).sum()), raft_hi_plus_1=int((has & (h2 > h1)).sum()), raft_tie=int((has & (h2 == h1)).sum()),
        hrmax_clamped=int(clamped.sum()), hi_below_puny=int(tiny.sum()),
        ice_with_zero_strength=int(((a > 0.0).any(axis=1) & ~takes_part.any(axis=1)).sum()))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))
