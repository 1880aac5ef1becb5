"""One set of device halo updates in its own process (the two environment switches of the halo code are read once per
process or per context).  Started by tests/test_gpu_halo.py:

    python tests/halo_device_case.py device   <domain>   cice_halo_update_ex_{r8,r4,i4} and cice_halo_update_dev_ex_r8:
                                                         every type x location x kind, 1 / 3 / 65 levels, two fill values
    python tests/halo_device_case.py blocked  <domain>   cice_halo_update_blocked_* and cice_halo_update_strided_r8 on HOST
                                                         arrays: on the device with CICE4_AMD_HALO_HOST_ON_DEVICE=1 in the
                                                         environment (gathered frame or whole field), else on the host
    python tests/halo_device_case.py selfcomm <domain>   the 'device' and 'blocked' calls with CICE4_AMD_SELF_COMM=1: copies
                                                         between blocks travel as pack -> message to the own rank -> unpack
    python tests/halo_device_case.py switch   <domain>   Halo::update_fold on either side of its switch from the one-workgroup
                                                         LDS kernel to the four kernels with a buffer in device memory
    python tests/halo_device_case.py ranks    <ns>       ranks as threads of this process: fold rows between ranks
    python tests/halo_device_case.py facts    <domain>   no device: what the cases above rely on (symmetric pairs, frame size)

Expected values: lib.Context.apply_halo_lists, the one-rank lists applied in numpy (plain indexing, one average per pair
in the field's own type), which tests/test_boundary.py holds equal to the compiled reference.  A halo update copies,
negates and halves: every comparison is np.array_equal.  Prints 'HALO-OK <n checks>' (and, in 'blocked' mode,
'HALO-DIGEST <sha256 of every updated array>') on success.
"""
import hashlib
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cice4_amd import lib  # noqa: E402

# nxg, nyg, bsx, bsy, ew, ns
GRID = {
    "u2x2": (24, 20, 12, 10, 1, 3),         # 2 x 2 blocks under the fold through U points
    "t2x2": (24, 20, 12, 10, 1, 4),         # ... and through T points
    "pad3x3": (26, 22, 12, 10, 1, 3),       # 3 x 3 blocks, last block column and row padded
    "tiny": (10, 6, 5, 3, 1, 3),            # blocks so small that the frame is more than half the field
    "lds-u": (128, 12, 128, 12, 1, 3),      # one block: one level of the fold buffer is 2 x 128 elements
    "lds-t": (128, 12, 128, 12, 1, 4),      # 3 x 128
    "elim": (26, 22, 12, 10, 1, 3),         # pad3x3 without a top-row block and without the interior block
    "closed": (24, 20, 12, 10, 2, 2),       # no neighbour beyond a closed edge: the lists of 'open'
    "open": (24, 20, 12, 10, 0, 0),
}
ELIMINATED = {"elim": (4, 7)}               # global block ids (row-major, 3 x 3): the centre block, the middle top-row block
FILL = {np.dtype(np.float64): -3.5, np.dtype(np.float32): -3.5, np.dtype(np.int32): 7}
DTYPES = (np.float64, np.float32, np.int32)
LOCS, KINDS = (1, 2, 3, 4), (1, 2, 3)
LDS_BYTES = 64 * 1024                       # Halo::update_fold: the LDS kernel while the fold buffer fits into this
FRAME_ENV, SELF_ENV = "CICE4_AMD_HALO_HOST_ON_DEVICE", "CICE4_AMD_SELF_COMM"
# cells in a copy, fill or fold list / cells of the field: which branch of halo_host_blocked the domain takes
FRAME_CELLS = {"u2x2": (324, 672), "t2x2": (324, 672), "tiny": (114, 140)}


def rand(rng, shape, dtype):
    if dtype == np.int32:
        return rng.integers(-1000, 1001, shape).astype(np.int32)
    return rng.uniform(-2.0, 2.0, shape).astype(dtype)


def create(c, name, **kw):
    nxg, nyg, bsx, bsy, ew, ns = GRID[name]
    if name in ELIMINATED:
        owner = np.zeros(((nxg - 1) // bsx + 1) * ((nyg - 1) // bsy + 1), np.int32)
        owner[list(ELIMINATED[name])] = -1
        return c.domain_create_map(nxg, nyg, bsx, bsy, owner, ew=ew, ns=ns)
    return c.domain_create(nxg, nyg, bsx, bsy, ew=ew, ns=ns, **kw)


class Lists:
    """the one-rank lists of a context's domain, and what they say about it"""

    def __init__(self, c, name):
        self.c, self.name = c, name
        d = c.domain()
        self.nxg = GRID[name][0]
        self.n = c.nblocks * c.ny * c.nx
        self.shape = (c.nblocks, c.ny, c.nx)
        self.hsrc, self.hdst, self.hfill, self.rsrc, self.rdst = d["hsrc"], d["hdst"], d["hfill"], d["rsrc"], d["rdst"]
        self.lsrc, self.bidx = c.domain_list("fold_lsrc"), c.domain_list("fold_bidx")
        self.fold = len(self.lsrc) > 0
        self.rows = int(self.bidx.max()) // self.nxg + 1 if self.fold else 0
        self.dst = {l: c.domain_list("fold_dst", l) for l in LOCS}
        self.src = {l: c.domain_list("fold_src", l) for l in LOCS}
        self.lo = {l: c.domain_list("fold_lo", l) for l in LOCS}
        self.hi = {l: c.domain_list("fold_hi", l) for l in LOCS}

    def written(self, loc):
        """mask of the cells an update of a field at `loc` may write"""
        m = np.zeros(self.n, bool)
        for v in (self.hdst, self.hfill, self.rdst, self.dst[loc]):
            m[v] = True
        return m

    def frame(self):
        """cells that occur in any list: what halo_host_blocked gathers"""
        m = np.zeros(self.n, bool)
        for v in (self.hsrc, self.hdst, self.hfill, self.rsrc, self.rdst, self.lsrc, *self.dst.values()):
            m[v] = True
        return int(m.sum())

    def buffer_level(self, a0, fill):
        """the fold buffer of one level before the symmetric pairs are averaged"""
        buf = np.full(self.rows * self.nxg, fill, a0.dtype)
        buf[self.bidx] = a0.reshape(-1)[self.lsrc]
        return buf


def facts(L):
    """What the comparisons rely on, from the lists alone (no device).  Returns the number of checks."""
    n, name, half = 0, L.name, L.nxg // 2
    ns = GRID[name][5]
    assert L.fold == (ns in (3, 4)), name
    if L.fold:
        # symmetric pairs by location (centre, NE corner, N face, E face): the U-fold has them where u, v and the N-face
        # fields lie on the fold, the T-fold at centres and E faces
        pairs = tuple(len(L.lo[l]) for l in LOCS)
        assert pairs == ((0, half - 1, half, 0) if ns == 3 else (half - 1, 0, 0, half)), (name, pairs)
        assert L.rows == (2 if ns == 3 else 3)
        if name in ("u2x2", "t2x2"):
            assert pairs == ((0, 11, 12, 0) if ns == 3 else (11, 0, 0, 12))
            assert all(len(L.dst[l]) in (28, 56) for l in LOCS), [len(L.dst[l]) for l in LOCS]
        for l in LOCS:
            assert len(L.dst[l]) > 0 and len(L.lo[l]) == len(L.hi[l]) and len(L.dst[l]) == len(L.src[l])
        n += 2 + len(LOCS)
    if name in ELIMINATED:
        # the eliminated top-row block leaves a gap in the buffer, and every location copies cells out of the gap
        gap = np.ones(L.rows * L.nxg, bool); gap[L.bidx] = False
        assert gap.any() and len(L.hfill) > 0
        assert all(gap[L.src[l]].any() for l in LOCS)
        n += 2
    if name in FRAME_CELLS:
        assert (L.frame(), L.n) == FRAME_CELLS[name], (name, L.frame(), L.n)
        n += 1
    if name == "closed":
        o = lib.Context(); create(o, "open")
        LO = Lists(o, "open")
        for k in ("hsrc", "hdst", "hfill", "rsrc", "rdst", "lsrc"):
            assert np.array_equal(getattr(L, k), getattr(LO, k)), k
        assert len(L.hsrc) > 0
        n += 1
    return n


def expected(L, a, loc, fill):
    """{kind: updated copy of a (nlev, nblocks, ny, nx)}; asserts that no comparison against them can be vacuous"""
    want = {k: L.c.apply_halo_lists(a.copy(), loc, k, fill) for k in KINDS}
    for k in KINDS:
        assert not np.array_equal(want[k], a), ("update changes nothing", L.name, a.dtype, loc, k)
    if L.fold:
        assert not np.array_equal(want[1], want[2]), ("scalar == vector", L.name, a.dtype, loc)
        assert np.array_equal(want[2], want[3])      # vector and angle: the same sign
        if a.dtype == np.int32 and len(L.lo[loc]):   # nint() of a half: an odd sum among the symmetric pairs
            buf = L.buffer_level(a[0], fill)
            assert ((buf[L.lo[loc]] + buf[L.hi[loc]]) % 2 != 0).any(), ("no odd pair", L.name, loc)
    if L.name in ELIMINATED:                         # the gap of the buffer comes out as sgn * fill
        gap = np.ones(L.rows * L.nxg, bool); gap[L.bidx] = False
        cells = L.dst[loc][gap[L.src[loc]] & ~np.isin(L.src[loc], np.concatenate([L.lo[loc], L.hi[loc]]))]
        assert len(cells) and (want[2][0].reshape(-1)[cells] == a.dtype.type(-fill)).all()
        assert (want[1][0].reshape(-1)[cells] == a.dtype.type(fill)).all()
    return want


def same(L, got, want, a, loc, tag):
    """got == want bit for bit, and cells outside the destination lists are the input's"""
    got, want, a = (x.reshape(-1, L.n) for x in (got, want, a))
    assert got.dtype == want.dtype
    assert np.array_equal(got, want), (tag, np.argwhere(got != want)[:6].tolist())
    keep = ~L.written(loc)
    assert keep.any() and np.array_equal(got[:, keep], a[:, keep]), (tag, "a cell outside the lists changed")
    return 1


def to_blocked(a):      # a copy of (nlev, nb, ny, nx) in the reference's layout (nb, nlev, ny, nx)
    return np.array(a.transpose(1, 0, 2, 3), order="C", copy=True)


def from_blocked(a):
    return np.array(a.transpose(1, 0, 2, 3), order="C", copy=True)


def run_level_major(c, L, rng, levels=(1, 3, 65), resident=True):
    """halo_update (host array through the device) and halo_update_resident against numpy"""
    n = 0
    for dtype in DTYPES:
        for loc in LOCS:
            for nlev in levels:
                for fill in (0, FILL[np.dtype(dtype)]):
                    a = rand(rng, (nlev,) + L.shape, dtype)
                    want = expected(L, a, loc, fill)
                    for kind in KINDS:
                        tag = (L.name, np.dtype(dtype).name, loc, kind, nlev, fill)
                        got = a.copy(); c.halo_update(got, loc, kind, fill)
                        n += same(L, got, want[kind], a, loc, ("halo_update",) + tag)
                        if resident and dtype == np.float64:
                            got = a.copy(); c.halo_update_resident(got, loc, kind, fill)
                            n += same(L, got, want[kind], a, loc, ("halo_update_resident",) + tag)
    return n


def run_blocked(c, L, rng, digest):
    """halo_update_blocked (1 and 3 levels, every type) and halo_update_strided (a section of a 4-d array) against numpy"""
    n = 0
    nb, ny, nx = L.shape
    for dtype in DTYPES:
        for loc in LOCS:
            for nlev in (1, 3):
                fill = FILL[np.dtype(dtype)] if nlev == 3 else 0
                a = rand(rng, (nlev,) + L.shape, dtype)
                want = expected(L, a, loc, fill)
                for kind in KINDS:
                    blk = to_blocked(a)
                    c.halo_update_blocked(blk, loc, kind, fill)
                    digest.update(blk.tobytes())
                    n += same(L, from_blocked(blk), want[kind], a, loc,
                              ("halo_update_blocked", L.name, np.dtype(dtype).name, loc, kind, nlev, fill))
    for loc in LOCS:        # trcrn(:,:,1:2,:,:) of an array with three tracers: the third must come back untouched
        for fill in (0, FILL[np.dtype(np.float64)]):
            base = rand(rng, (nb, 2, 3, ny, nx), np.float64)
            a = from_blocked(base[:, :, 0:2].reshape(nb, 4, ny, nx))
            want = expected(L, a, loc, fill)
            for kind in KINDS:
                arr = base.copy()
                c.halo_update_strided(arr[:, :, 0:2], loc, kind, fill)
                digest.update(arr.tobytes())
                assert np.array_equal(arr[:, :, 2], base[:, :, 2]), ("strided: a level outside the section changed", loc, kind)
                n += same(L, from_blocked(np.ascontiguousarray(arr[:, :, 0:2]).reshape(nb, 4, ny, nx)), want[kind], a, loc,
                          ("halo_update_strided", L.name, loc, kind, fill))
    return n


def lds_levels(L):
    """{dtype: (most levels on the LDS path, fewest on the four-kernel path)} of a domain's fold buffer"""
    out = {}
    for dtype in DTYPES:
        per_level = L.rows * L.nxg * np.dtype(dtype).itemsize
        out[dtype] = (LDS_BYTES // per_level, LDS_BYTES // per_level + 1)
    return out


def run_switch(c, L, rng, small):
    """either side of the switch in Halo::update_fold, every location x kind; then, on the small domain `small`, an
    LDS-sized call straight after a four-kernel call that had to grow the buffer in device memory"""
    n = 0
    lv = lds_levels(L)
    want_lv = {"lds-u": {np.float64: (32, 33), np.float32: (64, 65), np.int32: (64, 65)},
               "lds-t": {np.float64: (21, 22), np.float32: (42, 43), np.int32: (42, 43)}}[L.name]
    assert lv == want_lv, lv
    assert L.rows * L.nxg * 32 * 8 == LDS_BYTES or L.name != "lds-u"      # r8, U-fold: the largest allocation exactly
    for dtype in DTYPES:
        for nlev, on_lds in zip(lv[dtype], (True, False)):
            assert (L.rows * L.nxg * nlev * np.dtype(dtype).itemsize <= LDS_BYTES) == on_lds
            for loc in LOCS:
                fill = FILL[np.dtype(dtype)] if loc % 2 else 0
                a = rand(rng, (nlev,) + L.shape, dtype)
                want = expected(L, a, loc, fill)
                for kind in KINDS:
                    got = a.copy(); c.halo_update(got, loc, kind, fill)
                    n += same(L, got, want[kind], a, loc, ("switch", L.name, np.dtype(dtype).name, nlev, loc, kind, fill))
    c2 = lib.Context(); c2.sync()
    create(c2, small)
    S = Lists(c2, small)
    per_level = S.rows * S.nxg * 8
    for nlev in (200, 65, 300, 65):     # four kernels (the buffer is made), LDS, four kernels (it grows), LDS
        assert (per_level * nlev <= LDS_BYTES) == (nlev == 65)
        for loc, kind in ((2, 2), (1, 1)):
            a = rand(rng, (nlev,) + S.shape, np.float64)
            want = expected(S, a, loc, -3.5)
            got = a.copy(); c2.halo_update(got, loc, kind, -3.5)
            n += same(S, got, want[kind], a, loc, ("growth", small, nlev, loc, kind))
    return n


def run_ranks(ns, npx, npy, link):
    """R = npx x npy ranks (threads, one context each) on the 24 x 20 grid in blocks of 12 x 10: every block of every rank
    must come out as the block of the same global id of the one-rank domain updated in numpy"""
    nxg, nyg, bsx, bsy = 24, 20, 12, 10
    R = npx * npy
    one = lib.Context()
    dom1 = one.domain_create(nxg, nyg, bsx, bsy, ew=1, ns=ns)
    L = Lists(one, "u2x2" if ns == 3 else "t2x2")
    gid1 = [int(g) for g in dom1["gid"]]
    rng = np.random.default_rng(100 + ns)
    calls = []
    for dtype in DTYPES:
        for loc in (1, 2):          # U-fold: pairs at 2; T-fold: pairs at 1
            for nlev in (1, 3):
                a = rand(rng, (nlev,) + L.shape, dtype)
                want = expected(L, a, loc, 0)
                calls += [("update", a, want[kind], loc, kind) for kind in (1, 2)]
    a = rand(rng, (3,) + L.shape, np.float64)
    calls.append(("blocked", a, expected(L, a, 2, 0)[2], 2, 2))
    bar = threading.Barrier(R)
    done, errs = [0] * R, []

    def rank_fn(r):
        try:
            c = lib.Context(device=0); c.sync()
            bar.wait(timeout=120)            # every context (and its stream) exists before any domain is made
            dom = c.domain_create(nxg, nyg, bsx, bsy, ew=1, ns=ns, rank=r, npx=npx, npy=npy)
            assert dom["nblocks"] == 4 // R and dom["nsend"] >= 1
            top = any(int(g) >= 2 for g in dom["gid"])       # the rank holds a block of the top block row
            assert (len(c.halo_msgs(2)) > 0) == (len(c.halo_msgs(3)) > 0) == top, (r, "fold messages")
            c.comm_init_local(link, r, R)
            idx = [gid1.index(int(g)) for g in dom["gid"]]
            for what, a, want, loc, kind in calls:
                mine = np.ascontiguousarray(a[:, idx])
                if what == "blocked":
                    blk = to_blocked(mine)
                    c.halo_update_blocked(blk, loc, kind, 0)
                    mine = from_blocked(blk)
                else:
                    c.halo_update(mine, loc, kind, 0)
                assert np.array_equal(mine, want[:, idx]), (r, what, a.dtype.name, a.shape[0], loc, kind)
                done[r] += 1
            bar.wait(timeout=120)
        except BaseException as e:           # noqa: BLE001 -- reported by the main thread
            errs.append((r, repr(e)))
            bar.abort()

    th = [threading.Thread(target=rank_fn, args=(r,)) for r in range(R)]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    assert not errs, errs
    assert all(d == len(calls) for d in done), done
    return sum(done)


def main():
    mode, name = sys.argv[1:3]
    rng = np.random.default_rng(2024)
    nchk = 0
    if mode == "ranks":
        ns = int(name)
        for k, (npx, npy) in enumerate(((2, 1), (2, 2))):   # both ranks fold; two of four ranks fold
            nchk += run_ranks(ns, npx, npy, 7000 + 10 * ns + k)
        print("HALO-OK", nchk)
        return
    if mode == "facts":
        c = lib.Context(); create(c, name)
        print("HALO-OK", facts(Lists(c, name)))
        return
    if mode == "selfcomm":
        assert os.environ.get(SELF_ENV) == "1"
        c = lib.Context(); c.sync()
        dom = create(c, name)
        assert dom["nsend"] == 1 and dom["nsend_elems"] == dom["nrecv_elems"] > 0
        c.comm_init(c.comm_unique_id(), 0, 1)
        del os.environ[SELF_ENV]            # read by cice_domain_create*: the expected values need the plain lists
        plain = lib.Context(); create(plain, name)
        L = Lists(plain, name)
        assert len(L.hsrc) > dom["ncopy"]   # the copies between blocks have left the on-rank list
        nchk += facts(L)
        nchk += run_level_major(c, L, rng)
        nchk += run_blocked(c, L, rng, hashlib.sha256())
        print("HALO-OK", nchk)
        return
    assert SELF_ENV not in os.environ
    c = lib.Context()
    if mode != "blocked" or FRAME_ENV in os.environ:
        c.sync()
    create(c, name)
    L = Lists(c, name)
    nchk += facts(L)
    if mode == "device":
        assert FRAME_ENV not in os.environ
        nchk += run_level_major(c, L, rng)
    elif mode == "blocked":
        if name in FRAME_CELLS:     # the branch of halo_host_blocked this domain takes on the device
            assert (2 * L.frame() <= L.n) == (name != "tiny")
        digest = hashlib.sha256()
        nchk += run_blocked(c, L, rng, digest)
        print("HALO-DIGEST", digest.hexdigest())
    elif mode == "switch":
        nchk += run_switch(c, L, rng, "u2x2" if name == "lds-u" else "t2x2")
    else:
        raise SystemExit(f"unknown mode {mode}")
    print("HALO-OK", nchk)


if __name__ == "__main__":
    main()
