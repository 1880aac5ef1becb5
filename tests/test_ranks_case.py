"""tests/ranks_case.py's owned / assemble / assemble_blocks -- what turns the ranks' partial results into the one array
that the multi-rank GPU tests compare -- on domains cut without a device: every global cell comes from the one rank
that owns it, and from nowhere else."""
import numpy as np
import pytest

from cice4_amd import lib
import ranks_case

NOT_A_CELL = -1.0        # ghost cells and overlap rows: never a global cell id


def _fill(dom, ids):
    """a rank's block array: the global cell id on the cells it owns, NOT_A_CELL on ghost cells and overlap rows"""
    f = np.full((dom["nblocks"], dom["ny"], dom["nx"]), NOT_A_CELL)
    for b in range(dom["nblocks"]):
        for j in range(dom["own_jlo"][b], dom["own_jhi"][b] + 1):          # (1-based, as the library counts)
            for i in range(dom["ilo"][b], dom["ihi"][b] + 1):
                f[b, j - 1, i - 1] = ids[dom["j0"][b] + j - dom["jlo"][b], dom["i0"][b] + i - dom["ilo"][b]]
    return f


def _slabs(nxg, nyg):
    return [lib.Context().domain_create_slabs(nxg, nyg, 3, ew=1, ns=0, rank=r, nranks=3, overlap=4) for r in range(3)]


def _tasks(nxg, nyg, bx, by):
    return [lib.Context().domain_create(nxg, nyg, nxg // (2 * bx), nyg // (2 * by), ew=1, ns=0, rank=r, npx=2, npy=2) for r in range(4)]


@pytest.mark.parametrize("cut,assemble,nblocks", [(_slabs, ranks_case.assemble, 1),
                                                  (lambda nxg, nyg: _tasks(nxg, nyg, 1, 1), ranks_case.assemble_blocks, 1),
                                                  (lambda nxg, nyg: _tasks(nxg, nyg, 2, 1), ranks_case.assemble_blocks, 2)],
                         ids=["3-slabs-overlap4", "2x2-tasks", "2x2-tasks-2x1-blocks"])
def test_every_global_cell_comes_from_its_owner(cut, assemble, nblocks):
    nxg, nyg = 12, 36
    ids = np.arange(nyg * nxg, dtype=float).reshape(nyg, nxg)
    doms = cut(nxg, nyg)
    assert all(d["nblocks"] == nblocks for d in doms)
    out = [(d, {"f": _fill(d, ids)}) for d in doms]
    assert any((s["f"] == NOT_A_CELL).any() for _, s in out)
    got = assemble(out, "f", nxg, nyg)
    assert np.array_equal(got, ids)
    assert (got != 0)[ids != 0].all()                     # every cell written
    for r, (d, s) in enumerate(out):                      # one owned cell of one rank changed: that cell, and only that one
        b = d["nblocks"] - 1
        j, i = int(d["own_jhi"][b]), int(d["ilo"][b])
        cell = int(s["f"][b, j - 1, i - 1])
        s["f"][b, j - 1, i - 1] = -7.0
        got = assemble(out, "f", nxg, nyg)
        assert np.argwhere(got != ids).tolist() == [[cell // nxg, cell % nxg]] and got[cell // nxg, cell % nxg] == -7.0, r
        s["f"][b, j - 1, i - 1] = cell
    # a one-rank domain through `owned` (what the GPU tests compare with)
    one = lib.Context().domain_create_slabs(nxg, nyg, 3, ew=1, ns=0, overlap=4)
    assert one["nblocks"] == 3 and np.array_equal(ranks_case.owned(one, _fill(one, ids)), ids)
