"""The cell map of the joined image under a tripole fold (cice4_amd/csrc/join.hip, option "skew_join_fold"), through
cice_debug_join_map_fold -- lib.join_map(..., fold=True): host code, no device.  The image is the one a domain without a
fold gets, except that the top ghost row of the top block row -- which the fold writes, with a sign, from no copy source --
keeps its own place on the image's top ring, as beyond an open edge."""
import numpy as np
import pytest

from cice4_amd import lib
from test_join_map import blocks_of, OPEN, CYCLIC, CLOSED, TRIPOLE

TRIPOLET = 4
# 2 x 2, 4 x 1, 1 x 4, 20 x 2 (blocks 15 wide), and last blocks padded in both directions whose top block row keeps ten rows
LAYOUTS = [(96, 70, 48, 35), (96, 70, 24, 70), (96, 70, 96, 18), (300, 120, 15, 60), (96, 70, 40, 30)]


@pytest.mark.parametrize("flavour", ["standalone", "auscom"])
@pytest.mark.parametrize("ns", [TRIPOLE, TRIPOLET], ids=["tripole", "tripoleT"])
@pytest.mark.parametrize("nxg,nyg,bsx,bsy", LAYOUTS)
def test_every_cell_of_the_blocks_has_its_place_in_the_image_under_a_fold(nxg, nyg, bsx, bsy, ns, flavour):
    m = lib.join_map(nxg, nyg, bsx, bsy, ew=CYCLIC, ns=ns, fold=True, flavour=flavour)
    bl = blocks_of(nxg, nyg, bsx, bsy)
    assert m is not None and m.shape == (len(bl), bsy + 2, bsx + 2)
    inx, iny = nxg + 2, nyg + 2
    seen = np.zeros(inx * iny, np.int64)
    top_row_cells = 0
    for b, i0, j0, ni, nj in bl:
        want = (np.arange(nj)[:, None] + j0 + 1) * inx + (np.arange(ni)[None, :] + i0 + 1)
        assert np.array_equal(m[b, 1:nj + 1, 1:ni + 1], want), (b, "physical cells")
        np.add.at(seen, want.ravel(), 1)
        pad = np.ones((bsy + 2, bsx + 2), bool)
        pad[:nj + 2, :ni + 2] = False
        assert (m[b][pad] == -1).all() and (m[b][~pad] >= 0).all(), (b, "padding")
        for j in range(nj + 2):
            for i in range(ni + 2):
                if 1 <= i <= ni and 1 <= j <= nj:
                    continue
                gi, gj = (i0 + i - 1) % nxg, j0 + j - 1
                if 0 <= gj < nyg:      # between blocks and across the cyclic east-west edge: the source's image cell
                    assert m[b, j, i] == (gj + 1) * inx + (gi + 1), (b, j, i, "ghost cell with a source")
                else:                  # below the grid, and the row the fold writes: its own place on the ring
                    assert m[b, j, i] == (j0 + j) * inx + (i0 + i), (b, j, i, "ghost cell on the ring")
                    if gj == nyg:
                        top_row_cells += 1
                        assert m[b, j, i] // inx == iny - 1, (b, j, i, "the image's top ring")
    nbx = (nxg - 1) // bsx + 1
    assert top_row_cells == nxg + 2 * nbx, "every cell of the top ghost row of the top block row, corners included"
    phys = np.zeros((iny, inx), bool)
    phys[1:-1, 1:-1] = True
    assert (seen.reshape(iny, inx)[phys] == 1).all() and (seen.reshape(iny, inx)[~phys] == 0).all(), "exactly once"
    # no physical cell is aliased by the row the fold writes
    assert not np.isin(m[m // inx == iny - 1], np.flatnonzero(phys.ravel())).any()


@pytest.mark.parametrize("ns", [TRIPOLE, TRIPOLET])
@pytest.mark.parametrize("nxg,nyg,bsx,bsy", LAYOUTS)
def test_the_plain_call_still_refuses_a_fold(nxg, nyg, bsx, bsy, ns):
    assert lib.join_map(nxg, nyg, bsx, bsy, ew=CYCLIC, ns=ns) is None
    assert lib.join_map(nxg, nyg, bsx, bsy, ew=CYCLIC, ns=ns, fold=False) is None


@pytest.mark.parametrize("ew,ns", [(CYCLIC, OPEN), (OPEN, OPEN), (CLOSED, CLOSED), (CYCLIC, CLOSED)])
@pytest.mark.parametrize("nxg,nyg,bsx,bsy", LAYOUTS + [(200, 50, 64, 16)])
def test_without_a_fold_the_flag_changes_nothing(nxg, nyg, bsx, bsy, ew, ns):
    a, b = lib.join_map(nxg, nyg, bsx, bsy, ew=ew, ns=ns), lib.join_map(nxg, nyg, bsx, bsy, ew=ew, ns=ns, fold=True)
    assert a is not None and np.array_equal(a, b)


def test_what_the_flag_does_not_admit():
    """one block, a cyclic north-south boundary; bad arguments are still told apart"""
    assert lib.join_map(96, 70, 96, 70, ew=CYCLIC, ns=TRIPOLE, fold=True) is None
    assert lib.join_map(96, 70, 48, 35, ew=CYCLIC, ns=CYCLIC, fold=True) is None
    with pytest.raises(lib.CiceError):
        lib.join_map(96, 70, 48, 35, ew=OPEN, ns=TRIPOLE, fold=True)      # (a fold needs a cyclic east-west boundary)
    with pytest.raises(lib.CiceError):
        lib.join_map(0, 70, 48, 35, fold=True)
