"""The cell map of the image that a one-task domain of several blocks is joined into for the K-subcycle sweeps
(cice4_amd/csrc/join.hip, option "skew_join"), through cice_debug_join_map: host code, no device."""
import numpy as np
import pytest

from cice4_amd import lib

OPEN, CYCLIC, CLOSED, TRIPOLE = 0, 1, 2, 3


def blocks_of(nxg, nyg, bsx, bsy):
    """(block, i0, j0, columns, rows) in the library's order: i fastest (source/ice_blocks.F90:163-172)"""
    nbx, nby = (nxg - 1) // bsx + 1, (nyg - 1) // bsy + 1
    return [(jb * nbx + ib, ib * bsx, jb * bsy, min(bsx, nxg - ib * bsx), min(bsy, nyg - jb * bsy))
            for jb in range(nby) for ib in range(nbx)]


# 2 x 2, 4 x 1, 1 x 4, 20 x 2 (blocks 15 wide), and last blocks padded in both directions
LAYOUTS = [(96, 70, 48, 35), (96, 70, 24, 70), (96, 70, 96, 18), (300, 120, 15, 60), (200, 50, 64, 16), (26, 22, 12, 10)]


@pytest.mark.parametrize("ew", [CYCLIC, OPEN, CLOSED])
@pytest.mark.parametrize("nxg,nyg,bsx,bsy", LAYOUTS)
def test_every_cell_of_the_blocks_has_its_place_in_the_image(nxg, nyg, bsx, bsy, ew):
    m = lib.join_map(nxg, nyg, bsx, bsy, ew=ew, ns=OPEN)
    bl = blocks_of(nxg, nyg, bsx, bsy)
    assert m is not None and m.shape == (len(bl), bsy + 2, bsx + 2)
    inx, iny = nxg + 2, nyg + 2
    seen = np.zeros(inx * iny, np.int64)
    for b, i0, j0, ni, nj in bl:
        # physical cells (0-based local rows 1 .. nj, columns 1 .. ni) sit at their global place, ring excluded
        want = (np.arange(nj)[:, None] + j0 + 1) * inx + (np.arange(ni)[None, :] + i0 + 1)
        assert np.array_equal(m[b, 1:nj + 1, 1:ni + 1], want), (b, "physical cells")
        np.add.at(seen, want.ravel(), 1)
        # padding: everything beyond the ghost ring that lies around the physical cells
        pad = np.ones((bsy + 2, bsx + 2), bool)
        pad[:nj + 2, :ni + 2] = False
        assert (m[b][pad] == -1).all() and (m[b][~pad] >= 0).all(), (b, "padding")
        # ghost cells: the image cell of their source -- the physical cell with the same global index, wrapped across a
        # cyclic east-west edge -- or, beyond an open / closed edge (no source), their own place on the image's ring
        for j in range(nj + 2):
            for i in range(ni + 2):
                if 1 <= i <= ni and 1 <= j <= nj:
                    continue
                gi, gj = i0 + i - 1, j0 + j - 1
                if ew == CYCLIC:
                    gi %= nxg
                inside = 0 <= gi < nxg and 0 <= gj < nyg
                place = (gj + 1) * inx + (gi + 1) if inside else (j0 + j) * inx + (i0 + i)
                assert m[b, j, i] == place, (b, j, i, "ghost cell")
    phys = np.zeros((iny, inx), bool)
    phys[1:-1, 1:-1] = True
    assert (seen.reshape(iny, inx)[phys] == 1).all() and (seen.reshape(iny, inx)[~phys] == 0).all(), "exactly once"


@pytest.mark.parametrize("nxg,nyg,bsx,bsy,ew,ns", [(96, 70, 48, 35, CYCLIC, TRIPOLE), (96, 70, 48, 35, CYCLIC, 4),
                                                    (96, 70, 48, 35, CYCLIC, CYCLIC), (96, 70, 48, 35, OPEN, CYCLIC),
                                                    (96, 70, 96, 70, CYCLIC, OPEN), (96, 70, 100, 80, CLOSED, CLOSED)])
def test_layouts_that_are_not_joined(nxg, nyg, bsx, bsy, ew, ns):
    """a fold over several blocks and a cyclic north-south boundary keep today's path; one block has nothing to join"""
    assert lib.join_map(nxg, nyg, bsx, bsy, ew=ew, ns=ns) is None


def test_bad_arguments_are_told_apart_from_layouts_that_do_not_qualify():
    with pytest.raises(lib.CiceError):
        lib.join_map(0, 70, 48, 35)
    with pytest.raises(lib.CiceError):
        lib.join_map(96, 70, 48, 35, ew=7)
    m = lib.join_map(96, 70, 48, 35, ew=CYCLIC, ns=CLOSED)
    assert m is not None and m.min() == 0 and m.max() == 98 * 72 - 1      # the corners of the image's ring


def test_both_flavours_have_the_map():
    a, b = lib.join_map(200, 50, 64, 16), lib.join_map(200, 50, 64, 16, flavour="auscom")
    assert np.array_equal(a, b)
