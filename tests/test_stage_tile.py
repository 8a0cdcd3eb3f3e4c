"""bdg_stage_tile: the one workgroup -> tile mapping of the triangle solver's stage kernels (csrc/hip/sw2d_stage_tile.hpp), called
on the host. Workgroups go to the eight XCDs round robin; each XCD owns one contiguous chunk of tiles and walks it from its low
end (back = 0) or from its high end (back = 1). No GPU."""
import pytest

from blitzdg_amd import _capi

GRIDS = range(1, 201)


def tiles(grid, back):
    return [int(_capi.lib.bdg_stage_tile(b, grid, back)) for b in range(grid)]


def closed_form(block, grid):
    """The remap as the kernels spelled it before they shared one function."""
    xcd, q8, r8 = block % 8, grid // 8, grid % 8
    return (xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8) + block // 8


@pytest.mark.parametrize("back", [0, 1])
def test_every_grid_is_a_permutation(back):
    for grid in GRIDS:
        assert sorted(tiles(grid, back)) == list(range(grid)), grid


def test_forward_is_the_closed_form_of_the_kernels():
    for grid in GRIDS:
        assert tiles(grid, 0) == [closed_form(b, grid) for b in range(grid)], grid


def test_an_xcd_keeps_its_tiles_and_walks_them_from_the_other_end():
    for grid in GRIDS:
        fwd, bwd = tiles(grid, 0), tiles(grid, 1)
        for xcd in range(8):
            f, b = fwd[xcd::8], bwd[xcd::8]           # in the order the XCD's workgroups are dispatched
            assert set(f) == set(b), (grid, xcd)
            assert b == f[::-1], (grid, xcd)
            assert f == list(range(f[0], f[0] + len(f))) if f else True, (grid, xcd)   # one contiguous chunk, ascending


def test_any_nonzero_flag_means_backward():
    assert tiles(37, 7) == tiles(37, 1)
