// sw2d_stage_tile.hpp -- which tile of elements a workgroup of a stage launch takes: the one mapping every stage kernel of the
// triangle solver uses, also callable on the host (bdg_stage_tile, tests/test_stage_tile.py). No HIP types.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BDG_STAGE_TILE_HD __host__ __device__
#else
#define BDG_STAGE_TILE_HD
#endif

namespace bdg_dev {

// XCD-aware block remap. Workgroups go to the eight XCDs round robin (block % 8); each XCD gets one contiguous chunk of the
// numbers 0 .. grid-1 (the first grid % 8 chunks are one longer), so consecutive tiles of elements -- which share faces, hence
// gather lines -- meet in the same XCD's L2.
// first number and length of the chunk of the XCD `block` runs on
BDG_STAGE_TILE_HD inline unsigned stage_chunk_first(unsigned block, unsigned grid) {
    const unsigned xcd = block % 8u, q8 = grid / 8u, r8 = grid % 8u;
    return xcd < r8 ? xcd * (q8 + 1u) : r8 * (q8 + 1u) + (xcd - r8) * q8;
}
BDG_STAGE_TILE_HD inline unsigned stage_chunk_length(unsigned block, unsigned grid) {
    return grid / 8u + (block % 8u < grid % 8u ? 1u : 0u);
}

// The tile of workgroup `block` in a grid of one workgroup per tile. Bijective on 0 .. grid-1 for every grid size.
// back = 0: the XCD walks its chunk from the low end, back = 1: the same chunk from the high end. A whole-mesh stage launch
// that walks against the direction of the launch before it starts on the tiles that launch touched last: while the bytes moved
// since then stay below the Infinity Cache's size, their rows are read from the cache instead of from HBM.
BDG_STAGE_TILE_HD inline unsigned stage_tile(unsigned block, unsigned grid, unsigned back) {
    const unsigned at = block / 8u;
    return stage_chunk_first(block, grid) + (back ? stage_chunk_length(block, grid) - 1u - at : at);
}

// Kernels whose waves walk several tiles keep their (logical) walk and mirror it inside the XCD's range of tiles [lo, hi):
// logical tile t is tile lo + hi - 1 - t, so the tiles a forward launch took last are the first of a backward one.
BDG_STAGE_TILE_HD inline unsigned stage_tile_mirrored(unsigned t, unsigned lo, unsigned hi, unsigned back) {
    return back ? lo + hi - 1u - t : t;
}

} // namespace bdg_dev
