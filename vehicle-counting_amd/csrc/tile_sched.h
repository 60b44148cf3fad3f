// Chunk schedule of the claimed-tile persistent kernels (c3_fused.hip, bneck_fused.hip): pure integer functions, no HIP header, host and
// device alike (tests/native/tile_sched_host.cpp sweeps them on the CPU).
//
// Workgroup b of a grid of G starts with tile b.  The other R = ntiles - G tiles are cut into chunks of consecutive tiles, and a claim --
// one fetch_add(1) on the launch's counter (vc_common.h: tile_claim_chunk) -- returns a CHUNK index.  tile_chunk maps it to the chunk's
// first tile and its length, from (chunk index, ntiles, G) alone.  Cut from the END of the tile range: the last G tiles come singly, the
// 2 G before them in G pairs, the 4 G before those in G fours, ..., and everything in front of that in chunks of TILE_CHUNK_MAX; what does
// not divide (fewer than TILE_CHUNK_MAX tiles) goes, by its binary digits, as one more chunk to the shorter classes.  So the lengths never
// grow with the chunk index, every workgroup's last pieces of work are single tiles (a ragged end of about one tile, as with one claim per
// tile) and the number of claims is ntiles / TILE_CHUNK_MAX + 3 G + G (the claims past the end).
//
// Protocol invariant (vc_common.h, tile_claims_done): a workgroup claims again only while its last claim returned a chunk inside the
// range, so each workgroup makes exactly one claim that returns an index >= tile_chunk_count -- tile_chunk then gives first = ntiles,
// len = 0 -- and calls tile_claims_done after it.
//
// TILE_CHUNK_MAX = 8.  What is measured (profiles/dyn_tiles.md): front_fused_kernel's 25 600 claims per ms on the one address cost that
// kernel 1.8 % alone; c3_fused_kernel with one claim per 7 us tile (51 200 tiles in 0.8 ms on 480 workgroups, ~ 70 claims per us) slowed
// every tile down.  Eight tiles per chunk puts C3 at 5 920 + 1 440 + 480 claims in 0.8 ms, ~ 10 per us, under half the front kernel's
// rate, and the Bottleneck (12 800 tiles on 224 workgroups in 0.25 - 0.39 ms) at 2 270 claims, 6 - 9 per us.  Longer chunks buy nothing
// the measurements ask for and lengthen what a late workgroup leaves to the others.
#pragma once

#if defined(__HIPCC__)
#define VC_HD __host__ __device__
#else
#define VC_HD
#endif

namespace vc {

#define TILE_CHUNK_LOG2 3
#define TILE_CHUNK_MAX (1 << TILE_CHUNK_LOG2)

// chunks of length 1 << k, k = 0 .. TILE_CHUNK_LOG2, for `rest` tiles behind the workgroups' first ones
struct TileChunkCounts { int n[TILE_CHUNK_LOG2 + 1]; };

VC_HD static inline TileChunkCounts tile_chunk_counts(int ntiles, int grid) {
    TileChunkCounts c;
    int rest = ntiles > grid ? ntiles - grid : 0;
    for (int k = 0; k < TILE_CHUNK_LOG2; ++k) {
        const int m = rest >> k < grid ? rest >> k : grid;
        c.n[k] = m;
        rest -= m << k;
    }
    c.n[TILE_CHUNK_LOG2] = rest >> TILE_CHUNK_LOG2;
    rest -= c.n[TILE_CHUNK_LOG2] << TILE_CHUNK_LOG2;
    for (int k = 0; k < TILE_CHUNK_LOG2; ++k) c.n[k] += (rest >> k) & 1;     // rest < TILE_CHUNK_MAX
    return c;
}

VC_HD static inline int tile_chunk_count(int ntiles, int grid) {
    const TileChunkCounts c = tile_chunk_counts(ntiles, grid);
    int s = 0;
    for (int k = 0; k <= TILE_CHUNK_LOG2; ++k) s += c.n[k];
    return s;
}

// first tile of chunk `chunk` (0, 1, ... in the order the claims return them), its length in *len; chunk >= tile_chunk_count: ntiles, 0
VC_HD static inline int tile_chunk(int chunk, int ntiles, int grid, int* len) {
    const TileChunkCounts c = tile_chunk_counts(ntiles, grid);
    int first = grid;
    for (int k = TILE_CHUNK_LOG2; k >= 0; --k) {
        if (chunk < c.n[k]) { *len = 1 << k; return first + (chunk << k); }
        chunk -= c.n[k];
        first += c.n[k] << k;
    }
    *len = 0;
    return ntiles;
}

}  // namespace vc
