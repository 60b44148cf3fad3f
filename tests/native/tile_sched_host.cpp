// Host build of vehicle-counting_amd/csrc/tile_sched.h (the chunk schedule of the claimed-tile kernels: plain integer functions, no HIP)
// behind a C interface for tests/test_tile_sched_host.py, and -- with -DTILE_SCHED_MAIN -- a stand-alone program that runs the same sweep
// (built with -fsanitize=address,undefined it is the sanitizer run of the schedule).
//
// tsh_simulate plays the kernels' protocol on the host: workgroup b computes tile b, then claims (fetch_add(1) on `next`) and computes the
// chunk it got until a claim returns past the end, then adds one to `done`; the last one zeroes the pair.  Which workgroup moves next is
// the interleaving: 0 round-robin, 1 workgroup 0 takes everything before any other moves, 2 a seeded shuffle.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../vehicle-counting_amd/csrc/tile_sched.h"

namespace {

struct Rng {      // xorshift64*: the shuffle must not depend on the C library
    uint64_t s;
    uint32_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint32_t)((s * 2685821657736338717ull) >> 32); }
};

enum { OK = 0, E_TWICE = 1, E_MISSED = 2, E_PAST_END = 3, E_GROWS = 4, E_TAIL = 5, E_PAIR = 6, E_RANGE = 7, E_COUNT = 8, E_LEN = 9 };

// the schedule alone: chunks tile the range behind the first `grid` tiles in order, lengths in {1, 2, .., TILE_CHUNK_MAX} and never growing,
// the last min(rest, grid) tiles singly, everything at or past tile_chunk_count is the end mark
int check_schedule(int ntiles, int grid) {
    const int n = vc::tile_chunk_count(ntiles, grid);
    const int rest = ntiles > grid ? ntiles - grid : 0;
    int expect = grid, prev = TILE_CHUNK_MAX;
    for (int c = 0; c < n; ++c) {
        int len = -1;
        const int first = vc::tile_chunk(c, ntiles, grid, &len);
        if (first != expect) return E_RANGE;
        if (len < 1 || len > TILE_CHUNK_MAX || (len & (len - 1))) return E_LEN;
        if (len > prev) return E_GROWS;
        if (first + len > ntiles) return E_RANGE;
        if (first >= ntiles - (rest < grid ? rest : grid) && len != 1) return E_TAIL;
        prev = len;
        expect = first + len;
    }
    if (rest > 0 && expect != ntiles) return E_MISSED;
    if (rest == 0 && n != 0) return E_COUNT;
    for (int c = n; c < n + 3; ++c) {
        int len = -1;
        if (vc::tile_chunk(c, ntiles, grid, &len) < ntiles || len != 0) return E_PAST_END;
    }
    return OK;
}

int simulate(int ntiles, int grid, int mode, uint64_t seed) {
    std::vector<int> hits((size_t)ntiles, 0), past((size_t)grid, 0), state((size_t)grid, 0);   // state: 0 not started, 1 claiming, 2 gone
    unsigned pair[2] = {0u, 0u};
    std::vector<int> live((size_t)grid);
    for (int b = 0; b < grid; ++b) live[(size_t)b] = b;
    Rng rng{seed * 0x9E3779B97F4A7C15ull + 1};
    size_t rr = 0;
    while (!live.empty()) {
        size_t pick = mode == 0 ? rr % live.size() : mode == 1 ? 0 : rng.next() % live.size();
        const int b = live[pick];
        bool gone = false;
        if (state[(size_t)b] == 0) {                 // its first tile, no claim
            if (b < ntiles) ++hits[(size_t)b];
            state[(size_t)b] = 1;
        } else {
            const int chunk = (int)pair[0]++;        // the claim
            int len = -1;
            const int first = vc::tile_chunk(chunk, ntiles, grid, &len);
            if (first >= ntiles) {
                ++past[(size_t)b];
                if (pair[1]++ == (unsigned)grid - 1) { pair[0] = 0; pair[1] = 0; }    // tile_claims_done
                gone = true;
            } else {
                if (first + len > ntiles) return E_RANGE;
                for (int t = first; t < first + len; ++t) ++hits[(size_t)t];
            }
        }
        if (gone) {
            state[(size_t)b] = 2;
            live.erase(live.begin() + (long)pick);   // keeps the order: mode 1 then lets the next workgroup run to its end
        } else {
            ++rr;
        }
        if (gone && mode == 0 && !live.empty()) rr %= live.size();
    }
    for (int t = 0; t < ntiles; ++t) {
        if (hits[(size_t)t] > 1) return E_TWICE;
        if (hits[(size_t)t] < 1) return E_MISSED;
    }
    for (int b = 0; b < grid; ++b)
        if (past[(size_t)b] != 1) return E_PAST_END;
    if (pair[0] != 0 || pair[1] != 0) return E_PAIR;
    return OK;
}

}  // namespace

extern "C" {

int tsh_chunk_max() { return TILE_CHUNK_MAX; }
int tsh_chunk_count(int ntiles, int grid) { return vc::tile_chunk_count(ntiles, grid); }
int tsh_chunk(int chunk, int ntiles, int grid, int* len) { return vc::tile_chunk(chunk, ntiles, grid, len); }
int tsh_check_schedule(int ntiles, int grid) { return check_schedule(ntiles, grid); }
int tsh_simulate(int ntiles, int grid, int mode, unsigned seed) { return simulate(ntiles, grid, mode, seed); }

// ntiles lo .. hi on this grid, the schedule's own properties and the three interleavings; 0, or 1000 * (the failing ntiles + 1) + the error
int tsh_sweep(int grid, int lo, int hi, unsigned seed) {
    for (int n = lo; n <= hi; ++n) {
        int e = check_schedule(n, grid);
        for (int mode = 0; mode < 3 && !e; ++mode) e = simulate(n, grid, mode, seed + (unsigned)n);
        if (e) return 1000 * (n + 1) + e;
    }
    return 0;
}

}

#ifdef TILE_SCHED_MAIN
int main() {
    const int grids[] = {1, 2, 5, 224, 256, 480, 512};
    for (int g : grids) {
        const int e = tsh_sweep(g, 0, 4096, 1702u);
        if (e) { std::printf("grid %d: ntiles %d fails with %d\n", g, e / 1000 - 1, e % 1000); return 1; }
    }
    std::printf("TILE_SCHED_OK\n");
    return 0;
}
#endif
