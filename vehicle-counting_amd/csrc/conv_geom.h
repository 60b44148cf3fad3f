// Host-side launch geometry of the convolution kernels: pure integer functions and nothing else, no HIP header, so that a plain C++
// compiler can build them (tests/native/conv_geom_host.cpp pins their values).
#pragma once
#include <algorithm>

namespace vc {

// Grid of a persistent launch.  Workgroup b walks tiles b, b + G, ...: the launch lasts ceil(tiles / G) tile times.  The old rule -- every slot
// but a reserve of 64 for the other streams' kernels (never fewer than 256 slots) -- can cost a whole extra round on the configurations with
// several workgroups per CU (3200 tiles on 448 of 512 slots: eight rounds where seven do) and always occupies every slot it may, whatever the
// tile count.  Rounds first: the fewest rounds the chip allows (the reserve is given up only when that saves a round), then the smallest
// grid that still finishes in that many rounds (800 tiles in four rounds: 200 workgroups, not 256 -- the slots that are not needed stay free
// for the ReID queue and the tracker), a multiple of 8 for the XCD-aware tile order.  Measured + 0.5 % end to end, two alternations.
// balanced = false (VC_CONV_BALANCED=0): the old rule (A/B switch).
static inline int persistent_grid(int tiles, int slots_hw, int reserve, int slots_override, bool balanced) {
    if (slots_override > 0) return tiles > slots_override ? std::max(8, slots_override / 8 * 8) : tiles;
    const int cap = std::max(8, std::max(256, slots_hw - reserve) / 8 * 8);
    if (tiles <= cap) return tiles;
    if (!balanced) return cap;
    const int full = std::max(cap, slots_hw / 8 * 8);
    const int r_cap = (tiles + cap - 1) / cap, r_full = (tiles + full - 1) / full;
    const int rounds = std::min(r_cap, r_full);
    const int g = ((tiles + rounds - 1) / rounds + 7) / 8 * 8;
    return std::min(g, full);
}

// tile rectangle of the stride-2 halo kernel: the th x tw (th * tw <= bp) whose parity classes ((th + 1) x (tw + 1) pixels) fit the patch
// buffer and that covers the map with the fewest tiles (then the smallest patch): for bp = 128, 16 x 8 at 80 and at 40 columns, 25 x 5 at 20;
// for bp = 256, 16 x 16 at 80, 32 x 8 at 40, 51 x 5 at 20 (128 frames; the row space is G = batch * Ho rows deep, Wo columns wide)
static inline bool s2halo_geom(long G, int Wo, int bp, int* th_out, int* tw_out) {
    long best = -1;
    for (int tw = 1; tw <= std::min(Wo, 254); ++tw) {
        const int th = (int)std::min<long>(std::min(bp / tw, 254), G);
        const int cls = (th + 1) * (tw + 1);
        if (th < 1 || cls > bp / 128 * 5 * 32 - 1) continue;
        const long tiles = (long)((Wo + tw - 1) / tw) * ((G + th - 1) / th);
        const long cost = tiles * 4096 + cls;
        if (best < 0 || cost < best) { best = cost; *th_out = th; *tw_out = tw; }
    }
    return best >= 0;
}

}  // namespace vc
