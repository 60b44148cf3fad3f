// Host build of vehicle-counting_amd/csrc/conv_geom.h (the launch geometry of the convolution kernels: plain integer functions, no
// HIP) behind a C interface for tests/test_conv_geom_host.py.
#include "../../vehicle-counting_amd/csrc/conv_geom.h"

extern "C" {

int cgh_persistent_grid(int tiles, int slots_hw, int reserve, int slots_override, int balanced) {
    return vc::persistent_grid(tiles, slots_hw, reserve, slots_override, balanced != 0);
}

// the tile rectangle of a [B][Ho][Wo] output map for tiles of bp pixels; returns 1 and (th, tw) if there is one
int cgh_s2halo_geom(int B, int Ho, int Wo, int bp, int* th, int* tw) {
    return vc::s2halo_geom((long)B * Ho, Wo, bp, th, tw) ? 1 : 0;
}

}
