"""CPU: the launch geometry of the convolution kernels (vehicle-counting_amd/csrc/conv_geom.h -- the grid of a persistent launch and the
tile rectangle of the stride-2 halo kernel) compiled for the host (tests/native/conv_geom_host.cpp).  The expected values are those of
the functions as they stood inside conv_igemm.hip before the launchers were split into one file per kernel family: moving them must
not move a grid or a tile."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cgh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cgh") / "libcgh.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "native", "conv_geom_host.cpp")], check=True)
    lib = C.CDLL(so)
    lib.cgh_persistent_grid.argtypes = [C.c_int] * 5
    lib.cgh_s2halo_geom.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)] * 2
    return lib


# (tiles, slots_hw, reserve, override) -> grid, rounds-first rule (balanced)
GRID_CASES = [
    ((3200, 512, 64, 0), 464),         # seven rounds instead of the reserve's eight
    ((800, 256, 64, 0), 200),          # four rounds on the smallest grid that does them
    ((448, 512, 64, 0), 448),          # exactly the slots outside the reserve
    ((449, 512, 64, 0), 456),          # one tile more: the reserve is given up for a single round
    ((100, 512, 64, 0), 100),
    ((1000, 512, 64, 8), 8),           # override (tests): a short grid walks all tiles
    ((5, 512, 64, 8), 5),
    ((1000, 512, 64, 3), 8),           # ... never fewer than the 8 the XCD tile order needs
    ((3200, 256, 64, 0), 248),
    ((7, 256, 300, 0), 7),
    ((100000, 1024, 64, 0), 1024),
]


@pytest.mark.parametrize("args,want", GRID_CASES)
def test_persistent_grid(cgh, args, want):
    assert cgh.cgh_persistent_grid(*args, 1) == want


def test_persistent_grid_old_rule(cgh):
    """balanced off (VC_CONV_BALANCED=0): every slot but the reserve, a multiple of 8."""
    assert cgh.cgh_persistent_grid(3200, 512, 64, 0, 0) == 448


# (B, Ho, Wo) -> (th, tw) for tiles of 128 and of 256 pixels
S2_CASES = [
    ((128, 80, 80), (16, 8), (16, 16)),
    ((128, 40, 40), (16, 8), (32, 8)),
    ((128, 20, 20), (25, 5), (51, 5)),
    ((1, 20, 20), (20, 5), (20, 10)),
    ((5, 4, 3), (20, 3), (20, 3)),     # a tile spans all five images
    ((1, 1, 1), (1, 1), (1, 1)),
    ((2, 20, 16), (8, 16), (40, 6)),
]


@pytest.mark.parametrize("shape,want128,want256", S2_CASES)
def test_s2halo_geom(cgh, shape, want128, want256):
    for bp, want in ((128, want128), (256, want256)):
        th, tw = C.c_int(-1), C.c_int(-1)
        assert cgh.cgh_s2halo_geom(*shape, bp, C.byref(th), C.byref(tw)) == 1
        assert (th.value, tw.value) == want, (shape, bp)
