"""CPU: the chunk schedule of the claimed-tile kernels (vehicle-counting_amd/csrc/tile_sched.h, used by c3_fused.hip and bneck_fused.hip)
compiled for the host (tests/native/tile_sched_host.cpp), with the kernels' claim protocol played by a simulator: workgroup b computes tile b,
then claims chunks with fetch_add(1) until a claim returns past the end, then counts itself done; the last one zeroes the pair.

For ntiles 0 .. 4096 on grids of 1, 2, 5, 224, 256, 480 and 512 workgroups (grids at and above ntiles included), under three interleavings
-- round-robin, one workgroup taking everything before the others move, a seeded shuffle: every tile is computed exactly once, every workgroup
makes exactly one claim past the end, the pair is back at zero, chunk lengths never grow with the chunk index, and the last tiles come singly.
The same source with its own main() is the sanitizer run (g++ -DTILE_SCHED_MAIN -fsanitize=address,undefined -fno-sanitize-recover=all; it
prints TILE_SCHED_OK after the same sweep, 18 s, which is why it is not a test here)."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "tile_sched_host.cpp")
GRIDS = [1, 2, 5, 224, 256, 480, 512]
ERRORS = {1: "a tile computed twice", 2: "a tile never computed", 3: "not exactly one claim past the end per workgroup", 4: "a chunk longer than the one before it",
          5: "one of the last tiles is not a chunk of its own", 6: "the counter pair is not back at zero", 7: "a chunk outside the tile range or out of order",
          8: "chunks although no tile is left", 9: "a chunk length that is no power of two up to the maximum"}


@pytest.fixture(scope="module")
def tsh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tsh") / "libtsh.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC], check=True)
    lib = C.CDLL(so)
    lib.tsh_chunk.argtypes = [C.c_int] * 3 + [C.POINTER(C.c_int)]
    lib.tsh_sweep.argtypes = [C.c_int] * 3 + [C.c_uint]
    lib.tsh_simulate.argtypes = [C.c_int] * 3 + [C.c_uint]
    return lib


def _chunks(tsh, ntiles, grid):
    out = []
    for c in range(tsh.tsh_chunk_count(ntiles, grid)):
        n = C.c_int(-1)
        out.append((tsh.tsh_chunk(c, ntiles, grid, C.byref(n)), n.value))
    return out


@pytest.mark.parametrize("grid", GRIDS)
def test_every_tile_once_one_claim_past_the_end(tsh, grid):
    e = tsh.tsh_sweep(grid, 0, 4096, 1702)
    assert e == 0, (grid, "ntiles", e // 1000 - 1, ERRORS.get(e % 1000, e % 1000))


@pytest.mark.parametrize("grid", [1, 5])
def test_sixty_tiles_have_full_chunks_and_a_single_tile_tail(tsh, grid):
    """The shapes of tests/test_gpu_dyn_tiles_blocks.py (60 C3 tiles on 1 and on 5 workgroups) reach both ends of the schedule with the chunk
    length chosen: at least one chunk of the full length and a tail of single tiles."""
    full = tsh.tsh_chunk_max()
    ch = _chunks(tsh, 60, grid)
    lens = [n for _, n in ch]
    assert full == 8
    assert lens[0] == full and lens.count(full) >= 2, lens
    assert lens[-grid:] == [1] * grid, lens
    assert ch[0][0] == grid and ch[-1][0] == 59 and sum(lens) == 60 - grid
    assert lens == sorted(lens, reverse=True)


def test_claim_counts_of_the_product_shapes(tsh):
    """What tile_sched.h's comment says about the claim rate: C3 at 256 frames (51 200 tiles on 480 workgroups) and the Bottleneck (12 800 on 224)."""
    assert tsh.tsh_chunk_count(51200, 480) == 5920 + 3 * 480
    assert tsh.tsh_chunk_count(12800, 224) == 1376 + 3 * 224
    n = C.c_int(-1)
    assert tsh.tsh_chunk(5920 + 3 * 480, 51200, 480, C.byref(n)) == 51200 and n.value == 0
