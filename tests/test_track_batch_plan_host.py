"""CPU: what tracker.hip::track_enqueue decides about a batch before it touches a buffer (vehicle-counting_amd/csrc/track_batch_plan.h:
device order of the tasks, workgroup plans, step capacity, assignment-matrix LDS, table fit, rows-arena bound, block layouts, the
frame -> camera rule), compiled for the host (tests/native/track_batch_plan_host.cpp).  A wrong step capacity, matrix size or table fit
changes no output row -- it only selects a slower kernel instance -- so no parity test on the GPU notices; here each is held to literals
worked out by hand from the formulas, and the rows bound to a simulation of the kernel's own reservation rule (with the bound from
before ADVICE r02 as the negative control).  The cases and their numbers are in the native file; a case returns 0 or the source line of
its first failed check.  The same source with its own main() is the sanitizer run (g++ -DTRACK_BATCH_PLAN_MAIN
-fsanitize=address,undefined -fno-sanitize-recover=all; it prints TRACK_BATCH_PLAN_OK after the same cases)."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "track_batch_plan_host.cpp")
CASES = ["no_tasks", "device_order", "step_capacity", "assignment_matrix", "table_fit", "rows_arena", "layouts", "frame_cameras"]


@pytest.fixture(scope="module")
def tbp(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tbp") / "libtbp.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC], check=True)
    lib = C.CDLL(so)
    lib.tbp_case_name.restype = C.c_char_p
    return lib


def test_every_native_case_is_listed(tbp):
    assert [tbp.tbp_case_name(i).decode() for i in range(tbp.tbp_num_cases())] == CASES


@pytest.mark.parametrize("case", CASES)
def test_plan(tbp, case):
    line = tbp.tbp_run_case(CASES.index(case))
    assert line == 0, f"{case}: the check at tests/native/track_batch_plan_host.cpp:{line} fails"
