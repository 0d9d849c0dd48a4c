"""CPU-side checks of AssignUniqueId (pa_unique_id_pool_create / pa_assign_unique_id_create): exported, the ctypes mirror laid out as the
header lays it out, every invalid argument and every refusal of the contract reported at creation -- an invalid argument before a
refusal, both before the device is asked for --, no device -> a loud PA_ERR_NO_DEVICE, the JNI natives and the C++ mirror, and the
model the GPU tests compare against pinned by hand."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from presto_amd import abi
from presto_amd._lib import lib
from tests import unique_id_model as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["input_channel_count", "input_types", "input_type_params", "stage_id", "task_id", "output_mem", "stream"]
CARRIED = [abi.BIGINT, abi.INTEGER, abi.DATE, abi.DOUBLE, abi.REAL, abi.BOOLEAN, abi.VARCHAR, abi.decimal(12, 2), abi.decimal(30, 2)]


def has_gpu():
    return lib().pa_device_count() > 0


def make_pool(first_value=0):
    from presto_amd.operators import UniqueIdPool
    return UniqueIdPool(first_value)


def create(pool, input_types, **kw):
    """the status of pa_assign_unique_id_create; an operator that did come to be is closed again"""
    from presto_amd.operators import assign_unique_id_desc
    d, keep = assign_unique_id_desc(input_types, **kw)
    h = C.c_void_p()
    rc = lib().pa_assign_unique_id_create(C.byref(d), pool._h, C.byref(h))
    if rc == abi.OK:
        lib().pa_op_close(h)
    return rc


# what a descriptor without a defect gives: an operator on a GPU, a loud refusal to run without one
def accepted():
    return abi.OK if has_gpu() else abi.ERR_NO_DEVICE


def test_entry_points_are_exported():
    L = lib()
    for name in ["pa_unique_id_pool_create", "pa_unique_id_pool_destroy", "pa_assign_unique_id_create"]:
        assert getattr(L, name) is not None
    from presto_amd.operators import AssignUniqueIdOperator, AssignUniqueIdOperatorFactory, UniqueIdPool   # noqa: F401  (the Python mirrors)


def test_ctypes_layout_matches_the_header():
    """sizeof / offsetof of the descriptor, printed by a C program compiled against include/presto_amd.h."""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "layout.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "presto_amd.h"\nint main(void) {\n')
            f.write('    printf("%d\\n", (int)sizeof(pa_assign_unique_id_desc));\n')
            for name in FIELDS:
                f.write('    printf("%%d\\n", (int)offsetof(pa_assign_unique_id_desc, %s));\n' % name)
            f.write("    return 0;\n}\n")
        exe = os.path.join(d, "layout")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    cls = abi.pa_assign_unique_id_desc
    assert [name for name, _ in cls._fields_] == FIELDS
    assert got == [C.sizeof(cls)] + [getattr(cls, name).offset for name in FIELDS]


def test_pool_arguments():
    L = lib()
    h = C.c_void_p()
    assert L.pa_unique_id_pool_create(0, None) == abi.ERR_INVALID_ARGUMENT
    for first in (-1, (1 << 40) + 1, (1 << 63) - 1, -(1 << 63)):
        assert L.pa_unique_id_pool_create(first, C.byref(h)) == abi.ERR_INVALID_ARGUMENT, first
    for first in (0, (1 << 20) - 3, (1 << 40) - (1 << 20), 1 << 40):      # the limit itself is a start: the first request then fails
        assert L.pa_unique_id_pool_create(first, C.byref(h)) == abi.OK, first
        assert L.pa_unique_id_pool_destroy(h) == abi.OK
    assert L.pa_unique_id_pool_destroy(None) == abi.OK


def test_invalid_arguments():
    from presto_amd.operators import assign_unique_id_desc
    L = lib()
    pool = make_pool()
    h = C.c_void_p()
    d, keep = assign_unique_id_desc([abi.BIGINT])
    assert L.pa_assign_unique_id_create(None, pool._h, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    assert L.pa_assign_unique_id_create(C.byref(d), None, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    assert L.pa_assign_unique_id_create(C.byref(d), pool._h, None) == abi.ERR_INVALID_ARGUMENT
    for count in (-1, 0):
        d, keep = assign_unique_id_desc([abi.BIGINT])
        d.input_channel_count = count
        assert L.pa_assign_unique_id_create(C.byref(d), pool._h, C.byref(h)) == abi.ERR_INVALID_ARGUMENT, count
    d, keep = assign_unique_id_desc([abi.BIGINT])
    d.input_types = None
    assert L.pa_assign_unique_id_create(C.byref(d), pool._h, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    for bad in (-1, 10, 99):
        assert create(pool, [abi.BIGINT, bad]) == abi.ERR_INVALID_ARGUMENT, bad
    for mem in (-1, 2):
        assert create(pool, [abi.BIGINT], output_mem=mem) == abi.ERR_INVALID_ARGUMENT, mem
    # (stage_id << 54) leaves int64 from 2^9 on, (task_id << 40) from 2^23 on; a negative id would reach into the row id's 40 bits
    for stage in (-1, 1 << 9, (1 << 31) - 1, -(1 << 31)):
        assert create(pool, [abi.BIGINT], stage_id=stage) == abi.ERR_INVALID_ARGUMENT, stage
    for task in (-1, 1 << 23, (1 << 31) - 1, -(1 << 31)):
        assert create(pool, [abi.BIGINT], task_id=task) == abi.ERR_INVALID_ARGUMENT, task


def test_refusals_and_their_order():
    pool = make_pool()
    assert create(pool, [abi.BIGINT, abi.ROW]) == abi.ERR_NOT_SUPPORTED
    assert create(pool, [abi.BIGINT] * 65) == abi.ERR_NOT_SUPPORTED
    # an invalid argument before a refusal
    assert create(pool, [abi.ROW, 99]) == abi.ERR_INVALID_ARGUMENT
    assert create(pool, [abi.ROW], output_mem=5) == abi.ERR_INVALID_ARGUMENT
    assert create(pool, [abi.ROW], stage_id=1 << 9) == abi.ERR_INVALID_ARGUMENT
    assert create(pool, [abi.BIGINT] * 65, task_id=-1) == abi.ERR_INVALID_ARGUMENT
    assert create(pool, [abi.BIGINT] * 65 + [99]) == abi.ERR_INVALID_ARGUMENT


def test_what_the_contract_takes():
    """every carried type, 64 channels, the largest stage and task id: nothing but the device is missing"""
    pool = make_pool()
    assert create(pool, CARRIED) == accepted()
    assert create(pool, [abi.BIGINT] * 64) == accepted()
    assert create(pool, [abi.VARCHAR], stage_id=(1 << 9) - 1, task_id=(1 << 23) - 1, output_mem=abi.MEM_DEVICE) == accepted()


@pytest.mark.skipif(has_gpu(), reason="container without a GPU only")
def test_no_device_fails_loudly():
    pool = make_pool((1 << 20) - 3)
    assert create(pool, CARRIED) == abi.ERR_NO_DEVICE
    assert b"no" in lib().pa_last_error().lower()


def test_sources_and_build_list():
    makefile = open(os.path.join(ROOT, "presto_amd", "csrc", "Makefile")).read()
    assert "op_assign_unique_id.cpp" in makefile and "unique_id_kernels.hip" in makefile
    kernels = open(os.path.join(ROOT, "presto_amd", "csrc", "unique_id_kernels.hpp")).read()
    assert re.search(r"kUniqueIdSegments\s*=\s*\d+", kernels) and "launch_unique_ids(" in kernels


def test_jni_shim_and_java_natives():
    """jni/presto_amd_jni.c compiles against the stand-in jni.h and exports the three natives GpuNative.java declares"""
    shim = os.path.join(ROOT, "jni", "presto_amd_jni.c")
    with tempfile.TemporaryDirectory() as d:
        obj = os.path.join(d, "shim.o")
        subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-fPIC", "-I" + os.path.join(ROOT, "jni", "stub"), "-I" + os.path.join(ROOT, "include"), shim, "-o", obj], check=True)
        symbols = subprocess.run(["nm", "-g", "--defined-only", obj], check=True, capture_output=True, text=True).stdout
    java = open(os.path.join(ROOT, "java", "io", "trino", "gpu", "GpuNative.java")).read()
    for name in ("createUniqueIdPool", "destroyUniqueIdPool", "createAssignUniqueId"):
        assert re.search(r"\bT Java_io_trino_gpu_GpuNative_%s\b" % name, symbols), name
        assert re.search(r"static native \w+ %s\(" % name, java), name
    planner = open(os.path.join(ROOT, "java", "io", "trino", "gpu", "GpuAssignUniqueId.java")).read()
    assert "GpuNative.createAssignUniqueId(" in planner and "GpuNative.createUniqueIdPool(0)" in planner and "getStageId().getId()" in planner
    assert "GpuAssignUniqueId.create(" in open(os.path.join(ROOT, "java", "io", "trino", "gpu", "GpuOperatorFactories.java")).read()


def test_cpp_mirror_declares_the_classes():
    """include/presto_amd.hpp: the pool and the factory, and a translation unit that uses them compiles"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "mirror.cpp")
        with open(src, "w") as f:
            f.write('#include "presto_amd.hpp"\nusing namespace presto_amd;\n'
                    "std::vector<Page> run(const std::vector<Page>& pages) {\n"
                    "    AssignUniqueIdOperatorFactory factory({PA_BIGINT, PA_VARCHAR}, 3, 7, PA_MEM_HOST, {}, (int64_t(1) << 20) - 3);\n"
                    "    auto a = factory.createOperator();\n    auto b = factory.createOperator();\n"
                    "    UniqueIdPool pool(5);\n    (void)pool.handle();\n"
                    "    return runDriver(pages, {a.get(), b.get()});\n}\n")
        subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src], check=True)


# ---- the model, pinned by hand ----------------------------------------------------------------------------------------------------------
def test_model_first_block_and_mask():
    a = U.Assigner(U.Pool(), stage_id=2, task_id=5)
    mask = (2 << 54) | (5 << 40)
    assert a.ids(3) == [mask, mask | 1, mask | 2]
    assert a.ids(0) == [] and a.ids(1) == [mask | 3]


def test_model_block_end_in_the_middle_of_a_page():
    # the pool starts three ids before 2^20: the first block is [2^20 - 3, 2^21 - 3) -- a block is 2^20 ids from wherever it starts
    pool = U.Pool((1 << 20) - 3)
    a = U.Assigner(pool)
    b = U.Assigner(pool)                      # takes the block behind a's
    first = (1 << 20) - 3
    assert a.ids(2) == [first, first + 1]
    assert b.ids(2) == [first + (1 << 20), first + (1 << 20) + 1]
    rest = a.ids((1 << 20) - 2 + 2)           # the rest of a's block, then two ids of its next: the third block of the pool
    assert rest[(1 << 20) - 3] == first + (1 << 20) - 1
    assert rest[-2:] == [first + 2 * (1 << 20), first + 2 * (1 << 20) + 1]
    assert pool.next == first + 3 * (1 << 20)


def test_model_limit():
    pool = U.Pool((1 << 40) - (1 << 20))
    a = U.Assigner(pool)                      # the last block there is
    assert a.ids(1 << 20)[-1] == (1 << 40) - 1
    with pytest.raises(U.LimitExceeded):
        a.ids(1)
    with pytest.raises(U.LimitExceeded):
        U.Assigner(U.Pool(1 << 40))
    # a block that begins below the limit is capped at it
    b = U.Assigner(U.Pool((1 << 40) - 5))
    assert b.ids(5)[-1] == (1 << 40) - 1
    with pytest.raises(U.LimitExceeded):
        b.ids(1)
