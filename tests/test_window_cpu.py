"""CPU-side checks of the WINDOW entry point (WindowOperator, the ranking functions): exported, the ctypes mirrors laid out as the header
lays them out, every shape outside the device path refused -- and every bad descriptor reported -- before the device is asked for, and
no device -> a loud PA_ERR_NO_DEVICE.  No compute call is made here.  The library these tests load is linked from the Makefile's source
lists, so window_kernels.hip has been compiled for gfx950 (off the GPU) when the export test passes."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from presto_amd import abi
from presto_amd._lib import lib
from presto_amd.operators import WindowOperatorFactory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC_FIELDS = ["input_channel_count", "input_types", "input_type_params", "output_channel_count", "output_channels", "function_count", "functions",
               "partition_channel_count", "partition_channels", "sort_channel_count", "sort_channels", "sort_orders", "pre_grouped_channel_count",
               "pre_sorted_channel_prefix", "expected_positions", "output_mem", "stream"]
FUNCTION_FIELDS = ["function", "argument_count", "argument_channels"]
NO_ARGUMENT = [abi.WINDOW_ROW_NUMBER, abi.WINDOW_RANK, abi.WINDOW_DENSE_RANK, abi.WINDOW_PERCENT_RANK, abi.WINDOW_CUME_DIST]
ASC_NULLS_LAST = 1


def has_gpu():
    return lib().pa_device_count() > 0


def test_window_entry_point_is_exported():
    assert getattr(lib(), "pa_window_create") is not None
    from presto_amd.operators import WindowOperator   # noqa: F401  (the Python mirror)
    assert NO_ARGUMENT + [abi.WINDOW_NTILE] == [0, 1, 2, 3, 4, 5]


def test_the_kernels_are_in_the_makefile_source_lists():
    text = open(os.path.join(ROOT, "presto_amd", "csrc", "Makefile")).read()
    dev = [line for line in text.splitlines() if line.startswith("DEV_SRCS")][0]
    host = [line for line in text.splitlines() if line.startswith("HOST_SRCS")][0]
    assert "window_kernels.hip" in dev.split() and "op_window.cpp" in host.split()
    assert os.path.exists(os.path.join(ROOT, "presto_amd", "csrc", "window_kernels.hpp"))


def test_ctypes_layout_matches_the_header():
    """sizeof / offsetof of the C structs, printed by a C program compiled against include/presto_amd.h."""
    structs = [("pa_window_desc", DESC_FIELDS, abi.pa_window_desc), ("pa_window_function_desc", FUNCTION_FIELDS, abi.pa_window_function_desc)]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "layout.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "presto_amd.h"\nint main(void) {\n')
            for struct, fields, _ in structs:
                f.write('    printf("%%d\\n", (int)sizeof(%s));\n' % struct)
                for field in fields:
                    f.write('    printf("%%d\\n", (int)offsetof(%s, %s));\n' % (struct, field))
            f.write('    printf("%d %d %d %d %d %d\\n", (int)PA_WINDOW_ROW_NUMBER, (int)PA_WINDOW_RANK, (int)PA_WINDOW_DENSE_RANK, (int)PA_WINDOW_PERCENT_RANK,'
                    ' (int)PA_WINDOW_CUME_DIST, (int)PA_WINDOW_NTILE);\n')
            f.write("    return 0;\n}\n")
        exe = os.path.join(d, "layout")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for _, fields, cls in structs:
        assert [name for name, _ in cls._fields_] == fields
        want += [C.sizeof(cls)] + [getattr(cls, field).offset for field in fields]
    assert got == want + [0, 1, 2, 3, 4, 5]


def _create(factory):
    h = C.c_void_p()
    return factory._create(C.byref(factory._desc), C.byref(h))


def _window(types, output_channels=(0,), functions=(abi.WINDOW_RANK,), partition_channels=(0,), sort_channels=(0,), sort_orders=None, **kw):
    orders = [ASC_NULLS_LAST] * len(sort_channels) if sort_orders is None else sort_orders
    return WindowOperatorFactory(list(types), list(output_channels), list(functions), list(partition_channels), list(sort_channels), list(orders), **kw)


ALL_SIX = NO_ARGUMENT + [(abi.WINDOW_NTILE, [1])]


@pytest.mark.skipif(has_gpu(), reason="container without a GPU only")
def test_no_device_fails_loudly():
    """What the device path takes passes every check and then asks for the device."""
    for t in (abi.BIGINT, abi.DOUBLE, abi.VARCHAR, abi.REAL, abi.BOOLEAN, abi.DATE, abi.INTEGER, abi.decimal(12, 2)):
        for f in (_window([t, abi.BIGINT], [0, 1], ALL_SIX, [0], [0]),
                  _window([t, abi.INTEGER], [1], ALL_SIX + ALL_SIX[:4], [], [0, 1], [2, 3], output_mem=abi.MEM_DEVICE),
                  _window([t, abi.BIGINT], [], [abi.WINDOW_ROW_NUMBER], [], []),
                  _window([t] * 8, [0], [abi.WINDOW_CUME_DIST] * 16, list(range(8)), [], expected_positions=10)):
            assert _create(f) == abi.ERR_NO_DEVICE
    # a long decimal is carried as an output channel
    assert _create(_window([abi.BIGINT, abi.decimal(30, 2)], [0, 1])) == abi.ERR_NO_DEVICE


def test_pre_grouped_and_pre_sorted_input_is_refused_at_creation():
    assert _create(_window([abi.BIGINT], pre_grouped_channel_count=1)) == abi.ERR_NOT_SUPPORTED
    assert _create(_window([abi.BIGINT], pre_sorted_channel_prefix=1)) == abi.ERR_NOT_SUPPORTED


@pytest.mark.parametrize("t", [abi.decimal(30, 2), abi.ROW])
def test_partition_and_sort_types_outside_the_device_path_are_refused_at_creation(t):
    """The types OrderBy refuses as sort channels; the refusal comes before any device work (with or without a GPU)."""
    for f in (_window([abi.BIGINT, t], [0], partition_channels=[1]), _window([abi.BIGINT, t], [0], partition_channels=[0, 1]),
              _window([abi.BIGINT, t], [0], sort_channels=[1]), _window([abi.BIGINT, t], [0], partition_channels=[], sort_channels=[0, 1])):
        assert _create(f) == abi.ERR_NOT_SUPPORTED


def test_row_output_channels_are_refused_at_creation():
    assert _create(_window([abi.BIGINT, abi.ROW], [0, 1])) == abi.ERR_NOT_SUPPORTED
    assert _create(_window([abi.BIGINT, abi.ROW], [1], partition_channels=[])) == abi.ERR_NOT_SUPPORTED


def test_nine_partition_channels_are_refused_at_creation():
    assert _create(_window([abi.BIGINT] * 9, partition_channels=list(range(9)))) == abi.ERR_NOT_SUPPORTED


def test_bad_function_lists_are_invalid_arguments():
    two = [abi.BIGINT, abi.INTEGER]
    for functions in ([6], [-1], [abi.WINDOW_RANK, 99],                                       # unknown function ids
                      [(f, [0]) for f in NO_ARGUMENT][:1], [(abi.WINDOW_CUME_DIST, [0])],     # an argument where none is taken
                      [(abi.WINDOW_NTILE, [])], [(abi.WINDOW_NTILE, [0, 1])],                 # ntile takes exactly one
                      [(abi.WINDOW_NTILE, [2])], [(abi.WINDOW_NTILE, [-1])],                  # argument channel out of range
                      [],                                                                      # function_count outside 1 .. 16
                      [abi.WINDOW_RANK] * 17):
        assert _create(_window(two, functions=functions)) == abi.ERR_INVALID_ARGUMENT, functions
    for t in (abi.DOUBLE, abi.REAL, abi.VARCHAR, abi.BOOLEAN, abi.DATE, abi.decimal(12, 2), abi.decimal(30, 2)):   # a non-integer ntile argument
        assert _create(_window([abi.BIGINT, t], functions=[(abi.WINDOW_NTILE, [1])])) == abi.ERR_INVALID_ARGUMENT, t
    f = _window(two)
    f._desc.functions = None
    assert _create(f) == abi.ERR_INVALID_ARGUMENT
    f = _window(two, functions=[(abi.WINDOW_NTILE, [1])])
    f._desc.functions[0].argument_channels = None
    assert _create(f) == abi.ERR_INVALID_ARGUMENT
    f = _window(two)
    f._desc.function_count = -1
    assert _create(f) == abi.ERR_INVALID_ARGUMENT


def test_bad_descriptors_are_invalid_arguments():
    one = [abi.BIGINT]
    for f in (_window(one, sort_orders=[4]), _window(one, sort_orders=[-1]),                    # a sort order outside 0 .. 3
              _window(one, partition_channels=[1]), _window(one, partition_channels=[-1]),      # channels out of range
              _window(one, output_channels=[1]), _window(one, output_channels=[-1]),
              _window(one, sort_channels=[1]), _window(one, sort_channels=[-1]),
              _window(one, output_mem=7), _window(one, expected_positions=-1),
              _window([77])):                                                                    # unknown type
        assert _create(f) == abi.ERR_INVALID_ARGUMENT
    h = C.c_void_p()
    assert lib().pa_window_create(None, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    assert lib().pa_window_create(C.byref(_window(one)._desc), None) == abi.ERR_INVALID_ARGUMENT
    for field in ("partition_channels", "output_channels", "sort_channels", "sort_orders", "input_types"):   # a count without the array
        f = _window(one)
        setattr(f._desc, field, None)
        assert _create(f) == abi.ERR_INVALID_ARGUMENT, field
    for field in ("partition_channel_count", "sort_channel_count", "output_channel_count"):
        f = _window(one)
        setattr(f._desc, field, -1)
        assert _create(f) == abi.ERR_INVALID_ARGUMENT, field


def test_an_invalid_argument_is_reported_before_a_refusal():
    """Where a descriptor has both defects the bad argument decides, as for the sibling operators."""
    assert _create(_window([abi.BIGINT], functions=[7], pre_grouped_channel_count=1)) == abi.ERR_INVALID_ARGUMENT
    assert _create(_window([abi.BIGINT] * 9, partition_channels=list(range(8)) + [9])) == abi.ERR_INVALID_ARGUMENT


def test_the_jni_shim_exports_the_entry_point():
    """jni/presto_amd_jni.c against the stub jni.h: the symbol GpuNative.createWindow binds to."""
    with tempfile.TemporaryDirectory() as d:
        obj = os.path.join(d, "shim.o")
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-fPIC", "-c", "-I", os.path.join(ROOT, "jni", "stub"), "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "jni", "presto_amd_jni.c"), "-o", obj], check=True)
        symbols = subprocess.run(["nm", "-g", "--defined-only", obj], check=True, capture_output=True, text=True).stdout
    assert "Java_io_trino_gpu_GpuNative_createWindow" in symbols
    java = open(os.path.join(ROOT, "java", "io", "trino", "gpu", "GpuNative.java")).read()
    assert "createWindow" in java
    glue = open(os.path.join(ROOT, "java", "io", "trino", "gpu", "GpuWindow.java")).read()
    for name in ("row_number", "rank", "dense_rank", "percent_rank", "cume_dist", "ntile"):
        assert '"%s"' % name in glue
