"""CPU-side checks of the ROW_NUMBER entry points (RowNumberOperator): exported, the ctypes mirror laid out as the header lays it out,
shapes outside the device path refused before the device is asked for, and no device -> a loud PA_ERR_NO_DEVICE.  No compute call is
made here.  The library these tests load is linked from the Makefile's source lists, so row_number_kernels.hip has been compiled for
gfx950 (off the GPU) when the export test passes."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from presto_amd import abi
from presto_amd._lib import lib
from presto_amd.operators import RowNumberOperatorFactory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["pa_row_number_create", "pa_row_number_stats"]
FIELDS = ["input_channel_count", "input_types", "input_type_params", "output_channel_count", "output_channels", "partition_channel_count",
          "partition_channels", "hash_channel", "expected_positions", "max_rows_per_partition", "output_mem", "stream"]


def has_gpu():
    return lib().pa_device_count() > 0


def test_row_number_entry_points_are_exported():
    L = lib()
    for name in ENTRIES:
        assert getattr(L, name) is not None, name
    from presto_amd.operators import Operator, RowNumberOperator   # noqa: F401  (the third entry point: the Python mirror)
    assert callable(Operator.rowNumberStats)


def test_the_kernels_are_in_the_makefile_source_lists():
    text = open(os.path.join(ROOT, "presto_amd", "csrc", "Makefile")).read()
    dev = [line for line in text.splitlines() if line.startswith("DEV_SRCS")][0]
    host = [line for line in text.splitlines() if line.startswith("HOST_SRCS")][0]
    assert "row_number_kernels.hip" in dev.split() and "op_row_number.cpp" in host.split()
    assert os.path.exists(os.path.join(ROOT, "presto_amd", "csrc", "row_number_kernels.hpp"))


def test_ctypes_layout_matches_the_header():
    """sizeof / offsetof of the C struct, printed by a C program compiled against include/presto_amd.h."""
    struct = "pa_row_number_desc"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "layout.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "presto_amd.h"\nint main(void) {\n')
            f.write('    printf("%%d\\n", (int)sizeof(%s));\n' % struct)
            for field in FIELDS:
                f.write('    printf("%%d\\n", (int)offsetof(%s, %s));\n' % (struct, field))
            f.write("    return 0;\n}\n")
        exe = os.path.join(d, "layout")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    cls = abi.pa_row_number_desc
    assert [name for name, _ in cls._fields_] == FIELDS
    assert got == [C.sizeof(cls)] + [getattr(cls, field).offset for field in FIELDS]


def _create(factory):
    h = C.c_void_p()
    return factory._create(C.byref(factory._desc), C.byref(h))


def _modes(types, output_channels, partition_channels, **kw):
    """without a cap and with one"""
    return [RowNumberOperatorFactory(types, output_channels, partition_channels, **kw),
            RowNumberOperatorFactory(types, output_channels, partition_channels, 3, **kw)]


@pytest.mark.skipif(has_gpu(), reason="container without a GPU only")
def test_no_device_fails_loudly():
    for t in (abi.BIGINT, abi.DOUBLE, abi.VARCHAR, abi.decimal(12, 2)):
        for f in (_modes([t, abi.BIGINT], [0, 1], [0], hash_channel=1) + _modes([abi.BIGINT, t], [1], [1, 0], output_mem=abi.MEM_DEVICE)
                  + _modes([t], [0], [])):
            assert _create(f) == abi.ERR_NO_DEVICE
    assert _create(RowNumberOperatorFactory([abi.BIGINT], [0], [], 0)) == abi.ERR_NO_DEVICE


def test_stats_of_a_null_operator_is_an_invalid_argument():
    count, capacity = C.c_int64(), C.c_int64()
    assert lib().pa_row_number_stats(None, C.byref(count), C.byref(capacity)) == abi.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("key_type", [abi.decimal(30, 2), abi.ROW])
def test_partition_types_outside_the_device_path_are_refused_at_creation(key_type):
    """The planner keeps the reference operator for these: the refusal comes before any device work (with or without a GPU)."""
    for f in _modes([abi.BIGINT, key_type], [0], [1]) + _modes([abi.BIGINT, key_type], [0], [0, 1]):
        assert _create(f) == abi.ERR_NOT_SUPPORTED


def test_nine_partition_channels_are_refused_at_creation():
    for f in _modes([abi.BIGINT] * 9, [0], list(range(9))):
        assert _create(f) == abi.ERR_NOT_SUPPORTED


@pytest.mark.parametrize("t", [abi.decimal(30, 2), abi.ROW])
def test_output_channels_the_cap_cannot_copy_are_refused_at_creation(t):
    """Under a cap the kept rows are copied position by position; there is no such copy for 16-byte values and rows."""
    assert _create(RowNumberOperatorFactory([abi.BIGINT, t], [0, 1], [0], 5)) == abi.ERR_NOT_SUPPORTED


def test_bad_descriptors_are_invalid_arguments():
    one = [abi.BIGINT]
    for f in (_modes(one, [0], [1])                                        # partition channel out of range
              + _modes(one, [0], [-1])
              + _modes(one, [1], [0])                                      # output channel out of range
              + _modes(one, [-1], [0])
              + _modes([abi.BIGINT, abi.DOUBLE], [0], [0], hash_channel=1)  # $hashvalue not BIGINT
              + _modes(one, [0], [0], hash_channel=1)                      # $hashvalue out of range
              + _modes(one, [0], [0], hash_channel=-2)
              + _modes(one, [0], [0], output_mem=7)
              + _modes(one, [0], [0], expected_positions=-1)
              + _modes([77], [0], [0])                                     # unknown partition key type
              + [RowNumberOperatorFactory(one, [0], [0], -2),              # a negative cap other than "absent"
                 RowNumberOperatorFactory(one, [0], [], -5)]):
        assert _create(f) == abi.ERR_INVALID_ARGUMENT
    h = C.c_void_p()
    assert lib().pa_row_number_create(None, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    f = RowNumberOperatorFactory(one, [0], [0])
    assert lib().pa_row_number_create(C.byref(f._desc), None) == abi.ERR_INVALID_ARGUMENT
    f = RowNumberOperatorFactory(one, [0], [0])
    f._desc.partition_channels = None                                      # a count without the array
    assert _create(f) == abi.ERR_INVALID_ARGUMENT
    f = RowNumberOperatorFactory(one, [0], [0])
    f._desc.output_channels = None
    assert _create(f) == abi.ERR_INVALID_ARGUMENT
    f = RowNumberOperatorFactory(one, [0], [0])
    f._desc.input_types = None
    assert _create(f) == abi.ERR_INVALID_ARGUMENT
