"""CPU-side checks of the DISTINCT entry points (MarkDistinctOperator / DistinctLimitOperator): exported, their ctypes mirrors laid out
as the header lays them out, shapes outside the device path refused before the device is asked for, and no device -> a loud
PA_ERR_NO_DEVICE.  No compute call is made here.  The library these tests load is linked from the Makefile's source lists, so
distinct_kernels.hip has been compiled for gfx950 (off the GPU) when the export test passes."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from presto_amd import abi
from presto_amd._lib import lib
from presto_amd.operators import DistinctLimitOperatorFactory, MarkDistinctOperatorFactory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["pa_mark_distinct_create", "pa_distinct_limit_create", "pa_distinct_stats"]
COMMON = ["input_channel_count", "input_types", "input_type_params", "distinct_channel_count", "distinct_channels", "hash_channel",
          "expected_distinct", "output_mem"]


def has_gpu():
    return lib().pa_device_count() > 0


def test_distinct_entry_points_are_exported():
    L = lib()
    for name in ENTRIES:
        assert getattr(L, name) is not None, name


def test_the_kernels_are_in_the_makefile_source_lists():
    text = open(os.path.join(ROOT, "presto_amd", "csrc", "Makefile")).read()
    assert "distinct_kernels.hip" in text and "op_distinct.cpp" in text


@pytest.mark.parametrize("struct,fields", [
    ("pa_mark_distinct_desc", COMMON + ["stream"]),
    ("pa_distinct_limit_desc", COMMON + ["limit", "stream"]),
])
def test_ctypes_layout_matches_the_header(struct, fields):
    """sizeof / offsetof of the C structs, printed by a C program compiled against include/presto_amd.h."""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "layout.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "presto_amd.h"\nint main(void) {\n')
            f.write('    printf("%%d\\n", (int)sizeof(%s));\n' % struct)
            for field in fields:
                f.write('    printf("%%d\\n", (int)offsetof(%s, %s));\n' % (struct, field))
            f.write("    return 0;\n}\n")
        exe = os.path.join(d, "layout")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    cls = getattr(abi, struct)
    assert [name for name, _ in cls._fields_] == fields
    assert got == [C.sizeof(cls)] + [getattr(cls, field).offset for field in fields]


def _create(factory):
    h = C.c_void_p()
    return factory._create(C.byref(factory._desc), C.byref(h))


def _both(types, channels, **kw):
    return [MarkDistinctOperatorFactory(types, channels, **kw), DistinctLimitOperatorFactory(types, channels, 10, **kw)]


@pytest.mark.skipif(has_gpu(), reason="container without a GPU only")
def test_no_device_fails_loudly():
    for t in (abi.BIGINT, abi.DOUBLE, abi.VARCHAR, abi.decimal(12, 2)):
        for f in _both([t, abi.BIGINT], [0], hash_channel=1) + _both([abi.BIGINT, t], [1, 0], output_mem=abi.MEM_DEVICE):
            assert _create(f) == abi.ERR_NO_DEVICE
    count, capacity = C.c_int64(), C.c_int64()
    assert lib().pa_distinct_stats(None, C.byref(count), C.byref(capacity)) == abi.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("key_type", [abi.decimal(30, 2), abi.ROW])
def test_key_types_outside_the_device_path_are_refused_at_creation(key_type):
    """The planner keeps the reference operators for these: the refusal comes before any device work (with or without a GPU)."""
    for f in _both([abi.BIGINT, key_type], [1]) + _both([abi.BIGINT, key_type], [0, 1]):
        assert _create(f) == abi.ERR_NOT_SUPPORTED


def test_nine_distinct_channels_are_refused_at_creation():
    for f in _both([abi.BIGINT] * 9, list(range(9))):
        assert _create(f) == abi.ERR_NOT_SUPPORTED


def test_bad_descriptors_are_invalid_arguments():
    for f in (_both([abi.BIGINT], [1])                                     # distinct channel out of range
              + _both([abi.BIGINT], [-1])
              + _both([abi.BIGINT, abi.DOUBLE], [0], hash_channel=1)       # $hashvalue not BIGINT
              + _both([abi.BIGINT], [0], hash_channel=1)                   # $hashvalue out of range
              + _both([abi.BIGINT], [])                                    # no distinct channel
              + _both([abi.BIGINT], [0], output_mem=7)
              + [DistinctLimitOperatorFactory([abi.BIGINT], [0], -1)]):    # negative limit
        assert _create(f) == abi.ERR_INVALID_ARGUMENT
    h = C.c_void_p()
    assert lib().pa_mark_distinct_create(None, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    assert lib().pa_distinct_limit_create(None, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    f = MarkDistinctOperatorFactory([abi.BIGINT], [0])
    assert lib().pa_mark_distinct_create(C.byref(f._desc), None) == abi.ERR_INVALID_ARGUMENT
