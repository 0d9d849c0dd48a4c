"""CPU-side checks of the semi-join entry points (SetBuilderOperator / HashSemiJoinOperator): exported, their ctypes mirrors laid
out as the header lays them out, shapes outside the device path refused before the device is asked for, and no device -> a loud
PA_ERR_NO_DEVICE.  No compute call is made here."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from presto_amd import abi
from presto_amd._lib import check, lib
from presto_amd.operators import HashSemiJoinOperatorFactory, SetBuilderOperatorFactory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["pa_channel_set_create", "pa_channel_set_destroy", "pa_channel_set_stats", "pa_set_builder_create", "pa_hash_semi_join_create"]


def has_gpu():
    return lib().pa_device_count() > 0


def test_semi_join_entry_points_are_exported():
    L = lib()
    for name in ENTRIES:
        assert getattr(L, name) is not None, name


@pytest.mark.parametrize("struct,fields", [
    ("pa_set_builder_desc", ["input_channel_count", "input_types", "input_type_params", "set_channel", "hash_channel", "expected_positions", "stream"]),
    ("pa_hash_semi_join_desc", ["probe_channel_count", "probe_types", "probe_type_params", "probe_join_channel", "probe_hash_channel",
                                "output_mem", "stream"]),
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
    assert got == [C.sizeof(cls)] + [getattr(cls, field).offset for field in fields]


def _create(factory, set_handle):
    h = C.c_void_p()
    return factory._create(C.byref(factory._desc), set_handle, C.byref(h))


@pytest.mark.skipif(has_gpu(), reason="container without a GPU only")
def test_no_device_fails_loudly():
    s = C.c_void_p()
    check(lib().pa_channel_set_create(C.byref(s)))
    try:
        for t in (abi.BIGINT, abi.DOUBLE, abi.VARCHAR, abi.decimal(12, 2)):
            assert _create(SetBuilderOperatorFactory([t, abi.BIGINT], 0, hash_channel=1), s) == abi.ERR_NO_DEVICE
            assert _create(HashSemiJoinOperatorFactory([abi.BIGINT, t], 1, output_mem=abi.MEM_DEVICE), s) == abi.ERR_NO_DEVICE
        size, has_null = C.c_int64(), C.c_int32()
        assert lib().pa_channel_set_stats(s, C.byref(size), C.byref(has_null)) == abi.ERR_ILLEGAL_STATE
    finally:
        check(lib().pa_channel_set_destroy(s))


@pytest.mark.parametrize("key_type,status", [(abi.decimal(30, 2), abi.ERR_NOT_SUPPORTED), (abi.ROW, abi.ERR_NOT_SUPPORTED)])
def test_key_types_outside_the_device_path_are_refused_at_creation(key_type, status):
    """The planner keeps the reference operators for these: the refusal comes before any device work (with or without a GPU)."""
    s = C.c_void_p()
    check(lib().pa_channel_set_create(C.byref(s)))
    try:
        assert _create(SetBuilderOperatorFactory([abi.BIGINT, key_type], 1), s) == status
        assert _create(HashSemiJoinOperatorFactory([key_type], 0), s) == status
    finally:
        check(lib().pa_channel_set_destroy(s))


def test_bad_descriptors_are_invalid_arguments():
    s = C.c_void_p()
    check(lib().pa_channel_set_create(C.byref(s)))
    try:
        assert _create(SetBuilderOperatorFactory([abi.BIGINT], 1), s) == abi.ERR_INVALID_ARGUMENT            # set channel out of range
        assert _create(SetBuilderOperatorFactory([abi.BIGINT, abi.DOUBLE], 0, hash_channel=1), s) == abi.ERR_INVALID_ARGUMENT  # $hashvalue not BIGINT
        assert _create(HashSemiJoinOperatorFactory([abi.BIGINT], 2), s) == abi.ERR_INVALID_ARGUMENT           # join channel out of range
        assert _create(HashSemiJoinOperatorFactory([abi.BIGINT, abi.INTEGER], 0, probe_hash_channel=1), s) == abi.ERR_INVALID_ARGUMENT
        h = C.c_void_p()
        assert lib().pa_set_builder_create(None, s, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    finally:
        check(lib().pa_channel_set_destroy(s))
