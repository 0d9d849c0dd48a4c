"""CPU-side checks of the TOP-N RANKING entry points (TopNRankingOperator): exported, the ctypes mirror laid out as the header lays it
out, shapes outside the device path refused before the device is asked for, and no device -> a loud PA_ERR_NO_DEVICE.  No compute call
is made here.  The library these tests load is linked from the Makefile's source lists, so topn_ranking_kernels.hip has been compiled
for gfx950 (off the GPU) when the export test passes."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from presto_amd import abi
from presto_amd._lib import lib
from presto_amd.operators import TopNRankingOperatorFactory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["pa_topn_ranking_create", "pa_topn_ranking_stats"]
FIELDS = ["input_channel_count", "input_types", "input_type_params", "output_channel_count", "output_channels", "partition_channel_count",
          "partition_channels", "sort_channel_count", "sort_channels", "sort_orders", "ranking_type", "max_row_count_per_partition", "partial",
          "hash_channel", "expected_positions", "output_mem", "stream"]
ASC_NULLS_LAST = 1


def has_gpu():
    return lib().pa_device_count() > 0


def test_topn_ranking_entry_points_are_exported():
    L = lib()
    for name in ENTRIES:
        assert getattr(L, name) is not None, name
    from presto_amd.operators import Operator, TopNRankingOperator   # noqa: F401  (the Python mirror)
    assert callable(Operator.topNRankingStats)
    assert (abi.RANKING_ROW_NUMBER, abi.RANKING_RANK, abi.RANKING_DENSE_RANK) == (0, 1, 2)


def test_the_kernels_are_in_the_makefile_source_lists():
    text = open(os.path.join(ROOT, "presto_amd", "csrc", "Makefile")).read()
    dev = [line for line in text.splitlines() if line.startswith("DEV_SRCS")][0]
    host = [line for line in text.splitlines() if line.startswith("HOST_SRCS")][0]
    assert "topn_ranking_kernels.hip" in dev.split() and "op_topn_ranking.cpp" in host.split()
    assert os.path.exists(os.path.join(ROOT, "presto_amd", "csrc", "topn_ranking_kernels.hpp"))


def test_ctypes_layout_matches_the_header():
    """sizeof / offsetof of the C struct, printed by a C program compiled against include/presto_amd.h."""
    struct = "pa_topn_ranking_desc"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "layout.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "presto_amd.h"\nint main(void) {\n')
            f.write('    printf("%%d\\n", (int)sizeof(%s));\n' % struct)
            for field in FIELDS:
                f.write('    printf("%%d\\n", (int)offsetof(%s, %s));\n' % (struct, field))
            f.write('    printf("%d %d %d\\n", (int)PA_RANKING_ROW_NUMBER, (int)PA_RANKING_RANK, (int)PA_RANKING_DENSE_RANK);\n')
            f.write("    return 0;\n}\n")
        exe = os.path.join(d, "layout")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    cls = abi.pa_topn_ranking_desc
    assert [name for name, _ in cls._fields_] == FIELDS
    assert got == [C.sizeof(cls)] + [getattr(cls, field).offset for field in FIELDS] + [0, 1, 2]


def _create(factory):
    h = C.c_void_p()
    return factory._create(C.byref(factory._desc), C.byref(h))


def _modes(types, output_channels, partition_channels, sort_channels, sort_orders=None, n=3, **kw):
    """both ranking types, partial and not"""
    orders = [ASC_NULLS_LAST] * len(sort_channels) if sort_orders is None else sort_orders
    return [TopNRankingOperatorFactory(types, output_channels, partition_channels, sort_channels, orders, n, ranking_type=r, partial=p, **kw)
            for r in (abi.RANKING_ROW_NUMBER, abi.RANKING_RANK) for p in (False, True)]


@pytest.mark.skipif(has_gpu(), reason="container without a GPU only")
def test_no_device_fails_loudly():
    for t in (abi.BIGINT, abi.DOUBLE, abi.VARCHAR, abi.REAL, abi.BOOLEAN, abi.DATE, abi.INTEGER):
        for f in (_modes([t, abi.BIGINT], [0, 1], [0], [1], hash_channel=1) + _modes([abi.BIGINT, t], [1], [1, 0], [1, 0], [2, 3], output_mem=abi.MEM_DEVICE)
                  + _modes([t], [0], [], [0], n=2 ** 31 - 1)):
            assert _create(f) == abi.ERR_NO_DEVICE
    # a short decimal may be a partition and an output channel
    for f in _modes([abi.decimal(12, 2), abi.BIGINT], [0, 1], [0], [1]):
        assert _create(f) == abi.ERR_NO_DEVICE


def test_stats_of_a_null_operator_is_an_invalid_argument():
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    assert lib().pa_topn_ranking_stats(None, C.byref(a), C.byref(b), C.byref(c)) == abi.ERR_INVALID_ARGUMENT


def test_dense_rank_is_refused_at_creation():
    """The reference throws UnsupportedOperationException; the planner keeps its own operator (and fails there)."""
    for partial in (False, True):
        f = TopNRankingOperatorFactory([abi.BIGINT, abi.DOUBLE], [0, 1], [0], [1], [ASC_NULLS_LAST], 3, ranking_type=abi.RANKING_DENSE_RANK, partial=partial)
        assert _create(f) == abi.ERR_NOT_SUPPORTED


@pytest.mark.parametrize("t", [abi.decimal(30, 2), abi.ROW])
def test_types_outside_the_device_path_are_refused_at_creation(t):
    """The planner keeps the reference operator for these: the refusal comes before any device work (with or without a GPU)."""
    for f in (_modes([abi.BIGINT, t], [0], [1], [0]) + _modes([abi.BIGINT, t], [0], [0, 1], [0])   # partition channel
              + _modes([abi.BIGINT, t], [0], [0], [1]) + _modes([abi.BIGINT, t], [0], [], [0, 1])   # sort channel
              + _modes([abi.BIGINT, t], [0, 1], [0], [0]) + _modes([abi.BIGINT, t], [1], [], [0])):  # output channel
        assert _create(f) == abi.ERR_NOT_SUPPORTED


def test_a_short_decimal_sort_channel_is_refused_at_creation():
    """(declared BIGINT by the planner glue, as for sorts elsewhere)"""
    for f in _modes([abi.BIGINT, abi.decimal(12, 2)], [0], [0], [1]):
        assert _create(f) == abi.ERR_NOT_SUPPORTED


def test_nine_partition_channels_are_refused_at_creation():
    for f in _modes([abi.BIGINT] * 9, [0], list(range(9)), [0]):
        assert _create(f) == abi.ERR_NOT_SUPPORTED


def test_bad_descriptors_are_invalid_arguments():
    one = [abi.BIGINT]
    for f in (_modes(one, [0], [0], [0], n=0)                                  # n <= 0
              + _modes(one, [0], [0], [0], n=-1)
              + _modes(one, [0], [0], [])                                      # no sort channels
              + _modes(one, [0], [0], [0], [4])                                # a sort order outside 0..3
              + _modes(one, [0], [0], [0], [-1])
              + _modes(one, [0], [1], [0])                                     # partition channel out of range
              + _modes(one, [0], [-1], [0])
              + _modes(one, [1], [0], [0])                                     # output channel out of range
              + _modes(one, [-1], [0], [0])
              + _modes(one, [0], [0], [1])                                     # sort channel out of range
              + _modes(one, [0], [0], [-1])
              + _modes([abi.BIGINT, abi.DOUBLE], [0], [0], [0], hash_channel=1)  # $hashvalue not BIGINT
              + _modes(one, [0], [0], [0], hash_channel=1)                     # $hashvalue out of range
              + _modes(one, [0], [0], [0], hash_channel=-2)
              + _modes(one, [0], [0], [0], output_mem=7)
              + _modes(one, [0], [0], [0], expected_positions=-1)
              + _modes([77], [0], [0], [0])                                    # unknown type
              + [TopNRankingOperatorFactory(one, [0], [0], [0], [0], 3, ranking_type=3),
                 TopNRankingOperatorFactory(one, [0], [0], [0], [0], 3, ranking_type=-1),
                 TopNRankingOperatorFactory(one, [0], [0], [0], [0], 3, partial=2),
                 TopNRankingOperatorFactory(one, [0], [0], [0], [0], 3, partial=-1)]):
        assert _create(f) == abi.ERR_INVALID_ARGUMENT
    h = C.c_void_p()
    assert lib().pa_topn_ranking_create(None, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    f = _modes(one, [0], [0], [0])[0]
    assert lib().pa_topn_ranking_create(C.byref(f._desc), None) == abi.ERR_INVALID_ARGUMENT
    for field in ("partition_channels", "output_channels", "sort_channels", "sort_orders", "input_types"):   # a count without the array
        f = _modes(one, [0], [0], [0])[0]
        setattr(f._desc, field, None)
        assert _create(f) == abi.ERR_INVALID_ARGUMENT, field


def test_the_jni_shim_exports_the_entry_points():
    """jni/presto_amd_jni.c against the stub jni.h: the symbols GpuNative.createTopNRanking / topNRankingStats bind to."""
    with tempfile.TemporaryDirectory() as d:
        obj = os.path.join(d, "shim.o")
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-fPIC", "-c", "-I", os.path.join(ROOT, "jni", "stub"), "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "jni", "presto_amd_jni.c"), "-o", obj], check=True)
        symbols = subprocess.run(["nm", "-g", "--defined-only", obj], check=True, capture_output=True, text=True).stdout
    assert "Java_io_trino_gpu_GpuNative_createTopNRanking" in symbols
    assert "Java_io_trino_gpu_GpuNative_topNRankingStats" in symbols
    java = open(os.path.join(ROOT, "java", "io", "trino", "gpu", "GpuNative.java")).read()
    assert "createTopNRanking" in java and "topNRankingStats" in java
    assert os.path.exists(os.path.join(ROOT, "java", "io", "trino", "gpu", "GpuTopNRanking.java"))
