"""CPU-side checks of the framed WINDOW entry point (pa_framed_window_create: the ranking functions and count / sum / min / max over the
frames that start at UNBOUNDED PRECEDING): exported, the ctypes mirrors and enum values laid out as the header lays them out, every
invalid argument and every refusal of the contract reported at creation -- an invalid argument before a refusal, both before the device
is asked for -- and no device -> a loud PA_ERR_NO_DEVICE.  No compute call is made here."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from presto_amd import abi
from presto_amd._lib import lib
from presto_amd.operators import DEFAULT_FRAME, FramedWindowOperatorFactory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC_FIELDS = ["input_channel_count", "input_types", "input_type_params", "output_channel_count", "output_channels", "function_count", "functions",
               "partition_channel_count", "partition_channels", "sort_channel_count", "sort_channels", "sort_orders", "pre_grouped_channel_count",
               "pre_sorted_channel_prefix", "expected_positions", "output_mem", "stream"]
FUNCTION_FIELDS = ["function", "argument_count", "argument_channels", "frame_type", "start_type", "start_channel", "end_type", "end_channel", "ignore_nulls"]
ENUMS = [("PA_WINDOW_COUNT_STAR", abi.WINDOW_COUNT_STAR, 6), ("PA_WINDOW_COUNT", abi.WINDOW_COUNT, 7), ("PA_WINDOW_SUM", abi.WINDOW_SUM, 8),
         ("PA_WINDOW_MIN", abi.WINDOW_MIN, 9), ("PA_WINDOW_MAX", abi.WINDOW_MAX, 10),
         ("PA_FRAME_RANGE", abi.FRAME_RANGE, 0), ("PA_FRAME_ROWS", abi.FRAME_ROWS, 1), ("PA_FRAME_GROUPS", abi.FRAME_GROUPS, 2),
         ("PA_BOUND_UNBOUNDED_PRECEDING", abi.BOUND_UNBOUNDED_PRECEDING, 0), ("PA_BOUND_PRECEDING", abi.BOUND_PRECEDING, 1),
         ("PA_BOUND_CURRENT_ROW", abi.BOUND_CURRENT_ROW, 2), ("PA_BOUND_FOLLOWING", abi.BOUND_FOLLOWING, 3),
         ("PA_BOUND_UNBOUNDED_FOLLOWING", abi.BOUND_UNBOUNDED_FOLLOWING, 4)]
RANKING = [abi.WINDOW_ROW_NUMBER, abi.WINDOW_RANK, abi.WINDOW_DENSE_RANK, abi.WINDOW_PERCENT_RANK, abi.WINDOW_CUME_DIST]
AGGREGATES = [abi.WINDOW_COUNT_STAR, abi.WINDOW_COUNT, abi.WINDOW_SUM, abi.WINDOW_MIN, abi.WINDOW_MAX]
ASC_NULLS_LAST = 1
UP, P, CR, F, UF = abi.BOUND_UNBOUNDED_PRECEDING, abi.BOUND_PRECEDING, abi.BOUND_CURRENT_ROW, abi.BOUND_FOLLOWING, abi.BOUND_UNBOUNDED_FOLLOWING
# the frames the device path takes: every type x (UNBOUNDED PRECEDING .. CURRENT ROW | UNBOUNDED FOLLOWING)
TAKEN = [(t, UP, e) for t in (abi.FRAME_RANGE, abi.FRAME_ROWS, abi.FRAME_GROUPS) for e in (CR, UF)]
MIN_MAX_TYPES = [abi.BIGINT, abi.INTEGER, abi.DATE, abi.BOOLEAN, abi.decimal(12, 2), abi.DOUBLE, abi.REAL]


def has_gpu():
    return lib().pa_device_count() > 0


def _create(factory):
    h = C.c_void_p()
    return factory._create(C.byref(factory._desc), C.byref(h))


def _window(types, output_channels=(0,), functions=(abi.WINDOW_COUNT_STAR,), partition_channels=(0,), sort_channels=(0,), sort_orders=None, **kw):
    orders = [ASC_NULLS_LAST] * len(sort_channels) if sort_orders is None else sort_orders
    return FramedWindowOperatorFactory(list(types), list(output_channels), list(functions), list(partition_channels), list(sort_channels), list(orders), **kw)


def argument(f):
    return [] if f in RANKING + [abi.WINDOW_COUNT_STAR] else [1]


def test_framed_window_entry_point_is_exported():
    assert getattr(lib(), "pa_framed_window_create") is not None
    from presto_amd.operators import FramedWindowOperator   # noqa: F401  (the Python mirror)
    assert AGGREGATES == [6, 7, 8, 9, 10]
    assert DEFAULT_FRAME == (abi.FRAME_RANGE, abi.BOUND_UNBOUNDED_PRECEDING, abi.BOUND_CURRENT_ROW)


def test_ctypes_layout_and_enum_values_match_the_header():
    """sizeof / offsetof of the C structs and the enumerators, printed by a C program compiled against include/presto_amd.h."""
    structs = [("pa_framed_window_desc", DESC_FIELDS, abi.pa_framed_window_desc),
               ("pa_framed_window_function_desc", FUNCTION_FIELDS, abi.pa_framed_window_function_desc)]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "layout.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "presto_amd.h"\nint main(void) {\n')
            for struct, fields, _ in structs:
                f.write('    printf("%%d\\n", (int)sizeof(%s));\n' % struct)
                for field in fields:
                    f.write('    printf("%%d\\n", (int)offsetof(%s, %s));\n' % (struct, field))
            for name, _, _ in ENUMS:
                f.write('    printf("%%d\\n", (int)%s);\n' % name)
            # the framed descriptor is the unframed one around another function descriptor
            for field in DESC_FIELDS:
                f.write('    printf("%%d\\n", (int)(offsetof(pa_framed_window_desc, %s) == offsetof(pa_window_desc, %s)));\n' % (field, field))
            f.write("    return 0;\n}\n")
        exe = os.path.join(d, "layout")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for _, fields, cls in structs:
        assert [name for name, _ in cls._fields_] == fields
        want += [C.sizeof(cls)] + [getattr(cls, field).offset for field in fields]
    assert [mirror for _, mirror, _ in ENUMS] == [value for _, _, value in ENUMS]
    assert got == want + [value for _, _, value in ENUMS] + [1] * len(DESC_FIELDS)


@pytest.mark.skipif(has_gpu(), reason="container without a GPU only")
def test_no_device_fails_loudly():
    """What the device path takes passes every check and then asks for the device."""
    two = [abi.BIGINT, abi.BIGINT]
    for frame in TAKEN:
        assert _create(_window(two, functions=[(f, argument(f), frame) for f in AGGREGATES])) == abi.ERR_NO_DEVICE, frame
    assert _create(_window(two, functions=AGGREGATES[:1] + [(f, [1]) for f in AGGREGATES[1:]])) == abi.ERR_NO_DEVICE          # the default frame
    assert _create(_window([abi.BIGINT, abi.INTEGER], functions=[(abi.WINDOW_SUM, [1])])) == abi.ERR_NO_DEVICE
    for t in MIN_MAX_TYPES:
        assert _create(_window([abi.BIGINT, t], functions=[(abi.WINDOW_MIN, [1]), (abi.WINDOW_MAX, [1]), (abi.WINDOW_COUNT, [1])])) == abi.ERR_NO_DEVICE, t
    for t in (abi.VARCHAR, abi.decimal(30, 2)):                                                                                 # count reads the NULLs only
        assert _create(_window([abi.BIGINT, t], functions=[(abi.WINDOW_COUNT, [1], (abi.FRAME_ROWS, UP, CR))])) == abi.ERR_NO_DEVICE, t
    # the ranking functions: any well-formed frame, ignored
    six = RANKING + [(abi.WINDOW_NTILE, [1])]
    assert _create(_window(two, [0, 1], six + AGGREGATES[:1], [0], [0])) == abi.ERR_NO_DEVICE
    for frame in [(abi.FRAME_ROWS, P, F, 1, 1, 0), (abi.FRAME_RANGE, CR, CR), (abi.FRAME_GROUPS, F, UF, 0, -1, 0), (abi.FRAME_ROWS, UP, P, -1, 0, 0)]:
        assert _create(_window(two, functions=[(f, [], frame) for f in RANKING] + [(abi.WINDOW_NTILE, [1], frame)])) == abi.ERR_NO_DEVICE, frame
    # a channel is read only where the bound takes one
    assert _create(_window(two, functions=[(abi.WINDOW_SUM, [1], (abi.FRAME_ROWS, UP, CR, 99, -5, 0))])) == abi.ERR_NO_DEVICE
    # 16 functions, 8 partition channels, no partition and no sort channels, device output
    assert _create(_window([abi.BIGINT] * 8, [0], [(abi.WINDOW_MAX, [k % 8]) for k in range(16)], list(range(8)), [], expected_positions=10)) == abi.ERR_NO_DEVICE
    assert _create(_window(two, [], [(abi.WINDOW_SUM, [0])], [], [], output_mem=abi.MEM_DEVICE)) == abi.ERR_NO_DEVICE


def test_other_frames_of_an_aggregate_are_refused_at_creation():
    two = [abi.BIGINT, abi.BIGINT]
    refused = [(t, s, e, 1 if s in (P, F) else -1, 1 if e in (P, F) else -1, 0) for t in (abi.FRAME_RANGE, abi.FRAME_ROWS, abi.FRAME_GROUPS)
               for s in (UP, P, CR, F) for e in (P, CR, F, UF) if not (s == UP and e in (CR, UF))]
    assert len(refused) == 3 * 14
    for frame in refused:
        for f in AGGREGATES:
            assert _create(_window(two, functions=[(f, argument(f), frame)])) == abi.ERR_NOT_SUPPORTED, (f, frame)
    # ... also behind functions that are taken
    assert _create(_window(two, functions=[abi.WINDOW_RANK, (abi.WINDOW_SUM, [1]), (abi.WINDOW_SUM, [1], (abi.FRAME_ROWS, CR, UF))])) == abi.ERR_NOT_SUPPORTED


def test_argument_types_outside_the_device_path_are_refused_at_creation():
    for t in (abi.DOUBLE, abi.REAL, abi.decimal(12, 2), abi.decimal(30, 2)):
        assert _create(_window([abi.BIGINT, t], functions=[(abi.WINDOW_SUM, [1])])) == abi.ERR_NOT_SUPPORTED, t
    for t in (abi.VARCHAR, abi.decimal(30, 2), abi.ROW):
        for f in (abi.WINDOW_MIN, abi.WINDOW_MAX):
            assert _create(_window([abi.BIGINT, t], functions=[(f, [1])])) == abi.ERR_NOT_SUPPORTED, (f, t)
    assert _create(_window([abi.BIGINT, abi.ROW], functions=[(abi.WINDOW_COUNT, [1])])) == abi.ERR_NOT_SUPPORTED


def test_what_the_unframed_descriptor_refuses_is_refused():
    one = [abi.BIGINT]
    assert _create(_window(one, pre_grouped_channel_count=1)) == abi.ERR_NOT_SUPPORTED
    assert _create(_window(one, pre_sorted_channel_prefix=1)) == abi.ERR_NOT_SUPPORTED
    assert _create(_window([abi.BIGINT] * 9, partition_channels=list(range(9)))) == abi.ERR_NOT_SUPPORTED
    for t in (abi.decimal(30, 2), abi.ROW):
        assert _create(_window([abi.BIGINT, t], partition_channels=[1])) == abi.ERR_NOT_SUPPORTED
        assert _create(_window([abi.BIGINT, t], sort_channels=[1])) == abi.ERR_NOT_SUPPORTED
    assert _create(_window([abi.BIGINT, abi.ROW], [0, 1])) == abi.ERR_NOT_SUPPORTED


def test_malformed_frames_are_invalid_arguments():
    two = [abi.BIGINT, abi.BIGINT]
    malformed = [(3, UP, CR), (-1, UP, CR),                                    # frame type out of range
                 (abi.FRAME_ROWS, 5, CR), (abi.FRAME_ROWS, -1, CR),            # start type out of range
                 (abi.FRAME_ROWS, UP, 5), (abi.FRAME_ROWS, UP, -1),            # end type out of range
                 (abi.FRAME_RANGE, UF, UF), (abi.FRAME_ROWS, UF, CR),          # start UNBOUNDED FOLLOWING
                 (abi.FRAME_RANGE, UP, UP), (abi.FRAME_GROUPS, CR, UP),        # end UNBOUNDED PRECEDING
                 (abi.FRAME_ROWS, P, CR, 2, -1, 0), (abi.FRAME_ROWS, P, CR, -1, -1, 0), (abi.FRAME_ROWS, F, UF, 2, -1, 0),      # a bound's channel out of range
                 (abi.FRAME_ROWS, UP, F, -1, 2, 0), (abi.FRAME_ROWS, UP, P, -1, -1, 0), (abi.FRAME_GROUPS, CR, F, -1, -7, 0)]
    for frame in malformed:
        for f in AGGREGATES + RANKING:                                         # (range-checked for the ranking functions too)
            assert _create(_window(two, functions=[(f, argument(f), frame)])) == abi.ERR_INVALID_ARGUMENT, (f, frame)


def test_ignore_nulls_is_an_invalid_argument():
    two = [abi.BIGINT, abi.BIGINT]
    for f in AGGREGATES:
        for flag in (1, -1, 2):
            assert _create(_window(two, functions=[(f, argument(f), (abi.FRAME_RANGE, UP, CR, -1, -1, flag))])) == abi.ERR_INVALID_ARGUMENT, (f, flag)


def test_bad_function_lists_are_invalid_arguments():
    two = [abi.BIGINT, abi.INTEGER]
    for functions in ([11], [-1], [99], [(abi.WINDOW_SUM, [1]), 11],                     # unknown function ids
                      [(abi.WINDOW_COUNT_STAR, [0])], [(abi.WINDOW_RANK, [0])],                              # an argument where none is taken
                      [(abi.WINDOW_COUNT, [])], [(abi.WINDOW_SUM, [])], [(abi.WINDOW_MIN, [])], [(abi.WINDOW_MAX, [])], [(abi.WINDOW_NTILE, [])],
                      [(abi.WINDOW_COUNT, [0, 1])], [(abi.WINDOW_SUM, [0, 1])], [(abi.WINDOW_MIN, [0, 1])], [(abi.WINDOW_MAX, [0, 1])],
                      [(abi.WINDOW_SUM, [2])], [(abi.WINDOW_MIN, [-1])], [(abi.WINDOW_COUNT, [2])],          # argument channel out of range
                      [],                                                                                    # function_count outside 1 .. 16
                      [(abi.WINDOW_SUM, [1])] * 17):
        assert _create(_window(two, functions=functions)) == abi.ERR_INVALID_ARGUMENT, functions
    for t in (abi.VARCHAR, abi.BOOLEAN, abi.DATE):                                                           # there is no such sum
        assert _create(_window([abi.BIGINT, t], functions=[(abi.WINDOW_SUM, [1])])) == abi.ERR_INVALID_ARGUMENT, t
    for t in (abi.DOUBLE, abi.VARCHAR, abi.decimal(12, 2)):                                                  # ntile as through pa_window_create
        assert _create(_window([abi.BIGINT, t], functions=[(abi.WINDOW_NTILE, [1])])) == abi.ERR_INVALID_ARGUMENT, t
    f = _window(two)
    f._desc.functions = None
    assert _create(f) == abi.ERR_INVALID_ARGUMENT
    f = _window(two, functions=[(abi.WINDOW_SUM, [1])])
    f._desc.functions[0].argument_channels = None
    assert _create(f) == abi.ERR_INVALID_ARGUMENT
    f = _window(two)
    f._desc.function_count = -1
    assert _create(f) == abi.ERR_INVALID_ARGUMENT


def test_bad_descriptors_are_invalid_arguments():
    one = [abi.BIGINT]
    for f in (_window(one, sort_orders=[4]), _window(one, partition_channels=[1]), _window(one, output_channels=[-1]), _window(one, sort_channels=[1]),
              _window(one, output_mem=7), _window(one, expected_positions=-1), _window([77])):
        assert _create(f) == abi.ERR_INVALID_ARGUMENT
    h = C.c_void_p()
    assert lib().pa_framed_window_create(None, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    assert lib().pa_framed_window_create(C.byref(_window(one)._desc), None) == abi.ERR_INVALID_ARGUMENT
    for field in ("partition_channels", "output_channels", "sort_channels", "sort_orders", "input_types"):   # a count without the array
        f = _window(one)
        setattr(f._desc, field, None)
        assert _create(f) == abi.ERR_INVALID_ARGUMENT, field


def test_an_invalid_argument_is_reported_before_a_refusal():
    """Where a descriptor has both defects the bad argument decides, as for the sibling operators."""
    two = [abi.BIGINT, abi.DOUBLE]
    bounded = (abi.FRAME_ROWS, CR, UF)                                          # well formed, refused
    assert _create(_window(two, functions=[(abi.WINDOW_SUM, [0], bounded)])) == abi.ERR_NOT_SUPPORTED
    assert _create(_window(two, functions=[(abi.WINDOW_SUM, [0], bounded), 11])) == abi.ERR_INVALID_ARGUMENT
    assert _create(_window(two, functions=[(abi.WINDOW_SUM, [1]), (abi.WINDOW_COUNT, [])])) == abi.ERR_INVALID_ARGUMENT      # a DOUBLE sum, then a bad count
    assert _create(_window(two, functions=[(abi.WINDOW_SUM, [0], bounded), (abi.WINDOW_MIN, [0], (abi.FRAME_ROWS, UF, UF))])) == abi.ERR_INVALID_ARGUMENT
    assert _create(_window(two, functions=[(abi.WINDOW_SUM, [0], (abi.FRAME_ROWS, UP, CR, -1, -1, 1))], pre_grouped_channel_count=1)) == abi.ERR_INVALID_ARGUMENT
    assert _create(_window(two, functions=[(abi.WINDOW_SUM, [1])], output_mem=7)) == abi.ERR_INVALID_ARGUMENT
    assert _create(_window([abi.BIGINT] * 9, partition_channels=list(range(8)) + [9])) == abi.ERR_INVALID_ARGUMENT


def test_the_unframed_entry_point_still_knows_six_functions():
    from presto_amd.operators import WindowOperatorFactory
    for f in AGGREGATES:
        factory = WindowOperatorFactory([abi.BIGINT, abi.BIGINT], [0], [(f, argument(f))], [0], [0], [ASC_NULLS_LAST])
        assert _create(factory) == abi.ERR_INVALID_ARGUMENT
        assert b"unknown window function" in lib().pa_last_error()


def test_the_jni_shim_exports_the_entry_point():
    """jni/presto_amd_jni.c against the stub jni.h: the symbol GpuNative.createFramedWindow binds to, and the Java names."""
    with tempfile.TemporaryDirectory() as d:
        obj = os.path.join(d, "shim.o")
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-fPIC", "-c", "-I", os.path.join(ROOT, "jni", "stub"), "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "jni", "presto_amd_jni.c"), "-o", obj], check=True)
        symbols = subprocess.run(["nm", "-g", "--defined-only", obj], check=True, capture_output=True, text=True).stdout
    assert "Java_io_trino_gpu_GpuNative_createFramedWindow" in symbols
    java = open(os.path.join(ROOT, "java", "io", "trino", "gpu", "GpuNative.java")).read()
    assert "createFramedWindow" in java
    glue = open(os.path.join(ROOT, "java", "io", "trino", "gpu", "GpuWindow.java")).read()
    assert "GpuNative.createFramedWindow(" in glue and "GpuNative.createWindow(" in glue
    for name in ("count", "sum", "min", "max", "row_number", "rank", "dense_rank", "percent_rank", "cume_dist", "ntile"):
        assert '"%s"' % name in glue


def test_the_cpp_mirror_and_the_kernels_are_there():
    header = open(os.path.join(ROOT, "include", "presto_amd.hpp")).read()
    assert "struct FramedWindowFunctionDefinition" in header and "struct FramedWindowOperatorFactory" in header and "pa_framed_window_create(" in header
    kernels = open(os.path.join(ROOT, "presto_amd", "csrc", "window_kernels.hpp")).read()
    assert "kWindowScanTile" in kernels and "launch_window_scan(" in kernels and "launch_window_gather(" in kernels
