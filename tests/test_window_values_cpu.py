"""CPU-side checks of the value window functions (lag / lead / first_value / last_value / nth_value, ids 11 .. 15 of pa_framed_window_create):
the enum values laid out as the header lays them out, every accepted shape passing every check and asking for the device, every invalid
argument and every refusal of the contract reported at creation -- an invalid argument before a refusal, both before the device is asked
for.  No compute call is made here."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from presto_amd import abi
from presto_amd._lib import lib
from presto_amd.operators import FramedWindowOperatorFactory, WindowOperatorFactory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENUMS = [("PA_WINDOW_LAG", "WINDOW_LAG", 11), ("PA_WINDOW_LEAD", "WINDOW_LEAD", 12), ("PA_WINDOW_FIRST_VALUE", "WINDOW_FIRST_VALUE", 13),
         ("PA_WINDOW_LAST_VALUE", "WINDOW_LAST_VALUE", 14), ("PA_WINDOW_NTH_VALUE", "WINDOW_NTH_VALUE", 15)]
LAG, LEAD, FIRST_VALUE, LAST_VALUE, NTH_VALUE = 11, 12, 13, 14, 15
SHIFTS, FRAMED = [LAG, LEAD], [FIRST_VALUE, LAST_VALUE, NTH_VALUE]
ASC_NULLS_LAST = 1
UP, P, CR, F, UF = abi.BOUND_UNBOUNDED_PRECEDING, abi.BOUND_PRECEDING, abi.BOUND_CURRENT_ROW, abi.BOUND_FOLLOWING, abi.BOUND_UNBOUNDED_FOLLOWING
FRAME_TYPES = (abi.FRAME_RANGE, abi.FRAME_ROWS, abi.FRAME_GROUPS)
# the frames the device path takes: every type x (UNBOUNDED PRECEDING .. CURRENT ROW | UNBOUNDED FOLLOWING) ...
TAKEN = [(t, UP, e) for t in FRAME_TYPES for e in (CR, UF)]
# ... and every other well-formed frame
UNTAKEN = [(t, s, e, 1 if s in (P, F) else -1, 1 if e in (P, F) else -1, 0) for t in FRAME_TYPES for s in (UP, P, CR, F) for e in (P, CR, F, UF)
           if not (s == UP and e in (CR, UF))]
VALUE_TYPES = [abi.BIGINT, abi.INTEGER, abi.DATE, abi.DOUBLE, abi.REAL, abi.BOOLEAN, abi.decimal(12, 2), abi.decimal(30, 2)]
# channels of `TYPES`: 0 key, 1 a BIGINT value, 2 a BIGINT offset, 3 an INTEGER offset, 4 a BIGINT default
TYPES = [abi.BIGINT, abi.BIGINT, abi.BIGINT, abi.INTEGER, abi.BIGINT]


def has_gpu():
    return lib().pa_device_count() > 0


def _create(factory):
    h = C.c_void_p()
    status = factory._create(C.byref(factory._desc), C.byref(h))
    if status == 0 and h.value:                            # (with a device: the operator exists)
        lib().pa_op_close(h)
    return status


def _window(types, functions, output_channels=(0,), partition_channels=(0,), sort_channels=(0,), **kw):
    return FramedWindowOperatorFactory(list(types), list(output_channels), list(functions), list(partition_channels), list(sort_channels),
                                       [ASC_NULLS_LAST] * len(sort_channels), **kw)


def accepted_arguments(f):
    """every accepted argument list of function f over TYPES"""
    if f in SHIFTS:
        return [[1], [1, 2], [1, 3], [1, 2, 4], [1, 3, 4]]
    return [[1, 2], [1, 3]] if f == NTH_VALUE else [[1]]


def test_enum_values_match_the_header():
    """the enumerators, printed by a C program compiled against include/presto_amd.h, against the ids of the contract and abi.py"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "values.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include "presto_amd.h"\nint main(void) {\n')
            for name, _, _ in ENUMS:
                f.write('    printf("%%d\\n", (int)%s);\n' % name)
            f.write("    return 0;\n}\n")
        exe = os.path.join(d, "values")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [value for _, _, value in ENUMS]
    assert [getattr(abi, mirror) for _, mirror, _ in ENUMS] == got


@pytest.mark.skipif(has_gpu(), reason="container without a GPU only")
def test_accepted_shapes_ask_for_the_device():
    """What the device path takes passes every check and then asks for the device."""
    for f in SHIFTS + FRAMED:
        for args in accepted_arguments(f):
            assert _create(_window(TYPES, [(f, args)])) == abi.ERR_NO_DEVICE, (f, args)                 # the default frame
            for frame in TAKEN:
                assert _create(_window(TYPES, [(f, args, frame)])) == abi.ERR_NO_DEVICE, (f, args, frame)
            assert _create(_window(TYPES, [(f, args, (abi.FRAME_ROWS, UP, CR, -1, -1, 0))])) == abi.ERR_NO_DEVICE      # ignore_nulls = 0, spelled out
    # every value type; the default of lag / lead has the value's type
    for t in VALUE_TYPES:
        types = [abi.BIGINT, t, abi.BIGINT, t]
        functions = [(LAG, [1]), (LEAD, [1, 2]), (LAG, [1, 2, 3]), (LEAD, [3, 2, 1]), (FIRST_VALUE, [1]), (LAST_VALUE, [3]), (NTH_VALUE, [1, 2])]
        assert _create(_window(types, functions)) == abi.ERR_NO_DEVICE, t
    # lag / lead: any well-formed frame, ignored
    for frame in UNTAKEN + [(abi.FRAME_ROWS, P, F, 1, 1, 0), (abi.FRAME_ROWS, UP, CR, 99, -5, 0)]:
        assert _create(_window(TYPES, [(f, [1, 2, 4], frame) for f in SHIFTS])) == abi.ERR_NO_DEVICE, frame
    # next to the ranking functions and the aggregates; 16 functions; a value channel that is also the key; device output
    mixed = [abi.WINDOW_RANK, (abi.WINDOW_SUM, [1]), (LAG, [1]), (abi.WINDOW_NTILE, [2]), (LAST_VALUE, [1], (abi.FRAME_ROWS, UP, UF))]
    assert _create(_window(TYPES, mixed)) == abi.ERR_NO_DEVICE
    assert _create(_window(TYPES, [(LAG, [k % 5, 2 + k % 2]) for k in range(16)])) == abi.ERR_NO_DEVICE
    assert _create(_window(TYPES, [(LEAD, [0, 0, 0])], [], [], [], output_mem=abi.MEM_DEVICE)) == abi.ERR_NO_DEVICE


def test_wrong_argument_counts_are_invalid_arguments():
    for f in SHIFTS + FRAMED:
        assert _create(_window(TYPES, [(f, [])])) == abi.ERR_INVALID_ARGUMENT, f
        assert _create(_window(TYPES, [f])) == abi.ERR_INVALID_ARGUMENT, f
    for f in SHIFTS:
        assert _create(_window(TYPES, [(f, [1, 2, 4, 4])])) == abi.ERR_INVALID_ARGUMENT, f
    for f in (FIRST_VALUE, LAST_VALUE):
        assert _create(_window(TYPES, [(f, [1, 2])])) == abi.ERR_INVALID_ARGUMENT, f
    assert _create(_window(TYPES, [(NTH_VALUE, [1])])) == abi.ERR_INVALID_ARGUMENT
    assert _create(_window(TYPES, [(NTH_VALUE, [1, 2, 4])])) == abi.ERR_INVALID_ARGUMENT
    factory = _window(TYPES, [(LAG, [1])])
    factory._desc.functions[0].argument_channels = None
    assert _create(factory) == abi.ERR_INVALID_ARGUMENT


def test_argument_channels_out_of_range_are_invalid_arguments():
    for bad in (5, -1, 99):
        for f in SHIFTS:
            for args in ([bad], [bad, 2], [1, bad], [bad, 2, 4], [1, bad, 4], [1, 2, bad]):
                assert _create(_window(TYPES, [(f, args)])) == abi.ERR_INVALID_ARGUMENT, (f, args)
        for f in (FIRST_VALUE, LAST_VALUE):
            assert _create(_window(TYPES, [(f, [bad])])) == abi.ERR_INVALID_ARGUMENT, (f, bad)
        for args in ([bad, 2], [1, bad]):
            assert _create(_window(TYPES, [(NTH_VALUE, args)])) == abi.ERR_INVALID_ARGUMENT, args


def test_offset_channel_types_other_than_bigint_and_integer_are_invalid_arguments():
    for t in (abi.DOUBLE, abi.VARCHAR, abi.decimal(12, 2), abi.decimal(30, 2), abi.DATE, abi.BOOLEAN, abi.REAL):
        types = [abi.BIGINT, abi.BIGINT, t]
        for f, args in ((LAG, [1, 2]), (LEAD, [1, 2]), (LAG, [1, 2, 1]), (NTH_VALUE, [1, 2])):
            assert _create(_window(types, [(f, args)])) == abi.ERR_INVALID_ARGUMENT, (t, f)


def test_a_default_of_another_type_is_an_invalid_argument():
    others = [abi.BIGINT, abi.INTEGER, abi.DATE, abi.DOUBLE, abi.REAL, abi.BOOLEAN, abi.VARCHAR, abi.decimal(12, 2), abi.decimal(30, 2)]
    for value in others:
        for default in others:
            want = None if int(value) == int(default) else abi.ERR_INVALID_ARGUMENT
            for f in SHIFTS:
                got = _create(_window([abi.BIGINT, value, abi.BIGINT, default], [(f, [1, 2, 3])]))
                if want is not None:
                    assert got == want, (value, default)
                else:
                    assert got != abi.ERR_INVALID_ARGUMENT, (value, default)
    # DECIMAL: the same type parameter
    for value, default in ((abi.decimal(12, 2), abi.decimal(12, 3)), (abi.decimal(12, 2), abi.decimal(13, 2)), (abi.decimal(30, 2), abi.decimal(30, 4)),
                           (abi.decimal(30, 2), abi.decimal(31, 2))):
        for f in SHIFTS:
            assert _create(_window([abi.BIGINT, value, abi.BIGINT, default], [(f, [1, 2, 3])])) == abi.ERR_INVALID_ARGUMENT, (value, default)


def test_ignore_nulls():
    """0 is taken, 1 is well formed and refused, anything else is malformed; for ids 0 .. 10 non-zero stays malformed"""
    for f in SHIFTS + FRAMED:
        args = accepted_arguments(f)[-1]
        assert _create(_window(TYPES, [(f, args, (abi.FRAME_RANGE, UP, CR, -1, -1, 1))])) == abi.ERR_NOT_SUPPORTED, f
        for flag in (2, -1):
            assert _create(_window(TYPES, [(f, args, (abi.FRAME_RANGE, UP, CR, -1, -1, flag))])) == abi.ERR_INVALID_ARGUMENT, (f, flag)
    for f, args in ((abi.WINDOW_RANK, []), (abi.WINDOW_NTILE, [2]), (abi.WINDOW_COUNT_STAR, []), (abi.WINDOW_SUM, [1]), (abi.WINDOW_MAX, [1])):
        for flag in (1, 2, -1):
            assert _create(_window(TYPES, [(f, args, (abi.FRAME_RANGE, UP, CR, -1, -1, flag))])) == abi.ERR_INVALID_ARGUMENT, (f, flag)


def test_a_varchar_value_is_refused():
    types = [abi.BIGINT, abi.VARCHAR, abi.BIGINT, abi.VARCHAR]
    for f, args in ((LAG, [1]), (LEAD, [1, 2]), (LAG, [1, 2, 3]), (FIRST_VALUE, [1]), (LAST_VALUE, [1]), (NTH_VALUE, [1, 2])):
        assert _create(_window(types, [(f, args)])) == abi.ERR_NOT_SUPPORTED, f
    assert _create(_window([abi.BIGINT, abi.ROW], [(LAG, [1])])) == abi.ERR_NOT_SUPPORTED


def test_other_frames_of_first_last_and_nth_value_are_refused():
    assert len(UNTAKEN) == 14 * 3
    for frame in UNTAKEN:
        for f in FRAMED:
            assert _create(_window(TYPES, [(f, accepted_arguments(f)[0], frame)])) == abi.ERR_NOT_SUPPORTED, (f, frame)
    # ... also behind functions that are taken
    assert _create(_window(TYPES, [abi.WINDOW_RANK, (LAG, [1]), (FIRST_VALUE, [1], (abi.FRAME_ROWS, CR, UF))])) == abi.ERR_NOT_SUPPORTED


def test_malformed_frames_are_invalid_arguments():
    malformed = [(3, UP, CR), (abi.FRAME_ROWS, 5, CR), (abi.FRAME_ROWS, UP, -1), (abi.FRAME_RANGE, UF, UF), (abi.FRAME_RANGE, UP, UP),
                 (abi.FRAME_ROWS, P, CR, 5, -1, 0), (abi.FRAME_ROWS, UP, F, -1, -1, 0)]
    for frame in malformed:
        for f in SHIFTS + FRAMED:                          # (range-checked for lag / lead too)
            assert _create(_window(TYPES, [(f, accepted_arguments(f)[0], frame)])) == abi.ERR_INVALID_ARGUMENT, (f, frame)


def test_an_invalid_argument_is_reported_before_a_refusal():
    """An invalid argument in a later function wins over a refusal in an earlier one."""
    types = [abi.BIGINT, abi.VARCHAR, abi.DOUBLE, abi.BIGINT]
    bounded = (abi.FRAME_ROWS, CR, UF)                                          # well formed, refused
    ignoring = (abi.FRAME_RANGE, UP, CR, -1, -1, 1)                             # well formed, refused
    refused = [[(LAG, [1])], [(FIRST_VALUE, [3], bounded)], [(LEAD, [3], ignoring)], [(NTH_VALUE, [3, 3], bounded)]]
    invalid = [(LAG, [3, 2]), (NTH_VALUE, [3]), (LEAD, [3, 3, 2]), (LAST_VALUE, [3], (abi.FRAME_ROWS, UP, CR, -1, -1, 2)), (FIRST_VALUE, [4]),
               (abi.WINDOW_COUNT, [])]
    for first in refused:
        assert _create(_window(types, first)) == abi.ERR_NOT_SUPPORTED, first
        for second in invalid:
            assert _create(_window(types, first + [second])) == abi.ERR_INVALID_ARGUMENT, (first, second)
    assert _create(_window(types, [(LAG, [1])], output_mem=7)) == abi.ERR_INVALID_ARGUMENT
    assert _create(_window(types, [(LAG, [3, 2])], pre_grouped_channel_count=1)) == abi.ERR_INVALID_ARGUMENT


def test_the_unframed_entry_point_still_refuses_the_value_functions():
    for f in SHIFTS + FRAMED:
        for args in ([], [1], [1, 2]):
            factory = WindowOperatorFactory(TYPES, [0], [(f, args)], [0], [0], [ASC_NULLS_LAST])
            assert _create(factory) == abi.ERR_INVALID_ARGUMENT
            assert b"unknown window function" in lib().pa_last_error()
    assert _create(_window(TYPES, [16])) == abi.ERR_INVALID_ARGUMENT and b"unknown window function" in lib().pa_last_error()


def test_the_java_glue_knows_the_five_names():
    glue = open(os.path.join(ROOT, "java", "io", "trino", "gpu", "GpuWindow.java")).read()
    for name in ("lag", "lead", "first_value", "last_value", "nth_value"):
        assert '"%s"' % name in glue
    # the shim still compiles against the stub jni.h and keeps its entry point
    with tempfile.TemporaryDirectory() as d:
        obj = os.path.join(d, "shim.o")
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-fPIC", "-c", "-I", os.path.join(ROOT, "jni", "stub"), "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "jni", "presto_amd_jni.c"), "-o", obj], check=True)
        symbols = subprocess.run(["nm", "-g", "--defined-only", obj], check=True, capture_output=True, text=True).stdout
    assert "Java_io_trino_gpu_GpuNative_createFramedWindow" in symbols
