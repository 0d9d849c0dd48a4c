"""CPU: the staged-load plan of the fused operator (fused_plan.cpp: plan_stages) and the staged GLOBAL kernel (variant 9), which
generates and compiles for gfx950 without a device."""
import ctypes as C
import re

import pytest

from presto_amd import abi, tpch
from presto_amd._lib import lib
from presto_amd.expr import and_, constant, field, or_
from presto_amd.operators import fused_aggregation_desc

STAGED = 9


def q6_desc(filt=None, types=None, proj=None, aggs=None, params=None):
    return fused_aggregation_desc(types or tpch.Q6_TYPES, filt if filt is not None else tpch.q6_filter(), proj or tpch.q6_projections(), [],
                                  aggs or tpch.Q6_AGGREGATES, type_params=params)


def stages(desc):
    d, keep = desc
    n = d.filter_project.input_channel_count
    out = (C.c_int32 * n)()
    ns = lib().pa_codegen_fused_stages(C.byref(d), out, n)
    assert ns >= 0, lib().pa_last_error().decode()
    return ns, list(out)


def source(desc, variant):
    d, keep = desc
    need = lib().pa_codegen_fused(C.byref(d), variant, None, 0, None)
    if need <= 0:
        return None
    buf = C.create_string_buffer(need)
    lib().pa_codegen_fused(C.byref(d), variant, buf, need, None)
    return buf.value.decode()


def test_q6_stages():
    # channels: 0 shipdate, 1 discount, 2 quantity, 3 extendedprice
    assert stages(q6_desc()) == (4, [0, 1, 2, 3])


def test_q1_one_date_stage():
    d = fused_aggregation_desc(tpch.Q1_TYPES, tpch.q1_filter(), tpch.q1_projections(), tpch.Q1_GROUP_BY, tpch.Q1_AGGREGATES,
                               type_params=tpch.Q1_TYPE_PARAMS)
    ns, st = stages(d)
    # shipdate (6) and the VARCHAR keys (eager) in the date stage, the measures behind it
    assert ns == 2 and st[6] == 0 and st[0] == 0 and st[1] == 0 and st[2:6] == [1, 1, 1, 1]
    assert source(d, STAGED) is None  # grouped: no staged kernel, the few-groups tier runs as before


D = abi.decimal(12, 2)


def decimal_q6_desc():
    filt = and_(field(0, abi.DATE) >= constant(8766, abi.DATE), field(0, abi.DATE) < constant(9131, abi.DATE),
                field(1, D) >= constant(5, D), field(1, D) <= constant(7, D), field(2, D) < constant(2400, D))
    return q6_desc(filt, [abi.DATE, D, D, D], [field(3, D)], [(abi.AGG_SUM, 0, D)])


def test_decimal_q6_stages():
    assert stages(decimal_q6_desc()) == (4, [0, 1, 2, 3])
    src = source(decimal_q6_desc(), STAGED)
    assert src is not None and "pa_fused_global_staged" in src


def test_nested_and_flattens_in_order():
    q, p, disc, ship = (field(2, abi.DOUBLE), field(3, abi.DOUBLE), field(1, abi.DOUBLE), field(0, abi.DATE))
    filt = and_(and_(q < constant(24.0, abi.DOUBLE), disc >= constant(0.05, abi.DOUBLE)), and_(ship >= constant(8766, abi.DATE)))
    assert stages(q6_desc(filt)) == (4, [2, 1, 0, 3])


def test_or_at_the_top_does_not_split():
    filt = or_(field(0, abi.DATE) < constant(8766, abi.DATE), field(2, abi.DOUBLE) < constant(24.0, abi.DOUBLE))
    # one conjunct reading shipdate and quantity, then the projections' channels
    assert stages(q6_desc(filt)) == (2, [0, 1, 0, 1])


def test_conjunct_that_can_throw():
    types = [abi.BIGINT, abi.BIGINT]
    filt = and_(field(0, abi.BIGINT) >= constant(0, abi.BIGINT), (constant(100, abi.BIGINT) / field(1, abi.BIGINT)) > constant(1, abi.BIGINT))
    d = fused_aggregation_desc(types, filt, [field(0, abi.BIGINT)], [], [(abi.AGG_SUM, 0, abi.BIGINT)])
    assert stages(d) == (2, [0, 1])
    src = source(d, STAGED)
    # the division runs only for rows the first conjunct did not reject
    body = src[src.index("void pa_stage1("):]
    assert body.index("if (!dead)") < body.index("/")


def test_no_filter_no_stages():
    d = fused_aggregation_desc(tpch.Q6_TYPES, None, tpch.q6_projections(), [], tpch.Q6_AGGREGATES)
    assert stages(d)[0] == 0
    assert source(d, STAGED) is None


def test_plain_q6_source_unchanged_by_the_plan():
    # the plain kernel does not know about stages: no stage function, no counting
    src = source(q6_desc(), 0)
    assert "pa_stage" not in src and "pa_cnt" not in src and "pa_fused_global_staged" not in src


def test_staged_loads_are_unconditional():
    src = source(q6_desc(), STAGED)
    loop = src[src.index("for (i64 it = 0;"):]
    loop = loop[:loop.index("for (i64 r = (nq << 2)")]
    # every load of the loop is an indexed read whose index falls back to the first quad: no branch around a load
    loads = re.findall(r"\(\(const \w+\*\)a\.v\[\d\]\)\[(.*?)\];", loop)
    assert len(loads) == 7 and all(l.endswith(": 0") for l in loads)


@pytest.mark.parametrize("which", ["q6", "decimal"])
def test_staged_kernels_compile(which):
    d = q6_desc() if which == "q6" else decimal_q6_desc()
    dd, keep = d
    size = lib().pa_codegen_compile_fused(C.byref(dd), STAGED)
    assert size > 0, lib().pa_last_error().decode()
