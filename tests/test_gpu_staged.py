"""GPU: the staged page loop of the ungrouped fused kernel (V_GLOBAL_S) computes bit for bit what the plain loop computes.

PRESTO_AMD_STAGED=1 forces the staged kernel, =0 the plain one; under auto the first launch of a plan decides.  Device pages that
continue each other would be taken as a table of ranges (a kernel the staged loop is not part of), so the device-page tests set
PRESTO_AMD_NO_RANGES and the operator launches over its pages."""
import struct

import numpy as np
import pytest

from presto_amd import abi, tpch
from presto_amd._lib import PrestoAmdError
from presto_amd.expr import and_, constant, field
from presto_amd.operators import FusedAggregationOperator, to_pages
from presto_amd.page import Block, Page

pytestmark = pytest.mark.gpu


def q6_operator(filt=None):
    aggs = tpch.Q6_AGGREGATES + [(abi.AGG_COUNT_STAR, -1, None)]
    return FusedAggregationOperator(tpch.Q6_TYPES, filt if filt is not None else tpch.q6_filter(), tpch.q6_projections(), [], aggs)


def bits(rows):
    (revenue, count), = rows
    return (None if revenue is None else struct.pack("<d", revenue)), count


def run(monkeypatch, staged, make_op, pages):
    monkeypatch.setenv("PRESTO_AMD_STAGED", staged)
    op = make_op()
    out = to_pages(op, pages)
    name = op.kernelName()
    op.close()
    return [r for p in out for r in p.to_rows()], name


def host_q6(oracle, sf, n, null_rate=0.0, seed=3):
    rng = np.random.default_rng(seed)
    blocks = []
    for i, col in enumerate(tpch.Q6_COLUMNS):
        v, _ = oracle.tpch_column(col, sf, 0, n)
        nulls = (rng.random(n) < null_rate).astype(np.uint8) if null_rate and i >= 2 else None  # quantity, extendedprice
        blocks.append(Block(abi.TPCH_COLUMN_TYPE[col], abi.FLAT, n, values=v, nulls=nulls))
    return Page(blocks, n)


def test_staged_q6_sf1_bit_identical(gpu, monkeypatch):
    monkeypatch.setenv("PRESTO_AMD_NO_RANGES", "1")
    dev = tpch.DeviceColumns(tpch.Q6_COLUMNS, 1.0, tpch.lineitem_rows(1.0))
    eager, en = run(monkeypatch, "0", q6_operator, list(dev.pages(1 << 22)))
    staged, sn = run(monkeypatch, "1", q6_operator, list(dev.pages(1 << 22)))
    assert "staged" in sn and "staged" not in en
    assert bits(staged) == bits(eager) and eager[0][1] > 0


def test_staged_q6_odd_pages_and_unaligned(gpu, oracle, monkeypatch):
    monkeypatch.setenv("PRESTO_AMD_NO_RANGES", "1")
    dev = tpch.DeviceColumns(tpch.Q6_COLUMNS, 0.1, 3000003)
    for pr in (1000003, 2999999):
        eager, _ = run(monkeypatch, "0", q6_operator, list(dev.pages(pr)))
        staged, _ = run(monkeypatch, "1", q6_operator, list(dev.pages(pr)))
        assert bits(staged) == bits(eager)
    host = host_q6(oracle, 0.1, 400001)
    pages = [host.get_region(0, 123457), host.get_region(123457, 400001 - 123457)]  # the second is unaligned: scalar rows
    eager, _ = run(monkeypatch, "0", q6_operator, pages)
    staged, _ = run(monkeypatch, "1", q6_operator, pages)
    assert bits(staged) == bits(eager)


def test_staged_q6_nullable_later_stages(gpu, oracle, monkeypatch):
    host = host_q6(oracle, 0.1, 1 << 20, null_rate=0.1)
    eager, _ = run(monkeypatch, "0", q6_operator, [host])
    staged, sn = run(monkeypatch, "1", q6_operator, [host])
    assert "staged" in sn
    assert bits(staged) == bits(eager) and eager[0][1] > 0


def divide_page(n, zero_on_live):
    a = np.arange(n, dtype=np.int64) % 7 - 3          # a < 0: rejected by the first conjunct
    b = np.where(a < 0, 0, 5).astype(np.int64)
    if zero_on_live:
        b[n // 2 + (0 if a[n // 2] >= 0 else 3)] = 0
    return Page([Block.flat(abi.BIGINT, a), Block.flat(abi.BIGINT, b)], n)


def divide_operator():
    filt = and_(field(0, abi.BIGINT) >= constant(0, abi.BIGINT),
                (constant(100, abi.BIGINT) / field(1, abi.BIGINT)) > constant(1, abi.BIGINT))
    return FusedAggregationOperator([abi.BIGINT, abi.BIGINT], filt, [field(0, abi.BIGINT)], [],
                                    [(abi.AGG_SUM, 0, abi.BIGINT), (abi.AGG_COUNT_STAR, -1, None)])


def test_staged_later_conjunct_errors_only_on_live_rows(gpu, monkeypatch):
    n = 1 << 20
    eager, _ = run(monkeypatch, "0", divide_operator, [divide_page(n, False)])
    staged, sn = run(monkeypatch, "1", divide_operator, [divide_page(n, False)])
    assert "staged" in sn and staged == eager and eager[0][1] > 0
    for mode in ("0", "1"):
        with pytest.raises(PrestoAmdError):
            run(monkeypatch, mode, divide_operator, [divide_page(n, True)])


def test_staged_auto_choice(gpu, oracle, monkeypatch):
    host = host_q6(oracle, 1.0, tpch.lineitem_rows(1.0))
    _, name = run(monkeypatch, "auto", q6_operator, [host])
    assert "pa_fused_global_staged" in name
    # Q1 stays on its few-groups kernel
    monkeypatch.setenv("PRESTO_AMD_STAGED", "auto")
    dev = tpch.DeviceColumns(tpch.Q1_COLUMNS, 0.1, 1 << 20)
    op = FusedAggregationOperator(tpch.Q1_TYPES, tpch.q1_filter(), tpch.q1_projections(), tpch.Q1_GROUP_BY, tpch.Q1_AGGREGATES,
                                  type_params=tpch.Q1_TYPE_PARAMS)
    to_pages(op, list(dev.pages(1 << 20)))
    assert op.kernelName().startswith("pa_fused_lds_") and "staged" not in op.kernelName()
    op.close()
    # a filter that keeps 99 % of the rows: the first launch of the plan predicts no gain, later operators take the plain kernel
    loose = and_(field(0, abi.DATE) <= constant(10471, abi.DATE), field(2, abi.DOUBLE) < constant(51.0, abi.DOUBLE))
    first, _ = run(monkeypatch, "auto", lambda: q6_operator(loose), [host])
    second, name = run(monkeypatch, "auto", lambda: q6_operator(loose), [host])
    assert name.startswith("pa_fused_global_") and "staged" not in name
    assert bits(first) == bits(second)
