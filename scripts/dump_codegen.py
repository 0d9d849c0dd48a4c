"""Writes the generated source of every cell of tests/test_codegen_tiers.py's full matrix under a directory, one file per cell
(<shape>.<tier>.<mask>.hip), plus the probe-stage kernels, the FilterAndProject kernels (with and without the probe inside) and the
nested-loop pair kernels: `diff -r` of two dumps shows what a change of the generator changed."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_codegen_tiers as T
from presto_amd import abi, tpch, q3
from presto_amd._lib import lib
from tests import test_nested_loop_cpu as NL
from presto_amd.operators import _filter_project_desc, fused_join_aggregation_desc, fused_join_desc, hash_builder_desc
from presto_amd.expr import field

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
n = 0
for name, variant, mask in T.cells(True):
    src = T.source(name, variant, mask)
    with open(os.path.join(out, "%s.%s.%x.hip" % (name, T.TIER_NAMES[variant], mask)), "w") as f:
        f.write(src if src is not None else "REFUSED: " + lib().pa_last_error().decode() + "\n")
    n += 1
L = lib()
build, kb = hash_builder_desc(q3.ORDERS_JOINED_TYPES, [0], [1, 2])
for ai, aggs in enumerate((q3.AGG_AGGREGATES, [(abi.AGG_MAX, 1, abi.DOUBLE), (abi.AGG_SUM, 0, abi.BIGINT), (abi.AGG_COUNT_STAR, -1, None)])):
    for gi, (group_by, variants) in enumerate(((q3.AGG_GROUP_BY, (6, 2, 3)), ([2, 3], (2, 3, 1)), ([], (0,)))):
        d, keep = fused_join_aggregation_desc(tpch.Q3_LINEITEM_TYPES, tpch.q3_lineitem_filter(), tpch.q3_lineitem_projections(), [0], [0, 1], q3.AGG_TYPES, group_by, aggs)
        for v in variants:
            need = L.pa_codegen_fused_join(C.byref(d), C.byref(build), v, None, 0)
            buf = C.create_string_buffer(max(need, 1))
            if need > 0:
                L.pa_codegen_fused_join(C.byref(d), C.byref(build), v, buf, need)
            open(os.path.join(out, "probe.%d.%d.%s.hip" % (ai, gi, T.TIER_NAMES[v])), "wb").write(buf.value if need > 0 else b"REFUSED\n")
            n += 1


def write(name, source):
    """source: the translation unit, or the (negative) status of a refusal"""
    global n
    with open(os.path.join(out, name), "w") as f:
        f.write(source if isinstance(source, str) else "REFUSED: " + L.pa_last_error().decode() + "\n")
    n += 1


def sized(fn, *args):
    need = fn(*args, None, 0)
    if need <= 0:
        return need
    buf = C.create_string_buffer(need)
    fn(*args, buf, need)
    return buf.value.decode()


# FilterAndProject: the Q6 and Q1 shapes and a VARCHAR channel handed through
varchar_types = [abi.VARCHAR, abi.BIGINT]
for name, types, f, proj, params in (("q6", tpch.Q6_TYPES, tpch.q6_filter(), tpch.q6_projections(), None),
                                     ("q1", tpch.Q1_TYPES, tpch.q1_filter(), tpch.q1_projections(), tpch.Q1_TYPE_PARAMS),
                                     ("varchar_ref", varchar_types, field(1, abi.BIGINT) > 0, [field(0, abi.VARCHAR), field(1, abi.BIGINT) + 1], None)):
    fp, keep = _filter_project_desc(types, f, proj, abi.MEM_HOST, None, params)
    need = L.pa_codegen_filter_project(C.byref(fp), None, 0, None)
    buf = C.create_string_buffer(max(need, 1))
    if need > 0:
        L.pa_codegen_filter_project(C.byref(fp), buf, need, None)
    write("fp.%s.hip" % name, buf.value.decode() if need > 0 else need)
# ... with the probe inside: Q3's orders pipeline (no build column) and its lineitem pipeline over the joined orders (two build columns)
b0, kb0 = hash_builder_desc([abi.BIGINT], [0], [])
d0, k0 = fused_join_desc(tpch.ORDERS_TYPES, tpch.q3_orders_filter(), [field(i, t) for i, t in enumerate(tpch.ORDERS_TYPES)], [1], [0, 2, 3], output_mem=abi.MEM_DEVICE)
write("fp_probe.orders.hip", sized(L.pa_codegen_fused_join_probe, C.byref(d0), C.byref(b0)))
d1, k1 = fused_join_desc(tpch.Q3_LINEITEM_TYPES, tpch.q3_lineitem_filter(), [field(i, t) for i, t in enumerate(tpch.Q3_LINEITEM_TYPES)], [0], [0, 1, 2],
                         output_mem=abi.MEM_DEVICE)
write("fp_probe.lineitem.hip", sized(L.pa_codegen_fused_join_probe, C.byref(d1), C.byref(build)))
# the nested-loop pair kernels: both lane mappings, with and without NULL flags, and the shapes of tests/test_nested_loop_cpu.py
for v in range(4):
    write("nl.mixed.%d.hip" % v, NL.codegen(NL.PT, [0, 3], NL.BT, [3], NL.MIXED, variant=v))
for v in (0, 1):
    write("nl.less.%d.hip" % v, NL.codegen([abi.BIGINT], [0], [abi.BIGINT], [0], NL.lt(field(1, abi.BIGINT), field(0, abi.BIGINT)), variant=v))
    for t in NL.CARRIED:
        write("nl.carried.%s.%d.hip" % (abi.TYPE_NAMES[int(t)], v), NL.codegen([t], [0], [t], [0], NL.TRUE, variant=v))
    for width in (4, 2):  # build rows wider than one LDS chunk are not staged
        ld = abi.decimal(30, 2)
        eq = NL.and_(*[NL.call(abi.OP_EQUAL, abi.BOOLEAN, field(c, ld), field(c, ld)) for c in range(width)])
        write("nl.wide%d.%d.hip" % (width, v), NL.codegen([abi.BIGINT], [0], [ld] * width, [0], eq, variant=v))
print(n, "sources under", out)
