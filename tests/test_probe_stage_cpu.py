"""What the probe stage takes and what it refuses -- the inner join over a lookup source with one integer key and no duplicate keys, run
inside another operator's kernel -- as ONE table of join shapes, each pushed through both operators that carry the stage: the fused
join-aggregation (pa_codegen_compile_fused_join) and FilterAndProject with the probe inside (pa_codegen_compile_fused_join_probe), over a
lookup-source shape (no device needed).  Every refused shape stands beside a legal neighbour that compiles, so that refusing everything
passes nothing.

Where the two operators differ, the difference is real: the aggregation makes a virtual channel only of the build columns an aggregate
or a group key reads (a column it does not read is never looked at) and has no load for REAL; FilterAndProject carries every build
output channel."""
import ctypes as C

import pytest

from presto_amd import abi
from presto_amd._lib import lib
from presto_amd.expr import constant, field, serialize
from presto_amd.operators import fused_join_aggregation_desc, fused_join_desc, hash_builder_desc

COMPILES = "compiles"
INVALID, REFUSED = abi.ERR_INVALID_ARGUMENT, abi.ERR_NOT_SUPPORTED
PROBE = [abi.BIGINT, abi.DOUBLE]            # the probe page: the key and a value
DEC, LONG_DEC = abi.decimal(12, 2), abi.decimal(30, 2)


def shape(probe=PROBE, build=(abi.BIGINT, abi.DATE), build_out=(1,), build_join=(0,), probe_join=(0,), probe_out=None, reads=(),
          join_type=abi.JOIN_INNER, join_filter=None, probe_channel_count=None):
    """reads: the build output columns (indices into build_out) the aggregation counts"""
    return dict(probe=list(probe), build=list(build), build_out=list(build_out), build_join=list(build_join), probe_join=list(probe_join),
                probe_out=list(range(len(probe))) if probe_out is None else list(probe_out), reads=list(reads), join_type=join_type,
                join_filter=join_filter, probe_channel_count=probe_channel_count)


def patch_join(jd, s, keep):
    jd.join_type = s["join_type"]
    if s["join_filter"] is not None:
        f, kf = serialize(s["join_filter"])
        keep += [f, kf]
        jd.filter = C.pointer(f)
    if s["probe_channel_count"] is not None:
        jd.probe_channel_count = s["probe_channel_count"]


def run(s):
    """(FilterAndProject probe, aggregation): COMPILES or the status"""
    L = lib()
    projections = [field(i, t) for i, t in enumerate(s["probe"])]
    build, kb = hash_builder_desc(s["build"], s["build_join"], s["build_out"])
    keep = []
    d, k1 = fused_join_desc(s["probe"], None, projections, s["probe_join"], s["probe_out"], output_mem=abi.MEM_DEVICE)
    patch_join(d.join, s, keep)
    fp = L.pa_codegen_compile_fused_join_probe(C.byref(d), C.byref(build))
    n_probe_out = len(s["probe_out"])
    joined = [s["probe"][c] if 0 <= c < len(s["probe"]) else abi.BIGINT for c in s["probe_out"]] + [s["build"][c] for c in s["build_out"]]
    aggregates = [(abi.AGG_COUNT, n_probe_out + v, joined[n_probe_out + v]) for v in s["reads"]] + [(abi.AGG_COUNT_STAR, -1, None)]
    a, k2 = fused_join_aggregation_desc(s["probe"], None, projections, s["probe_join"], s["probe_out"], joined, [], aggregates)
    patch_join(a.join, s, keep)
    ag = L.pa_codegen_compile_fused_join(C.byref(a), C.byref(build), -1)
    verdict = lambda rc: COMPILES if rc > 1000 else rc
    return verdict(fp), verdict(ag)


TEN = [abi.BIGINT] * 10
TABLE = [
    # name, shape, FilterAndProject probe, aggregation
    ("legal: DATE build column, read", shape(reads=[0]), COMPILES, COMPILES),
    ("legal: no build column", shape(build=[abi.BIGINT], build_out=[]), COMPILES, COMPILES),
    ("legal: INTEGER key", shape(probe=[abi.INTEGER, abi.DOUBLE], build=[abi.INTEGER, abi.DOUBLE], reads=[0]), COMPILES, COMPILES),
    ("legal: DATE key", shape(probe=[abi.DATE, abi.DOUBLE], build=[abi.DATE, abi.BOOLEAN], reads=[0]), COMPILES, COMPILES),
    ("LEFT join", shape(join_type=abi.JOIN_PROBE_OUTER), REFUSED, REFUSED),
    ("FULL join", shape(join_type=abi.JOIN_FULL_OUTER), REFUSED, REFUSED),
    ("a join filter", shape(join_filter=constant(True, abi.BOOLEAN)), REFUSED, REFUSED),
    ("two join channels", shape(probe=[abi.BIGINT, abi.BIGINT], build=[abi.BIGINT, abi.BIGINT, abi.DATE], build_out=[2], build_join=[0, 1],
                                probe_join=[0, 1]), REFUSED, REFUSED),
    ("DOUBLE key", shape(probe=[abi.DOUBLE, abi.BIGINT], build=[abi.DOUBLE, abi.DATE]), REFUSED, REFUSED),
    ("VARCHAR key", shape(probe=[abi.VARCHAR, abi.BIGINT], build=[abi.VARCHAR, abi.DATE]), REFUSED, REFUSED),
    ("BIGINT probe key, INTEGER build key", shape(build=[abi.INTEGER, abi.DATE]), INVALID, INVALID),
    ("probe join channel out of range", shape(probe_join=[2]), INVALID, INVALID),
    ("probe join channel negative", shape(probe_join=[-1]), INVALID, INVALID),
    ("probe output channel out of range", shape(probe_out=[0, 2]), INVALID, INVALID),
    ("probe_channel_count is not the projection count", shape(probe_channel_count=3), INVALID, INVALID),
    ("VARCHAR build column, not read", shape(build=[abi.BIGINT, abi.VARCHAR]), REFUSED, COMPILES),
    ("VARCHAR build column, read", shape(build=[abi.BIGINT, abi.VARCHAR], reads=[0]), REFUSED, REFUSED),
    ("DECIMAL build column, not read", shape(build=[abi.BIGINT, DEC]), REFUSED, COMPILES),
    ("DECIMAL build column, read", shape(build=[abi.BIGINT, DEC], reads=[0]), REFUSED, REFUSED),
    ("long DECIMAL build column, read", shape(build=[abi.BIGINT, LONG_DEC], reads=[0]), REFUSED, REFUSED),
    ("eight build columns, read", shape(build=TEN, build_out=range(1, 9), reads=range(8)), COMPILES, COMPILES),
    ("nine build columns, eight read", shape(build=TEN, build_out=range(1, 10), reads=range(8)), REFUSED, COMPILES),
    ("nine build columns, read", shape(build=TEN, build_out=range(1, 10), reads=range(9)), REFUSED, REFUSED),
    ("REAL build column, not read", shape(build=[abi.BIGINT, abi.REAL]), COMPILES, COMPILES),
    ("REAL build column, read", shape(build=[abi.BIGINT, abi.REAL], reads=[0]), COMPILES, REFUSED),
    ("every carried type at once", shape(build=[abi.BIGINT, abi.BIGINT, abi.INTEGER, abi.DATE, abi.DOUBLE, abi.BOOLEAN], build_out=range(1, 6),
                                         reads=range(5)), COMPILES, COMPILES),
]


@pytest.mark.parametrize("name,s,want_fp,want_ag", TABLE, ids=[row[0] for row in TABLE])
def test_probe_stage_takes_or_refuses(name, s, want_fp, want_ag):
    got_fp, got_ag = run(s)
    assert (got_fp, got_ag) == (want_fp, want_ag), (name, lib().pa_last_error())


def test_every_refused_row_has_a_neighbour_that_compiles():
    """the table itself: no operator's column is all refusals, and each refusal has the legal shape it was made from in the table"""
    assert sum(1 for row in TABLE if row[2] == COMPILES) >= 5 and sum(1 for row in TABLE if row[3] == COMPILES) >= 5
    assert TABLE[0][2:] == (COMPILES, COMPILES)      # the shape every other row departs from
