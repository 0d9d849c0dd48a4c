"""StreamingAggregationOperator restated in plain Python (StreamingAggregationOperator.java:171-367): a list of rows is cut into runs of
consecutive rows that are NOT DISTINCT on the group channels, and tests/agg_model.py is applied to each run's value lists.  The key of
a run is its FIRST row's (the reference takes it from whichever page flushes the run).

Values as in agg_model: None = NULL, int for BIGINT / INTEGER / DATE / short DECIMAL, float for DOUBLE, numpy.float32 for REAL, bool for
BOOLEAN, bytes for VARCHAR."""
from presto_amd import abi
from tests import agg_model as A


def canon(t, v):
    """a key value under IS NOT DISTINCT FROM: NULL is one value, every NaN one value, -0.0 is +0.0, a BOOLEAN is zero / non-zero"""
    if v is None:
        return None
    if t in (abi.DOUBLE, abi.REAL):
        v = float(v)
        return "nan" if v != v else (0.0 if v == 0 else v)
    if t == abi.BOOLEAN:
        return bool(v)
    if t == abi.VARCHAR:
        return bytes(v)
    return int(v)


def not_distinct(key_types, a, b):
    return all(canon(t, x) == canon(t, y) for t, x, y in zip(key_types, a, b))


def runs(rows, types, group_channels):
    """rows (tuples over `types`) -> [(first row, [rows of the run])], in input order; page cuts do not matter"""
    key_types = [types[c] for c in group_channels]
    out = []
    for row in rows:
        key = [row[c] for c in group_channels]
        if out and not_distinct(key_types, [out[-1][0][c] for c in group_channels], key):
            out[-1][1].append(row)
        else:
            out.append((row, [row]))
    return out


def outcomes(rows, types, group_channels, aggregates):
    """-> [(key tuple of the run's first row, [agg_model.Result per aggregate], [agg_model.order_free per aggregate])];
    aggregates: (fn, input channel, input type[, mask channel])"""
    out = []
    for first, members in runs(rows, types, group_channels):
        results, exact = [], []
        for a in aggregates:
            fn, channel = a[0], a[1]
            t = abi.BIGINT if fn == abi.AGG_COUNT_STAR else a[2]
            mask_channel = a[3] if len(a) > 3 else -1
            values = [0 if fn == abi.AGG_COUNT_STAR else r[channel] for r in members]      # count(*) looks at no value
            mask = None if mask_channel < 0 else [None if r[mask_channel] is None else bool(r[mask_channel]) for r in members]
            results.append(A.aggregate(fn, t, values, mask))
            exact.append(A.order_free(fn, t, A.counted(fn, values, mask)))
        out.append((tuple(first[c] for c in group_channels), results, exact))
    return out


def expected_rows(rows, types, group_channels, aggregates):
    """the output rows where every run has a row_order value (None = NULL), or ("error", status) from the first run that has none on:
    rows before it may have been handed out, nothing after"""
    out = []
    for key, results, _ in outcomes(rows, types, group_channels, aggregates):
        values = []
        for r in results:
            if r.row_order[0] == "error":
                return out, r.row_order
            values.append(None if r.row_order[0] == "null" else r.row_order[1])
        out.append(key + tuple(values))
    return out, None
