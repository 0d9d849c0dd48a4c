"""The contract of the nested-loop join (include/presto_amd.h, pa_nested_loop_join_desc) as two plain loops: for every probe row i in
order and every build row j in order, the pair is emitted when there is no filter or the filter is TRUE over the pair's row
[build channels..., probe channels...] -- evaluated by tests/expr_model.py, the independent statement of the expression semantics.  The
filter is evaluated on EVERY pair: the first error in probe-major order is the error of the product."""
from tests import expr_model as M


def pair_row(build_row, probe_row):
    """the filter's input: the build page's channels first, then the probe page's (the numbering of pa_lookup_join_desc.filter)"""
    return tuple(build_row) + tuple(probe_row)


def pairs(probe_rows, build_rows, filter_expr=None):
    """The surviving (i, j) in probe-major order, or raises expr_model.ModelError(status)."""
    out = []
    for i, p in enumerate(probe_rows):
        for j, b in enumerate(build_rows):
            if filter_expr is None or M.evaluate(filter_expr, pair_row(b, p)) is True:   # (NULL counts as false)
                out.append((i, j))
    return out


def nested_loop(probe_rows, build_rows, probe_out, build_out, filter_expr=None):
    """Output rows in probe-major order, or raises expr_model.ModelError(status)."""
    return [tuple(probe_rows[i][c] for c in probe_out) + tuple(build_rows[j][c] for c in build_out) for i, j in pairs(probe_rows, build_rows, filter_expr)]


def outcome(probe_rows, build_rows, probe_out, build_out, filter_expr=None):
    """('rows', rows) or ('error', status)"""
    try:
        return "rows", nested_loop(probe_rows, build_rows, probe_out, build_out, filter_expr)
    except M.ModelError as e:
        return "error", e.status
