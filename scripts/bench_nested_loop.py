"""NestedLoopJoinOperator over device-resident pages, operator to operator: 2^24-row probe pages of one BIGINT channel against M = 1, 16,
256, 4096, 65536 build rows, the filters p.x < b.y and b.lo <= p.x AND p.x < b.hi at two selectivities (about one surviving pair per
probe row, and about 1 % of the pairs), and the plain product at M = 1 and 16.  Per shape: both lane mappings of the pair kernels
(PRESTO_AMD_NL_VARIANT=0 / 1), pairs/s and probe rows/s of the whole operator life (create, every page in, every page out, close; the
build side is built once, outside the clock).  Beside each shape, in the same process and on the same pages:
  lookup_join       the only way to compute the same rows without this operator: HashBuilder + LookupJoin over a constant BIGINT key
                    column added to both sides, with the same expression as the join filter.  Its candidate lists hold M entries per probe
                    row, so it is given the first --baseline-pairs / M probe rows, in pages of --baseline-page-pairs / M rows; the ratio
                    compares pairs/s.  Left out above --baseline-max-m (every probe row's lane walks the one chain of M rows).
  filter_project    (M = 1 only) FilterAndProjectOperator evaluating x > constant over the same pages: the floor the scalar-subquery shape
                    can approach; the difference is the price of the position lists and the gather.
Prints one JSON object; --out also writes it, after every shape, to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from presto_amd import _lib, abi  # noqa: E402
from presto_amd.expr import and_, call, constant, field  # noqa: E402
from presto_amd.operators import (FilterAndProjectOperator, HashBuilderOperator, LookupJoinOperator, LookupSourceFactory, NestedLoopBuildOperator,  # noqa: E402
                                  NestedLoopJoinBridge, NestedLoopJoinOperator, upload_page)
from presto_amd.page import Block, Page  # noqa: E402

RANGE = 1 << 40   # p.x is uniform in [0, RANGE)


def device_pages(columns, rows, page_rows):
    """columns: [numpy int64 array] -> stable PA_MEM_DEVICE pages of BIGINT channels"""
    pages = []
    for at in range(0, rows, page_rows):
        n = min(page_rows, rows - at)
        p = upload_page(Page([Block.bigint(a[at:at + n]) for a in columns], n))
        p.stable = True
        pages.append(p)
    return pages


def timed(fn, reps):
    times = []
    for _ in range(reps + 1):       # the first pass warms up (code objects, the pool)
        _lib.device_synchronize()
        t = time.perf_counter()
        fn()
        _lib.device_synchronize()
        times.append(time.perf_counter() - t)
    times = sorted(times[1:])
    return times[len(times) // 2], times[0]


def drive(op, pages):
    """every page in, every page out; returns the output rows"""
    rows = 0
    for p in pages:
        op.addInput(p)
        while True:
            out = op.getOutput()
            if out is None:
                break
            rows += out.position_count
    op.finish()
    op.close()
    return rows


def build_columns(kind, m, keep, rng):
    """the build side of a shape: [y] for p.x < b.y, [lo, hi] for the band; `keep` = the share of the pairs that survives"""
    if kind == "lt":
        return [np.full(m, int(keep * RANGE), dtype=np.int64) + rng.integers(0, 1000, m, dtype=np.int64)]
    width = int(keep * RANGE)
    lo = (np.arange(m, dtype=np.int64) * (RANGE // m)) if keep * m >= 0.999 and keep * m <= 1.001 else rng.integers(0, RANGE - width, m, dtype=np.int64)
    return [lo, lo + width]


def pair_filter(kind, nb, const_key=0):
    """over [build channels, probe channels]; const_key = 1 when both sides carry the constant key column in front"""
    x = field(nb + const_key, abi.BIGINT)
    if kind == "lt":
        return call(abi.OP_LESS_THAN, abi.BOOLEAN, x, field(const_key, abi.BIGINT))
    return and_(call(abi.OP_LESS_THAN_OR_EQUAL, abi.BOOLEAN, field(const_key, abi.BIGINT), x), call(abi.OP_LESS_THAN, abi.BOOLEAN, x, field(const_key + 1, abi.BIGINT)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--page-rows", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="one shape by name (profiling runs), e.g. band_4096_one")
    ap.add_argument("--variants", default="0,1")
    ap.add_argument("--build-rows", default="1,16,256,4096,65536")
    ap.add_argument("--filters", default="lt,band")
    ap.add_argument("--shares", default="one,pct", help="one: about one surviving pair per probe row; pct: about one pair in a hundred")
    ap.add_argument("--no-baseline", action="store_true", help="skip the LookupJoin and FilterAndProject comparisons (profiling runs)")
    ap.add_argument("--baseline-max-m", type=int, default=4096)
    ap.add_argument("--baseline-pairs", type=int, default=1 << 30)
    ap.add_argument("--baseline-page-pairs", type=int, default=1 << 26)
    ap.add_argument("--budget-s", type=float, default=1e9, help="no further shape is started after this many seconds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.init(0)
    started = time.perf_counter()
    rng = np.random.default_rng(1)
    rows = args.rows
    x = rng.integers(0, RANGE, rows, dtype=np.int64)
    probe_pages = device_pages([x], rows, args.page_rows)
    sizes = [int(m) for m in args.build_rows.split(",")]
    shapes = [("product_%d" % m, None, m, 1.0) for m in sizes if m <= 16]
    for kind in args.filters.split(","):
        for m in sizes:
            shapes += [("%s_%d_%s" % (kind, m, share), kind, m, 1.0 / m if share == "one" else 0.01) for share in args.shares.split(",")]
    out = {"rows": rows, "page_rows": args.page_rows, "reps": args.reps, "range": RANGE, "shapes": []}

    def save():
        text = json.dumps(out)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return text

    for name, kind, m, keep in shapes:
        if args.only and args.only != name:
            continue
        if time.perf_counter() - started > args.budget_s:
            out.setdefault("not_run", []).append(name)
            continue
        cols = build_columns(kind, m, keep, rng) if kind else [rng.integers(0, RANGE, m, dtype=np.int64)]
        nb = len(cols)
        types = [abi.BIGINT] * nb
        build_pages = device_pages(cols, m, m)
        bridge = NestedLoopJoinBridge()
        builder = NestedLoopBuildOperator(bridge, types)
        for p in build_pages:
            builder.addInput(p)
        builder.finish()
        f = pair_filter(kind, nb) if kind else None
        e = {"shape": name, "filter": kind, "build_rows": m, "pairs": rows * m, "kept_share_aimed_at": keep}
        seen = {}
        for variant in (args.variants.split(",") if kind else ["-"]):
            if kind:
                os.environ["PRESTO_AMD_NL_VARIANT"] = variant

            def join():
                op = NestedLoopJoinOperator(bridge, [abi.BIGINT], [0], [0], filter=f, output_mem=abi.MEM_DEVICE)
                seen["rows"] = drive(op, probe_pages)

            med, best = timed(join, args.reps)
            key = "variant_%s" % variant if kind else "product"
            e[key] = {"s_median": med, "s_best": best, "pairs_per_s": rows * m / med, "probe_rows_per_s": rows / med, "output_rows": seen["rows"]}
        os.environ.pop("PRESTO_AMD_NL_VARIANT", None)
        if kind:
            runs = {v: e["variant_%s" % v]["s_median"] for v in args.variants.split(",")}
            e["faster_variant"] = min(runs, key=runs.get)
            e["kept_share"] = seen["rows"] / (rows * m)
        best_pairs_per_s = max(v["pairs_per_s"] for k, v in e.items() if isinstance(v, dict))
        if kind and not args.no_baseline and m <= args.baseline_max_m:
            # the same rows through HashBuilder + LookupJoin: a constant key in front of both sides, the expression as the join filter
            try:
                b_rows = max(1, min(rows, args.baseline_pairs // m))
                b_page = max(1, min(b_rows, args.baseline_page_pairs // m))
                ls = LookupSourceFactory()
                hb = HashBuilderOperator(ls, [abi.BIGINT] * (nb + 1), [0], [1], stream=None)
                for p in device_pages([np.zeros(m, dtype=np.int64)] + cols, m, m):
                    hb.addInput(p)
                hb.finish()
                keyed_pages = device_pages([np.zeros(b_rows, dtype=np.int64), x[:b_rows]], b_rows, b_page)
                bf = pair_filter(kind, nb + 1, const_key=1)

                def lookup():
                    op = LookupJoinOperator(ls, [abi.BIGINT, abi.BIGINT], [0], [1], output_mem=abi.MEM_DEVICE, filter=bf)
                    seen["b_rows_out"] = drive(op, keyed_pages)

                med, best = timed(lookup, max(1, args.reps - 1))
                e["lookup_join"] = {"probe_rows": b_rows, "page_rows": b_page, "s_median": med, "s_best": best, "pairs_per_s": b_rows * m / med,
                                    "probe_rows_per_s": b_rows / med, "output_rows": seen["b_rows_out"]}
                e["nested_loop_over_lookup_join"] = best_pairs_per_s / (b_rows * m / med)
                hb.close()
                del keyed_pages
            except Exception as ex:   # a shape the lookup join does not take is a finding, not a failure of this script
                e["lookup_join_error"] = str(ex)[:300]
        if kind == "lt" and m == 1 and not args.no_baseline:
            threshold = int(cols[0][0])

            def floor():
                op = FilterAndProjectOperator([abi.BIGINT], call(abi.OP_LESS_THAN, abi.BOOLEAN, field(0, abi.BIGINT), constant(threshold, abi.BIGINT)),
                                              [field(0, abi.BIGINT)], output_mem=abi.MEM_DEVICE)
                seen["fp_rows"] = drive(op, probe_pages)

            med, best = timed(floor, args.reps)
            e["filter_project"] = {"s_median": med, "s_best": best, "probe_rows_per_s": rows / med, "output_rows": seen["fp_rows"]}
            e["nested_loop_time_over_filter_project_time"] = min(v["s_median"] for k, v in e.items() if k.startswith("variant_")) / med
        builder.close()
        bridge.destroy()
        out["shapes"].append(e)
        save()
        print(json.dumps(e), file=sys.stderr, flush=True)
    print(save())


if __name__ == "__main__":
    main()
