"""MarkDistinctOperator over device-resident pages, operator to operator: one BIGINT key, 64 Mi rows in 2^24-row pages, at
4 / 1 K / 100 K / 3 M / all-distinct keys, and a two-channel (BIGINT, DOUBLE) key at 100 K.  Beside each shape, in the same process and
on the same pages, the path that did the nearest job before: HashAggregationOperator grouping by the same key with count(*).
Per shape: rows/s of the whole operator life (create, every page in and out, close), the table passes' time from pa_op_kernel_time
(insert + mark + scan + publish of every page), and `frac` = (key columns read once + one mark byte per row written) / kernel time
over 8 TB/s.  Prints one JSON object; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from presto_amd import _lib, abi  # noqa: E402
from presto_amd.operators import HashAggregationOperator, MarkDistinctOperator, upload_page  # noqa: E402
from presto_amd.page import Block, Page  # noqa: E402

HBM_BYTES_PER_S = 8e12


def device_pages(columns, rows, page_rows):
    """columns: [(type, numpy array)] -> stable PA_MEM_DEVICE pages of page_rows rows."""
    pages = []
    for at in range(0, rows, page_rows):
        n = min(page_rows, rows - at)
        p = upload_page(Page([Block.flat(t, a[at:at + n]) for t, a in columns], n))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 26)
    ap.add_argument("--page-rows", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="one shape by name (profiling runs), e.g. bigint_100000")
    ap.add_argument("--no-aggregation", action="store_true", help="skip the HashAggregation comparison (profiling runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.init(0)
    rows = args.rows
    rng = np.random.default_rng(1)
    shapes = [("bigint_%d" % g, g, False) for g in (4, 1000, 100_000, 3_000_000)] + [("bigint_all_distinct", rows, False), ("bigint_double_100000", 100_000, True)]
    out = {"rows": rows, "page_rows": args.page_rows, "reps": args.reps, "shapes": []}
    for name, groups, two in shapes:
        if args.only and args.only != name:
            continue
        keys = rng.permutation(rows).astype(np.int64) if groups >= rows else rng.integers(0, groups, rows, dtype=np.int64)
        columns = [(abi.BIGINT, keys)] + ([(abi.DOUBLE, keys.astype(np.float64) * 0.5)] if two else [])
        types = [t for t, _ in columns]
        channels = list(range(len(types)))
        pages = device_pages(columns, rows, args.page_rows)
        seen = {}

        def mark():
            op = MarkDistinctOperator(types, channels, expected_distinct=min(groups, (1 << 31) - 1), output_mem=abi.MEM_DEVICE)
            for p in pages:
                op.addInput(p)
                op.getOutput()
            op.finish()
            seen["distinct"], seen["capacity"] = op.distinctStats()
            seen["kernel_ms"], _ = op.kernelTime()
            seen["kernel"] = op.kernelName()
            op.close()

        def aggregate():
            op = HashAggregationOperator(types, channels, [(abi.AGG_COUNT_STAR, -1, None)], expected_groups=min(groups, (1 << 31) - 1), output_mem=abi.MEM_DEVICE)
            for p in pages:
                op.addInput(p)
            op.finish()
            got = 0
            while True:
                page = op.getOutput()
                if page is None:
                    break
                got += page.position_count
            seen["groups_out"] = got
            op.close()

        med, best = timed(mark, args.reps)
        bytes_per_row = 8 * len(types) + 1
        kernel_s = seen["kernel_ms"] / 1e3
        e = {"shape": name, "keys": groups, "channels": len(types), "distinct_count": seen["distinct"], "table_capacity": seen["capacity"],
             "kernel": seen["kernel"], "mark_distinct_s_median": med, "mark_distinct_s_best": best, "mark_distinct_rows_per_s": rows / med,
             "table_passes_s": kernel_s, "table_passes_rows_per_s": rows / kernel_s, "bytes_per_row": bytes_per_row,
             "frac": rows * bytes_per_row / kernel_s / HBM_BYTES_PER_S}
        if not args.no_aggregation:
            try:
                amed, abest = timed(aggregate, args.reps)
                e.update({"aggregation_s_median": amed, "aggregation_s_best": abest, "aggregation_rows_per_s": rows / amed,
                          "aggregation_groups_out": seen["groups_out"], "mark_distinct_over_aggregation": amed / med})
            except Exception as ex:   # a shape the aggregation does not take is a finding, not a failure of this script
                e["aggregation_error"] = str(ex)[:200]
        out["shapes"].append(e)
        del pages
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
