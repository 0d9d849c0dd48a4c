"""RowNumberOperator over device-resident pages, operator to operator: one BIGINT key, 64 Mi rows in 2^24-row pages, at
4 / 1 K / 100 K / 3 M / all-distinct keys, and a two-channel (BIGINT, DOUBLE) key at 100 K (scripts/bench_distinct.py's shapes), without a
cap and with max_rows_per_partition = 1, plus the mode without partition channels.  Beside each shape, in the same process and on the same
pages: MarkDistinctOperator, which runs the same insert pass -- the difference is the price of the group ids, the sort and the rank
passes -- and once per run OrderByOperator on one page of 2^24 BIGINT keys, the rate of the pair sort the operator sits on.
Per shape: seconds and rows/s of the whole operator life (create, every page in and out, close), every shape warmed up once, median of
--reps.  Prints one JSON object; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from presto_amd import _lib, abi  # noqa: E402
from presto_amd.operators import MarkDistinctOperator, OrderByOperator, RowNumberOperator, upload_page  # noqa: E402
from presto_amd.page import Block, Page  # noqa: E402


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
    ap.add_argument("--no-compare", action="store_true", help="skip MarkDistinct, the capped mode and OrderBy (profiling runs)")
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
        expected = min(groups, (1 << 31) - 1)
        seen = {}

        def row_number(cap):
            op = RowNumberOperator(types, channels, channels, cap, expected_positions=expected, output_mem=abi.MEM_DEVICE)
            kept = 0
            for p in pages:
                op.addInput(p)
                page = op.getOutput()
                kept += page.position_count if page is not None else 0
            op.finish()
            seen["partitions"], seen["capacity"] = op.rowNumberStats()
            seen["kept"] = kept
            seen["table_passes_ms"], _ = op.kernelTime()
            seen["memory_bytes"] = op.memoryBytes()
            op.close()

        def mark():
            op = MarkDistinctOperator(types, channels, expected_distinct=expected, output_mem=abi.MEM_DEVICE)
            for p in pages:
                op.addInput(p)
                op.getOutput()
            op.finish()
            seen["mark_table_passes_ms"], _ = op.kernelTime()
            op.close()

        med, best = timed(lambda: row_number(None), args.reps)
        e = {"shape": name, "keys": groups, "channels": len(types), "partition_count": seen["partitions"], "table_capacity": seen["capacity"],
             "row_number_s_median": med, "row_number_s_best": best, "row_number_rows_per_s": rows / med, "row_number_ms_per_page": med * 1e3 / len(pages),
             "row_number_table_passes_s": seen["table_passes_ms"] / 1e3, "memory_bytes": seen["memory_bytes"]}
        if not args.no_compare:
            cmed, cbest = timed(lambda: row_number(1), args.reps)
            e.update({"cap1_s_median": cmed, "cap1_s_best": cbest, "cap1_rows_per_s": rows / cmed, "cap1_rows_kept": seen["kept"]})
            mmed, mbest = timed(mark, args.reps)
            e.update({"mark_distinct_s_median": mmed, "mark_distinct_s_best": mbest, "mark_distinct_rows_per_s": rows / mmed,
                      "mark_distinct_table_passes_s": seen["mark_table_passes_ms"] / 1e3, "row_number_over_mark_distinct": med / mmed,
                      "extra_ms_per_page": (med - mmed) * 1e3 / len(pages)})
        out["shapes"].append(e)
        del pages
    if not args.only and not args.no_compare:
        # no partition channels: the running count alone
        keys = np.arange(rows, dtype=np.int64)
        pages = device_pages([(abi.BIGINT, keys)], rows, args.page_rows)

        def single(cap):
            op = RowNumberOperator([abi.BIGINT], [0], [], cap, output_mem=abi.MEM_DEVICE)
            for p in pages:
                if not op.needsInput():
                    break
                op.addInput(p)
                op.getOutput()
            op.finish()
            op.close()

        med, best = timed(lambda: single(None), args.reps)
        cmed, cbest = timed(lambda: single(args.page_rows + 5), args.reps)
        out["unpartitioned"] = {"s_median": med, "s_best": best, "rows_per_s": rows / med, "cap_s_median": cmed, "cap_rows": args.page_rows + 5}
        del pages
        # the pair sort underneath, as OrderByOperator runs it: one page of 2^24 BIGINT keys
        n = args.page_rows
        page = device_pages([(abi.BIGINT, rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64))], n, n)[0]

        def order_by():
            op = OrderByOperator([abi.BIGINT], [0], [0], [abi.ASC_NULLS_LAST], output_mem=abi.MEM_DEVICE)
            op.addInput(page)
            op.finish()
            op.getOutput()
            op.close()

        try:
            med, best = timed(order_by, args.reps)
            out["order_by"] = {"rows": n, "s_median": med, "s_best": best, "rows_per_s": n / med}
        except Exception as ex:   # a finding, not a failure of this script
            out["order_by"] = {"error": str(ex)[:200]}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
