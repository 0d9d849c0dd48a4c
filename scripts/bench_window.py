"""WindowOperator (the ranking functions) over device-resident pages, operator to operator: 64 Mi rows in 2^24-row pages, one BIGINT
partition key at 4 / 1 K / 100 K / 3 M / all-distinct keys, a random DOUBLE sort key, rank() alone and all six functions together
(ntile over a BIGINT bucket channel).

The yardstick is OrderByOperator over the same channel list (partition key, sort key) and the same output channels on the same pages in
the same process, alternated with it run by run: it does the same sort and the same gathers, so the ratio shows what the window's own
passes (flags, scans, starts, functions) and its function columns cost.  The payload columns of the two are compared bit for bit before
anything is timed.  The pages are handed over as plain device pages, so both operators copy them on arrival; with --stable they are
flagged PA_PAGE_STABLE, which OrderBy lists instead of copying and the window operator copies all the same.
Per shape: seconds and rows/s of the whole operator life (create, every page in, finish, output taken, close), every shape warmed up once,
median and min-max of --reps.  Prints one JSON object; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from presto_amd import _lib, abi  # noqa: E402
from presto_amd.operators import OrderByOperator, WindowOperator, download_page, upload_page  # noqa: E402
from presto_amd.page import Block, Page  # noqa: E402

ASC_NULLS_LAST = 1
SIX = [abi.WINDOW_ROW_NUMBER, abi.WINDOW_RANK, abi.WINDOW_DENSE_RANK, abi.WINDOW_PERCENT_RANK, abi.WINDOW_CUME_DIST, (abi.WINDOW_NTILE, [2])]


def device_pages(blocks_of, rows, page_rows, stable):
    """blocks_of(at, n) -> host blocks of rows [at, at + n) -> PA_MEM_DEVICE pages of page_rows rows."""
    pages = []
    for at in range(0, rows, page_rows):
        n = min(page_rows, rows - at)
        p = upload_page(Page(blocks_of(at, n), n))
        p.stable = stable
        pages.append(p)
    return pages


def alternated(fns, reps):
    """every function once to warm up (code objects, the pool), then reps rounds of all of them in turn -> [(median, min, max)]"""
    times = [[] for _ in fns]
    for r in range(reps + 1):
        for i, fn in enumerate(fns):
            _lib.device_synchronize()
            t = time.perf_counter()
            fn()
            _lib.device_synchronize()
            if r > 0:
                times[i].append(time.perf_counter() - t)
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in times]


def columns_of(pages, count):
    pages = [download_page(p) if p.mem == abi.MEM_DEVICE else p for p in pages]
    return [np.concatenate([p.blocks[c].values[:p.position_count] for p in pages]) for c in range(count)]


def run(op, pages):
    for p in pages:
        op.addInput(p)
    op.finish()
    result = []
    while True:
        page = op.getOutput()
        if page is None:
            break
        result.append(page)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 26)
    ap.add_argument("--page-rows", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="one shape by name (profiling runs), e.g. bigint_100000_six")
    ap.add_argument("--no-compare", action="store_true", help="the window operator alone (profiling runs)")
    ap.add_argument("--stable", action="store_true", help="PA_PAGE_STABLE input pages")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.init(0)
    rows, page_rows = args.rows, args.page_rows
    rng = np.random.default_rng(1)
    out = {"rows": rows, "page_rows": page_rows, "reps": args.reps, "stable_pages": bool(args.stable), "command": " ".join(["python"] + sys.argv), "shapes": []}
    for groups in (4, 1000, 100_000, 3_000_000, rows):
        label = "bigint_all_distinct" if groups >= rows else "bigint_%d" % groups
        if args.only and not args.only.startswith(label + "_"):
            continue
        keys = rng.permutation(rows).astype(np.int64) if groups >= rows else rng.integers(0, groups, rows, dtype=np.int64)
        sort_key = rng.random(rows)
        buckets = rng.integers(1, 101, rows, dtype=np.int64)
        columns = [(abi.BIGINT, keys), (abi.DOUBLE, sort_key), (abi.BIGINT, buckets)]
        types = [t for t, _ in columns]
        pages = device_pages(lambda at, m: [Block.flat(t, a[at:at + m]) for t, a in columns], rows, page_rows, args.stable)
        del keys, sort_key, buckets
        outputs, partition, sort, orders = [0, 1], [0], [1], [ASC_NULLS_LAST]
        for suffix, functions in (("rank", [abi.WINDOW_RANK]), ("six", SIX)):
            name = label + "_" + suffix
            if args.only and args.only != name:
                continue
            seen = {}

            def window():
                op = WindowOperator(types, outputs, functions, partition, sort, orders, output_mem=abi.MEM_DEVICE)
                result = run(op, pages)
                seen["passes_ms"], _ = op.kernelTime()
                seen["memory_bytes"] = op.memoryBytes()
                seen["result"] = columns_of(result, len(outputs)) if seen.get("keep_result") else None
                del result
                op.close()

            def order_by():
                op = OrderByOperator(types, outputs, partition + sort, [ASC_NULLS_LAST] + orders, output_mem=abi.MEM_DEVICE)
                result = run(op, pages)
                seen["sorted"] = columns_of(result, len(outputs)) if seen.get("keep_result") else None
                del result
                op.close()

            e = {"shape": name, "keys": groups, "functions": len(functions)}
            compare = not args.no_compare
            if compare:
                # the same payload first
                seen["keep_result"] = True
                window()
                order_by()
                got, want = seen.pop("result"), seen.pop("sorted")
                seen["keep_result"] = False
                same = all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(got, want))
                e["same_payload_as_order_by"] = bool(same)
                assert same, name
                del got, want
            measured = alternated([window] + ([order_by] if compare else []), args.reps)
            med, lo, hi = measured[0]
            # flags + scans + starts + functions, between two events on the operator's stream
            e.update({"window_s_median": med, "window_s_min": lo, "window_s_max": hi, "window_rows_per_s": rows / med,
                      "window_passes_s": seen["passes_ms"] / 1e3, "memory_bytes_at_end": seen["memory_bytes"]})
            if compare:
                cmed, clo, chi = measured[1]
                e.update({"order_by_s_median": cmed, "order_by_s_min": clo, "order_by_s_max": chi, "order_by_rows_per_s": rows / cmed,
                          "window_over_order_by": med / cmed, "spread": max((hi - lo) / med, (chi - clo) / cmed)})
            out["shapes"].append(e)
            print(json.dumps(e), file=sys.stderr, flush=True)
        del pages
    text_out = json.dumps(out)
    print(text_out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text_out + "\n")


if __name__ == "__main__":
    main()
