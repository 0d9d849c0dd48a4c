"""StreamingAggregationOperator over device-resident pages, operator to operator: a BIGINT key and a BIGINT argument, 64 Mi rows in
2^24-row pages, pre-grouped in runs of 1 / 4 / 32 / 1024 / 2^20 rows and as one run over everything, with count(*), sum, min.  Beside
each shape, alternated run by run in the same process and on the same pages, HashAggregationOperator with the same aggregates: the
path such a plan took before.  Both results are checked on the host against numpy before anything is timed.
Per shape: seconds of the whole operator life (create, every page in, every output page out, close) as median and min-max of --reps
alternated runs, and the reduction's time from pa_op_kernel_time.  Prints one JSON object; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from presto_amd import _lib, abi  # noqa: E402
from presto_amd.operators import HashAggregationOperator, StreamingAggregationOperator, download_page, upload_page  # noqa: E402
from presto_amd.page import Block, Page  # noqa: E402

AGGREGATES = [(abi.AGG_COUNT_STAR, -1, None), (abi.AGG_SUM, 1, abi.BIGINT), (abi.AGG_MIN, 1, abi.BIGINT)]
TYPES = [abi.BIGINT, abi.BIGINT]


def device_pages(keys, values, page_rows):
    pages = []
    for at in range(0, len(keys), page_rows):
        n = min(page_rows, len(keys) - at)
        p = upload_page(Page([Block.bigint(keys[at:at + n]), Block.bigint(values[at:at + n])], n))
        p.stable = True
        pages.append(p)
    return pages


def streaming(pages, seen, keep):
    op = StreamingAggregationOperator(TYPES, [0], AGGREGATES, output_mem=abi.MEM_DEVICE)
    outs, rows = [], 0
    for p in pages:
        op.addInput(p)
        out = op.getOutput()
        if out is not None:
            rows += out.position_count
            if keep:
                outs.append(download_page(out))
    op.finish()
    out = op.getOutput()
    if out is not None:
        rows += out.position_count
        if keep:
            outs.append(download_page(out))
    seen["streaming_rows_out"] = rows
    seen["reduce_ms"], _ = op.kernelTime()
    op.close()
    return outs


def hashed(pages, seen, keep, groups):
    op = HashAggregationOperator(TYPES, [0], AGGREGATES, expected_groups=min(groups, (1 << 31) - 1), output_mem=abi.MEM_DEVICE)
    for p in pages:
        op.addInput(p)
    op.finish()
    outs, rows = [], 0
    while True:
        out = op.getOutput()
        if out is None:
            break
        rows += out.position_count
        if keep:
            outs.append(download_page(out))
    seen["hash_rows_out"] = rows
    op.close()
    return outs


def columns_of(outs):
    return [np.concatenate([p.blocks[c].values[:p.position_count] for p in outs]) for c in range(4)]


def check(outs, reference, ordered, what):
    got = columns_of(outs)
    if not ordered:
        order = np.argsort(got[0], kind="stable")
        got = [c[order] for c in got]
    for name, g, r in zip(("key", "count", "sum", "min"), got, reference):
        if not np.array_equal(g, r):
            raise SystemExit("%s: column %s differs from numpy" % (what, name))


def summary(times):
    s = sorted(times)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 26)
    ap.add_argument("--page-rows", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", type=int, default=None, help="one run length (0 = one run over everything): profiling runs")
    ap.add_argument("--no-hash", action="store_true", help="skip the HashAggregation side (profiling runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.init(0)
    rows = args.rows
    rng = np.random.default_rng(1)
    values = rng.integers(-1000, 1000, rows, dtype=np.int64)
    out = {"rows": rows, "page_rows": args.page_rows, "reps": args.reps, "aggregates": "count(*), sum(BIGINT), min(BIGINT)", "shapes": []}
    for run_length in (1, 4, 32, 1024, 1 << 20, 0):
        if args.only is not None and args.only != run_length:
            continue
        keys = np.arange(rows, dtype=np.int64) // run_length if run_length else np.zeros(rows, dtype=np.int64)
        starts = np.arange(0, rows, run_length) if run_length else np.zeros(1, dtype=np.int64)
        reference = [keys[starts], np.diff(np.append(starts, rows)), np.add.reduceat(values, starts), np.minimum.reduceat(values, starts)]
        pages = device_pages(keys, values, args.page_rows)
        seen = {}
        e = {"run_length": run_length or rows, "runs": len(starts)}
        check(streaming(pages, seen, True), reference, True, "streaming, runs of %d" % (run_length or rows))
        hash_ok = not args.no_hash
        if hash_ok:
            try:
                check(hashed(pages, seen, True, len(starts)), reference, False, "hash, runs of %d" % (run_length or rows))
            except SystemExit:
                raise
            except Exception as ex:   # a shape the hash aggregation does not take is a finding, not a failure of this script
                e["hash_error"] = str(ex)[:200]
                hash_ok = False
        streaming_s, hash_s = [], []
        for _ in range(args.reps):    # alternated: streaming, hash, streaming, ...
            _lib.device_synchronize()
            t = time.perf_counter()
            streaming(pages, seen, False)
            _lib.device_synchronize()
            streaming_s.append(time.perf_counter() - t)
            if hash_ok:
                t = time.perf_counter()
                hashed(pages, seen, False, len(starts))
                _lib.device_synchronize()
                hash_s.append(time.perf_counter() - t)
        e.update({"streaming_s": summary(streaming_s), "streaming_rows_per_s": rows / summary(streaming_s)["median"], "reduce_s": seen["reduce_ms"] / 1e3,
                  "rows_out": seen["streaming_rows_out"]})
        if hash_ok:
            e.update({"hash_s": summary(hash_s), "hash_rows_per_s": rows / summary(hash_s)["median"],
                      "hash_over_streaming": summary(hash_s)["median"] / summary(streaming_s)["median"]})
        out["shapes"].append(e)
        del pages
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
