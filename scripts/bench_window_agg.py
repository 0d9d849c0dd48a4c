"""The aggregate window functions of WindowOperator (pa_framed_window_create) over device-resident pages, operator to operator, in the
setting of scripts/bench_window.py: 64 Mi rows in 2^24-row pages, one BIGINT partition key at 4 / 1 K / 100 K / 3 M / all-distinct keys, a
random DOUBLE sort key, a BIGINT argument.

The yardstick is rank() alone through pa_window_create on the same pages in the same process, alternated run by run: it is the operator
as it was before the aggregates existed, so a ratio shows what the gather, the scans and the extra columns of the function pass cost.
Measured against it: sum(x) with the default frame (RANGE .. CURRENT ROW), min(x) ROWS .. CURRENT ROW, and rank() with all five
aggregates in one operator.  Before anything is timed the function columns of every configuration are checked on the host against numpy
over the operator's own sorted output (partition key, sort key, argument).
Per configuration: seconds and rows/s of the whole operator life (create, every page in, finish, output taken, close), warmed up once,
median and min-max of --reps; `passes_s` is flags + scans + starts + gather + aggregate scans + functions between two events on the
operator's stream.  Prints one JSON object; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from presto_amd import _lib, abi  # noqa: E402
from presto_amd.operators import FramedWindowOperator, WindowOperator, download_page, upload_page  # noqa: E402
from presto_amd.page import Block, Page  # noqa: E402

ASC_NULLS_LAST = 1
UP, CR = abi.BOUND_UNBOUNDED_PRECEDING, abi.BOUND_CURRENT_ROW
ROWS_FRAME = (abi.FRAME_ROWS, UP, CR)
CONFIGS = [("sum_range", [(abi.WINDOW_SUM, [2])]),
           ("min_rows", [(abi.WINDOW_MIN, [2], ROWS_FRAME)]),
           ("rank_and_five", [abi.WINDOW_RANK, abi.WINDOW_COUNT_STAR, (abi.WINDOW_COUNT, [2]), (abi.WINDOW_SUM, [2]), (abi.WINDOW_MIN, [2]), (abi.WINDOW_MAX, [2])])]
OUTPUTS = [0, 1, 2]


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


def columns_of(pages, count):
    pages = [download_page(p) if p.mem == abi.MEM_DEVICE else p for p in pages]
    return [np.concatenate([p.blocks[c].values[:p.position_count] for p in pages]) for c in range(count)]


def expected(key, sort_key, x, functions):
    """the function columns over the operator's own sorted output (no NULLs, |x| < 2^20): numpy restatement of the frames"""
    n = len(key)
    at = np.arange(n, dtype=np.int64)
    head = np.ones(n, bool)
    head[1:] = key[1:] != key[:-1]
    peer_head = head.copy()
    peer_head[1:] |= sort_key[1:] != sort_key[:-1]
    first = np.maximum.accumulate(np.where(head, at, 0))
    part_id = np.cumsum(head) - 1
    peer_first = np.flatnonzero(peer_head)
    peer_last = np.append(peer_first[1:], n) - 1
    peer_id = np.cumsum(peer_head) - 1
    e_range = peer_last[peer_id]
    run_sum = np.cumsum(x)
    run_sum -= (run_sum - x)[first]
    big = np.int64(1) << 22
    run_min = np.minimum.accumulate(x - part_id * big) + part_id * big
    run_max = np.maximum.accumulate(x + part_id * big) - part_id * big
    out = []
    for f in functions:
        f = (f, []) if isinstance(f, int) else f
        e = at if len(f) > 2 and f[2][0] == abi.FRAME_ROWS else e_range
        if f[0] == abi.WINDOW_RANK:
            out.append(peer_first[peer_id] - first + 1)
        elif f[0] in (abi.WINDOW_COUNT_STAR, abi.WINDOW_COUNT):
            out.append(e - first + 1)
        else:
            out.append({abi.WINDOW_SUM: run_sum, abi.WINDOW_MIN: run_min, abi.WINDOW_MAX: run_max}[f[0]][e])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 26)
    ap.add_argument("--page-rows", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="one key count by label (profiling runs), e.g. bigint_100000")
    ap.add_argument("--config", default=None, help="one configuration by name (profiling runs), e.g. rank_and_five")
    ap.add_argument("--no-check", action="store_true", help="skip the output check (profiling runs)")
    ap.add_argument("--no-compare", action="store_true", help="without the rank() yardstick (profiling runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.init(0)
    rows, page_rows = args.rows, args.page_rows
    rng = np.random.default_rng(1)
    out = {"rows": rows, "page_rows": page_rows, "reps": args.reps, "command": " ".join(["python"] + sys.argv), "shapes": []}
    types = [abi.BIGINT, abi.DOUBLE, abi.BIGINT]
    partition, sort, orders = [0], [1], [ASC_NULLS_LAST]
    for groups in (4, 1000, 100_000, 3_000_000, rows):
        label = "bigint_all_distinct" if groups >= rows else "bigint_%d" % groups
        if args.only and args.only != label:
            continue
        keys = rng.permutation(rows).astype(np.int64) if groups >= rows else rng.integers(0, groups, rows, dtype=np.int64)
        columns = [keys, rng.random(rows), rng.integers(-(1 << 20) + 1, 1 << 20, rows, dtype=np.int64)]
        pages = []
        for at in range(0, rows, page_rows):
            m = min(page_rows, rows - at)
            pages.append(upload_page(Page([Block.flat(t, c[at:at + m]) for t, c in zip(types, columns)], m)))
        del keys, columns
        seen = {}

        def baseline():
            op = WindowOperator(types, OUTPUTS, [abi.WINDOW_RANK], partition, sort, orders, output_mem=abi.MEM_DEVICE)
            result = run(op, pages)
            seen["rank_passes_ms"], _ = op.kernelTime()
            del result
            op.close()

        def framed(functions, keep=False):
            def life():
                op = FramedWindowOperator(types, OUTPUTS, functions, partition, sort, orders, output_mem=abi.MEM_DEVICE)
                result = run(op, pages)
                seen["passes_ms"], _ = op.kernelTime()
                seen["memory_bytes"] = op.memoryBytes()
                if keep:
                    seen["result"] = columns_of(result, len(OUTPUTS) + len(functions))
                del result
                op.close()
            return life

        for name, functions in CONFIGS:
            if args.config and args.config != name:
                continue
            e = {"shape": label + "_" + name, "keys": groups, "functions": len(functions)}
            if not args.no_check:
                framed(functions, keep=True)()
                got = seen.pop("result")
                want = expected(got[0], got[1], got[2], functions)
                same = all(g.dtype == np.int64 and np.array_equal(g, w) for g, w in zip(got[len(OUTPUTS):], want))
                e["outputs_checked"] = bool(same)
                assert same, e["shape"]
                del got, want
            measured = alternated([framed(functions)] + ([] if args.no_compare else [baseline]), args.reps)
            med, lo, hi = measured[0]
            e.update({"window_s_median": med, "window_s_min": lo, "window_s_max": hi, "window_rows_per_s": rows / med, "passes_s": seen["passes_ms"] / 1e3,
                      "memory_bytes_at_end": seen["memory_bytes"]})
            if not args.no_compare:
                bmed, blo, bhi = measured[1]
                e.update({"rank_s_median": bmed, "rank_s_min": blo, "rank_s_max": bhi, "rank_passes_s": seen["rank_passes_ms"] / 1e3, "over_rank": med / bmed,
                          "spread": max((hi - lo) / med, (bhi - blo) / bmed)})
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
