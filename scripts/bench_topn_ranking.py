"""TopNRankingOperator over device-resident pages, operator to operator: 64 Mi rows in 2^24-row pages, one BIGINT partition key at
4 / 1 K / 100 K / 3 M / all-distinct keys and (BIGINT, DOUBLE) at 100 K, a random DOUBLE sort key, n = 10, ROW_NUMBER; the 1 K shape also
with RANK, with n = 1 and n = 1 000, and with a second (VARCHAR) sort channel; and the mode without partition channels.

Measured against the best the operators that existed before can do for the same answer on the same pages in the same process, alternated
with it run by run: OrderByOperator over (key, sort channels) feeding RowNumberOperator with cap n -- the two results are compared row
for row (beyond 2^23 kept rows: row counts and an order-independent 64-bit checksum of the rows) before anything is timed -- and, without
partition channels, TopNOperator.  RANK has no such composition (RowNumber does not rank): its shape is timed beside the ROW_NUMBER one.
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
from presto_amd.operators import OrderByOperator, RowNumberOperator, TopNOperator, TopNRankingOperator, download_page, upload_page  # noqa: E402
from presto_amd.page import Block, Page  # noqa: E402

ASC_NULLS_LAST = 1


def device_pages(blocks_of, rows, page_rows):
    """blocks_of(at, n) -> host blocks of rows [at, at + n) -> stable PA_MEM_DEVICE pages of page_rows rows."""
    pages = []
    for at in range(0, rows, page_rows):
        n = min(page_rows, rows - at)
        p = upload_page(Page(blocks_of(at, n), n))
        p.stable = True
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


def columns_of(pages):
    pages = [download_page(p) if p.mem == abi.MEM_DEVICE else p for p in pages]
    if not pages:
        return []
    return [np.concatenate([p.blocks[c].values[:p.position_count] for p in pages]) for c in range(len(pages[0].blocks)) if pages[0].blocks[c].type != abi.VARCHAR]


def checksum(cols):
    """order-independent: the wrapping sum over the rows of a mix of the columns' bit patterns"""
    mix = np.zeros(len(cols[0]), np.uint64)
    for i, c in enumerate(cols):
        mix = mix * np.uint64(0x9E3779B97F4A7C15) + np.ascontiguousarray(c).view(np.uint64) * np.uint64(2 * i + 3)
    return int(np.sum(mix, dtype=np.uint64)), len(cols[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 26)
    ap.add_argument("--page-rows", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="one shape by name (profiling runs), e.g. bigint_100000")
    ap.add_argument("--no-compare", action="store_true", help="the new operator alone (profiling runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.init(0)
    rows, page_rows = args.rows, args.page_rows
    rng = np.random.default_rng(1)
    # (name, partition keys, two partition channels, ranking, n, VARCHAR second sort channel)
    shapes = [("bigint_%d" % g, g, False, abi.RANKING_ROW_NUMBER, 10, False) for g in (4, 1000, 100_000, 3_000_000)]
    shapes += [("bigint_all_distinct", rows, False, abi.RANKING_ROW_NUMBER, 10, False), ("bigint_double_100000", 100_000, True, abi.RANKING_ROW_NUMBER, 10, False),
               ("bigint_1000_rank", 1000, False, abi.RANKING_RANK, 10, False), ("bigint_1000_n1", 1000, False, abi.RANKING_ROW_NUMBER, 1, False),
               ("bigint_1000_n1000", 1000, False, abi.RANKING_ROW_NUMBER, 1000, False), ("bigint_1000_varchar", 1000, False, abi.RANKING_ROW_NUMBER, 10, True),
               ("unpartitioned", 0, False, abi.RANKING_ROW_NUMBER, 10, False)]
    out = {"rows": rows, "page_rows": page_rows, "reps": args.reps, "command": " ".join(["python"] + sys.argv), "shapes": []}
    for name, groups, two, ranking, n, text in shapes:
        if args.only and args.only != name:
            continue
        keys = rng.permutation(rows).astype(np.int64) if groups >= rows else rng.integers(0, max(groups, 1), rows, dtype=np.int64)
        # a random DOUBLE sort key; beside a VARCHAR channel 100 values, so that the second channel decides most places
        sort_key = rng.integers(0, 100, rows).astype(np.float64) if text else rng.random(rows)
        columns = [(abi.BIGINT, keys)] + ([(abi.DOUBLE, (keys % 7).astype(np.float64) * 0.5)] if two else []) + [(abi.DOUBLE, sort_key)]
        types = [t for t, _ in columns] + ([abi.VARCHAR] if text else [])
        letters = rng.integers(97, 123, (rows, 4)).astype(np.uint8) if text else None

        def blocks_of(at, m):
            blocks = [Block.flat(t, a[at:at + m]) for t, a in columns]
            if text:
                blocks.append(Block.varwidth(letters[at:at + m].reshape(-1), np.arange(m + 1, dtype=np.int32) * 4))
            return blocks

        pages = device_pages(blocks_of, rows, page_rows)
        partition = [] if groups == 0 else ([0, 1] if two else [0])
        first_sort = len(columns) - 1
        sort = [first_sort] + ([first_sort + 1] if text else [])
        orders = [ASC_NULLS_LAST] * len(sort)
        outputs = list(range(len(columns)))                      # the fixed-width channels
        expected = min(max(groups, 1), (1 << 31) - 1)
        seen = {}

        def topn_ranking():
            op = TopNRankingOperator(types, outputs, partition, sort, orders, n, ranking_type=ranking, expected_positions=expected, output_mem=abi.MEM_DEVICE)
            for p in pages:
                op.addInput(p)
            op.finish()
            result = []
            while True:
                page = op.getOutput()
                if page is None:
                    break
                result.append(page)
            seen["stats"] = op.topNRankingStats()
            seen["filter_ms"], seen["filter_launches"] = op.kernelTime()
            seen["memory_bytes"] = op.memoryBytes()
            seen["result"] = columns_of(result) if seen.get("keep_result") else None
            del result
            op.close()

        def composition():
            if not partition:
                # TopNOperator emits every input channel
                op = TopNOperator(types, n, sort, orders, output_mem=abi.MEM_DEVICE)
                for p in pages:
                    op.addInput(p)
                op.finish()
                result = []
                while True:
                    page = op.getOutput()
                    if page is None:
                        break
                    result.append(page)
                seen["composed"] = columns_of(result) if seen.get("keep_result") else None
                del result
                op.close()
                return
            order_by = OrderByOperator(types, list(range(len(types))), partition + sort, [ASC_NULLS_LAST] * (len(partition) + len(sort)), output_mem=abi.MEM_DEVICE)
            for p in pages:
                order_by.addInput(p)
            order_by.finish()
            row_number = RowNumberOperator(types, outputs, partition, n, expected_positions=expected, output_mem=abi.MEM_DEVICE)
            result = []
            while True:
                page = order_by.getOutput()
                if page is None:
                    break
                row_number.addInput(page)
                numbered = row_number.getOutput()
                if numbered is not None:
                    result.append(numbered)
            row_number.finish()
            seen["composed"] = columns_of(result) if seen.get("keep_result") else None
            del result
            row_number.close()
            order_by.close()

        e = {"shape": name, "keys": groups, "partition_channels": len(partition), "sort_channels": len(sort), "n": n,
             "ranking": "rank" if ranking == abi.RANKING_RANK else "row_number"}
        compare = not args.no_compare and ranking == abi.RANKING_ROW_NUMBER
        if compare:
            # the same answer first
            seen["keep_result"] = True
            topn_ranking()
            composition()
            got, want = seen.pop("result"), seen.pop("composed")
            seen["keep_result"] = False
            if not partition:
                got = got[:-1]                                   # TopN has no ranking column; its rows come in the same order
                want = want[:len(got)]
                same = all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(got, want))
            elif len(got[0]) <= (1 << 23):
                # the composition emits partitions in key order, the operator in first-seen order: regroup, keep the order inside
                regroup = np.lexsort(tuple(reversed([got[c] for c in range(len(partition))])))
                same = len(got[0]) == len(want[0]) and all(np.array_equal(a[regroup].view(np.uint64), b.view(np.uint64)) for a, b in zip(got, want))
            else:
                same = checksum(got) == checksum(want)
            e["rows_kept"] = int(len(got[0]))
            e["same_rows_as_composition"] = bool(same)
            assert same, name
            del got, want
        fns = [topn_ranking] + ([composition] if compare else [])
        measured = alternated(fns, args.reps)
        med, lo, hi = measured[0]
        partitions, capacity, held = seen["stats"]
        e.update({"topn_ranking_s_median": med, "topn_ranking_s_min": lo, "topn_ranking_s_max": hi, "topn_ranking_rows_per_s": rows / med,
                  "partition_count": partitions, "table_capacity": capacity, "rows_held_at_end": held, "filter_kernel_s": seen["filter_ms"] / 1e3,
                  "filter_launches": seen["filter_launches"], "memory_bytes_at_end": seen["memory_bytes"]})
        if seen["filter_ms"] > 0:
            # a whole-pass figure: the filter's algorithmic bytes (8 B id + 8 B image per row) over its measured time
            e["filter_whole_pass_bytes_per_s"] = 16.0 * rows / (seen["filter_ms"] / 1e3)
            e["filter_fraction_of_8TBps"] = e["filter_whole_pass_bytes_per_s"] / 8e12
        if compare:
            cmed, clo, chi = measured[1]
            spread = max((hi - lo) / med, (chi - clo) / cmed, 0.03)
            e.update({"composition": "TopN" if not partition else "OrderBy -> RowNumber(cap n)", "composition_s_median": cmed, "composition_s_min": clo,
                      "composition_s_max": chi, "composition_rows_per_s": rows / cmed, "composition_over_topn_ranking": cmed / med, "spread": spread,
                      "faster_by_more_than_the_spread": bool(cmed / med > 1 + spread)})
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
