#!/usr/bin/env python3
"""What the value window functions add to WindowOperator's passes: the operator's own timer (the passes behind the sort, flags to function
pass, between two events on its stream) with `rank, sum` and with `rank, sum, lag(x, 1), last_value(x)` on the same device pages, the
configurations alternated life by life; a third configuration reads lag's offset from a channel.  Every value column is checked on the
host against numpy over the operator's own sorted output before anything is timed.  One JSON line: min / median / max per configuration
and the added time and bytes per row and value column.

    python scripts/bench_window_values.py [--rows 4194304] [--keys 1000] [--reps 7] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from presto_amd import _lib, abi  # noqa: E402
from presto_amd.operators import FramedWindowOperator, download_page, upload_page  # noqa: E402
from presto_amd.page import Block, Page  # noqa: E402

ASC_NULLS_LAST = 1
TYPES = [abi.BIGINT, abi.DOUBLE, abi.BIGINT, abi.BIGINT]          # partition key, sort key, x, the constant 1
BASE = [abi.WINDOW_RANK, (abi.WINDOW_SUM, [2])]
CONFIGS = [("rank_sum", BASE),
           ("rank_sum_lag_last", BASE + [(abi.WINDOW_LAG, [2]), (abi.WINDOW_LAST_VALUE, [2])]),
           ("rank_sum_lag_channel_last", BASE + [(abi.WINDOW_LAG, [2, 3]), (abi.WINDOW_LAST_VALUE, [2])])]


def life(functions, pages, keep=False):
    """one operator life -> (ms of the passes, the output pages on the host when `keep`)"""
    op = FramedWindowOperator(TYPES, [0, 1, 2], functions, [0], [1], [ASC_NULLS_LAST], output_mem=abi.MEM_DEVICE)
    for p in pages:
        op.addInput(p)
    op.finish()
    out = []
    while True:
        page = op.getOutput()
        if page is None:
            break
        out.append(download_page(page) if keep else page)
    _lib.device_synchronize()
    ms, _ = op.kernelTime()
    del page
    if not keep:
        out = None
    op.close()
    return ms, out


def check(pages, functions):
    """lag(x, 1) and last_value(x) over RANGE .. CURRENT ROW against numpy over the sorted output (the sort key is random: no peers)"""
    cols = [np.concatenate([p.blocks[c].values[:p.position_count] for p in pages]) for c in range(3 + len(functions))]
    nulls = [np.concatenate([np.zeros(p.position_count, bool) if p.blocks[c].nulls is None else p.blocks[c].nulls[:p.position_count].astype(bool) for p in pages])
             for c in range(3 + len(functions))]
    key, x = cols[0], cols[2]
    head = np.ones(len(key), bool)
    head[1:] = key[1:] != key[:-1]
    lag = np.where(head, 0, np.concatenate([[0], x[:-1]]))
    ok = np.array_equal(nulls[5], head) and np.array_equal(np.where(head, 0, cols[5]), lag)
    return bool(ok and not nulls[6].any() and np.array_equal(cols[6], x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--keys", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.init(0)
    rng = np.random.default_rng(7)
    rows = args.rows
    columns = [rng.integers(0, args.keys, rows, dtype=np.int64), rng.random(rows), rng.integers(-(1 << 20) + 1, 1 << 20, rows, dtype=np.int64), np.ones(rows, np.int64)]
    pages = [upload_page(Page([Block.flat(t, c) for t, c in zip(TYPES, columns)], rows))]
    del columns
    out = {"rows": rows, "keys": args.keys, "reps": args.reps, "configs": {}}
    for name, functions in CONFIGS[1:]:
        _, result = life(functions, pages, keep=True)
        out.setdefault("outputs_checked", True)
        out["outputs_checked"] = out["outputs_checked"] and check(result, functions)
        assert out["outputs_checked"], name
        del result
    times = {name: [] for name, _ in CONFIGS}
    for r in range(args.reps + 1):                                 # one round to warm up (code objects, the pool), then alternated
        for name, functions in CONFIGS:
            ms, _ = life(functions, pages)
            if r > 0:
                times[name].append(ms)
    for name, t in times.items():
        out["configs"][name] = {"passes_ms_min": min(t), "passes_ms_median": sorted(t)[len(t) // 2], "passes_ms_max": max(t)}
    base = out["configs"]["rank_sum"]["passes_ms_median"]
    for name in ("rank_sum_lag_last", "rank_sum_lag_channel_last"):
        added = [a - b for a, b in zip(times[name], times["rank_sum"])]                 # round by round: neighbours in time
        out["configs"][name].update({"added_ms_min": min(added), "added_ms_median": sorted(added)[len(added) // 2], "added_ms_max": max(added),
                                     "added_ns_per_row_per_value_column": (out["configs"][name]["passes_ms_median"] - base) * 1e6 / rows / 2})
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
