"""SqlSemiJoinInPredicateBenchmark's shape on device-resident TPC-H data:
    SELECT orderkey FROM lineitem WHERE orderkey IN (SELECT orderkey FROM orders WHERE orderkey % 2 = 0)
Build: orders' o_orderkey filtered by % 2 = 0; probe: lineitem's l_orderkey in 2^26-row device pages.  Extra cases time the generic
path: the same probe keys against a VARCHAR set and a DOUBLE set of 1 M values.  For comparison, LookupJoinOperator
(output_single_match) probes the same pages against a lookup source of the same keys.  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from presto_amd import _lib, abi, tpch  # noqa: E402
from presto_amd.operators import (HashBuilderOperator, HashSemiJoinOperator, LookupJoinOperator, LookupSourceFactory,  # noqa: E402
                                  SetBuilderOperator, SetSupplier, download, to_pages, upload_page)
from presto_amd.page import Block, Page  # noqa: E402

HBM_BYTES_PER_S = 8e12


def timed_pages(op, pages, reps):
    """Seconds per pass of `pages` through a probe operator (device output pages, completed on return)."""
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        for p in pages:
            op.addInput(p)
            while op.getOutput() is not None:
                pass
        best = min(best, time.perf_counter() - t)
    return best


def digits(keys, width=8):
    """VARCHAR page values of the keys as zero-padded decimal strings (fixed width)."""
    k = np.asarray(keys, np.int64)
    cols = [((k // 10 ** (width - 1 - i)) % 10 + 48).astype(np.uint8) for i in range(width)]
    return np.stack(cols, 1).reshape(-1), (np.arange(len(k) + 1, dtype=np.int32) * width)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=10.0)
    ap.add_argument("--page-rows", type=int, default=1 << 26)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--extra-rows", type=int, default=1 << 22, help="probe rows of the VARCHAR / DOUBLE cases")
    args = ap.parse_args()
    _lib.init(0)
    no, nl = tpch.orders_rows(args.sf), tpch.lineitem_rows(args.sf)
    orders = tpch.DeviceColumns([abi.O_ORDERKEY], args.sf, no)
    lineitem = tpch.DeviceColumns([abi.L_ORDERKEY], args.sf, nl)
    okeys = download(orders.page().blocks[0].values, np.int64, no)
    even = okeys[okeys % 2 == 0]
    build_page = upload_page(Page([Block.bigint(even)], len(even)))
    build_page.stable = True
    probe_pages = list(lineitem.pages(args.page_rows))
    out = {"sf": args.sf, "build_rows": int(len(even)), "probe_rows": nl, "page_rows": args.page_rows}

    # semi-join: build
    best_build = float("inf")
    for _ in range(args.reps):
        s = SetSupplier()
        b = SetBuilderOperator(s, [abi.BIGINT], 0, expected_positions=len(even))
        t = time.perf_counter()
        to_pages(b, [build_page])
        best_build = min(best_build, time.perf_counter() - t)
        b.close()
    j = HashSemiJoinOperator(s, [abi.BIGINT], 0, output_mem=abi.MEM_DEVICE)
    timed_pages(j, probe_pages, 1)
    sec = timed_pages(j, probe_pages, args.reps)
    ms, launches = j.kernelTime()
    kernel_s = ms / 1e3 / max(launches, 1) * len(probe_pages)
    bytes_per_row = 8 + 1   # the key read, the mark written (the bitmap's lines hit the caches: DESIGN.md section 4)
    out.update({
        "semi_kernel": j.kernelName(),
        "set_size": s.stats()[0],
        "build_rows_per_s": len(even) / best_build,
        "probe_rows_per_s": nl / sec,
        "probe_kernel_rows_per_s": nl / kernel_s,
        "probe_kernel_bytes_per_row": bytes_per_row,
        "probe_kernel_fraction_of_8TBs": nl / kernel_s * bytes_per_row / HBM_BYTES_PER_S,
    })
    j.close()

    # the inner join's single-match probe over the same pages and keys
    bridge = LookupSourceFactory()
    hb = HashBuilderOperator(bridge, [abi.BIGINT], [0], [], expected_positions=len(even))
    to_pages(hb, [build_page])
    lj = LookupJoinOperator(bridge, [abi.BIGINT], [0], [0], output_mem=abi.MEM_DEVICE, output_single_match=True)
    timed_pages(lj, probe_pages, 1)
    sec_join = timed_pages(lj, probe_pages, args.reps)
    out.update({"single_match_join_rows_per_s": nl / sec_join, "semi_over_join_speedup": sec_join / sec})
    lj.close()

    # generic path: VARCHAR and DOUBLE sets of 1 M values, probed by the first extra-rows lineitem keys
    m = min(args.extra_rows, nl)
    lkeys = download(probe_pages[0].blocks[0].values, np.int64, min(m, probe_pages[0].position_count))
    set_keys = even[: 1 << 20]
    for name, t, mk in (("varchar", abi.VARCHAR, lambda k: Block.varwidth(*digits(k))), ("double", abi.DOUBLE, lambda k: Block.double(k.astype(np.float64)))):
        sp = upload_page(Page([mk(set_keys)], len(set_keys)))
        pp = upload_page(Page([mk(lkeys)], len(lkeys)))
        pp.stable = True
        s2 = SetSupplier()
        t0 = time.perf_counter()
        to_pages(SetBuilderOperator(s2, [t], 0), [sp])
        tb = time.perf_counter() - t0
        j2 = HashSemiJoinOperator(s2, [t], 0, output_mem=abi.MEM_DEVICE)
        timed_pages(j2, [pp], 1)
        sec2 = timed_pages(j2, [pp], args.reps)
        out.update({name + "_kernel": j2.kernelName(), name + "_build_rows_per_s": len(set_keys) / tb, name + "_probe_rows_per_s": len(lkeys) / sec2})
        j2.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
