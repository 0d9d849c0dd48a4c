#!/usr/bin/env python3
"""String matching in generated code: FilterAndProject over one device page of 16 Mi rows with a VARCHAR column shaped like TPC-H's p_type
(150 distinct values of about 20 bytes) and one shaped like o_comment (19 .. 78 random bytes), under five filters each: `col = 'lit'`
(what the generator could do before LIKE: the comparison), LIKE 'lit%', LIKE '%lit%', LIKE '%a%b%' and LIKE '%a_b%'.  The operator
projects a BIGINT row id to a device page; a pass is addInput .. getOutput between two device synchronisations.  The selected rows are
checked against tests/scalar_model.py (the whole p_type column through its 150 values, the first 65536 rows of the comment column) before
anything is timed.  One JSON line: min / median / max ms per configuration, rows/s and string bytes/s as ranges, and the fraction of the
6.3 TB/s streaming ceiling (README.md) that the filter's input -- the string bytes and 4 bytes of offset per row -- amounts to.

    python scripts/bench_like.py [--rows 16777216] [--reps 7] [--only equality] [--out FILE]
    PRESTO_AMD_LIB=<another build's libpresto_amd.so> python scripts/bench_like.py --only equality      # the comparison on another build"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from presto_amd import _lib, abi  # noqa: E402
from presto_amd.expr import constant, field  # noqa: E402
from presto_amd.operators import FilterAndProjectOperator, upload_page  # noqa: E402
from presto_amd.page import Block, Page  # noqa: E402
from tests import scalar_model as S  # noqa: E402

STREAMING_CEILING = 6.3e12      # bytes/s, README.md
TYPES = [abi.VARCHAR, abi.BIGINT]
P_TYPES = ["%s %s %s" % (a, b, c) for a in ("STANDARD", "SMALL", "MEDIUM", "LARGE", "ECONOMY", "PROMO")
           for b in ("ANODIZED", "BURNISHED", "PLATED", "POLISHED", "BRUSHED") for c in ("TIN", "NICKEL", "BRASS", "STEEL", "COPPER")]
# column -> [(configuration, pattern or literal)]
FILTERS = {
    "p_type": [("equality", "PROMO BURNISHED COPPER"), ("prefix", "PROMO%"), ("contains", "%BRASS%"), ("chain", "%BURN%COP%"), ("general", "%BUR_ISHED%")],
    "o_comment": [("equality", "the quick"), ("prefix", "th%"), ("contains", "%the%"), ("chain", "%th%qu%"), ("general", "%th_q%")],
}
LETTERS = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz  eeetthq", dtype=np.uint8)


def p_type_column(rows, rng):
    ids = rng.integers(0, len(P_TYPES), rows)
    words = [w.encode() for w in P_TYPES]
    data = np.frombuffer(b"".join(words[i] for i in ids.tolist()), dtype=np.uint8)
    lengths = np.array([len(w) for w in words], dtype=np.int64)[ids]
    return data, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), ids


def comment_column(rows, rng):
    lengths = rng.integers(19, 79, rows)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return LETTERS[rng.integers(0, len(LETTERS), int(offsets[-1]))], offsets


def make_filter(name, literal):
    s = field(0, abi.VARCHAR)
    return s.eq(constant(literal, abi.VARCHAR)) if name == "equality" else s.like(literal)


def model(name, literal, value):
    return value == literal if name == "equality" else S.like(value, literal)


def one_pass(op_args, page):
    """one operator life over the page -> (selected rows, ms between two device synchronisations)"""
    op = FilterAndProjectOperator(*op_args, output_mem=abi.MEM_DEVICE)
    _lib.device_synchronize()
    t0 = time.perf_counter()
    op.addInput(page)
    selected = 0
    while True:
        out = op.getOutput()
        if out is None:
            break
        selected += out.position_count
    _lib.device_synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    del out
    op.close()
    return selected, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default=None, help="run one configuration (equality, prefix, contains, chain, general)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.init(0)
    rng = np.random.default_rng(7)
    rows = args.rows
    ids = np.arange(rows, dtype=np.int64)
    out = {"rows": rows, "reps": args.reps, "library": _lib.LIB_PATH if os.environ.get("PRESTO_AMD_LIB") else "this build",
           "streaming_ceiling_bytes_per_s": STREAMING_CEILING, "columns": {}}
    for column in ("p_type", "o_comment"):
        if column == "p_type":
            data, offsets, word_ids = p_type_column(rows, rng)
        else:
            data, offsets = comment_column(rows, rng)
        page = upload_page(Page([Block.varwidth(data, offsets), Block.bigint(ids)], rows))
        string_bytes = int(offsets[-1])
        result = {"string_bytes": string_bytes, "bytes_per_row": string_bytes / rows, "configs": {}}
        for name, literal in FILTERS[column]:
            if args.only and name != args.only:
                continue
            op_args = (TYPES, make_filter(name, literal), [field(1, abi.BIGINT)])
            selected, _ = one_pass(op_args, page)                       # (warms the code object up, too)
            if column == "p_type":
                want = int(np.array([model(name, literal, w) for w in P_TYPES], dtype=np.int64)[word_ids].sum())
            else:                                                       # the first rows, on a page of their own
                n = min(rows, 65536)
                small = upload_page(Page([Block.varwidth(data[:offsets[n]], offsets[:n + 1]), Block.bigint(ids[:n])], n))
                want = sum(model(name, literal, bytes(data[offsets[i]:offsets[i + 1]]).decode()) for i in range(n))
                got_small, _ = one_pass(op_args, small)
                assert got_small == want, (column, name, got_small, want)
                want = selected
            assert selected == want, (column, name, selected, want)
            times = sorted(one_pass(op_args, page)[1] for _ in range(args.reps))
            moved = string_bytes + 4 * rows
            result["configs"][name] = {
                "filter": literal, "selected": selected, "ms_min": times[0], "ms_median": times[len(times) // 2], "ms_max": times[-1],
                "rows_per_s": [rows / (times[-1] * 1e-3), rows / (times[0] * 1e-3)],
                "string_bytes_per_s": [string_bytes / (times[-1] * 1e-3), string_bytes / (times[0] * 1e-3)],
                "fraction_of_streaming_ceiling": [moved / (times[-1] * 1e-3) / STREAMING_CEILING, moved / (times[0] * 1e-3) / STREAMING_CEILING],
            }
        out["columns"][column] = result
        del page
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
