"""ctypes binding of the CPU oracle (oracle/liboracle.so).

TEST INFRASTRUCTURE ONLY -- imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline
leg, never by anything under presto_amd/.  See oracle/presto_oracle.h.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from presto_amd import abi
from presto_amd.expr import serialize, serialize_many
from presto_amd.page import Block, Page, page_from_c

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE])


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "liboracle.so")
        if not os.path.exists(path):
            build()
        L = C.CDLL(path)
        L.orc_last_error.restype = C.c_char_p
        L.orc_xxh64.restype = C.c_uint64
        L.orc_xxh64.argtypes = [C.c_void_p, C.c_int64, C.c_uint64]
        for name in ("orc_xxh64_long", "orc_hash_bigint", "orc_murmur3_fmix"):
            getattr(L, name).restype = C.c_int64
            getattr(L, name).argtypes = [C.c_int64]
        L.orc_hash_integer.restype = C.c_int64
        L.orc_hash_integer.argtypes = [C.c_int32]
        L.orc_hash_boolean.restype = C.c_int64
        L.orc_hash_boolean.argtypes = [C.c_int32]
        L.orc_hash_double.restype = C.c_int64
        L.orc_hash_double.argtypes = [C.c_double]
        L.orc_combine_hash.restype = C.c_int64
        L.orc_combine_hash.argtypes = [C.c_int64, C.c_int64]
        L.orc_array_size.argtypes = [C.c_int32, C.c_float]
        L.orc_hash_agg_create.restype = C.c_void_p
        L.orc_hash_agg_create.argtypes = [C.POINTER(abi.pa_hash_aggregation_desc)]
        L.orc_hash_agg_add_page.argtypes = [C.c_void_p, C.POINTER(abi.pa_page), C.c_void_p]
        L.orc_hash_agg_group_count.argtypes = [C.c_void_p]
        L.orc_hash_agg_capacity.argtypes = [C.c_void_p]
        L.orc_hash_agg_contains.argtypes = [C.c_void_p, C.POINTER(abi.pa_page), C.c_int32]
        L.orc_hash_agg_build_result.argtypes = [C.c_void_p, C.POINTER(abi.pa_page)]
        L.orc_hash_agg_default_output.argtypes = [C.POINTER(abi.pa_hash_aggregation_desc), C.POINTER(abi.pa_page)]
        L.orc_hash_agg_destroy.argtypes = [C.c_void_p]
        L.orc_join_create.restype = C.c_void_p
        L.orc_join_create.argtypes = [C.POINTER(abi.pa_hash_builder_desc)]
        L.orc_join_add_build_page.argtypes = [C.c_void_p, C.POINTER(abi.pa_page)]
        L.orc_join_build.argtypes = [C.c_void_p]
        L.orc_join_build_positions.argtypes = [C.c_void_p]
        L.orc_join_tables.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]
        L.orc_join_probe.argtypes = [C.c_void_p, C.POINTER(abi.pa_lookup_join_desc), C.POINTER(abi.pa_page),
                                     C.POINTER(abi.pa_page), C.POINTER(C.POINTER(C.c_int32)),
                                     C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_int32)]
        L.orc_join_outer.argtypes = [C.c_void_p, C.POINTER(abi.pa_lookup_join_desc), C.POINTER(abi.pa_page)]
        L.orc_join_destroy.argtypes = [C.c_void_p]
        L.orc_free.argtypes = [C.c_void_p]
        L.orc_free_page.argtypes = [C.POINTER(abi.pa_page)]
        L.orc_filter.argtypes = [C.POINTER(abi.pa_page), C.POINTER(abi.pa_expr), C.c_void_p,
                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.orc_filter_project.argtypes = [C.POINTER(abi.pa_page), C.POINTER(abi.pa_expr), C.c_int32,
                                         C.POINTER(abi.pa_expr), C.POINTER(abi.pa_page)]
        L.orc_hash_page.argtypes = [C.POINTER(abi.pa_page), C.c_int32, C.POINTER(C.c_int32), C.c_void_p]
        L.orc_partition_ids.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        L.orc_partition_positions.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.orc_tpch_generate.argtypes = [C.c_int32, C.c_double, C.c_int64, C.c_int64, C.c_uint64, C.c_void_p,
                                        C.c_void_p]
        L.orc_q6.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double),
                             C.POINTER(C.c_int64)]
        L.orc_q1_add.argtypes = [C.c_void_p] + [C.c_void_p] * 9 + [C.c_int64]
        L.orc_decimal_state_after.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
        L.orc_sort_positions_bigint.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.orc_topn_double_desc_bigint_asc.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        _LIB = L
    return _LIB


class OracleError(Exception):
    def __init__(self, status, message):
        super().__init__("%s: %s" % (abi.STATUS_NAMES.get(status, status), message))
        self.status = status


def _check(rc):
    if rc < 0:
        raise OracleError(rc, lib().orc_last_error().decode())
    return rc


# ---- hashes ---------------------------------------------------------------------------------
def xxh64(data, seed=0):
    buf = C.create_string_buffer(bytes(data), max(len(data), 1))
    return lib().orc_xxh64(buf, len(data), seed)


def _s64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def xxh64_long(v): return lib().orc_xxh64_long(_s64(v))
def hash_bigint(v): return lib().orc_hash_bigint(_s64(v))
def hash_integer(v): return lib().orc_hash_integer(v)
def hash_double(v): return lib().orc_hash_double(v)
def hash_boolean(v): return lib().orc_hash_boolean(1 if v else 0)
def murmur3_fmix(v): return lib().orc_murmur3_fmix(_s64(v))
def combine_hash(a, b): return lib().orc_combine_hash(_s64(a), _s64(b))
def array_size(expected, fill=0.75): return lib().orc_array_size(expected, fill)


def hash_page(page, channels):
    cpage, keep = page.to_c()
    out = np.zeros(page.position_count, dtype=np.int64)
    ch = abi.int32_array(channels)
    _check(lib().orc_hash_page(C.byref(cpage), len(channels), ch, out.ctypes.data))
    return out


def partition_ids(raw_hash, partition_count, local=True):
    raw_hash = np.ascontiguousarray(raw_hash, dtype=np.int64)
    out = np.zeros(len(raw_hash), dtype=np.int32)
    _check(lib().orc_partition_ids(raw_hash.ctypes.data, len(raw_hash), partition_count, 1 if local else 0,
                                   out.ctypes.data))
    return out


def partition_positions(partition, partition_count):
    partition = np.ascontiguousarray(partition, dtype=np.int32)
    pos = np.zeros(len(partition), dtype=np.int32)
    counts = np.zeros(partition_count, dtype=np.int64)
    _check(lib().orc_partition_positions(partition.ctypes.data, len(partition), partition_count, pos.ctypes.data,
                                         counts.ctypes.data))
    return pos, counts


# ---- filter / project -------------------------------------------------------------------------
def filter_positions(page, filter_expr):
    """PageFilter.filter -> SelectedPositions: returns (is_list, positions ndarray | range count)."""
    cpage, keep = page.to_c()
    e, k2 = serialize(filter_expr)
    pos = np.zeros(max(page.position_count, 1), dtype=np.int32)
    count = C.c_int32()
    is_list = C.c_int32()
    _check(lib().orc_filter(C.byref(cpage), C.byref(e), pos.ctypes.data, C.byref(count), C.byref(is_list)))
    if is_list.value:
        return True, pos[:count.value].copy()
    return False, count.value


def filter_project(page, filter_expr, projections):
    """PageProcessor over one page -> Page or None."""
    cpage, keep = page.to_c()
    fe = None
    if filter_expr is not None:
        f, kf = serialize(filter_expr)
        fe = C.byref(f)
    arr, kp = serialize_many(projections)
    out = abi.pa_page()
    rc = _check(lib().orc_filter_project(C.byref(cpage), fe, len(projections), arr, C.byref(out)))
    if rc == 0:
        return None
    result = page_from_c(out)
    lib().orc_free_page(C.byref(out))
    return result


# ---- aggregation --------------------------------------------------------------------------------
def make_aggregates(aggregates):
    """aggregates: list of (fn, input_channel, input_type[, mask_channel])."""
    arr = (abi.pa_aggregate * max(len(aggregates), 1))()
    for i, a in enumerate(aggregates):
        arr[i].fn = a[0]
        arr[i].input_channel = a[1]
        arr[i].input_type = a[2] if a[2] is not None else 0
        arr[i].mask_channel = a[3] if len(a) > 3 else -1
    return arr


def make_hash_agg_desc(input_types, group_by_channels, aggregates, hash_channel=-1, expected_groups=10000,
                       step=abi.STEP_SINGLE, output_mem=abi.MEM_HOST, stream=None, global_aggregation_group_ids=None, group_id_channel=None,
                       produce_default_output=False):
    d = abi.pa_hash_aggregation_desc()
    keep = []
    types = abi.int32_array(input_types)
    gb = abi.int32_array(group_by_channels)
    aggs = make_aggregates(aggregates)
    d.input_channel_count = len(input_types)
    d.input_types = C.cast(types, C.POINTER(C.c_int32))
    d.group_by_count = len(group_by_channels)
    d.group_by_channels = C.cast(gb, C.POINTER(C.c_int32))
    d.hash_channel = hash_channel
    d.step = step
    d.aggregate_count = len(aggregates)
    d.aggregates = C.cast(aggs, C.POINTER(abi.pa_aggregate))
    d.expected_groups = expected_groups
    d.output_mem = output_mem
    d.stream = stream
    d.produce_default_output = 1 if produce_default_output else 0
    d.group_id_channel = -1 if group_id_channel is None else group_id_channel
    if global_aggregation_group_ids:
        ids = abi.int32_array(global_aggregation_group_ids)
        d.global_aggregation_group_id_count = len(global_aggregation_group_ids)
        d.global_aggregation_group_ids = C.cast(ids, C.POINTER(C.c_int32))
        keep.append(ids)
    keep += [types, gb, aggs]
    return d, keep


def page_builder_row_bytes(page):
    """Bytes every row of `page` adds to a PageBuilder's status (PageBuilderStatus via BlockBuilderStatus.addBytes): fixed-width
    builders add 1 (the null flag) + the value width per entry (LongArrayBlockBuilder.java / IntArrayBlockBuilder / ByteArrayBlockBuilder:
    `Byte.BYTES + Long.BYTES` ...), VariableWidthBlockBuilder 1 + 4 + the entry's bytes (entryAdded)."""
    n = page.position_count
    total = np.zeros(n, dtype=np.int64)
    for b in page.blocks:
        if b.encoding == abi.VARWIDTH:
            total += 5 + np.diff(np.asarray(b.offsets[:n + 1], dtype=np.int64))
        elif b.type == abi.LONG_DECIMAL:
            total += 17
        else:
            total += 1 + abi.TYPE_WIDTH[b.type]
    return total


class HashAggregationOperator:
    """HashAggregationOperator.java:348-543 as the Driver sees it (Operator.java:21-103), over this module's
    InMemoryHashAggregationBuilder restatement; no spill, no memory revocation.
      addInput   :380-439   inputProcessed = true; the builder takes the page
      finish     :366-370
      getOutput  :455-513   finishing && !inputProcessed && produceDefaultOutput -> getGlobalAggregationOutput (:545-587) and finished;
                            else buildResult once finishing -- a WorkProcessor of pages cut by the PageBuilder: rows are appended while
                            !pageBuilder.isFull() (InMemoryHashAggregationBuilder.java:283-298; PageBuilderStatus.DEFAULT_MAX_PAGE_SIZE_IN_BYTES
                            = 1 MB, PageBuilder.java:116-180)"""

    MAX_PAGE_BYTES = 1024 * 1024

    def __init__(self, input_types, group_by_channels, aggregates, hash_channel=-1, expected_groups=10000, step=abi.STEP_SINGLE,
                 global_aggregation_group_ids=None, group_id_channel=None, produce_default_output=False):
        self._args = (input_types, group_by_channels, aggregates, hash_channel, expected_groups, step)
        self._desc, self._keep = make_hash_agg_desc(input_types, group_by_channels, aggregates, hash_channel, expected_groups, step,
                                                    global_aggregation_group_ids=global_aggregation_group_ids, group_id_channel=group_id_channel,
                                                    produce_default_output=produce_default_output)
        self.produce_default_output = produce_default_output
        self.builder = None
        self.input_processed = False
        self.finishing = False
        self.finished = False
        self.output_pages = None

    def needsInput(self):
        return not self.finishing and self.output_pages is None

    def addInput(self, page):
        assert self.needsInput()
        self.input_processed = True
        if self.builder is None:
            self.builder = HashAggregation(*self._args)
        self.builder.add_page(page)

    def finish(self):
        self.finishing = True

    def isFinished(self):
        return self.finished

    def getOutput(self):
        if self.finished:
            return None
        if self.output_pages is None:
            if self.finishing:
                if not self.input_processed and self.produce_default_output:
                    self.finished = True
                    out = abi.pa_page()
                    _check(lib().orc_hash_agg_default_output(C.byref(self._desc), C.byref(out)))
                    if out.position_count == 0:
                        return None
                    page = page_from_c(out)
                    lib().orc_free_page(C.byref(out))
                    return page
                if self.builder is None:
                    self.finished = True
                    return None
            else:
                return None   # (Step.PARTIAL's early flush when the builder is full is HashAggregation's caller's business here)
            result = self.builder.build_result()
            # buildResult's pages: a row goes into the current page while the PageBuilder is not full
            sizes = page_builder_row_bytes(result)
            cuts, at, acc = [], 0, 0
            for i in range(result.position_count):
                if acc >= self.MAX_PAGE_BYTES:
                    cuts.append((at, i - at))
                    at, acc = i, 0
                acc += int(sizes[i])
            if result.position_count > at:
                cuts.append((at, result.position_count - at))
            self.output_pages = [result.get_region(o, n) for o, n in cuts]
        if not self.output_pages:
            self.builder.close()
            self.builder = None
            self.finished = True   # closeAggregationBuilder; with `finishing` the operator is done (:529-531)
            return None
        return self.output_pages.pop(0)


class HashAggregation:
    """InMemoryHashAggregationBuilder (+ GroupByHash) / AggregationOperator restatement."""

    def __init__(self, input_types, group_by_channels, aggregates, hash_channel=-1, expected_groups=10000,
                 step=abi.STEP_SINGLE):
        self._desc, self._keep = make_hash_agg_desc(input_types, group_by_channels, aggregates, hash_channel,
                                                    expected_groups, step)
        self._h = lib().orc_hash_agg_create(C.byref(self._desc))

    def add_page(self, page, want_group_ids=False):
        cpage, keep = page.to_c()
        gids = None
        ptr = None
        if want_group_ids:
            gids = np.zeros(max(page.position_count, 1), dtype=np.int32)
            ptr = gids.ctypes.data
        _check(lib().orc_hash_agg_add_page(self._h, C.byref(cpage), ptr))
        return gids[:page.position_count] if want_group_ids else None

    def group_count(self): return lib().orc_hash_agg_group_count(self._h)
    def capacity(self): return lib().orc_hash_agg_capacity(self._h)

    def contains(self, page, position):
        cpage, keep = page.to_c()
        return bool(lib().orc_hash_agg_contains(self._h, C.byref(cpage), position))

    def build_result(self):
        out = abi.pa_page()
        _check(lib().orc_hash_agg_build_result(self._h, C.byref(out)))
        result = page_from_c(out)
        lib().orc_free_page(C.byref(out))
        return result

    def close(self):
        if self._h:
            lib().orc_hash_agg_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


# ---- join -----------------------------------------------------------------------------------------
def make_hash_builder_desc(input_types, join_channels, output_channels, hash_channel=-1, expected_positions=0,
                           stream=None):
    d = abi.pa_hash_builder_desc()
    types = abi.int32_array(input_types)
    jc = abi.int32_array(join_channels)
    oc = abi.int32_array(output_channels)
    d.input_channel_count = len(input_types)
    d.input_types = C.cast(types, C.POINTER(C.c_int32))
    d.join_channel_count = len(join_channels)
    d.join_channels = C.cast(jc, C.POINTER(C.c_int32))
    d.hash_channel = hash_channel
    d.output_channel_count = len(output_channels)
    d.output_channels = C.cast(oc, C.POINTER(C.c_int32))
    d.expected_positions = expected_positions
    d.stream = stream
    return d, [types, jc, oc]


def make_lookup_join_desc(probe_types, probe_join_channels, probe_output_channels, probe_hash_channel=-1,
                          output_mem=abi.MEM_HOST, stream=None, join_type=abi.JOIN_INNER, output_single_match=False):
    d = abi.pa_lookup_join_desc()
    types = abi.int32_array(probe_types)
    jc = abi.int32_array(probe_join_channels)
    oc = abi.int32_array(probe_output_channels)
    d.probe_channel_count = len(probe_types)
    d.probe_types = C.cast(types, C.POINTER(C.c_int32))
    d.join_channel_count = len(probe_join_channels)
    d.probe_join_channels = C.cast(jc, C.POINTER(C.c_int32))
    d.probe_hash_channel = probe_hash_channel
    d.probe_output_channel_count = len(probe_output_channels)
    d.probe_output_channels = C.cast(oc, C.POINTER(C.c_int32))
    d.output_mem = output_mem
    d.stream = stream
    d.join_type = join_type
    d.output_single_match = 1 if output_single_match else 0
    return d, [types, jc, oc]


class HashJoin:
    """PagesIndex + PagesHash + ArrayPositionLinks + DefaultPageJoiner restatement (inner join)."""

    def __init__(self, build_types, join_channels, output_channels, hash_channel=-1):
        self._desc, self._keep = make_hash_builder_desc(build_types, join_channels, output_channels, hash_channel)
        self._h = lib().orc_join_create(C.byref(self._desc))

    def add_build_page(self, page):
        cpage, keep = page.to_c()
        _check(lib().orc_join_add_build_page(self._h, C.byref(cpage)))

    def build(self):
        _check(lib().orc_join_build(self._h))

    def tables(self):
        hs = C.c_int32()
        lib().orc_join_tables(self._h, C.byref(hs), None, None)
        key = np.zeros(hs.value, dtype=np.int32)
        links = np.zeros(max(lib().orc_join_build_positions(self._h), 1), dtype=np.int32)
        lib().orc_join_tables(self._h, C.byref(hs), key.ctypes.data, links.ctypes.data)
        return key, links[:lib().orc_join_build_positions(self._h)]

    def probe(self, page, probe_types, probe_join_channels, probe_output_channels, probe_hash_channel=-1, join_type=abi.JOIN_INNER,
              output_single_match=False):
        """Returns (output Page, probe indices, build positions) in the reference's emission order; build position -1 =
        the NULL-extended row of a probe-outer join."""
        d, keep = make_lookup_join_desc(probe_types, probe_join_channels, probe_output_channels, probe_hash_channel, join_type=join_type,
                                        output_single_match=output_single_match)
        cpage, k2 = page.to_c()
        out = abi.pa_page()
        pi = C.POINTER(C.c_int32)()
        bi = C.POINTER(C.c_int32)()
        cnt = C.c_int32()
        _check(lib().orc_join_probe(self._h, C.byref(d), C.byref(cpage), C.byref(out), C.byref(pi), C.byref(bi),
                                    C.byref(cnt)))
        n = cnt.value
        p = np.ctypeslib.as_array(pi, shape=(max(n, 1),))[:n].copy()
        b = np.ctypeslib.as_array(bi, shape=(max(n, 1),))[:n].copy()
        lib().orc_free(pi)
        lib().orc_free(bi)
        result = page_from_c(out)
        lib().orc_free_page(C.byref(out))
        return result, p, b

    def outer(self, probe_types, probe_output_channels):
        """LookupOuterOperator: the build rows no probe row was joined with (after LOOKUP_OUTER / FULL_OUTER probes)."""
        d, keep = make_lookup_join_desc(probe_types, [], probe_output_channels, join_type=abi.JOIN_LOOKUP_OUTER)
        out = abi.pa_page()
        _check(lib().orc_join_outer(self._h, C.byref(d), C.byref(out)))
        result = page_from_c(out)
        lib().orc_free_page(C.byref(out))
        return result

    def close(self):
        if self._h:
            lib().orc_join_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def join_with_filter(build_pages, build_types, join_channels, build_output_channels, probe_page, probe_types, probe_join_channels,
                     probe_output_channels, filter_expr, join_type=abi.JOIN_INNER, output_single_match=False):
    """LookupJoinOperator with a JoinFilterFunction, restated over this module's pieces: the candidates of every probe row are the
    positions of its chain in chain order (HashJoin.probe: PagesHash.getAddressIndex + ArrayPositionLinks); a candidate is joined
    when the filter -- an expression over [build page channels, probe page channels], JoinFilterFunctionCompiler's numbering --
    is TRUE for the pair (JoinHash.isJoinPositionEligible, JoinHash.java:116-120); DefaultPageJoiner.joinCurrentPosition
    (DefaultPageJoiner.java:266-292) stops at the first eligible position under outputSingleMatch, and a probe row that produced
    no row is emitted NULL-extended by a probe-outer join (outerJoinCurrentPosition, :296-303).
    Returns (output rows, [(probe position, build position or -1)], visited build positions)."""
    nb, npr = len(build_types), len(probe_types)
    j = HashJoin(build_types, join_channels, list(range(nb)))
    for p in build_pages:
        j.add_build_page(p)
    j.build()
    cand, pi, bi = j.probe(probe_page, probe_types, probe_join_channels, list(range(npr)))
    eligible = set()
    if cand.position_count:
        pairs = Page(cand.blocks[npr:] + cand.blocks[:npr], cand.position_count)   # [build channels, probe channels]
        is_list, sel = filter_positions(pairs, filter_expr)
        eligible = set(int(i) for i in sel) if is_list else set(range(int(sel)))
    cand_rows = cand.to_rows()
    by_row = {}
    for i, p in enumerate(pi):
        by_row.setdefault(int(p), []).append(i)
    probe_rows = probe_page.to_rows()
    rows, out_pairs, visited = [], [], set()
    outer = join_type in (abi.JOIN_PROBE_OUTER, abi.JOIN_FULL_OUTER)
    for r in range(probe_page.position_count):
        produced = False
        for i in by_row.get(r, []):
            if i not in eligible:
                continue
            produced = True
            c = cand_rows[i]
            rows.append(tuple(c[ch] for ch in probe_output_channels) + tuple(c[npr + ch] for ch in build_output_channels))
            out_pairs.append((r, int(bi[i])))
            visited.add(int(bi[i]))
            if output_single_match:
                break
        if not produced and outer:
            rows.append(tuple(probe_rows[r][ch] for ch in probe_output_channels) + (None,) * len(build_output_channels))
            out_pairs.append((r, -1))
    return rows, out_pairs, visited


# ---- synthetic TPC-H ---------------------------------------------------------------------------------
def tpch_column(column, scale_factor, first_row, row_count, seed=0x5EED0000):
    """Returns (values ndarray, offsets ndarray | None)."""
    t = abi.TPCH_COLUMN_TYPE[column]
    offsets = None
    if t == abi.VARCHAR:
        values = np.zeros(max(row_count * 10, 1), dtype=np.uint8)
        offsets = np.zeros(row_count + 1, dtype=np.int32)
    elif t in (abi.BIGINT,):
        values = np.zeros(row_count, dtype=np.int64)
    elif t == abi.DOUBLE:
        values = np.zeros(row_count, dtype=np.float64)
    else:
        values = np.zeros(row_count, dtype=np.int32)
    _check(lib().orc_tpch_generate(column, scale_factor, first_row, row_count, seed, values.ctypes.data,
                                   offsets.ctypes.data if offsets is not None else None))
    if offsets is not None:
        values = values[:max(int(offsets[-1]), 1)].copy()
    return values, offsets


def q6(shipdate, discount, quantity, extendedprice):
    s = C.c_double()
    c = C.c_int64()
    lib().orc_q6(shipdate.ctypes.data, discount.ctypes.data, quantity.ctypes.data, extendedprice.ctypes.data,
                 len(shipdate), C.byref(s), C.byref(c))
    return s.value, c.value


def q1(columns, chunks=1):
    """Hand-written Q1 pipeline twin over whole columns (returnflag bytes, rf offsets, linestatus bytes, ls offsets,
    quantity, extendedprice, discount, tax, shipdate); returns the result rows."""
    from presto_amd import tpch
    agg = HashAggregation([p.type for p in tpch.q1_projections()], tpch.Q1_GROUP_BY, tpch.Q1_AGGREGATES)
    n = len(columns[8])
    _check(lib().orc_q1_add(agg._h, *[c.ctypes.data for c in columns], n))
    return agg.build_result().to_rows()


# ---- MergePages ---------------------------------------------------------------------------------------------------
def q3(customer, orders, lineitem, top_n=0):
    """TPC-H Q3 as the composition of the oracle's operators (the plan of presto_amd/q3.py: customer -> filter -> HashBuilder;
    orders -> filter -> LookupJoin -> HashBuilder; lineitem -> filter / project -> LookupJoin -> HashAggregation(orderkey, orderdate,
    shippriority; sum(revenue), count(*)) [-> TopN(revenue DESC, orderdate ASC)]) over host pages: (rows, orders rows joined,
    lineitem rows joined).  The parity tests' checker and bench.py's q3.cpu_baseline."""
    from presto_amd import tpch
    from presto_amd.expr import field
    c = filter_project(customer, tpch.q3_customer_filter(), [field(0, abi.BIGINT)])
    j1 = HashJoin([abi.BIGINT], [0], [])
    if c is not None:
        j1.add_build_page(c)
    j1.build()
    o = filter_project(orders, tpch.q3_orders_filter(), [field(i, t) for i, t in enumerate(tpch.ORDERS_TYPES)])
    oc, _, _ = j1.probe(o, tpch.ORDERS_TYPES, [1], [0, 2, 3])
    j2 = HashJoin([abi.BIGINT, abi.DATE, abi.INTEGER], [0], [1, 2])
    j2.add_build_page(oc)
    j2.build()
    l = filter_project(lineitem, tpch.q3_lineitem_filter(), tpch.q3_lineitem_projections())
    joined, _, _ = j2.probe(l, [abi.BIGINT, abi.DOUBLE], [0], [0, 1])
    agg = HashAggregation([abi.BIGINT, abi.DOUBLE, abi.DATE, abi.INTEGER], [0, 2, 3], [(abi.AGG_SUM, 1, abi.DOUBLE), (abi.AGG_COUNT_STAR, -1, None)],
                          expected_groups=100000)
    agg.add_page(joined)
    grouped = agg.build_result()
    if top_n:
        # ORDER BY revenue DESC, o_orderdate LIMIT n: the C heap (TopNProcessor) over the grouped columns
        cols = [np.asarray(b.values) for b in grouped.blocks]   # BIGINT, DATE, INTEGER, DOUBLE, BIGINT: flat, no NULLs
        keep = topn_positions_double_desc_bigint_asc(cols[3], cols[1].astype(np.int64), top_n)
        return [tuple(c[i].item() for c in cols) for i in keep.tolist()], oc.position_count, joined.position_count
    return grouped.to_rows(), oc.position_count, joined.position_count


def block_size_in_bytes(block):
    """Block.getSizeInBytes of the flat block kinds: LongArrayBlock / IntArrayBlock / ByteArrayBlock
    (core/trino-spi/src/main/java/io/trino/spi/block/LongArrayBlock.java:55-57: (value width + 1) * positions) and
    VariableWidthBlock (VariableWidthBlock.java:66-68: bytes + (4 + 1) * positions)."""
    from presto_amd import abi
    n = block.position_count
    if block.type == abi.VARCHAR:
        off = block.offsets
        return int(off[n]) - int(off[0]) + 5 * n
    return (abi.TYPE_WIDTH[block.type] + 1) * n


def page_size_in_bytes(page):
    return sum(block_size_in_bytes(b) for b in page.blocks)


def concat_pages(pages):
    """PageBuilder contents after appendPage of every page (MergePages.java:155-164)."""
    import numpy as np
    from presto_amd import abi
    from presto_amd.page import Block, Page
    blocks = []
    for c in range(pages[0].channel_count):
        t = pages[0].blocks[c].type
        vals = [v for p in pages for v in p.blocks[c].to_pylist()]
        if t == abi.VARCHAR:
            blocks.append(Block.varchar(vals))
        else:
            blocks.append(Block.flat(t, [0 if v is None else v for v in vals], [v is None for v in vals]))
    return Page(blocks, sum(p.position_count for p in pages))


class MergePages:
    """MergePages.MergePagesTransformation (core/trino-main/src/main/java/io/trino/operator/project/MergePages.java:
    86-172) as a push-style state machine: process(page) / finish() return the pages that come out."""

    DEFAULT_MAX_PAGE_SIZE_IN_BYTES = 1024 * 1024  # PageBuilderStatus.java:18

    def __init__(self, min_page_size_in_bytes, min_row_count, max_page_size_in_bytes=0):
        self.min_bytes = min_page_size_in_bytes
        self.min_rows = min_row_count
        self.max_bytes = max_page_size_in_bytes or self.DEFAULT_MAX_PAGE_SIZE_IN_BYTES
        self.buffered = []
        self.buffered_bytes = 0

    def _flush(self):
        out = concat_pages(self.buffered)
        self.buffered, self.buffered_bytes = [], 0
        return out

    def process(self, page):
        out = []
        if page.position_count >= self.min_rows or page_size_in_bytes(page) >= self.min_bytes:  # :128
            if self.buffered:
                out.append(self._flush())  # :133-138: the buffered rows first, the big page on the next call
            out.append(page)
            return out
        self.buffered.append(page)  # :141
        self.buffered_bytes += page_size_in_bytes(page)
        if self.buffered_bytes >= self.max_bytes:  # :143 pageBuilder.isFull(), PageBuilderStatus.java:49-52
            out.append(self._flush())
        return out

    def finish(self):
        return [self._flush()] if self.buffered else []  # :117-124


# ---- TopN ---------------------------------------------------------------------------------------------------------
def topn(pages, n, sort_channels, sort_orders):
    """TopNOperator / TopNProcessor / GroupedTopNBuilder with one group (core/trino-main/src/main/java/io/trino/operator/
    TopNProcessor.java:35-110): the n first rows under SimplePageWithPositionComparator (…/SimplePageWithPositionComparator.java:
    45-70) with SortOrder.compareBlockValue (core/trino-spi/src/main/java/io/trino/spi/connector/SortOrder.java:58-84), as
    rows.  Fully tied rows keep arrival order here (the reference leaves it open).  Type orders: BIGINT / INTEGER / DATE
    numeric, DECIMAL / LONG_DECIMAL by unscaled value (one scale per channel), DOUBLE / REAL Double.compare (-0.0 < 0.0, NaN last),
    VARCHAR unsigned bytes (Slice.compareTo), BOOLEAN false < true."""
    import functools
    import math
    import struct
    from presto_amd import abi
    rows = [r for p in pages for r in p.to_rows()]
    types = [b.type for b in pages[0].blocks] if pages else []

    def value_cmp(t, a, b):
        if t in (abi.DOUBLE, abi.REAL):  # (RealType's comparison is Float.compare: the same order on the widened values)
            def image(d):
                bits = 0x7ff8000000000000 if math.isnan(d) else struct.unpack("<Q", struct.pack("<d", d))[0]
                return (~bits) & 0xFFFFFFFFFFFFFFFF if bits >> 63 else bits | 0x8000000000000000
            a, b = image(a), image(b)
        return -1 if a < b else (1 if a > b else 0)

    def cmp(x, y):
        for ch, order in zip(sort_channels, sort_orders):
            a, b = x[ch], y[ch]
            ascending, nulls_first = order < 2, (order & 1) == 0
            if a is None and b is None:
                c = 0
            elif a is None:
                c = -1 if nulls_first else 1
            elif b is None:
                c = 1 if nulls_first else -1
            else:
                c = value_cmp(types[ch], a, b)
                c = c if ascending else -c
            if c:
                return c
        return 0

    if n == 0:
        return []
    ordered = sorted(rows, key=functools.cmp_to_key(cmp))
    return ordered if n is None else ordered[:n]


def order_by(pages, output_channels, sort_channels, sort_orders):
    """OrderByOperator (core/trino-main/src/main/java/io/trino/operator/OrderByOperator.java:45-330): PagesIndex.sort with the same
    comparator as TopN (SimplePagesIndexComparator / SortOrder.compareBlockValue), every row kept; output channels only."""
    return [tuple(r[c] for c in output_channels) for r in topn(pages, None, sort_channels, sort_orders)]


def decimal_state_after(values, want_average=False):
    """LongDecimalWithOverflow(AndLong)State after inputLongDecimal of `values` (unscaled Python ints) in order:
    (overflow, unscaled value of the state's Slice -- its sign bit may be set on a zero magnitude: returned as (negative, magnitude)),
    and DecimalAverageAggregation.average at scale 0 when asked."""
    from presto_amd.page import long_decimal_value, long_decimal_words
    buf = np.zeros((max(len(values), 1), 2), dtype=np.uint64)
    for i, v in enumerate(values):
        buf[i, 0], buf[i, 1] = long_decimal_words(int(v))
    overflow = C.c_int64()
    state = np.zeros(2, dtype=np.uint64)
    avg = np.zeros(2, dtype=np.uint64)
    _check(lib().orc_decimal_state_after(buf.ctypes.data, len(values), C.byref(overflow), state.ctypes.data, avg.ctypes.data if want_average else None))
    negative = bool(int(state[1]) >> 63)
    magnitude = ((int(state[1]) & ((1 << 63) - 1)) << 64) | int(state[0])
    out = (overflow.value, negative, magnitude)
    return out + (long_decimal_value(avg[0], avg[1]),) if want_average else out


def sort_positions_bigint(keys):
    """PagesIndex.sort over row positions by one BIGINT key ascending (PagesIndexOrdering.quickSort restated in C): the
    positions in output order.  Not stable, like the reference's."""
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    pos = np.arange(len(keys), dtype=np.int32)
    _check(lib().orc_sort_positions_bigint(keys.ctypes.data, len(keys), pos.ctypes.data))
    return pos


def topn_positions_double_desc_bigint_asc(values, keys, limit):
    """TopNProcessor's bounded heap under (DOUBLE DESC, BIGINT ASC) in C: positions of the kept rows, best first."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    out = np.zeros(max(limit, 1), dtype=np.int32)
    n = _check(lib().orc_topn_double_desc_bigint_asc(values.ctypes.data, keys.ctypes.data, len(values), limit, out.ctypes.data))
    return out[:n]


# ---- dynamic filter source -----------------------------------------------------------------------------------------
class DynamicFilterSource:
    """DynamicFilterSourceOperator (core/trino-main/src/main/java/io/trino/operator/DynamicFilterSourceOperator.java:164-418)
    as a row-at-a-time restatement: TypedSet per channel -> min / max of the orderable non-floating channels -> give up.
    `predicate` is what dynamicPredicateConsumer received (None while not called): "all", or one entry per channel:
    ("all",) | ("none",) | ("values", ascending list) | ("range", low, high).  As in the device operator the size of a
    value set is its values' bytes (VARCHAR: 8-byte padded + 4 B offsets); the reference's figure
    (TypedSet.getRetainedSizeInBytes) depends on the JVM's object layout and has no portable restatement."""

    def __init__(self, input_types, filter_channels, max_distinct_values, max_filter_size_bytes, min_max_collection_limit):
        self.types = [input_types[c] for c in filter_channels]
        self.channels = list(filter_channels)
        self.max_distinct, self.max_bytes, self.limit = max_distinct_values, max_filter_size_bytes, min_max_collection_limit
        # :183-203
        # ("Skipping DOUBLE and REAL in collectMinMaxValues to avoid dealing with NaN values", :187-188)
        self.min_max_channels = [i for i, t in enumerate(self.types) if min_max_collection_limit > 0 and t not in (abi.DOUBLE, abi.REAL)]
        self.sets = [dict() for _ in self.types]  # canonical key -> first seen value (TypedSet keeps the first of equal values)
        self.has_null = [False] * len(self.types)
        self.min = [None] * len(self.types) if self.min_max_channels else None
        self.max = [None] * len(self.types)
        self.predicate = None
        self.finished = False

    @staticmethod
    def _key(t, v):
        if t in (abi.DOUBLE, abi.REAL):  # IS DISTINCT FROM: NaN equals NaN, -0.0 equals 0.0
            return "nan" if v != v else (0.0 if v == 0.0 else v)
        return v

    def _update_min_max(self, i, values):  # updateMinMaxValues :303-347 (comparison operator of the type)
        vals = [v for v in values if v is not None]
        if not vals:
            return
        lo, hi = min(vals), max(vals)
        self.min[i] = lo if self.min[i] is None else min(self.min[i], lo)
        self.max[i] = hi if self.max[i] is None else max(self.max[i], hi)

    def add_page(self, page):  # addInput :225-267; the page itself passes through
        assert not self.finished
        cols = [page.blocks[c].to_pylist() for c in self.channels]
        if self.sets is None:
            if self.min is None:
                return page
            self.limit -= page.position_count
            if self.limit < 0:
                self.predicate, self.min = "all", None  # handleMinMaxCollectionLimitExceeded
                return page
            for i in self.min_max_channels:
                self._update_min_max(i, cols[i])
            return page
        self.limit -= page.position_count
        size_bytes, most = 0, 0
        for i, (t, col) in enumerate(zip(self.types, cols)):
            for v in col:
                if v is None:
                    self.has_null[i] = True
                else:
                    self.sets[i].setdefault(self._key(t, v), v)
            n = len(self.sets[i])
            if t == abi.VARCHAR:
                size_bytes += sum(-(-len(v) // 8) * 8 for v in self.sets[i]) + 4 * n
            else:
                size_bytes += n * {abi.BIGINT: 8, abi.DOUBLE: 8, abi.INTEGER: 4, abi.DATE: 4, abi.BOOLEAN: 1, abi.REAL: 4}[t]
            most = max(most, n + (1 if self.has_null[i] else 0))
        if most > self.max_distinct or size_bytes > self.max_bytes:  # handleTooLargePredicate :268-292
            if not self.min_max_channels:
                self.predicate = "all"
            elif self.limit < 0:
                self.predicate, self.min = "all", None
            else:
                for i in self.min_max_channels:
                    self._update_min_max(i, list(self.sets[i].values()))
            self.sets = None
        return page

    def finish(self):  # :358-401
        if self.finished:
            return
        self.finished = True
        if self.sets is None:
            if self.min is None:
                return
            out = [("all",)] * len(self.types)
            for i in self.min_max_channels:
                out[i] = ("none",) if self.min[i] is None else ("range", self.min[i], self.max[i])
            self.predicate = out
            return
        out = []
        for t, values in zip(self.types, self.sets):  # convertToDomain :403-418: no NULL, no NaN
            vals = [v for k, v in values.items() if k != "nan"]
            if t in (abi.DOUBLE, abi.REAL):
                vals = [0.0 if v == 0.0 else v for v in vals]  # the device keeps +0.0 for the {-0.0, 0.0} element (DESIGN)
            out.append(("values", sorted(vals)) if vals else ("none",))
        self.predicate = out


# ---- page wire format -------------------------------------------------------------------------------------------------
_ENCODING = {abi.BIGINT: (b"LONG_ARRAY", "<i8"), abi.DOUBLE: (b"LONG_ARRAY", "<f8"), abi.INTEGER: (b"INT_ARRAY", "<i4"), abi.DATE: (b"INT_ARRAY", "<i4"),
             abi.BOOLEAN: (b"BYTE_ARRAY", "u1"), abi.VARCHAR: (b"VARIABLE_WIDTH", None),
             abi.REAL: (b"INT_ARRAY", "<f4")}   # RealType: floatToRawIntBits in an IntArrayBlock


def serialize_page(page):
    """PagesSerde.serialize without compression / encryption / checksum: the SerializedPage frame of
    PagesSerdeUtil.writeSerializedPage (core/trino-main/src/main/java/io/trino/execution/buffer/PagesSerdeUtil.java:66-74)
    around writeRawPage (:45-52); per block the length-prefixed encoding name (InternalBlockEncodingSerde.java:56-80) and
    LongArrayBlockEncoding.writeBlock (core/trino-spi/.../block/LongArrayBlockEncoding.java:38-61; Int / Byte alike),
    VariableWidthBlockEncoding.writeBlock (:37-58), EncoderUtil.encodeNullsAsBits (:35-72).  Little endian (Slice)."""
    import struct
    n = page.position_count
    payload = bytearray(struct.pack("<i", page.channel_count))
    for b in page.blocks:
        name, dtype = _ENCODING[b.type]
        payload += struct.pack("<i", len(name)) + name + struct.pack("<i", n)
        nulls = None if b.nulls is None else np.asarray(b.nulls[:n], dtype=np.uint8)

        def null_bits():
            out = bytearray([0 if nulls is None else 1])
            if nulls is not None:
                out += np.packbits(nulls != 0, bitorder="big").tobytes()
            return out
        if b.type == abi.VARCHAR:
            off = np.asarray(b.offsets[:n + 1], dtype=np.int64)
            payload += (off[1:] - off[0]).astype("<i4").tobytes()
            payload += null_bits()
            total = int(off[n] - off[0])
            payload += struct.pack("<i", total) + np.asarray(b.values, dtype=np.uint8)[int(off[0]):int(off[0]) + total].tobytes()
            continue
        payload += null_bits()
        values = np.asarray(b.values[:n]).astype(dtype)
        if nulls is None:
            payload += values.tobytes()
        else:
            keep = values[nulls == 0]
            payload += struct.pack("<i", len(keep)) + keep.tobytes()
    return struct.pack("<ibii", n, 0, len(payload), len(payload)) + bytes(payload)


def deserialize_page(data):
    """PagesSerde.deserialize of serialize_page's form -> host Page (LONG_ARRAY -> BIGINT, INT_ARRAY -> INTEGER, BYTE_ARRAY ->
    BOOLEAN blocks: LongArrayBlockEncoding.readBlock :63-95 leaves 0 at NULL positions)."""
    import struct
    from presto_amd.page import Block, Page
    n, markers, uncompressed, size = struct.unpack_from("<ibii", data, 0)
    assert markers == 0 and uncompressed == size
    pos = 13
    (channels,) = struct.unpack_from("<i", data, pos)
    pos += 4
    blocks = []
    for _ in range(channels):
        (ln,) = struct.unpack_from("<i", data, pos)
        name = data[pos + 4:pos + 4 + ln]
        pos += 4 + ln
        (count,) = struct.unpack_from("<i", data, pos)
        pos += 4
        assert count == n
        ends = None
        if name == b"VARIABLE_WIDTH":
            ends = np.frombuffer(data, dtype="<i4", count=n, offset=pos)
            pos += 4 * n
        has_null = data[pos] != 0
        pos += 1
        nulls = None
        if has_null:
            nb = (n + 7) // 8
            nulls = np.unpackbits(np.frombuffer(data, dtype=np.uint8, count=nb, offset=pos), bitorder="big")[:n].astype(np.uint8)
            pos += nb
        if name == b"VARIABLE_WIDTH":
            (total,) = struct.unpack_from("<i", data, pos)
            pos += 4
            raw = np.frombuffer(data, dtype=np.uint8, count=total, offset=pos).copy() if total else np.zeros(1, np.uint8)
            pos += total
            blocks.append(Block(abi.VARCHAR, abi.VARWIDTH, n, values=raw, offsets=np.concatenate([[0], ends]).astype(np.int32), nulls=nulls))
            continue
        t, dtype = {b"LONG_ARRAY": (abi.BIGINT, "<i8"), b"INT_ARRAY": (abi.INTEGER, "<i4"), b"BYTE_ARRAY": (abi.BOOLEAN, "u1")}[name]
        width = np.dtype(dtype).itemsize
        if not has_null:
            values = np.frombuffer(data, dtype=dtype, count=n, offset=pos).copy()
            pos += n * width
        else:
            (nn,) = struct.unpack_from("<i", data, pos)
            pos += 4
            values = np.zeros(n, dtype=dtype)
            values[nulls == 0] = np.frombuffer(data, dtype=dtype, count=nn, offset=pos)
            pos += nn * width
        blocks.append(Block(t, abi.FLAT, n, values=values, nulls=nulls))
    assert pos == len(data)
    return Page(blocks, n)


# ---- intermediate states in the reference's serialized form -----------------------------------------------------------------
# The C restatement keeps Step.PARTIAL / FINAL states as plain channels ([count] / [count, value], presto_amd.h).  The
# reference serialises ONE block per aggregate, typed by the aggregate's AccumulatorStateSerializer
# (core/trino-main/src/main/java/io/trino/operator/aggregation/state/StateCompiler.java:127-185; fields of a generated
# serializer sorted by name, :586-625):
#   count            LongState                               -> BIGINT
#   sum(DOUBLE)      LongDoubleState + TwoNullableValueState -> ROW(first BIGINT, firstNull BOOLEAN, second DOUBLE, secondNull BOOLEAN)
#   sum(BIGINT)      LongLongState + TwoNullableValueState   -> ROW(first BIGINT, firstNull BOOLEAN, second BIGINT, secondNull BOOLEAN)
#                    (…/aggregation/DoubleSumAggregation.java:33-63 / LongSumAggregation.java:34-64 never set the two null
#                    flags: they keep TwoNullableValueState's initial value true, minmaxby/TwoNullableValueState.java)
#   avg              LongAndDoubleState                      -> ROW(double DOUBLE, long BIGINT)   (…/state/LongAndDoubleState.java)
#   min / max        NullableLongState / NullableDoubleState / NullableBooleanState with their own serializers
#                    (…/state/NullableLongStateSerializer.java: BIGINT, NULL when state.isNull()) -- a long for INTEGER / DATE too
def states_to_reference(page, leading, aggregates):
    """Flat PARTIAL output page -> the reference's form.  aggregates: (fn, input channel, input type[, mask])."""
    blocks = list(page.blocks[:leading])
    n = page.position_count
    at = leading
    for a in aggregates:
        fn, in_type = a[0], a[2]
        cnt = page.blocks[at]
        if fn in (abi.AGG_COUNT, abi.AGG_COUNT_STAR):
            blocks.append(cnt)
            at += 1
            continue
        val = page.blocks[at + 1]
        at += 2
        true = Block.boolean(np.ones(n, dtype=np.uint8))
        if fn == abi.AGG_SUM:
            blocks.append(Block.row([Block.bigint(cnt.values), true, Block.flat(val.type, val.values), true]))
        elif fn == abi.AGG_AVG:
            blocks.append(Block.row([Block.double(val.values), Block.bigint(cnt.values)]))
        else:
            if in_type in (abi.INTEGER, abi.DATE):
                val = Block.flat(abi.BIGINT, np.asarray(val.values).astype(np.int64), val.nulls)
            blocks.append(val)
    return Page(blocks, n)


def states_from_reference(page, leading, aggregates):
    """The reverse: the reference's form -> the flat channels a Step.FINAL restatement takes."""
    blocks = list(page.blocks[:leading])
    n = page.position_count
    for k, a in enumerate(aggregates):
        fn, in_type = a[0], a[2]
        b = page.blocks[leading + k]
        if fn in (abi.AGG_COUNT, abi.AGG_COUNT_STAR):
            blocks.append(b)
        elif fn == abi.AGG_SUM:
            blocks += [b.fields[0], b.fields[2]]
        elif fn == abi.AGG_AVG:
            blocks += [b.fields[1], b.fields[0]]
        else:
            nulls = np.zeros(n, dtype=np.uint8) if b.nulls is None else np.asarray(b.nulls)
            blocks.append(Block.bigint((nulls == 0).astype(np.int64)))
            if in_type in (abi.INTEGER, abi.DATE):
                b = Block.flat(in_type, np.asarray(b.values).astype(np.int32), b.nulls)
            blocks.append(b)
    return Page(blocks, n)


# ---- LZ4 block format (PagesSerde's compressor: io.airlift:aircompressor Lz4Compressor / Lz4Decompressor, un-vendored) ------
# Restated from the public LZ4 block-format description, independently of presto_amd/csrc/page_serde.cpp; pure Python, for
# test-sized inputs.  A block is a run of sequences: token (literal length << 4 | match length - 4), literal-length extension
# bytes (255 ... < 255) when the nibble is 15, the literals, a 2-byte little-endian match offset, match-length extension bytes
# when the nibble is 15; the last sequence stops after its literals.
def lz4_decompress(data, uncompressed_size):
    data = bytes(data)
    out = bytearray()
    i = 0
    while i < len(data):
        token = data[i]
        i += 1
        lit = token >> 4
        if lit == 15:
            while True:
                b = data[i]
                i += 1
                lit += b
                if b != 255:
                    break
        out += data[i:i + lit]
        i += lit
        if i >= len(data):
            break
        offset = data[i] | (data[i + 1] << 8)
        i += 2
        assert 0 < offset <= len(out), "bad match offset"
        ml = token & 15
        if ml == 15:
            while True:
                b = data[i]
                i += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        for _ in range(ml):   # overlapping copy: byte by byte
            out.append(out[-offset])
    assert len(out) == uncompressed_size, (len(out), uncompressed_size)
    return bytes(out)


def lz4_compress(data):
    """A greedy encoder of the same format (another encoder than the library's: the decoder must not depend on whose output it reads)."""
    data = bytes(data)
    n = len(data)
    out = bytearray()

    def emit(lit, match_len, offset):
        token_at = len(out)
        out.append(0)
        ll = len(lit)
        if ll >= 15:
            out[token_at] = 15 << 4
            rest = ll - 15
            while rest >= 255:
                out.append(255)
                rest -= 255
            out.append(rest)
        else:
            out[token_at] = ll << 4
        out.extend(lit)
        if match_len == 0:
            return
        out.append(offset & 255)
        out.append(offset >> 8)
        m = match_len - 4
        if m >= 15:
            out[token_at] |= 15
            rest = m - 15
            while rest >= 255:
                out.append(255)
                rest -= 255
            out.append(rest)
        else:
            out[token_at] |= m

    anchor = i = 0
    last = {}
    while n >= 13 and i < n - 12:
        key = data[i:i + 4]
        cand = last.get(key)
        last[key] = i
        if cand is None or i - cand > 65535:
            i += 1
            continue
        j = i + 4
        while j < n - 5 and data[j] == data[cand + (j - i)]:
            j += 1
        emit(data[anchor:i], j - i, i - cand)
        i = anchor = j
    emit(data[anchor:], 0, 0)
    return bytes(out)


def compress_frame(frame):
    """An uncompressed SerializedPage frame -> the COMPRESSED one a Java worker with a compressor would send (if it pays)."""
    import struct
    positions, markers, uncompressed, size = struct.unpack_from("<ibii", frame, 0)
    assert markers == 0 and uncompressed == size
    packed = lz4_compress(frame[13:])
    if len(packed) / max(uncompressed, 1) > 0.8:   # PagesSerde.java:84 MINIMUM_COMPRESSION_RATIO
        return frame
    return struct.pack("<ibii", positions, 1, uncompressed, len(packed)) + packed
