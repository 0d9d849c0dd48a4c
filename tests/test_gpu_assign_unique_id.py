"""GPU checks of AssignUniqueIdOperator against tests/unique_id_model.py (AssignUniqueIdOperator.java:115-162 restated): the ids across
the end of a block in the middle of a page, two operators on one pool, the stage / task bits, the 2^40 limit, the pass-through of the
input page (zero copy for device pages, encodings included) and retained pages.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from presto_amd import abi
from presto_amd._lib import check, lib
from presto_amd.operators import AssignUniqueIdOperator, AssignUniqueIdOperatorFactory, UniqueIdPool, download, download_page, upload_page
from presto_amd.page import Block, DeviceBuffer, Page
from tests import unique_id_model as U
from tests.test_gpu_row_number import host_page_of, raw_output

pytestmark = pytest.mark.gpu
BLOCK = 1 << 20


def ids_of(out):
    """The id column of a C output page: BIGINT, flat, no nulls, behind the input's channels."""
    n = out.position_count
    col = out.columns[out.channel_count - 1]
    assert col.type == abi.BIGINT and col.encoding == abi.FLAT and not col.nulls
    if out.mem == abi.MEM_DEVICE:
        return download(DeviceBuffer(col.values, 8 * n), np.int64, n)
    return np.frombuffer(C.string_at(col.values, 8 * n), np.int64).copy() if n else np.zeros(0, np.int64)


def payload_page(lo, n, device):
    page = Page([Block.bigint(np.arange(lo, lo + n, dtype=np.int64))], n)
    return upload_page(page) if device else page


def feed(op, page):
    assert op.needsInput()
    op.addInput(page)
    assert not op.needsInput()          # a page is pending
    out = raw_output(op)
    assert out is not None and out.position_count == page.position_count
    ids = ids_of(out)
    payload = host_page_of(op, out).blocks[0].values[:out.position_count].copy()
    assert op.needsInput() and not op.isFinished()
    return ids, payload


def model_ids(assigner, n):
    """the model walks row by row; the expected ids of a long page by block, which is the same thing (pinned in the CPU tests)"""
    out = np.empty(n, np.int64)
    at = 0
    while at < n:
        if assigner.counter >= assigner.max:
            assigner.request_values()
        take = min(n - at, assigner.max - assigner.counter)
        out[at:at + take] = assigner.mask | (assigner.counter + np.arange(take, dtype=np.int64))
        assigner.counter += take
        at += take
    return out


def test_model_ids_by_block_is_the_model():
    a, b = U.Assigner(U.Pool(BLOCK - 3), 1, 2), U.Assigner(U.Pool(BLOCK - 3), 1, 2)
    for n in (2, BLOCK, 5):
        assert model_ids(a, n).tolist() == b.ids(n)


@pytest.mark.parametrize("device", [False, True])
def test_block_end_in_the_middle_of_a_page(gpu, device):
    """The pool starts at 2^20 - 3 and a second operator sits on the block behind the first one's: where the first operator's block
    ends -- inside its second page -- its ids jump over the other's block."""
    mem = abi.MEM_DEVICE if device else abi.MEM_HOST
    factory = AssignUniqueIdOperatorFactory([abi.BIGINT], pool=UniqueIdPool(BLOCK - 3), output_mem=mem)
    mpool = U.Pool(BLOCK - 3)
    a, ma = factory.createOperator(), U.Assigner(mpool)
    b, mb = factory.createOperator(), U.Assigner(mpool)
    at = 0
    seen = []
    # 1000 rows, then a page that crosses the end of a's block at an odd row, then pages of one row and of a few around a tile of 1024
    for op, model, n in ((a, ma, 1000), (b, mb, 7), (a, ma, BLOCK - 1000 + 1025), (a, ma, 1), (b, mb, 1023), (a, ma, 1025)):
        ids, payload = feed(op, payload_page(at, n, device))
        want = model_ids(model, n)
        assert np.array_equal(ids, want), (n, ids[:4], want[:4])
        assert np.array_equal(payload, np.arange(at, at + n))
        seen.append(ids)
        at += n
    everything = np.concatenate(seen)
    assert len(np.unique(everything)) == len(everything)
    third = seen[2]
    assert third[BLOCK - 1000 - 1] == 2 * BLOCK - 4 and third[BLOCK - 1000] == 3 * BLOCK - 3       # over b's block
    for op in (a, b):
        op.finish()
        assert op.isFinished()
        op.close()


def test_several_block_ends_in_one_page(gpu):
    """a page longer than eight blocks: more segments than one launch of the id kernel takes"""
    n = 9 * BLOCK + 17
    pool, mpool = UniqueIdPool(BLOCK - 5), U.Pool(BLOCK - 5)
    op, model = AssignUniqueIdOperator([abi.BOOLEAN], pool=pool, output_mem=abi.MEM_DEVICE), U.Assigner(mpool)
    other, mother = AssignUniqueIdOperator([abi.BOOLEAN], pool=pool, output_mem=abi.MEM_DEVICE), U.Assigner(mpool)
    op.addInput(upload_page(Page([Block.flat(abi.BOOLEAN, np.zeros(n, np.uint8))], n)))
    ids = ids_of(raw_output(op))
    want = model_ids(model, n)
    assert np.array_equal(ids, want)
    assert ids[0] == BLOCK - 5 and ids[BLOCK] == 3 * BLOCK - 5          # the second block went to `other`
    other.addInput(upload_page(Page([Block.flat(abi.BOOLEAN, np.zeros(3, np.uint8))], 3)))
    assert np.array_equal(ids_of(raw_output(other)), model_ids(mother, 3))
    op.close()
    other.close()


def test_two_operators_on_one_pool_never_overlap(gpu):
    factory = AssignUniqueIdOperatorFactory([abi.BIGINT], stage_id=1, task_id=1, output_mem=abi.MEM_DEVICE)
    ops = [factory.createOperator() for _ in range(3)]
    rng = np.random.default_rng(7)
    seen = []
    for step in range(12):
        op = ops[int(rng.integers(0, 3))]
        n = int(rng.choice([1, 5, 1024, BLOCK // 2 + 3]))
        ids, _ = feed(op, payload_page(0, n, True))
        assert np.all(np.diff(ids) > 0)
        seen.append(ids)
    everything = np.concatenate(seen)
    assert len(np.unique(everything)) == len(everything)
    assert np.all(everything >> 40 == (1 << 14) | 1)
    for op in ops:
        op.close()


@pytest.mark.parametrize("stage,task", [(0, 0), (1, 0), (0, 1), (5, 9), ((1 << 9) - 1, (1 << 14) - 1), (3, (1 << 23) - 1)])
def test_stage_and_task_bits(gpu, stage, task):
    op = AssignUniqueIdOperator([abi.BIGINT], stage_id=stage, task_id=task, pool=UniqueIdPool(BLOCK - 2))
    ids, _ = feed(op, payload_page(0, 4, False))
    rows = np.array([BLOCK - 2, BLOCK - 1, BLOCK, BLOCK + 1], dtype=np.int64)
    mask = (stage << 54) | (task << 40)
    assert mask < (1 << 63)
    assert ids.tolist() == [mask | int(r) for r in rows]
    assert ids.tolist() == U.Assigner(U.Pool(BLOCK - 2), stage, task).ids(4)
    assert np.all(ids >= 0) and np.all((ids & ((1 << 40) - 1)) == rows)
    op.close()


def test_the_limit(gpu):
    L = lib()
    # the last block there is: 2^20 rows go through, the next row asks for a block at 2^40
    op = AssignUniqueIdOperator([abi.BIGINT], pool=UniqueIdPool((1 << 40) - BLOCK), output_mem=abi.MEM_DEVICE)
    ids, _ = feed(op, payload_page(0, BLOCK, True))
    assert ids[0] == (1 << 40) - BLOCK and ids[-1] == (1 << 40) - 1
    one = payload_page(0, 1, True)
    assert L.pa_op_add_input(op._h, C.byref(one.to_c()[0])) == abi.ERR_ILLEGAL_STATE
    assert b"Unique row id exceeds a limit" in L.pa_last_error()
    assert op.getOutput() is None
    op.finish()
    op.close()
    # a block that begins below the limit is capped at it: the limit is reached in the middle of a page
    op = AssignUniqueIdOperator([abi.BIGINT], pool=UniqueIdPool((1 << 40) - 5))
    ids, _ = feed(op, payload_page(0, 5, False))
    assert ids.tolist() == list(range((1 << 40) - 5, 1 << 40))
    three = payload_page(0, 3, False)
    assert L.pa_op_add_input(op._h, C.byref(three.to_c()[0])) == abi.ERR_ILLEGAL_STATE
    op.close()
    # a pool that starts at the limit: no operator
    from presto_amd.operators import assign_unique_id_desc
    pool = UniqueIdPool(1 << 40)
    d, keep = assign_unique_id_desc([abi.BIGINT])
    h = C.c_void_p()
    assert L.pa_assign_unique_id_create(C.byref(d), pool._h, C.byref(h)) == abi.ERR_ILLEGAL_STATE
    assert b"Unique row id exceeds a limit" in L.pa_last_error()


def test_pool_and_operators_go_in_any_order(gpu):
    pool = UniqueIdPool()
    op = AssignUniqueIdOperator([abi.BIGINT], pool=pool)
    pool.destroy()
    ids, _ = feed(op, payload_page(0, BLOCK + 2, False))            # the next block comes out of the counter the operator shares
    assert ids.tolist() == list(range(BLOCK + 2))
    op.close()


def test_pass_through_channels_are_the_input(gpu):
    names = Block.varchar(["a", None, "ccc", "a"])
    dic = Block.dictionary_block(Block.varchar(["x", "yy"]), [1, 0, 0, 1])
    rle = Block.rle(Block.bigint([4]), 4)
    types = [abi.VARCHAR, abi.BIGINT, abi.VARCHAR, abi.DOUBLE, abi.BIGINT]
    host = Page([names, Block.flat(abi.BIGINT, [1, 5, 0, 1], [0, 0, 1, 0]), dic, Block.double([0.5, -1.0, 2.0, 3.0]), rle], 4)
    for output_mem in (abi.MEM_HOST, abi.MEM_DEVICE):       # host in -> host out / device out
        op = AssignUniqueIdOperator(types, output_mem=output_mem)
        op.addInput(host)
        out = op.getOutput()
        assert out.mem == output_mem
        if out.mem == abi.MEM_DEVICE:
            out = download_page(out)
        assert [r[:-1] for r in out.to_rows()] == host.to_rows()
        assert [r[-1] for r in out.to_rows()] == [0, 1, 2, 3]
        op.close()

    # device -> device: the input blocks themselves, dictionary and RLE encodings included; only the id column is new
    dev = upload_page(host)
    op = AssignUniqueIdOperator(types, output_mem=abi.MEM_DEVICE)
    cpage, _keep = dev.to_c()
    check(lib().pa_op_add_input(op._h, C.byref(cpage)))
    out = abi.pa_page()
    assert check(lib().pa_op_get_output(op._h, C.byref(out))) == 1
    assert out.channel_count == 6 and out.position_count == 4 and out.mem == abi.MEM_DEVICE
    for c in range(5):
        assert out.columns[c].encoding == cpage.columns[c].encoding
        assert out.columns[c].values == cpage.columns[c].values
        assert out.columns[c].offsets == cpage.columns[c].offsets
        assert out.columns[c].nulls == cpage.columns[c].nulls
        assert out.columns[c].ids == cpage.columns[c].ids
    assert out.columns[2].encoding == abi.DICTIONARY and out.columns[4].encoding == abi.RLE
    assert out.columns[2].dictionary[0].values == cpage.columns[2].dictionary[0].values
    assert out.columns[4].dictionary[0].values == cpage.columns[4].dictionary[0].values
    assert ids_of(out).tolist() == [0, 1, 2, 3]
    op.close()


def test_retained_pages_are_released_exactly_once(gpu):
    """A PA_PAGE_RETAINED page is released once its output page has been let go -- not before (the zero-copy output page IS the input's
    blocks: the release callback scribbles over them) -- and exactly once, also when the operator is closed over a pending output."""
    from tests.test_gpu_small_pages import retained_pages
    n = 5000
    host = Page([Block.bigint(np.arange(n, dtype=np.int64) * 3), Block.double(np.arange(n, dtype=np.float64))], n)
    bounds = [0, 700, 701, 2000, n]
    released = []
    pages = retained_pages(host, bounds, released)
    op = AssignUniqueIdOperator([abi.BIGINT, abi.DOUBLE], output_mem=abi.MEM_DEVICE)
    for i, p in enumerate(pages):
        lo, hi = bounds[i], bounds[i + 1]
        assert op.needsInput()
        op.addInput(p)
        assert released == list(range(i))                                # page i is still held
        out = raw_output(op)
        assert out is not None and out.mem == abi.MEM_DEVICE and out.position_count == hi - lo and out.channel_count == 3
        got = host_page_of(op, out)                                      # reads the caller's blocks: they must still be intact
        assert np.array_equal(got.blocks[0].values[:hi - lo], np.arange(lo, hi) * 3)
        assert np.array_equal(got.blocks[1].values[:hi - lo], np.arange(lo, hi, dtype=np.float64))
        assert np.array_equal(got.blocks[2].values[:hi - lo], np.arange(lo, hi))
        assert released == list(range(i))                                # ... while its output page is out
        op.needsInput()                                                  # the output page has been let go
        assert released == list(range(i + 1))
    op.finish()
    op.close()
    assert released == list(range(len(pages)))

    # closed while an output page is still pending: the page goes back once, at close
    released = []
    pages = retained_pages(host, bounds, released)
    op = AssignUniqueIdOperator([abi.BIGINT, abi.DOUBLE], output_mem=abi.MEM_DEVICE)
    op.addInput(pages[0])
    assert not op.needsInput() and released == []
    op.close()
    assert released == [0]
    del op
    assert released == [0]

    # a page that fails at the limit is let go all the same, once
    released = []
    pages = retained_pages(host, bounds, released)
    op = AssignUniqueIdOperator([abi.BIGINT, abi.DOUBLE], pool=UniqueIdPool((1 << 40) - 3), output_mem=abi.MEM_DEVICE)
    with pytest.raises(Exception):
        op.addInput(pages[0])
    op.close()
    assert released == [0]


def test_empty_pages_and_protocol(gpu):
    op = AssignUniqueIdOperator([abi.BIGINT])
    empty = Page([Block.bigint([])], 0)
    check(lib().pa_op_add_input(op._h, C.byref(empty.to_c()[0])))
    assert op.getOutput() is None and op.needsInput()
    page = Page([Block.bigint([1, 1])], 2)
    op.addInput(page)
    assert lib().pa_op_add_input(op._h, C.byref(page.to_c()[0])) == abi.ERR_ILLEGAL_STATE      # a page is pending
    wrong = Page([Block.bigint([1]), Block.bigint([1])], 1)
    op.finish()
    assert not op.isFinished()                                                                # finishing, but a page is pending
    assert ids_of(raw_output(op)).tolist() == [0, 1]                                          # the empty page took no id
    assert op.isFinished() and not op.needsInput()
    assert lib().pa_op_add_input(op._h, C.byref(page.to_c()[0])) == abi.ERR_ILLEGAL_STATE
    assert op.kernelName() == "k_unique_ids"
    ms, launches = op.kernelTime()
    assert launches == 1 and ms > 0
    op.close()
    op = AssignUniqueIdOperator([abi.BIGINT])
    assert lib().pa_op_add_input(op._h, C.byref(wrong.to_c()[0])) == abi.ERR_INVALID_ARGUMENT   # two channels into one
    op.close()
