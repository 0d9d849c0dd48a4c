// C++ driver test of WindowOperator with frames through include/presto_amd.hpp (the C++ host mirror), on the GPU:
//   wf-1  rank(), sum(x) with the default frame (RANGE .. CURRENT ROW), sum(x) ROWS .. CURRENT ROW, min(x) over the whole partition and
//         count(x) ROWS OVER (PARTITION BY a VARCHAR ORDER BY a DOUBLE) over three pages, x a BIGINT with NULLs: peers share the RANGE
//         sum and not the ROWS sum, a frame without a non-null row gives a NULL sum and the count 0
//   wf-2  a frame the device path does not take (ROWS BETWEEN UNBOUNDED PRECEDING AND 1 FOLLOWING) is refused at creation
// Built by __graft_entry__.build(); executed by tests/test_gpu_window_frames.py.  Exit code 0 = all cases pass.
#include <cstdio>

#include "presto_amd.hpp"

using namespace presto_amd;

static int failures = 0;
#define EXPECT(cond, ...)                              \
    do {                                               \
        if (!(cond)) {                                 \
            failures++;                                \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);              \
            fprintf(stderr, "\n");                     \
        }                                              \
    } while (0)

static const int64_t NUL = INT64_MIN;   // a NULL in the tables below

static Page page(const std::vector<std::string>& keys, const std::vector<double>& order, const std::vector<int64_t>& x)
{
    std::vector<int64_t> values(x);
    std::vector<uint8_t> nulls(x.size());
    for (size_t i = 0; i < x.size(); i++) {
        nulls[i] = x[i] == NUL;
        if (nulls[i]) values[i] = 0;
    }
    return Page({Block::varchar(keys), Block::doubles(order), Block::flat<int64_t>(PA_BIGINT, values, nulls)});
}

static FramedWindowFunctionDefinition function(int32_t id, std::vector<int32_t> arguments, int32_t frameType, int32_t endType)
{
    FramedWindowFunctionDefinition f;
    f.function = id;
    f.argumentChannels = std::move(arguments);
    f.frameType = frameType;
    f.endType = endType;
    return f;
}

struct Row {
    std::string key;
    double order;
    int64_t rank, rangeSum, rowsSum, min, count;   // NUL = NULL
};

static void testAggregatesWithFrames()
{
    // a: (0.1, NULL) (0.3, 5) (0.3, 7) (0.9, -2)     b: (0.2, NULL) (0.5, NULL)     c: (7.0, 4)
    std::vector<Page> pages = {page({"b", "a", "a", "c"}, {0.5, 0.3, 0.1, 7.0}, {NUL, 5, NUL, 4}), page({"a"}, {0.3}, {7}), page({"b", "a"}, {0.2, 0.9}, {NUL, -2})};
    FramedWindowFunctionDefinition rank;
    rank.function = PA_WINDOW_RANK;
    FramedWindowFunctionDefinition rangeSum;   // the default frame
    rangeSum.function = PA_WINDOW_SUM;
    rangeSum.argumentChannels = {2};
    FramedWindowOperatorFactory factory({PA_VARCHAR, PA_DOUBLE, PA_BIGINT}, {0, 1},
                                        {rank, rangeSum, function(PA_WINDOW_SUM, {2}, PA_FRAME_ROWS, PA_BOUND_CURRENT_ROW),
                                         function(PA_WINDOW_MIN, {2}, PA_FRAME_RANGE, PA_BOUND_UNBOUNDED_FOLLOWING),
                                         function(PA_WINDOW_COUNT, {2}, PA_FRAME_ROWS, PA_BOUND_CURRENT_ROW)},
                                        {0}, {1}, {PA_ASC_NULLS_LAST}, 10);
    auto op = factory.createOperator();
    std::vector<Row> got;
    auto value = [](const Block& b, int32_t i) { return b.isNull(i) ? NUL : b.getLong(i); };
    for (const auto& p : runDriver(pages, {op.get()})) {
        EXPECT(p.getChannelCount() == 7, "channels %d", p.getChannelCount());
        for (int c = 2; c < 7; c++) EXPECT(p.getBlock(c).type == PA_BIGINT, "function column %d is BIGINT", c);
        for (int32_t i = 0; i < p.getPositionCount(); i++)
            got.push_back(Row{p.getBlock(0).getSlice(i), p.getBlock(1).getDouble(i), value(p.getBlock(2), i), value(p.getBlock(3), i), value(p.getBlock(4), i),
                              value(p.getBlock(5), i), value(p.getBlock(6), i)});
    }
    const std::vector<Row> want = {{"a", 0.1, 1, NUL, NUL, -2, 0}, {"a", 0.3, 2, 12, 5, -2, 1}, {"a", 0.3, 2, 12, 12, -2, 2}, {"a", 0.9, 4, 10, 10, -2, 3},
                                   {"b", 0.2, 1, NUL, NUL, NUL, 0}, {"b", 0.5, 2, NUL, NUL, NUL, 0},
                                   {"c", 7.0, 1, 4, 4, 4, 1}};
    EXPECT(got.size() == want.size(), "wf-1: %zu rows, expected %zu", got.size(), want.size());
    for (size_t i = 0; i < got.size() && i < want.size(); i++)
        EXPECT(got[i].key == want[i].key && got[i].order == want[i].order && got[i].rank == want[i].rank && got[i].rangeSum == want[i].rangeSum &&
                   got[i].rowsSum == want[i].rowsSum && got[i].min == want[i].min && got[i].count == want[i].count,
               "wf-1 row %zu: (%s, %g, %ld, %ld, %ld, %ld, %ld)", i, got[i].key.c_str(), got[i].order, (long)got[i].rank, (long)got[i].rangeSum,
               (long)got[i].rowsSum, (long)got[i].min, (long)got[i].count);
    EXPECT(op->isFinished(), "wf-1: finished once the page is taken");
}

static void testBoundedFrameIsRefused()
{
    FramedWindowFunctionDefinition f = function(PA_WINDOW_SUM, {2}, PA_FRAME_ROWS, PA_BOUND_FOLLOWING);
    f.endChannel = 2;
    FramedWindowOperatorFactory factory({PA_VARCHAR, PA_DOUBLE, PA_BIGINT}, {0, 1}, {f}, {0}, {1}, {PA_ASC_NULLS_LAST});
    bool refused = false;
    try {
        factory.createOperator();
    }
    catch (const std::exception&) {
        refused = true;
    }
    EXPECT(refused, "a bounded frame must be refused");
}

int main()
{
    try {
        check(pa_init(0));
        testAggregatesWithFrames();
        testBoundedFrameIsRefused();
        pa_shutdown();
    }
    catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("window frames ok\n");
    return 0;
}
