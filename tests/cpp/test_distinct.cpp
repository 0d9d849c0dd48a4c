// C++ driver test of MarkDistinctOperator / DistinctLimitOperator through include/presto_amd.hpp (the C++ host mirror), on the GPU:
//   md-1  TestMarkDistinctOperator.testMarkDistinct   two sequence pages 0..99: the first all true, the second all false
//   dl-1  TestDistinctLimitOperator.testDistinctLimit  sequence pages (3, 1), (5, 2), limit 5 -> 1, 2, 3, 4, 5
//   a VARCHAR key with NULLs through runDriver.
// Built by __graft_entry__.build(); executed by tests/test_gpu_distinct.py.  Exit code 0 = all cases pass.
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

static Page sequencePage(int32_t length, int64_t start)
{
    std::vector<int64_t> v;
    for (int32_t i = 0; i < length; i++) v.push_back(start + i);
    return Page({Block::bigint(v)});
}

static void testMarkDistinct()
{
    auto op = createMarkDistinctOperator({PA_BIGINT}, {0});
    auto out = runDriver({sequencePage(100, 0), sequencePage(100, 0)}, {op.get()});
    int64_t rows = 0;
    for (const auto& p : out) {
        EXPECT(p.getChannelCount() == 2, "md-1 channels %d", p.getChannelCount());
        for (int32_t i = 0; i < p.getPositionCount(); i++, rows++) {
            EXPECT(p.getBlock(0).getLong(i) == rows % 100, "md-1 row %ld value %ld", (long)rows, (long)p.getBlock(0).getLong(i));
            EXPECT(p.getBlock(1).type == PA_BOOLEAN && !p.getBlock(1).isNull(i), "md-1 row %ld mark block", (long)rows);
            EXPECT(p.getBlock(1).values[i] == (rows < 100 ? 1 : 0), "md-1 row %ld mark %d", (long)rows, (int)p.getBlock(1).values[i]);
        }
    }
    EXPECT(rows == 200, "md-1 expected 200 rows, got %ld", (long)rows);
    EXPECT(distinctCount(*op) == 100, "md-1 distinct count %ld", (long)distinctCount(*op));
}

static void testDistinctLimit()
{
    auto op = createDistinctLimitOperator({PA_BIGINT}, {0}, 5);
    auto out = runDriver({sequencePage(3, 1), sequencePage(5, 2)}, {op.get()});
    std::vector<int64_t> got;
    for (const auto& p : out)
        for (int32_t i = 0; i < p.getPositionCount(); i++) got.push_back(p.getBlock(0).getLong(i));
    EXPECT(got == std::vector<int64_t>({1, 2, 3, 4, 5}), "dl-1 got %zu rows", got.size());
}

static void testVarcharKeys()
{
    Block keys = Block::varchar({"a", "", "a", "", "bb", "", "bb"});
    keys.nulls = {0, 0, 0, 1, 0, 1, 0};   // "" and NULL are different keys
    auto mark = createMarkDistinctOperator({PA_VARCHAR, PA_BIGINT}, {0});
    auto out = runDriver({Page({keys, Block::bigint({0, 1, 2, 3, 4, 5, 6})})}, {mark.get()});
    std::vector<int> got;
    for (const auto& p : out)
        for (int32_t i = 0; i < p.getPositionCount(); i++) got.push_back(p.getBlock(2).values[i]);
    EXPECT(got == std::vector<int>({1, 1, 0, 1, 1, 0, 0}), "varchar marks: %zu rows", got.size());
}

int main()
{
    try {
        check(pa_init(0));
        testMarkDistinct();
        testDistinctLimit();
        testVarcharKeys();
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
    printf("distinct ok\n");
    return 0;
}
