// C++ driver test of TopNRankingOperator through include/presto_amd.hpp (the C++ host mirror), on the GPU: the known answers of the
// reference's TestTopNRankingOperator
//   tr-1  testPartitioned      VARCHAR partition key, DOUBLE ASC_NULLS_LAST, n = 3, four pages: 3 / 3 / 2 rows, numbered in order
//   tr-2  testUnPartitioned    no partition channels, partial and not: the three smallest values
//   tr-3  testRankNullAndNan   RANK, ASC_NULLS_FIRST, n = 3: NULL ties with NULL, NaN with NaN -- a partition keeps four rows
// Built by __graft_entry__.build(); executed by tests/test_gpu_topn_ranking.py.  Exit code 0 = all cases pass.
#include <cmath>
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

static Page page(const std::vector<std::string>& keys, const std::vector<double>& values, const std::vector<uint8_t>& valueIsNull = {})
{
    Block v = Block::doubles(values);
    v.nulls = valueIsNull;
    return Page({Block::varchar(keys), v});
}

static std::vector<Page> katPages()
{
    return {page({"a", "b", "c", "c"}, {0.3, 0.2, 0.1, 0.91}), page({"a"}, {0.4}), page({"a", "a", "b", "b"}, {0.5, 0.6, 0.7, 0.8}), page({"b"}, {0.9})};
}

struct Row {
    bool isNull;
    double value;
    std::string key;
    int64_t ranking;   // -1: no ranking column
};
static std::vector<Row> rowsOf(const std::vector<Page>& out, int channels)
{
    std::vector<Row> rows;
    for (const auto& p : out) {
        EXPECT(p.getChannelCount() == channels, "channels %d", p.getChannelCount());
        for (int32_t i = 0; i < p.getPositionCount(); i++) {
            if (channels == 3) EXPECT(p.getBlock(2).type == PA_BIGINT && !p.getBlock(2).isNull(i), "ranking block");
            rows.push_back(Row{p.getBlock(0).isNull(i), p.getBlock(0).getDouble(i), p.getBlock(1).getSlice(i), channels == 3 ? p.getBlock(2).getLong(i) : -1});
        }
    }
    return rows;
}
static void expectRows(const char* what, const std::vector<Row>& got, const std::vector<Row>& want)
{
    EXPECT(got.size() == want.size(), "%s: %zu rows, expected %zu", what, got.size(), want.size());
    for (size_t i = 0; i < got.size() && i < want.size(); i++) {
        const bool same_value = got[i].isNull == want[i].isNull && (got[i].isNull || (std::isnan(want[i].value) ? std::isnan(got[i].value) : got[i].value == want[i].value));
        EXPECT(same_value && got[i].key == want[i].key && got[i].ranking == want[i].ranking, "%s row %zu: (%g, %s, %ld)", what, i, got[i].value,
               got[i].key.c_str(), (long)got[i].ranking);
    }
}

static void testPartitioned()
{
    TopNRankingOperatorFactory factory(PA_RANKING_ROW_NUMBER, {PA_VARCHAR, PA_DOUBLE}, {1, 0}, {0}, {1}, {PA_ASC_NULLS_LAST}, 3, false, -1, 10);
    auto op = factory.createOperator();
    auto rows = rowsOf(runDriver(katPages(), {op.get()}), 3);
    expectRows("tr-1", rows, {{false, 0.3, "a", 1}, {false, 0.4, "a", 2}, {false, 0.5, "a", 3}, {false, 0.2, "b", 1}, {false, 0.7, "b", 2},
                             {false, 0.8, "b", 3}, {false, 0.1, "c", 1}, {false, 0.91, "c", 2}});
    const TopNRankingStats st = topNRankingStats(*op);
    EXPECT(st.partitions == 3 && st.rowsHeld == 8 && st.capacity > 0, "tr-1 stats: %ld partitions, %ld held", (long)st.partitions, (long)st.rowsHeld);
}

static void testUnPartitioned(bool partial)
{
    TopNRankingOperatorFactory factory(PA_RANKING_ROW_NUMBER, {PA_VARCHAR, PA_DOUBLE}, {1, 0}, {}, {1}, {PA_ASC_NULLS_LAST}, 3, partial, -1, 10);
    auto op = factory.createOperator();
    auto rows = rowsOf(runDriver(katPages(), {op.get()}), partial ? 2 : 3);
    expectRows(partial ? "tr-2 partial" : "tr-2", rows,
               {{false, 0.1, "c", partial ? -1 : 1}, {false, 0.2, "b", partial ? -1 : 2}, {false, 0.3, "a", partial ? -1 : 3}});
    EXPECT(op->isFinished(), "tr-2: finished once the page is taken");
}

static void testRankNullAndNan()
{
    const double nan = std::nan("");
    std::vector<Page> pages = {page({"a", "b", "b", "c", "c"}, {0, 0.2, nan, 0.1, 0.91}, {1, 0, 0, 0, 0}), page({"a"}, {0.4}),
                               page({"a", "a", "a", "b", "b"}, {0.5, 0, 0.6, 0.7, nan}, {0, 1, 0, 0, 0})};
    TopNRankingOperatorFactory factory(PA_RANKING_RANK, {PA_VARCHAR, PA_DOUBLE}, {1, 0}, {0}, {1}, {PA_ASC_NULLS_FIRST}, 3, false, -1, 10);
    auto op = factory.createOperator();
    auto rows = rowsOf(runDriver(pages, {op.get()}), 3);
    expectRows("tr-3", rows, {{true, 0, "a", 1}, {true, 0, "a", 1}, {false, 0.4, "a", 3}, {false, 0.2, "b", 1}, {false, 0.7, "b", 2},
                             {false, nan, "b", 3}, {false, nan, "b", 3}, {false, 0.1, "c", 1}, {false, 0.91, "c", 2}});
}

static void testDenseRankIsRefused()
{
    TopNRankingOperatorFactory factory(PA_RANKING_DENSE_RANK, {PA_VARCHAR, PA_DOUBLE}, {1, 0}, {0}, {1}, {PA_ASC_NULLS_LAST}, 3, false);
    bool refused = false;
    try {
        factory.createOperator();
    }
    catch (const std::exception&) {
        refused = true;
    }
    EXPECT(refused, "dense_rank must be refused");
}

int main()
{
    try {
        check(pa_init(0));
        testPartitioned();
        testUnPartitioned(false);
        testUnPartitioned(true);
        testRankNullAndNan();
        testDenseRankIsRefused();
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
    printf("topn ranking ok\n");
    return 0;
}
