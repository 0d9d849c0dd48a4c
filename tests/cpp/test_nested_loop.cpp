// C++ driver test of NestedLoopBuildOperator / NestedLoopJoinOperator through include/presto_amd.hpp (the C++ host mirror), on the GPU:
//   nl-1  a VARCHAR build column and the filter p.x < b.y: the surviving pairs in probe-major order
//   nl-2  the builder -> bridge -> join order of a Driver pair: the join is blocked until the builder finished, then the plain product
// Built and executed by tests/test_gpu_nested_loop.py.  Exit code 0 = all cases pass.
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

static void testFilteredJoinWithVarcharBuildColumn()
{
    NestedLoopJoinBridge bridge;
    NestedLoopBuildOperatorFactory buildFactory({PA_BIGINT, PA_VARCHAR});
    // the pair's channels: 0 = b.y, 1 = b.name, 2 = p.x
    NestedLoopJoinOperatorFactory joinFactory({PA_BIGINT}, {0}, {1, 0}, call(PA_OP_LESS_THAN, PA_BOOLEAN, {field(2, PA_BIGINT), field(0, PA_BIGINT)}));
    auto build = buildFactory.createOperator(bridge);
    auto join = joinFactory.createOperator(bridge);
    auto none = runDriver({Page({Block::bigint({5, 1}), Block::varchar({"five", "one"})}), Page({Block::bigint({3}), Block::varchar({""})})}, {build.get()});
    EXPECT(none.empty(), "nl-1 the builder produced output");
    EXPECT(bridge.rows() == 3, "nl-1 build rows %ld", (long)bridge.rows());
    auto out = runDriver({Page({Block::bigint({0, 4})}), Page({Block::bigint({2, 9})})}, {join.get()});
    std::vector<int64_t> x, y;
    std::vector<std::string> name;
    for (const auto& p : out) {
        EXPECT(p.getChannelCount() == 3, "nl-1 channels %d", p.getChannelCount());
        for (int32_t i = 0; i < p.getPositionCount(); i++) {
            x.push_back(p.getBlock(0).getLong(i));
            name.push_back(p.getBlock(1).getSlice(i));
            y.push_back(p.getBlock(2).getLong(i));
        }
    }
    EXPECT(x == std::vector<int64_t>({0, 0, 0, 4, 2, 2}), "nl-1 probe column: %zu rows", x.size());
    EXPECT(y == std::vector<int64_t>({5, 1, 3, 5, 5, 3}), "nl-1 build column: %zu rows", y.size());
    EXPECT(name == std::vector<std::string>({"five", "one", "", "five", "five", ""}), "nl-1 build names: %zu rows", name.size());
}

static void testBuilderBridgeJoinOrder()
{
    NestedLoopJoinBridge bridge;
    bool refused = false;
    try {
        NestedLoopJoinOperatorFactory({PA_BIGINT}, {0}, {0}).createOperator(bridge);   // no builder on the bridge yet
    }
    catch (const TrinoException&) {
        refused = true;
    }
    EXPECT(refused, "nl-2 a join was created on a bridge without a builder");
    auto build = NestedLoopBuildOperatorFactory({PA_BIGINT}).createOperator(bridge);
    auto join = NestedLoopJoinOperatorFactory({PA_BIGINT}, {0}, {0}).createOperator(bridge);
    EXPECT(join->isBlocked() && !join->needsInput(), "nl-2 the join is not blocked before the builder finished");
    runDriver({Page({Block::bigint({10, 20})})}, {build.get()});
    EXPECT(!join->isBlocked() && join->needsInput(), "nl-2 the join is still blocked after the builder finished");
    auto out = runDriver({Page({Block::bigint({1, 2, 3})})}, {join.get()});
    std::vector<int64_t> got;
    for (const auto& p : out)
        for (int32_t i = 0; i < p.getPositionCount(); i++) got.push_back(p.getBlock(0).getLong(i) * 100 + p.getBlock(1).getLong(i));
    EXPECT(got == std::vector<int64_t>({110, 120, 210, 220, 310, 320}), "nl-2 product: %zu rows", got.size());
    EXPECT(join->isFinished(), "nl-2 the join did not finish");
}

int main()
{
    try {
        check(pa_init(0));
        testFilteredJoinWithVarcharBuildColumn();
        testBuilderBridgeJoinOrder();
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
    printf("nested loop ok\n");
    return 0;
}
