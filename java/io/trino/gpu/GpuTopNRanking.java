package io.trino.gpu;

import io.trino.operator.OperatorFactory;
import io.trino.spi.connector.SortOrder;
import io.trino.spi.type.BigintType;
import io.trino.spi.type.Type;
import io.trino.sql.planner.plan.PlanNodeId;
import io.trino.sql.planner.plan.TopNRankingNode.RankingType;

import java.util.ArrayList;
import java.util.List;
import java.util.Optional;

/**
 * LocalExecutionPlanner.visitTopNRanking on the device: called in place of `new TopNRankingOperator.TopNRankingOperatorFactory(...)`.
 * Optional.empty() when the device path does not take the shape -- DENSE_RANK, partition / sort / output channel types the library
 * refuses with PA_ERR_NOT_SUPPORTED (long decimals, rows; a short decimal as a sort channel is handed over as BIGINT: same order),
 * more partition channels than it takes -- and the planner keeps the reference factory.  RANK peers follow the comparator: -0.0 and
 * +0.0 in a sort channel are not peers (include/presto_amd.h).
 */
public final class GpuTopNRanking
{
    // pa_type codes (include/presto_amd.h) and the library's caps
    private static final int PA_BIGINT = 0, PA_ROW = 6, PA_DECIMAL = 8, PA_LONG_DECIMAL = 9;
    private static final int PA_RANKING_ROW_NUMBER = 0, PA_RANKING_RANK = 1;
    private static final int MAX_PARTITION_CHANNELS = 8;
    private static final int MAX_CHANNELS = 64;

    private GpuTopNRanking() {}

    public static Optional<OperatorFactory> topNRanking(int operatorId, PlanNodeId planNodeId, RankingType rankingType, List<Type> sourceTypes,
            List<Integer> outputChannels, List<Integer> partitionChannels, List<Integer> sortChannels, List<SortOrder> sortOrders,
            int maxRowCountPerPartition, boolean partial, Optional<Integer> hashChannel, int expectedPositions)
    {
        int ranking;
        switch (rankingType) {
            case ROW_NUMBER:
                ranking = PA_RANKING_ROW_NUMBER;
                break;
            case RANK:
                ranking = PA_RANKING_RANK;
                break;
            default:
                return Optional.empty();   // DENSE_RANK: the reference operator throws; that is its business
        }
        int[] types;
        int[] params;
        try {
            types = sourceTypes.stream().mapToInt(RowExpressionSerializer::typeOf).toArray();
            params = sourceTypes.stream().mapToInt(RowExpressionSerializer::typeParamOf).toArray();
        }
        catch (RuntimeException unsupported) {
            return Optional.empty();
        }
        if (types.length == 0 || types.length > MAX_CHANNELS || outputChannels.size() > MAX_CHANNELS || sortChannels.size() > MAX_CHANNELS
                || partitionChannels.size() > MAX_PARTITION_CHANNELS || sortChannels.isEmpty() || sortChannels.size() != sortOrders.size()
                || maxRowCountPerPartition <= 0) {
            return Optional.empty();
        }
        for (int channel : partitionChannels) {
            if (types[channel] == PA_ROW || types[channel] == PA_LONG_DECIMAL) {
                return Optional.empty();
            }
        }
        for (int channel : outputChannels) {
            if (types[channel] == PA_ROW || types[channel] == PA_LONG_DECIMAL) {
                return Optional.empty();
            }
        }
        for (int channel : sortChannels) {
            if (types[channel] == PA_ROW || types[channel] == PA_LONG_DECIMAL) {
                return Optional.empty();
            }
            // a short decimal sorts as its unscaled long; declared BIGINT only when nothing else reads the channel as a decimal key
            if (types[channel] == PA_DECIMAL) {
                if (partitionChannels.contains(channel)) {
                    return Optional.empty();
                }
                types[channel] = PA_BIGINT;
                params[channel] = 0;
            }
        }
        // TopNRankingOperator: the output channels in order, then -- unless partial -- the ranking
        List<Type> output = new ArrayList<>();
        for (int channel : outputChannels) {
            output.add(sourceTypes.get(channel));
        }
        if (!partial) {
            output.add(BigintType.BIGINT);
        }
        int[] out = outputChannels.stream().mapToInt(Integer::intValue).toArray();
        int[] partition = partitionChannels.stream().mapToInt(Integer::intValue).toArray();
        int[] sort = sortChannels.stream().mapToInt(Integer::intValue).toArray();
        int[] orders = sortOrders.stream().mapToInt(SortOrder::ordinal).toArray();   // ASC_NULLS_FIRST, ASC_NULLS_LAST, DESC_NULLS_FIRST, DESC_NULLS_LAST
        int expected = Math.max(expectedPositions, 0);
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuTopNRankingOperator", sourceTypes, output,
                () -> GpuNative.createTopNRanking(ranking, types, params, out, partition, sort, orders, maxRowCountPerPartition, partial,
                        hashChannel.orElse(-1), expected, 0)));
    }
}
