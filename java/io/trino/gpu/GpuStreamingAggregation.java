package io.trino.gpu;

import io.trino.operator.OperatorFactory;
import io.trino.spi.type.Type;
import io.trino.sql.planner.plan.PlanNodeId;

import java.util.List;
import java.util.Optional;

/**
 * The streamable branch of LocalExecutionPlanner.visitAggregation (the pre-grouped symbols are all grouping keys) with step SINGLE on
 * the device: called in place of `StreamingAggregationOperator.createOperatorFactory(...)`
 * (core/trino-main/src/main/java/io/trino/operator/StreamingAggregationOperator.java).  The planner hook resolves every
 * AggregatorFactory to a pa_agg_fn, its argument channel and its mask channel (-1: none), as it does for the hash aggregation.
 * Optional.empty() when the device path does not take the shape -- a step other than SINGLE, a key type or an aggregate over a type the
 * library refuses with PA_ERR_NOT_SUPPORTED (DECIMAL sums, VARCHAR min / max, long decimals, rows), more group channels or aggregates
 * than it takes, anything RowExpressionSerializer has no code for -- and the planner keeps the reference factory.
 */
public final class GpuStreamingAggregation
{
    // pa_type codes, pa_agg_fn ids and the caps of include/presto_amd.h
    private static final int PA_VARCHAR = 5, PA_ROW = 6, PA_DECIMAL = 8, PA_LONG_DECIMAL = 9;
    private static final int AGG_COUNT_STAR = 0, AGG_COUNT = 1, AGG_SUM = 2, AGG_AVG = 3;
    private static final int STEP_SINGLE = 0;
    private static final int MAX_GROUP_CHANNELS = 8, MAX_AGGREGATES = 16, MAX_CHANNELS = 64;

    private GpuStreamingAggregation() {}

    public static Optional<OperatorFactory> create(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, List<Integer> groupByChannels, int step,
            int[] aggFns, int[] aggInputs, int[] aggMasks, List<Type> outputTypes)
    {
        int[] types;
        int[] params;
        try {
            types = sourceTypes.stream().mapToInt(RowExpressionSerializer::typeOf).toArray();
            params = sourceTypes.stream().mapToInt(RowExpressionSerializer::typeParamOf).toArray();
        }
        catch (RuntimeException unsupported) {
            return Optional.empty();
        }
        if (step != STEP_SINGLE || types.length > MAX_CHANNELS || groupByChannels.isEmpty() || groupByChannels.size() > MAX_GROUP_CHANNELS
                || aggFns.length > MAX_AGGREGATES) {
            return Optional.empty();
        }
        for (int channel : groupByChannels) {
            if (types[channel] == PA_ROW || types[channel] == PA_LONG_DECIMAL) {
                return Optional.empty();
            }
        }
        int[] aggInputTypes = new int[aggFns.length];
        for (int i = 0; i < aggFns.length; i++) {
            if (aggFns[i] == AGG_COUNT_STAR) {
                continue;
            }
            int type = types[aggInputs[i]];
            aggInputTypes[i] = type;
            boolean refused;
            if (aggFns[i] == AGG_COUNT) {
                refused = type == PA_ROW;
            }
            else if (aggFns[i] == AGG_SUM || aggFns[i] == AGG_AVG) {
                refused = type == PA_DECIMAL || type == PA_LONG_DECIMAL;
            }
            else {
                refused = type == PA_VARCHAR || type == PA_LONG_DECIMAL || type == PA_ROW;
            }
            if (refused) {
                return Optional.empty();
            }
        }
        int[] channels = groupByChannels.stream().mapToInt(Integer::intValue).toArray();
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuStreamingAggregationOperator", sourceTypes, outputTypes,
                () -> GpuNative.createStreamingAggregation(types, params, channels, step, aggFns, aggInputs, aggMasks, aggInputTypes, 0)));
    }
}
