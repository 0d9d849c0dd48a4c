package io.trino.gpu;

import io.trino.operator.OperatorFactory;
import io.trino.spi.type.BigintType;
import io.trino.spi.type.Type;
import io.trino.sql.planner.plan.PlanNodeId;

import java.util.ArrayList;
import java.util.List;
import java.util.Optional;

/**
 * LocalExecutionPlanner.visitRowNumber (core/trino-main/src/main/java/io/trino/sql/planner/LocalExecutionPlanner.java:900-938) on the
 * device: called in place of `new RowNumberOperator.RowNumberOperatorFactory(...)`.  Optional.empty() when the device path does not take
 * the shape -- partition key types the library refuses with PA_ERR_NOT_SUPPORTED (long decimals, rows; anything
 * RowExpressionSerializer has no code for), more partition channels than it takes, or, under maxRowsPerPartition, an output channel it
 * cannot copy position by position -- and the planner keeps the reference factory.
 */
public final class GpuRowNumber
{
    // pa_type codes the library refuses as partition keys with PA_ERR_NOT_SUPPORTED, and its cap on partition channels (include/presto_amd.h)
    private static final int PA_ROW = 6, PA_LONG_DECIMAL = 9;
    private static final int MAX_PARTITION_CHANNELS = 8;
    private static final int MAX_CHANNELS = 64;

    private GpuRowNumber() {}

    public static Optional<OperatorFactory> rowNumber(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, List<Integer> outputChannels,
            List<Integer> partitionChannels, Optional<Integer> maxRowsPerPartition, Optional<Integer> hashChannel, int expectedPositions)
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
        if (types.length == 0 || types.length > MAX_CHANNELS || outputChannels.size() > MAX_CHANNELS || partitionChannels.size() > MAX_PARTITION_CHANNELS) {
            return Optional.empty();
        }
        if (maxRowsPerPartition.isPresent() && maxRowsPerPartition.get() < 0) {
            return Optional.empty();
        }
        for (int channel : partitionChannels) {
            if (types[channel] == PA_ROW || types[channel] == PA_LONG_DECIMAL) {
                return Optional.empty();
            }
        }
        if (maxRowsPerPartition.isPresent()) {
            for (int channel : outputChannels) {
                if (types[channel] == PA_ROW || types[channel] == PA_LONG_DECIMAL) {
                    return Optional.empty();
                }
            }
        }
        // RowNumberOperator: the output channels in order, then the row number
        List<Type> output = new ArrayList<>();
        for (int channel : outputChannels) {
            output.add(sourceTypes.get(channel));
        }
        output.add(BigintType.BIGINT);
        int[] out = outputChannels.stream().mapToInt(Integer::intValue).toArray();
        int[] partition = partitionChannels.stream().mapToInt(Integer::intValue).toArray();
        long cap = maxRowsPerPartition.map(Integer::longValue).orElse(-1L);
        int expected = Math.max(expectedPositions, 0);
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuRowNumberOperator", sourceTypes, output,
                () -> GpuNative.createRowNumber(types, params, out, partition, cap, hashChannel.orElse(-1), expected, 0)));
    }
}
