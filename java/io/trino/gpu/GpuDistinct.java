package io.trino.gpu;

import io.trino.operator.OperatorFactory;
import io.trino.spi.type.BooleanType;
import io.trino.spi.type.Type;
import io.trino.sql.planner.plan.PlanNodeId;

import java.util.ArrayList;
import java.util.List;
import java.util.Optional;
import java.util.OptionalInt;

/**
 * LocalExecutionPlanner.visitMarkDistinct (core/trino-main/src/main/java/io/trino/sql/planner/LocalExecutionPlanner.java:1540) and
 * visitDistinctLimit (:1455) on the device: called in place of `new MarkDistinctOperatorFactory(...)` and
 * `new DistinctLimitOperatorFactory(...)`.  Optional.empty() when the device path does not take the shape -- the key types the
 * library refuses with PA_ERR_NOT_SUPPORTED (long decimals, rows; anything RowExpressionSerializer has no code for) or more distinct
 * channels than it takes -- and the planner keeps the reference factory.
 */
public final class GpuDistinct
{
    // pa_type codes the library refuses as distinct keys with PA_ERR_NOT_SUPPORTED, and its cap on distinct channels (include/presto_amd.h)
    private static final int PA_ROW = 6, PA_LONG_DECIMAL = 9;
    private static final int MAX_DISTINCT_CHANNELS = 8;

    private GpuDistinct() {}

    public static Optional<OperatorFactory> markDistinct(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, List<Integer> markDistinctChannels,
            OptionalInt hashChannel)
    {
        Optional<Shape> shape = Shape.of(sourceTypes, markDistinctChannels);
        if (shape.isEmpty()) {
            return Optional.empty();
        }
        Shape s = shape.get();
        List<Type> output = new ArrayList<>(sourceTypes);
        output.add(BooleanType.BOOLEAN);   // MarkDistinctOperator: the input page with the mark appended
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuMarkDistinctOperator", sourceTypes, output,
                () -> GpuNative.createMarkDistinct(s.types, s.params, s.channels, hashChannel.orElse(-1), 0, 0)));
    }

    public static Optional<OperatorFactory> distinctLimit(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, List<Integer> distinctChannels,
            long limit, OptionalInt hashChannel)
    {
        Optional<Shape> shape = Shape.of(sourceTypes, distinctChannels);
        if (shape.isEmpty() || limit < 0) {
            return Optional.empty();
        }
        Shape s = shape.get();
        // DistinctLimitOperator.java:76-79: the distinct channels in order, then the hash channel
        List<Type> output = new ArrayList<>();
        for (int channel : distinctChannels) {
            output.add(sourceTypes.get(channel));
        }
        hashChannel.ifPresent(channel -> output.add(sourceTypes.get(channel)));
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuDistinctLimitOperator", sourceTypes, output,
                () -> GpuNative.createDistinctLimit(s.types, s.params, s.channels, limit, hashChannel.orElse(-1), 0, 0)));
    }

    private static final class Shape
    {
        final int[] types;
        final int[] params;
        final int[] channels;

        private Shape(int[] types, int[] params, int[] channels)
        {
            this.types = types;
            this.params = params;
            this.channels = channels;
        }

        static Optional<Shape> of(List<Type> sourceTypes, List<Integer> distinctChannels)
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
            if (distinctChannels.isEmpty() || distinctChannels.size() > MAX_DISTINCT_CHANNELS) {
                return Optional.empty();
            }
            for (int channel : distinctChannels) {
                if (types[channel] == PA_ROW || types[channel] == PA_LONG_DECIMAL) {
                    return Optional.empty();
                }
            }
            return Optional.of(new Shape(types, params, distinctChannels.stream().mapToInt(Integer::intValue).toArray()));
        }
    }
}
