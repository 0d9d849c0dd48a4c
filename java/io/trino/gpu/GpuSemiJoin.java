package io.trino.gpu;

import io.trino.operator.OperatorFactory;
import io.trino.spi.type.BooleanType;
import io.trino.spi.type.Type;
import io.trino.sql.planner.plan.PlanNodeId;

import java.util.ArrayList;
import java.util.List;
import java.util.Optional;
import java.util.OptionalInt;
import java.util.concurrent.atomic.AtomicInteger;

/**
 * LocalExecutionPlanner.visitSemiJoin (core/trino-main/src/main/java/io/trino/sql/planner/LocalExecutionPlanner.java:2749-2835) on
 * the device: called in place of `new SetBuilderOperatorFactory(...)` and `HashSemiJoinOperator.createOperatorFactory(...)`.  Both
 * factories share one pa_channel_set (the SetSupplier); it is destroyed when the last factory had noMoreOperators (the operators
 * already created hold the set natively).  Optional.empty() when the device path does not take the shape -- the key types the
 * library refuses with PA_ERR_NOT_SUPPORTED (long decimals, rows; anything RowExpressionSerializer has no code for), or build
 * and probe key types that differ -- and the planner keeps the reference factories.
 */
public final class GpuSemiJoin
{
    // pa_type codes the library refuses as set keys with PA_ERR_NOT_SUPPORTED (include/presto_amd.h)
    private static final int PA_ROW = 6, PA_DECIMAL = 8, PA_LONG_DECIMAL = 9;

    public final OperatorFactory setBuilder;
    public final OperatorFactory semiJoin;

    private GpuSemiJoin(OperatorFactory setBuilder, OperatorFactory semiJoin)
    {
        this.setBuilder = setBuilder;
        this.semiJoin = semiJoin;
    }

    public static Optional<GpuSemiJoin> create(int setBuilderOperatorId, PlanNodeId buildNodeId, List<Type> buildTypes, int setChannel,
            OptionalInt buildHashChannel, int expectedPositions, int semiJoinOperatorId, PlanNodeId probeNodeId, List<Type> probeTypes,
            int probeJoinChannel, OptionalInt probeHashChannel)
    {
        int[] build;
        int[] buildParams;
        int[] probe;
        int[] probeParams;
        try {
            build = buildTypes.stream().mapToInt(RowExpressionSerializer::typeOf).toArray();
            buildParams = buildTypes.stream().mapToInt(RowExpressionSerializer::typeParamOf).toArray();
            probe = probeTypes.stream().mapToInt(RowExpressionSerializer::typeOf).toArray();
            probeParams = probeTypes.stream().mapToInt(RowExpressionSerializer::typeParamOf).toArray();
        }
        catch (RuntimeException unsupported) {
            return Optional.empty();
        }
        int key = build[setChannel];
        // (VARCHAR(n) bounds need not agree: the set compares bytes; a DECIMAL's precision and scale must)
        if (key == PA_ROW || key == PA_LONG_DECIMAL || key != probe[probeJoinChannel]
                || (key == PA_DECIMAL && buildParams[setChannel] != probeParams[probeJoinChannel])) {
            return Optional.empty();
        }
        long set = GpuNative.channelSetCreate();
        GpuOperatorFactory.SharedHandle shared = new GpuOperatorFactory.SharedHandle()
        {
            private final AtomicInteger refs = new AtomicInteger();

            @Override
            public void retain()
            {
                refs.incrementAndGet();
            }

            @Override
            public void release()
            {
                if (refs.decrementAndGet() == 0) {
                    GpuNative.channelSetDestroy(set);
                }
            }
        };
        List<Type> probeOutput = new ArrayList<>(probeTypes);
        probeOutput.add(BooleanType.BOOLEAN);   // HashSemiJoinOperator: the probe page with the mark appended
        OperatorFactory builder = new GpuOperatorFactory(setBuilderOperatorId, buildNodeId, "GpuSetBuilderOperator", buildTypes, List.of(),
                () -> GpuNative.createSetBuilder(set, build, buildParams, setChannel, buildHashChannel.orElse(-1), expectedPositions), shared);
        OperatorFactory semi = new GpuOperatorFactory(semiJoinOperatorId, probeNodeId, "GpuHashSemiJoinOperator", probeTypes, probeOutput,
                () -> GpuNative.createHashSemiJoin(set, probe, probeParams, probeJoinChannel, probeHashChannel.orElse(-1), 0), shared);
        return Optional.of(new GpuSemiJoin(builder, semi));
    }
}
