package io.trino.gpu;

import io.trino.execution.TaskId;
import io.trino.operator.DriverContext;
import io.trino.operator.Operator;
import io.trino.operator.OperatorContext;
import io.trino.operator.OperatorFactory;
import io.trino.spi.type.BigintType;
import io.trino.spi.type.Type;
import io.trino.sql.planner.plan.PlanNodeId;

import java.util.ArrayList;
import java.util.List;
import java.util.Optional;

/**
 * LocalExecutionPlanner.visitAssignUniqueId on the device: called in place of `AssignUniqueIdOperator.createOperatorFactory(...)`
 * (core/trino-main/src/main/java/io/trino/operator/AssignUniqueIdOperator.java:42-97).  The factory owns the pool of row ids (the
 * reference's AtomicLong valuePool) its operators draw blocks of 2^20 from; an operator learns its stage and task id from the
 * DriverContext it is created in, as the reference's does from its ProcessorContext.  duplicate() starts a pool of its own, as the
 * reference's Factory.duplicate() does.  Optional.empty() when the device path does not take the shape -- a source type the library
 * refuses (rows; anything RowExpressionSerializer has no code for) or more than 64 channels -- and the planner keeps the reference factory.
 */
public final class GpuAssignUniqueId
        implements OperatorFactory
{
    private static final int PA_ROW = 6;
    private static final int MAX_CHANNELS = 64;

    private final int operatorId;
    private final PlanNodeId planNodeId;
    private final List<Type> sourceTypes;
    private final List<Type> outputTypes;
    private final int[] types;
    private final int[] params;
    private long pool;       // pa_unique_id_pool*, 0 once closed
    private boolean closed;

    public static Optional<OperatorFactory> create(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes)
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
        if (types.length == 0 || types.length > MAX_CHANNELS) {
            return Optional.empty();
        }
        for (int type : types) {
            if (type == PA_ROW) {
                return Optional.empty();
            }
        }
        return Optional.of(new GpuAssignUniqueId(operatorId, planNodeId, sourceTypes, types, params));
    }

    private GpuAssignUniqueId(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, int[] types, int[] params)
    {
        this.operatorId = operatorId;
        this.planNodeId = planNodeId;
        this.sourceTypes = sourceTypes;
        this.types = types;
        this.params = params;
        List<Type> output = new ArrayList<>(sourceTypes);
        output.add(BigintType.BIGINT);   // AssignUniqueIdOperator: the input page with the id appended
        this.outputTypes = output;
        this.pool = GpuNative.createUniqueIdPool(0);
    }

    @Override
    public synchronized Operator createOperator(DriverContext driverContext)
    {
        if (closed) {
            throw new IllegalStateException("Factory is already closed");
        }
        OperatorContext context = driverContext.addOperatorContext(operatorId, planNodeId, "GpuAssignUniqueIdOperator");
        TaskId taskId = driverContext.getTaskId();
        long handle = GpuNative.createAssignUniqueId(pool, types, params, taskId.getStageId().getId(), taskId.getId(), 0);
        return new GpuOperator(context, handle, outputTypes, new PinnedPagePool(sourceTypes), driverContext.getYieldExecutor());
    }

    @Override
    public synchronized void noMoreOperators()
    {
        if (!closed && pool != 0) {
            GpuNative.destroyUniqueIdPool(pool);   // (the operators created so far share the counter natively)
            pool = 0;
        }
        closed = true;
    }

    @Override
    public OperatorFactory duplicate()
    {
        return new GpuAssignUniqueId(operatorId, planNodeId, sourceTypes, types, params);
    }
}
