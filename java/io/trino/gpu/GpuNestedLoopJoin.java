package io.trino.gpu;

import io.trino.operator.OperatorFactory;
import io.trino.spi.type.Type;
import io.trino.sql.planner.plan.PlanNodeId;
import io.trino.sql.relational.RowExpression;

import java.util.ArrayList;
import java.util.List;
import java.util.Optional;
import java.util.concurrent.atomic.AtomicInteger;

/**
 * LocalExecutionPlanner.createNestedLoopJoin (core/trino-main/src/main/java/io/trino/sql/planner/LocalExecutionPlanner.java: a JoinNode
 * without equi-criteria -- CROSS JOIN, an uncorrelated scalar subquery, an inner join over an inequality alone) on the device: called in
 * place of `new NestedLoopBuildOperatorFactory(...)` and `new NestedLoopJoinOperatorFactory(...)`.  Both factories share one
 * pa_nested_loop_pages (the NestedLoopJoinBridge); it is destroyed when the last factory had noMoreOperators (the operators already
 * created hold the rows natively).  The build factory's operator must be created before the join factory's: the join needs the build
 * types to check and compile its filter -- the build pipeline of a join is planned and started first.
 *
 * The filter.  When the next factory of the probe pipeline is a FilterAndProject whose filter RowExpressionSerializer can serialise,
 * the planner hook passes that filter here: it is renumbered from the join's OUTPUT layout [probe output channels, build output
 * channels] to the PAIR layout of pa_nested_loop_join_desc.filter [build page channels, probe page channels] and moved into the join,
 * which then emits only the surviving pairs; the FilterAndProject keeps its projections and loses its filter (`filterMoved`).  A filter
 * the serialiser does not cover stays where it is, above a join that emits the plain product.
 *
 * Optional.empty() when the device path does not take the shape (a type RowExpressionSerializer has no code for, no output channel at
 * all): the planner keeps the reference factories.  The output order is probe-major, not the reference's; no consumer may rely on the
 * order of a cross join.
 */
public final class GpuNestedLoopJoin
{
    public final OperatorFactory build;
    public final OperatorFactory join;
    /** the FilterAndProject above the join is to be created without its filter: the join evaluates it */
    public final boolean filterMoved;

    private GpuNestedLoopJoin(OperatorFactory build, OperatorFactory join, boolean filterMoved)
    {
        this.build = build;
        this.join = join;
        this.filterMoved = filterMoved;
    }

    public static Optional<GpuNestedLoopJoin> create(int buildOperatorId, PlanNodeId buildNodeId, List<Type> buildTypes, int joinOperatorId, PlanNodeId joinNodeId,
            List<Type> probeTypes, List<Integer> probeChannels, List<Integer> buildChannels, Optional<RowExpression> filterAbove)
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
        if (probeChannels.isEmpty() && buildChannels.isEmpty()) {
            return Optional.empty();   // position-count-only pages are not modelled (PA_ERR_NOT_SUPPORTED)
        }
        int[] probeOut = probeChannels.stream().mapToInt(Integer::intValue).toArray();
        int[] buildOut = buildChannels.stream().mapToInt(Integer::intValue).toArray();
        // output channel k of the join -> channel of the pair: probe channel c is B + c, build channel c is c
        int[] outputToPair = new int[probeOut.length + buildOut.length];
        for (int k = 0; k < probeOut.length; k++) {
            outputToPair[k] = build.length + probeOut[k];
        }
        for (int k = 0; k < buildOut.length; k++) {
            outputToPair[probeOut.length + k] = buildOut[k];
        }
        long filter = 0;
        if (filterAbove.isPresent()) {
            try {
                filter = RowExpressionSerializer.serialize(filterAbove.get(), outputToPair);
            }
            catch (RuntimeException unsupported) {
                filter = 0;   // the filter stays in the FilterAndProject, the join emits the product
            }
        }
        long pairFilter = filter;
        long pages = GpuNative.createNestedLoopPages();
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
                    GpuNative.destroyNestedLoopPages(pages);
                    if (pairFilter != 0) {
                        GpuNative.freeExpression(pairFilter);
                    }
                }
            }
        };
        List<Type> outputTypes = new ArrayList<>();
        for (int c : probeOut) {
            outputTypes.add(probeTypes.get(c));
        }
        for (int c : buildOut) {
            outputTypes.add(buildTypes.get(c));
        }
        OperatorFactory builder = new GpuOperatorFactory(buildOperatorId, buildNodeId, "GpuNestedLoopBuildOperator", buildTypes, List.of(),
                () -> GpuNative.createNestedLoopBuild(pages, build, buildParams), shared);
        OperatorFactory joiner = new GpuOperatorFactory(joinOperatorId, joinNodeId, "GpuNestedLoopJoinOperator", probeTypes, outputTypes,
                () -> GpuNative.createNestedLoopJoin(pages, probe, probeParams, probeOut, buildOut, pairFilter, 0), shared);
        return Optional.of(new GpuNestedLoopJoin(builder, joiner, pairFilter != 0));
    }
}
