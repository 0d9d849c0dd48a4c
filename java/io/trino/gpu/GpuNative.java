/*
 * The native methods of jni/presto_amd_jni.c, one per entry of include/presto_amd.h.  Not compiled in the authoring image
 * (no JDK there); the C side is kept in step with the header by tests/test_lib_cpu.py.
 */
package io.trino.gpu;

import java.nio.ByteBuffer;

final class GpuNative
{
    static {
        System.loadLibrary("presto_amd_jni"); // links libpresto_amd.so
        if (abiVersion() != 10) {
            throw new IllegalStateException("libpresto_amd.so ABI version " + abiVersion() + " != 10");
        }
    }

    private GpuNative() {}

    static native int abiVersion();
    static native void init(int device);
    static native int deviceCount();
    static native ByteBuffer hostMallocPinned(long bytes);
    static native void hostFreePinned(ByteBuffer buffer);

    static native long newExpression(int root, int[] kinds, int[] ops, int[] types, int[] typeParams, int[] channels, int[] isNull, int[] nargs,
            int[] firstArg, long[] longs, double[] doubles, byte[][] strings, int[] args);
    static native void freeExpression(long expression);

    static native long createFilterProject(int[] inputTypes, int[] typeParams, long filter, long[] projections, long minOutputPageBytes,
            int minOutputPageRows, int outputMem);
    /**
     * HashAggregationOperatorFactory's arguments: globalAggregationGroupIds (may be null), groupIdChannel (an index among the group-by
     * columns, -1 = Optional.empty()), produceDefaultOutput, maxPartialMemory in bytes (0 = no early flush of a PARTIAL step),
     * stateFormat 0 = flat state channels, 1 = the reference's own intermediate types (ROW(...) / BIGINT per aggregate).
     */
    static native long createHashAggregation(int[] inputTypes, int[] typeParams, int[] groupByChannels, int[] globalAggregationGroupIds, int hashChannel,
            int groupIdChannel, int step, boolean produceDefaultOutput, int[] aggFns, int[] aggInputs, int[] aggMasks, int[] aggInputTypes,
            int expectedGroups, long maxPartialMemory, int stateFormat, int outputMem);
    /** AggregationOperator: ungrouped aggregates. */
    static native long createAggregation(int[] inputTypes, int step, int[] aggFns, int[] aggInputs, int[] aggMasks, int[] aggInputTypes, int stateFormat,
            int outputMem);
    static native long createOrderBy(int[] inputTypes, int[] outputChannels, int[] sortChannels, int[] sortOrders, int outputMem);
    static native long createDynamicFilterSource(int[] inputTypes, int[] filterChannels, int maxDistinctValues, int minMaxCollectionLimit,
            long maxFilterSizeBytes);
    /** null while the operator has not finished; else long[1 + 6 * channels]: isAll, then per channel kind, valueCount, type, values address, values bytes, offsets address. */
    static native long[] dynamicFilterPoll(long dynamicFilterSourceOperator, int channels);
    /** ScanFilterAndProjectOperator over a page source that stays on the Java side (GpuPageSource: nextPage / loadBlock / close are called back). */
    static native long createScanFilterProject(GpuPageSource pageSource, int[] inputTypes, int[] typeParams, long filter, long[] projections,
            long minOutputPageBytes, int minOutputPageRows, int outputMem);
    /** long[4]: processed positions, materialised bytes, lazy blocks loaded, lazy blocks never loaded. */
    static native long[] scanStats(long scanOperator);
    static native void memorySetLimit(long bytes);
    /** long[3]: bytes held by operators, bytes cached for reuse, the limit. */
    static native long[] memoryStats();
    /** [Scan]FilterAndProject -> (Hash)Aggregation of one pipeline as one device pass; aggregate channels index the projections. */
    static native long createFusedAggregation(int[] inputTypes, int[] typeParams, long filter, long[] projections, int[] projectionTypes,
            int[] groupByChannels, int step, int[] aggFns, int[] aggInputs, int[] aggMasks, int[] aggInputTypes, int expectedGroups, int outputMem);
    static native long createLookupSource();
    static native void destroyLookupSource(long lookupSource);
    static native long createHashBuilder(long bridge, int[] inputTypes, int[] joinChannels, int hashChannel, int[] outputChannels, int expectedPositions);
    static native long createLookupJoin(long bridge, int[] probeTypes, int[] probeJoinChannels, int probeHashChannel, int[] probeOutputChannels,
            int joinType, boolean outputSingleMatch, boolean outer, int outputMem, long filterExpression);
    /** FilterAndProject -> LookupJoin [-> aggregation] of one pipeline behind one handle (aggFns == null: no aggregation). */
    static native long createFusedJoin(long bridge, int[] inputTypes, int[] typeParams, long filter, long[] projections, int[] projectionTypes,
            int[] probeJoinChannels, int[] probeOutputChannels, int[] joinedTypes, int[] groupByChannels, int step, int[] aggFns, int[] aggInputs,
            int[] aggMasks, int[] aggInputTypes, int expectedGroups, int outputMem);
    /** SetBuilderOperator.SetSupplier: the pa_channel_set a semi-join's set builder and probe operators share (GpuSemiJoin). */
    static native long channelSetCreate();
    static native void channelSetDestroy(long channelSet);
    /** SetBuilderOperatorFactory(setChannel, hashChannel, expectedPositions); typeParams may be null. */
    static native long createSetBuilder(long channelSet, int[] inputTypes, int[] typeParams, int setChannel, int hashChannel, int expectedPositions);
    /** HashSemiJoinOperator.createOperatorFactory(probeTypes, probeJoinChannel, probeJoinHashChannel): the probe page plus a BOOLEAN mark. */
    static native long createHashSemiJoin(long channelSet, int[] probeTypes, int[] typeParams, int probeJoinChannel, int probeHashChannel, int outputMem);
    /** NestedLoopJoinBridge: the pa_nested_loop_pages a nested-loop join's builder and join operators share (GpuNestedLoopJoin). */
    static native long createNestedLoopPages();
    static native void destroyNestedLoopPages(long nestedLoopPages);
    /** NestedLoopBuildOperatorFactory; created before the join operators of the same pages (they need the build types); typeParams may be null. */
    static native long createNestedLoopBuild(long nestedLoopPages, int[] inputTypes, int[] typeParams);
    /** NestedLoopJoinOperatorFactory(probeTypes, probeChannels, buildChannels); filterExpression: over [build page channels, probe page
     *  channels], 0 = the plain product.  One row per surviving pair, probe-major. */
    static native long createNestedLoopJoin(long nestedLoopPages, int[] probeTypes, int[] typeParams, int[] probeOutputChannels, int[] buildOutputChannels,
            long filterExpression, int outputMem);
    /** MarkDistinctOperatorFactory(sourceTypes, markDistinctChannels, hashChannel): the input page plus a BOOLEAN mark (GpuDistinct). */
    static native long createMarkDistinct(int[] inputTypes, int[] typeParams, int[] distinctChannels, int hashChannel, int expectedDistinct, int outputMem);
    /** DistinctLimitOperatorFactory(sourceTypes, distinctChannels, limit, hashChannel): the first `limit` distinct keys in arrival order. */
    static native long createDistinctLimit(int[] inputTypes, int[] typeParams, int[] distinctChannels, long limit, int hashChannel, int expectedDistinct, int outputMem);
    /** {distinct keys seen so far, slots of the table} of a MarkDistinct / DistinctLimit operator (GroupByHash.getGroupCount / getCapacity). */
    static native long[] distinctStats(long operator);
    /** StreamingAggregationOperator.createOperatorFactory(sourceTypes, groupByTypes, groupByChannels, step, aggregatorFactories): one row per
     *  run of consecutive rows with one group key; the aggregates as for createHashAggregation (GpuStreamingAggregation). */
    static native long createStreamingAggregation(int[] inputTypes, int[] typeParams, int[] groupByChannels, int step, int[] aggFns, int[] aggInputs,
            int[] aggMasks, int[] aggInputTypes, int outputMem);
    /** The AtomicLong valuePool of AssignUniqueIdOperator's factory: row ids in blocks of 2^20, starting at firstValue (GpuAssignUniqueId). */
    static native long createUniqueIdPool(long firstValue);
    static native void destroyUniqueIdPool(long uniqueIdPool);
    /** AssignUniqueIdOperator: the input page plus a BIGINT id, (stageId << 54) | (taskId << 40) | row id; typeParams may be null. */
    static native long createAssignUniqueId(long uniqueIdPool, int[] inputTypes, int[] typeParams, int stageId, int taskId, int outputMem);
    /** RowNumberOperatorFactory(sourceTypes, outputChannels, partitionChannels, partitionTypes, maxRowsPerPartition, hashChannel, expectedPositions);
     *  maxRowsPerPartition = -1: absent (GpuRowNumber). */
    static native long createRowNumber(int[] inputTypes, int[] typeParams, int[] outputChannels, int[] partitionChannels, long maxRowsPerPartition,
            int hashChannel, int expectedPositions, int outputMem);
    /** {partitions seen so far, slots of the table} of a RowNumber operator (GroupByHash.getGroupCount / getCapacity). */
    static native long[] rowNumberStats(long operator);
    /** TopNRankingOperatorFactory(rankingType, sourceTypes, outputChannels, partitionChannels, partitionTypes, sortChannels, sortOrder,
     *  maxRowCountPerPartition, partial, hashChannel, expectedPositions); rankingType 0 = ROW_NUMBER, 1 = RANK (GpuTopNRanking). */
    static native long createTopNRanking(int rankingType, int[] inputTypes, int[] typeParams, int[] outputChannels, int[] partitionChannels,
            int[] sortChannels, int[] sortOrders, int maxRowCountPerPartition, boolean partial, int hashChannel, int expectedPositions, int outputMem);
    /** {partitions seen so far, slots of the table, rows held right now} of a TopNRanking operator (what getEstimatedSizeInBytes watches). */
    static native long[] topNRankingStats(long operator);
    /** WindowOperatorFactory(sourceTypes, outputChannels, windowFunctionDefinitions, partitionChannels, preGroupedChannels, sortChannels,
     *  sortOrder, preSortedChannelPrefix, expectedPositions) for the ranking functions: functions = pa_window_function ids,
     *  functionArguments = one argument channel per function, -1 where it takes none (GpuWindow). */
    static native long createWindow(int[] inputTypes, int[] typeParams, int[] outputChannels, int[] functions, int[] functionArguments,
            int[] partitionChannels, int[] sortChannels, int[] sortOrders, int preGroupedChannelCount, int preSortedChannelPrefix,
            int expectedPositions, int outputMem);
    /** The same with frames: the ranking functions, count / sum / min / max (ids 6 .. 10) and lag / lead / first_value / last_value /
     *  nth_value (ids 11 .. 15).  frames = six ints per function: frame type, start type, start channel, end type, end channel, ignore
     *  nulls (FrameInfo; pa_framed_window_function_desc).  functionArguments = one channel per function or three, -1 ending a list. */
    static native long createFramedWindow(int[] inputTypes, int[] typeParams, int[] outputChannels, int[] functions, int[] functionArguments,
            int[] frames, int[] partitionChannels, int[] sortChannels, int[] sortOrders, int preGroupedChannelCount, int preSortedChannelPrefix,
            int expectedPositions, int outputMem);
    static native long createTopN(int[] inputTypes, int count, int[] sortChannels, int[] sortOrders, int outputMem);
    static native boolean setDynamicFilter(long filterProjectOperator, int channel, long lookupSource);

    /** The only consumer of the aggregation's output is TopNOperator(n, sortChannels, sortOrders): groups that cannot be among its n best rows may be left out. */
    static native boolean setOutputTopNHint(long aggregationOperator, long n, int[] sortChannels, int[] sortOrders);

    static native void commUniqueId(byte[] out128);
    static native long commCreate(byte[] id128, int rank, int world);
    static native void commDestroy(long comm);
    static native long exchangeCreate(long comm, int[] types, int[] partitionChannels, int hashChannel, int sinkCount);
    static native void exchangeDestroy(long exchange);
    static native long createPartitionedOutput(long exchange);
    static native long createExchangeSource(long exchange, int outputMem);

    static native boolean needsInput(long operator);
    static native boolean isBlocked(long operator);
    static native boolean isFinished(long operator);
    static native void finish(long operator);
    static native void close(long operator);
    static native long memoryBytes(long operator);
    /**
     * retention: 0 = the slab may be reused when the call returns; 1 = it is kept until the operator is closed; 2 = it is kept until the
     * operator releases the page -- releaseToken then shows up in drainReleased.
     */
    static native void addInput(long operator, int positions, int channels, int[] types, int[] encodings, long[] valueOffsets, long[] offsetOffsets,
            long[] nullOffsets, long[] idOffsets, int[] dictionaryChannel, int[] dictionarySize, ByteBuffer pinned, int retention, long releaseToken);
    /** Moves up to out.length tokens of released pages into out; returns how many. */
    static native int drainReleased(long[] out);
    /** The operator's next output page as a SerializedPage frame in `out` (0 = no page); works for operators with device output. */
    static native long getOutputSerialized(long operator, ByteBuffer out, boolean compress);
    /** A SerializedPage frame decoded on the device and handed to the operator as its next input page. */
    static native void addInputSerialized(long operator, ByteBuffer frame, long size, int[] expectedTypes);
    static native long[] getOutput(long operator);
    static native ByteBuffer wrapAddress(long address, long bytes);
    static native long bufferAddress(ByteBuffer directBuffer);
}
