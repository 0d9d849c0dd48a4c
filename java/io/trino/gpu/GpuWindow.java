package io.trino.gpu;

import io.trino.operator.OperatorFactory;
import io.trino.spi.connector.SortOrder;
import io.trino.spi.type.BigintType;
import io.trino.spi.type.DoubleType;
import io.trino.spi.type.Type;
import io.trino.sql.planner.plan.PlanNodeId;

import java.util.ArrayList;
import java.util.List;
import java.util.Locale;
import java.util.Optional;

/**
 * LocalExecutionPlanner.visitWindow on the device: called in place of `new WindowOperator.WindowOperatorFactory(...)` with the names of
 * the node's window functions (the resolved signature names) and their argument channels.  Optional.empty() when the device path does
 * not take the shape, and the planner keeps the reference factory: any function but the six ranking functions (they ignore frames;
 * lag / lead / first_value / last_value / nth_value and aggregates do not and have no id in the library), pre-grouped or pre-sorted
 * input, pattern recognition measures, more than 16 functions or 8 partition channels, partition / sort channels of long decimals or
 * rows, row output channels, an ntile argument that is not BIGINT / INTEGER.  Peers are found with IS NOT DISTINCT FROM as in
 * RegularWindowPartition: -0.0 and +0.0 in a sort channel are peers (include/presto_amd.h).
 */
public final class GpuWindow
{
    // pa_type codes and pa_window_function ids (include/presto_amd.h), and the library's caps
    private static final int PA_BIGINT = 0, PA_INTEGER = 1, PA_ROW = 6, PA_LONG_DECIMAL = 9;
    private static final int PA_WINDOW_ROW_NUMBER = 0, PA_WINDOW_RANK = 1, PA_WINDOW_DENSE_RANK = 2, PA_WINDOW_PERCENT_RANK = 3,
            PA_WINDOW_CUME_DIST = 4, PA_WINDOW_NTILE = 5;
    private static final int MAX_FUNCTIONS = 16;
    private static final int MAX_PARTITION_CHANNELS = 8;
    private static final int MAX_CHANNELS = 64;

    private GpuWindow() {}

    /** pa_window_function of a window function name, or -1: not one the device path takes */
    static int functionOf(String name)
    {
        switch (name.toLowerCase(Locale.ENGLISH)) {
            case "row_number":
                return PA_WINDOW_ROW_NUMBER;
            case "rank":
                return PA_WINDOW_RANK;
            case "dense_rank":
                return PA_WINDOW_DENSE_RANK;
            case "percent_rank":
                return PA_WINDOW_PERCENT_RANK;
            case "cume_dist":
                return PA_WINDOW_CUME_DIST;
            case "ntile":
                return PA_WINDOW_NTILE;
            default:
                return -1;
        }
    }

    public static Optional<OperatorFactory> window(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, List<Integer> outputChannels,
            List<String> functionNames, List<List<Integer>> functionArgumentChannels, List<Integer> partitionChannels,
            List<Integer> preGroupedChannels, List<Integer> sortChannels, List<SortOrder> sortOrders, int preSortedChannelPrefix,
            int expectedPositions, List<Type> measureTypes)
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
        if (types.length == 0 || types.length > MAX_CHANNELS || functionNames.isEmpty() || functionNames.size() > MAX_FUNCTIONS
                || functionNames.size() != functionArgumentChannels.size() || partitionChannels.size() > MAX_PARTITION_CHANNELS
                || sortChannels.size() != sortOrders.size() || !preGroupedChannels.isEmpty() || preSortedChannelPrefix != 0
                || !measureTypes.isEmpty()) {
            return Optional.empty();
        }
        int[] functions = new int[functionNames.size()];
        int[] arguments = new int[functionNames.size()];
        List<Type> output = new ArrayList<>();
        for (int channel : outputChannels) {
            if (types[channel] == PA_ROW) {
                return Optional.empty();
            }
            output.add(sourceTypes.get(channel));
        }
        for (int i = 0; i < functions.length; i++) {
            functions[i] = functionOf(functionNames.get(i));
            List<Integer> args = functionArgumentChannels.get(i);
            if (functions[i] < 0 || args.size() != (functions[i] == PA_WINDOW_NTILE ? 1 : 0)) {
                return Optional.empty();
            }
            arguments[i] = args.isEmpty() ? -1 : args.get(0);
            if (arguments[i] >= 0 && types[arguments[i]] != PA_BIGINT && types[arguments[i]] != PA_INTEGER) {
                return Optional.empty();
            }
            boolean real = functions[i] == PA_WINDOW_PERCENT_RANK || functions[i] == PA_WINDOW_CUME_DIST;
            output.add(real ? DoubleType.DOUBLE : BigintType.BIGINT);
        }
        for (int channel : partitionChannels) {
            if (types[channel] == PA_ROW || types[channel] == PA_LONG_DECIMAL) {
                return Optional.empty();
            }
        }
        for (int channel : sortChannels) {
            if (types[channel] == PA_ROW || types[channel] == PA_LONG_DECIMAL) {
                return Optional.empty();
            }
        }
        int[] out = outputChannels.stream().mapToInt(Integer::intValue).toArray();
        int[] partition = partitionChannels.stream().mapToInt(Integer::intValue).toArray();
        int[] sort = sortChannels.stream().mapToInt(Integer::intValue).toArray();
        int[] orders = sortOrders.stream().mapToInt(SortOrder::ordinal).toArray();   // ASC_NULLS_FIRST, ASC_NULLS_LAST, DESC_NULLS_FIRST, DESC_NULLS_LAST
        int expected = Math.max(expectedPositions, 0);
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuWindowOperator", sourceTypes, output,
                () -> GpuNative.createWindow(types, params, out, functions, arguments, partition, sort, orders, 0, 0, expected, 0)));
    }
}
