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
 *
 * The overload that also takes each function's frame (the FrameInfo fields) goes through pa_framed_window_create and takes count(*) /
 * count(x) / sum(x) / min(x) / max(x) and lag / lead / first_value / last_value / nth_value next to the ranking functions, over the
 * frames UNBOUNDED PRECEDING .. CURRENT ROW (ROWS, RANGE, GROUPS) and UNBOUNDED PRECEDING .. UNBOUNDED FOLLOWING (lag and lead ignore
 * their frame).  It is empty for every other frame of an aggregate or of first_value / last_value / nth_value, for IGNORE NULLS, for sum
 * over anything but BIGINT / INTEGER, for min / max over VARCHAR, long decimals or rows, for a value function over VARCHAR or rows, with
 * an offset that is not BIGINT / INTEGER or a default of another type than the value, and for any other function (avg).
 */
public final class GpuWindow
{
    // pa_type codes and pa_window_function ids (include/presto_amd.h), and the library's caps
    private static final int PA_BIGINT = 0, PA_INTEGER = 1, PA_ROW = 6, PA_LONG_DECIMAL = 9;
    private static final int PA_WINDOW_ROW_NUMBER = 0, PA_WINDOW_RANK = 1, PA_WINDOW_DENSE_RANK = 2, PA_WINDOW_PERCENT_RANK = 3,
            PA_WINDOW_CUME_DIST = 4, PA_WINDOW_NTILE = 5;
    private static final int PA_DATE = 2, PA_DOUBLE = 3, PA_BOOLEAN = 4, PA_REAL = 7, PA_DECIMAL = 8;
    private static final int PA_WINDOW_COUNT_STAR = 6, PA_WINDOW_COUNT = 7, PA_WINDOW_SUM = 8, PA_WINDOW_MIN = 9, PA_WINDOW_MAX = 10;
    private static final int PA_VARCHAR = 5;
    private static final int PA_WINDOW_LAG = 11, PA_WINDOW_LEAD = 12, PA_WINDOW_FIRST_VALUE = 13, PA_WINDOW_LAST_VALUE = 14, PA_WINDOW_NTH_VALUE = 15;
    // pa_window_frame_type = WindowFrameType.ordinal(), pa_window_frame_bound = FrameBoundType.ordinal()
    private static final int PA_BOUND_UNBOUNDED_PRECEDING = 0, PA_BOUND_CURRENT_ROW = 2, PA_BOUND_UNBOUNDED_FOLLOWING = 4;
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

    /** One window function's FrameInfo: getType().ordinal() (RANGE, ROWS, GROUPS), getStartType().ordinal() / getEndType().ordinal()
     *  (UNBOUNDED_PRECEDING, PRECEDING, CURRENT_ROW, FOLLOWING, UNBOUNDED_FOLLOWING), getStartChannel() / getEndChannel() (-1: none). */
    public static final class Frame
    {
        final int type, startType, startChannel, endType, endChannel;

        public Frame(int type, int startType, int startChannel, int endType, int endChannel)
        {
            this.type = type;
            this.startType = startType;
            this.startChannel = startChannel;
            this.endType = endType;
            this.endChannel = endChannel;
        }
    }

    /** pa_window_function of an aggregate window function by name and argument count, or -1 */
    static int aggregateOf(String name, int argumentCount)
    {
        switch (name.toLowerCase(Locale.ENGLISH)) {
            case "count":
                return argumentCount == 0 ? PA_WINDOW_COUNT_STAR : argumentCount == 1 ? PA_WINDOW_COUNT : -1;
            case "sum":
                return argumentCount == 1 ? PA_WINDOW_SUM : -1;
            case "min":
                return argumentCount == 1 ? PA_WINDOW_MIN : -1;
            case "max":
                return argumentCount == 1 ? PA_WINDOW_MAX : -1;
            default:
                return -1;
        }
    }

    /** pa_window_function of a value window function by name and argument count, or -1 */
    static int valueFunctionOf(String name, int argumentCount)
    {
        switch (name.toLowerCase(Locale.ENGLISH)) {
            case "lag":
                return argumentCount >= 1 && argumentCount <= 3 ? PA_WINDOW_LAG : -1;
            case "lead":
                return argumentCount >= 1 && argumentCount <= 3 ? PA_WINDOW_LEAD : -1;
            case "first_value":
                return argumentCount == 1 ? PA_WINDOW_FIRST_VALUE : -1;
            case "last_value":
                return argumentCount == 1 ? PA_WINDOW_LAST_VALUE : -1;
            case "nth_value":
                return argumentCount == 2 ? PA_WINDOW_NTH_VALUE : -1;
            default:
                return -1;
        }
    }

    /** the window node with each function's frame, whether it ignores NULLs, and its argument types (which the channels' types repeat) */
    public static Optional<OperatorFactory> window(int operatorId, PlanNodeId planNodeId, List<Type> sourceTypes, List<Integer> outputChannels,
            List<String> functionNames, List<List<Integer>> functionArgumentChannels, List<List<Type>> functionArgumentTypes, List<Frame> frames,
            List<Boolean> ignoreNulls, List<Integer> partitionChannels, List<Integer> preGroupedChannels, List<Integer> sortChannels,
            List<SortOrder> sortOrders, int preSortedChannelPrefix, int expectedPositions, List<Type> measureTypes)
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
        int count = functionNames.size();
        if (types.length == 0 || types.length > MAX_CHANNELS || count == 0 || count > MAX_FUNCTIONS || count != functionArgumentChannels.size()
                || count != functionArgumentTypes.size() || count != frames.size() || count != ignoreNulls.size()
                || partitionChannels.size() > MAX_PARTITION_CHANNELS || sortChannels.size() != sortOrders.size() || !preGroupedChannels.isEmpty()
                || preSortedChannelPrefix != 0 || !measureTypes.isEmpty()) {
            return Optional.empty();
        }
        int[] functions = new int[count];
        int[] arguments = new int[3 * count];   // three channels per function: value / argument, offset, default; -1 ends the list
        java.util.Arrays.fill(arguments, -1);
        int[] frameWords = new int[6 * count];
        List<Type> output = new ArrayList<>();
        for (int channel : outputChannels) {
            if (types[channel] == PA_ROW) {
                return Optional.empty();
            }
            output.add(sourceTypes.get(channel));
        }
        for (int i = 0; i < count; i++) {
            List<Integer> args = functionArgumentChannels.get(i);
            Frame frame = frames.get(i);
            int value = valueFunctionOf(functionNames.get(i), args.size());
            if (args.size() != functionArgumentTypes.get(i).size() || args.size() > (value >= 0 ? 3 : 1) || ignoreNulls.get(i)) {
                return Optional.empty();
            }
            for (int k = 0; k < args.size(); k++) {
                arguments[3 * i + k] = args.get(k);
            }
            int argument = args.isEmpty() ? -1 : types[arguments[3 * i]];
            functions[i] = functionOf(functionNames.get(i));
            if (value >= 0) {
                functions[i] = value;
                boolean shift = value == PA_WINDOW_LAG || value == PA_WINDOW_LEAD;
                boolean prefix = frame.startType == PA_BOUND_UNBOUNDED_PRECEDING
                        && (frame.endType == PA_BOUND_CURRENT_ROW || frame.endType == PA_BOUND_UNBOUNDED_FOLLOWING);
                if (argument == PA_VARCHAR || argument == PA_ROW || (!shift && !prefix)) {
                    return Optional.empty();
                }
                if (args.size() >= 2 && types[args.get(1)] != PA_BIGINT && types[args.get(1)] != PA_INTEGER) {
                    return Optional.empty();
                }
                if (args.size() == 3 && (types[args.get(2)] != argument || params[args.get(2)] != params[args.get(0)])) {
                    return Optional.empty();
                }
                output.add(sourceTypes.get(args.get(0)));
            }
            else if (functions[i] >= 0) {
                // a ranking function: the frame is passed on and ignored
                if (args.size() != (functions[i] == PA_WINDOW_NTILE ? 1 : 0) || (argument >= 0 && argument != PA_BIGINT && argument != PA_INTEGER)) {
                    return Optional.empty();
                }
                boolean real = functions[i] == PA_WINDOW_PERCENT_RANK || functions[i] == PA_WINDOW_CUME_DIST;
                output.add(real ? DoubleType.DOUBLE : BigintType.BIGINT);
            }
            else {
                functions[i] = aggregateOf(functionNames.get(i), args.size());
                boolean prefix = frame.startType == PA_BOUND_UNBOUNDED_PRECEDING
                        && (frame.endType == PA_BOUND_CURRENT_ROW || frame.endType == PA_BOUND_UNBOUNDED_FOLLOWING);
                if (functions[i] < 0 || !prefix) {
                    return Optional.empty();
                }
                switch (functions[i]) {
                    case PA_WINDOW_COUNT:
                        if (argument == PA_ROW) {
                            return Optional.empty();
                        }
                        break;
                    case PA_WINDOW_SUM:
                        if (argument != PA_BIGINT && argument != PA_INTEGER) {
                            return Optional.empty();
                        }
                        break;
                    case PA_WINDOW_MIN:
                    case PA_WINDOW_MAX:
                        if (argument != PA_BIGINT && argument != PA_INTEGER && argument != PA_DATE && argument != PA_BOOLEAN && argument != PA_DECIMAL
                                && argument != PA_DOUBLE && argument != PA_REAL) {
                            return Optional.empty();
                        }
                        break;
                    default:
                        break;
                }
                boolean minMax = functions[i] == PA_WINDOW_MIN || functions[i] == PA_WINDOW_MAX;
                output.add(minMax ? sourceTypes.get(arguments[3 * i]) : BigintType.BIGINT);
            }
            frameWords[6 * i] = frame.type;
            frameWords[6 * i + 1] = frame.startType;
            frameWords[6 * i + 2] = frame.startChannel;
            frameWords[6 * i + 3] = frame.endType;
            frameWords[6 * i + 4] = frame.endChannel;
            frameWords[6 * i + 5] = 0;
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
        int[] orders = sortOrders.stream().mapToInt(SortOrder::ordinal).toArray();
        int expected = Math.max(expectedPositions, 0);
        return Optional.of(new GpuOperatorFactory(operatorId, planNodeId, "GpuWindowOperator", sourceTypes, output,
                () -> GpuNative.createFramedWindow(types, params, out, functions, arguments, frameWords, partition, sort, orders, 0, 0, expected, 0)));
    }
}
