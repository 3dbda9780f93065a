"""ctypes declarations of the C ABI in include/evql_gpu.h.

Only struct layouts and constants live here; loading libevql_mi355x.so is done
in eventql_amd/__init__.py.
"""
import ctypes as C

# evql_status
EVQL_OK = 0
EVQL_EIO = -1
EVQL_EARG = -2
EVQL_ERUNTIME = -3
EVQL_ENOTSUP = -4
EVQL_EDEVICE = -5
EVQL_ENOMEM = -6

# evql_stype (csql::SType, sql/svalue.h:41-49)
T_NIL, T_UINT64, T_INT64, T_FLOAT64, T_BOOL, T_STRING, T_TIMESTAMP64 = range(7)
STAG_NULL = 1

# cstable column types / encodings (io/cstable/cstable.h:113-131)
COL_SUBRECORD, COL_BOOLEAN, COL_UNSIGNED_INT, COL_SIGNED_INT, COL_STRING, \
    COL_FLOAT, COL_DATETIME = range(7)
ENC_BOOLEAN_BITPACKED = 1
ENC_UINT32_BITPACKED = 10
ENC_UINT32_PLAIN = 11
ENC_UINT64_PLAIN = 12
ENC_UINT64_LEB128 = 13
ENC_FLOAT_IEEE754 = 14
ENC_STRING_PLAIN = 100

# opcodes (runtime/vm.h:44-52)
X_CALL_PURE, X_CALL_INSTANCE, X_LITERAL, X_INPUT, X_JUMP, X_CJUMP, X_RETURN = \
    range(1, 8)

# type slots / function families
TS_UINT64, TS_INT64, TS_FLOAT64, TS_BOOL, TS_STRING, TS_TIMESTAMP64, TS_NIL = \
    range(7)
(FAM_LOGICAL_AND, FAM_LOGICAL_OR, FAM_NEG, FAM_CMP, FAM_EQ, FAM_NEQ, FAM_LT,
 FAM_LTE, FAM_GT, FAM_GTE, FAM_ADD, FAM_SUB, FAM_MUL, FAM_DIV, FAM_MOD, FAM_POW,
 FAM_TO_NIL, FAM_TO_INT64, FAM_TO_TIMESTAMP64, FAM_TO_STRING, FAM_CONCAT, FAM_LCASE, FAM_UCASE,
 FAM_SUBSTRING, FAM_LTRIM, FAM_RTRIM, FAM_STARTSWITH, FAM_ENDSWITH) = range(1, 29)


def FN(family, type_slot):
    return family * 16 + type_slot


(AGG_NONE, AGG_COUNT, AGG_SUM_UINT64, AGG_SUM_INT64, AGG_SUM_FLOAT64,
 AGG_MIN_UINT64, AGG_MAX_UINT64, AGG_MIN_INT64, AGG_MAX_INT64, AGG_MIN_FLOAT64,
 AGG_MAX_FLOAT64, AGG_MEAN_UINT64, AGG_MEAN_INT64, AGG_MEAN_FLOAT64,
 AGG_COUNT_DISTINCT_UINT64) = range(15)

INSTANCE_ACCUMULATE = 1
INSTANCE_GET = 2

MODE_FINAL, MODE_PARTIAL = 0, 1
SCAN_FLAT, SCAN_NESTED, SCAN_NESTED_WITHIN_RECORD = 0, 1, 2


class Instr(C.Structure):
    _fields_ = [("op", C.c_uint32), ("argt", C.c_uint32), ("arg0", C.c_int64)]


class Program(C.Structure):
    _fields_ = [
        ("code", C.POINTER(Instr)),
        ("code_len", C.c_uint32),
        ("method_call", C.c_uint32),
        ("method_accumulate", C.c_uint32),
        ("return_type", C.c_uint32),
        ("aggregate_fn", C.c_uint32),
        ("static_storage", C.POINTER(C.c_uint8)),
        ("static_storage_len", C.c_size_t),
    ]


class PlanDesc(C.Structure):
    _fields_ = [
        ("scan_columns", C.POINTER(C.c_char_p)),
        ("scan_column_types", C.POINTER(C.c_uint32)),
        ("n_scan_columns", C.c_uint32),
        ("where", C.POINTER(Program)),
        ("scan_select", C.POINTER(Program)),
        ("n_scan_select", C.c_uint32),
        ("group_exprs", C.POINTER(Program)),
        ("n_group", C.c_uint32),
        ("select_exprs", C.POINTER(Program)),
        ("n_select", C.c_uint32),
        ("row_filter_bits", C.POINTER(C.c_uint8)),
        ("row_filter_len", C.c_uint64),
        ("group_mode", C.c_uint32),
        ("scan_mode", C.c_uint32),
        ("groups_hint", C.c_uint64),
        ("row_begin", C.c_uint64),
        ("row_end", C.c_uint64),
        ("float_sum_mode", C.c_uint32),
        ("float_sum_bound", C.c_double),
    ]


class ColumnInfo(C.Structure):
    _fields_ = [
        ("name", C.c_char * 256),
        ("logical_type", C.c_int32),
        ("storage_type", C.c_int32),
        ("column_id", C.c_uint64),
        ("rlevel_max", C.c_uint32),
        ("dlevel_max", C.c_uint32),
        ("n_data_pages", C.c_uint32),
        ("n_rlevel_pages", C.c_uint32),
        ("n_dlevel_pages", C.c_uint32),
        ("payload_bytes", C.c_uint64),
    ]


class SynthSpec(C.Structure):
    _fields_ = [
        ("num_rows", C.c_uint64),
        ("seed", C.c_uint64),
        ("k_mod", C.c_uint64),
        ("u_mod", C.c_uint64),
        ("columns", C.c_uint32),
        ("k_bits", C.c_uint32),
    ]


class ColumnSpec(C.Structure):
    _fields_ = [
        ("name", C.c_char_p),
        ("logical_type", C.c_int32),
        ("storage_type", C.c_int32),
        ("column_id", C.c_uint64),
        ("rlevel_max", C.c_uint32),
        ("dlevel_max", C.c_uint32),
        ("bitpack_max_value", C.c_uint32),
    ]


class DeviceColumn(C.Structure):
    _fields_ = [("values", C.c_void_p), ("nulls", C.c_void_p), ("bytes", C.c_void_p),
                ("rlevels", C.c_void_p), ("dlevels", C.c_void_p), ("num_slots", C.c_uint64)]


class ColumnBuf(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_uint8)), ("size", C.c_size_t)]


class SortSpec(C.Structure):
    _fields_ = [("expr", Program), ("descending", C.c_uint32)]


class QueryStats(C.Structure):
    _fields_ = [
        ("rows_scanned", C.c_uint64),
        ("rows_passed", C.c_uint64),
        ("num_groups", C.c_uint64),
        ("algorithmic_bytes", C.c_uint64),
        ("kernel_ms", C.c_double),
        ("total_ms", C.c_double),
        ("n_kernel_launches", C.c_uint32),
        ("used_lds_table", C.c_uint32),
        ("estimated_groups", C.c_uint64),
    ]


class ZoneStats(C.Structure):
    """evql_zone_stats_t"""
    _fields_ = [
        ("conjuncts_used", C.c_uint32),
        ("zone_rows", C.c_uint32),
        ("zones_total", C.c_uint64),
        ("zones_excluded", C.c_uint64),
        ("tile_rows", C.c_uint64),
        ("tiles_total", C.c_uint64),
        ("tiles_skipped", C.c_uint64),
    ]


class MergeStats(C.Structure):
    """evql_merge_stats_t"""
    _fields_ = [
        ("on_device", C.c_uint32),
        ("packed_on_device", C.c_uint32),
        ("frames", C.c_uint64),
        ("rows_added", C.c_uint64),
        ("rows_pending", C.c_uint64),
        ("groups", C.c_uint64),
        ("compactions", C.c_uint64),
        ("sort_passes", C.c_uint64),
        ("prefix_collisions", C.c_uint64),
        ("full_key_sorts", C.c_uint64),
        ("device_bytes", C.c_uint64),
        ("host_index_ms", C.c_double),
        ("upload_ms", C.c_double),
        ("merge_ms", C.c_double),
        ("pack_ms", C.c_double),
    ]


class EmitStats(C.Structure):
    """evql_emit_stats_t"""
    _fields_ = [
        ("device_packed", C.c_uint32),
        ("partial", C.c_uint32),
        ("rows", C.c_uint64),
        ("key_bytes", C.c_uint64),
        ("data_bytes", C.c_uint64),
        ("n_kernel_launches", C.c_uint32),
        ("n_host_waits", C.c_uint32),
        ("pack_ms", C.c_double),
    ]


# *decision of evql_plan_partial_emit
PEMIT_DEVICE, PEMIT_NOT_PARTIAL, PEMIT_FEW_GROUPS, PEMIT_SWITCHED_OFF, PEMIT_GROUP_EXPR = range(5)
PEMIT_SELECT_EXPR, PEMIT_AGGREGATE, PEMIT_TOO_WIDE, PEMIT_NIL_COLUMN, PEMIT_NESTED = range(5, 10)
DEVICE_EMIT_MIN_GROUPS = 1 << 16


def bind_partial_emit(lib):
    """declares evql_query_emit_stats, evql_ctx_sha1_ranges and evql_plan_partial_emit"""
    lib.evql_query_emit_stats.argtypes = [C.c_void_p, C.POINTER(EmitStats)]
    lib.evql_ctx_sha1_ranges.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t,
                                         C.POINTER(C.c_uint64), C.c_size_t, C.c_char_p]
    lib.evql_plan_partial_emit.argtypes = [C.POINTER(PlanDesc), C.POINTER(ColumnInfo), C.c_int,
                                           C.c_uint64, C.c_int, C.POINTER(C.c_int)]


class OrderStats(C.Structure):
    """evql_order_stats_t"""
    _fields_ = [
        ("sorted_on_device", C.c_uint32),
        ("decision", C.c_uint32),
        ("records", C.c_uint64),
        ("rows", C.c_uint64),
        ("n_keys", C.c_uint32),
        ("n_sort_passes", C.c_uint32),
        ("n_passes_skipped", C.c_uint32),
        ("n_kernel_launches", C.c_uint32),
        ("n_host_waits", C.c_uint32),
        ("sort_ms", C.c_double),
    ]


# *decision of evql_plan_order_sort / OrderStats.decision
OSORT_DEVICE, OSORT_NO_ORDER, OSORT_FEW_RECORDS, OSORT_SWITCHED_OFF, OSORT_EXPRESSION = range(5)
OSORT_UNREADABLE, OSORT_TOO_MANY_SPECS, OSORT_TOO_MANY_RECORDS, OSORT_NAN_KEY = range(5, 9)
ORDER_SORT_MAX_SPECS = 8


def bind_order_sort(lib):
    """declares evql_query_order_stats and evql_plan_order_sort"""
    lib.evql_query_order_stats.argtypes = [C.c_void_p, C.POINTER(OrderStats)]
    lib.evql_plan_order_sort.argtypes = [C.POINTER(PlanDesc), C.POINTER(ColumnInfo), C.c_int,
                                         C.POINTER(SortSpec), C.c_uint32, C.c_uint64,
                                         C.POINTER(C.c_int)]


class KernelCacheStats(C.Structure):
    _fields_ = [
        ("memory_hits", C.c_uint64),
        ("disk_hits", C.c_uint64),
        ("compiles", C.c_uint64),
        ("compile_ms", C.c_double),
    ]


class PartialView(C.Structure):
    _fields_ = [
        ("device_words", C.c_void_p),
        ("capacity", C.c_uint64),
        ("words_per_group", C.c_uint32),
        ("num_groups", C.c_uint64),
    ]


HEARTBEAT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)


class ExchangeStats(C.Structure):
    _fields_ = [("groups_sent", C.c_uint64), ("groups_received", C.c_uint64),
                ("bytes_sent", C.c_uint64), ("export_ms", C.c_double),
                ("transfer_ms", C.c_double), ("merge_ms", C.c_double),
                ("merge_buckets", C.c_uint64)]


EXCHANGE_GATHER_ALL = 0
EXCHANGE_BY_OWNER = 1
LSM_HAS_SKIPLIST, LSM_HAS_UPDATES = 1, 2

# evql_transport_t callbacks
ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64,
                            C.POINTER(C.c_uint64))
ALL_TO_ALL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p,
                            C.POINTER(C.c_uint64), C.c_void_p)


class Transport(C.Structure):
    _fields_ = [("user", C.c_void_p), ("all_gather_u64", ALL_GATHER_FN),
                ("all_to_all_words", ALL_TO_ALL_FN), ("name", C.c_char_p)]

PAGE_ORDER_COLUMNS, PAGE_ORDER_ROWS = 0, 1

# evql_compact_order_t
COMPACT_SCAN_ORDER, COMPACT_FILE_ORDER = 0, 1


class CompactStats(C.Structure):
    """evql_compact_stats_t"""
    _fields_ = [("rows_in", C.c_uint64), ("rows_written", C.c_uint64),
                ("string_bytes", C.c_uint64), ("n_tables", C.c_uint32),
                ("n_kernel_launches", C.c_uint32), ("n_host_waits", C.c_uint32),
                ("gather_ms", C.c_float), ("encode_ms", C.c_float)]


def bind_chain_compact(lib):
    """declares evql_lsm_chain_compact on the loaded library"""
    lib.evql_lsm_chain_compact.restype = C.c_int
    lib.evql_lsm_chain_compact.argtypes = [C.c_void_p, C.POINTER(ColumnSpec), C.c_int, C.c_int,
                                           C.c_int, C.POINTER(C.c_void_p), C.POINTER(CompactStats)]


# pairs per workgroup of the k_sort_* kernels (kSortTile, csrc/aot_kernels.h)
COMPACT_SORT_TILE = 2048


class CompactSortStats(C.Structure):
    """evql_compact_sort_stats_t"""
    _fields_ = [("rows", C.c_uint64), ("key_min", C.c_uint64), ("key_max", C.c_uint64),
                ("presorted", C.c_uint32), ("passes", C.c_uint32),
                ("n_kernel_launches", C.c_uint32), ("n_host_waits", C.c_uint32),
                ("sort_ms", C.c_float), ("permute_ms", C.c_float)]


def bind_chain_compact_sorted(lib):
    """declares evql_lsm_chain_compact_sorted on the loaded library"""
    lib.evql_lsm_chain_compact_sorted.restype = C.c_int
    lib.evql_lsm_chain_compact_sorted.argtypes = [
        C.c_void_p, C.POINTER(ColumnSpec), C.c_int, C.c_char_p, C.c_int, C.c_int,
        C.POINTER(C.c_void_p), C.POINTER(CompactStats), C.POINTER(CompactSortStats)]


# *decision of evql_plan_materialize
(MAT_DEVICE, MAT_PARTIAL_MODE, MAT_COLUMN_COUNT, MAT_NESTED_SPEC, MAT_TYPE_MISMATCH,
 MAT_SORT_COLUMN, MAT_BARE_SCAN, MAT_ORDER_LIMIT, MAT_TOO_WIDE, MAT_POST_AGGREGATE,
 MAT_EXACT_SUM, MAT_INT64, MAT_NIL, MAT_KEY_EXPR, MAT_FIRST_ROW, MAT_SORT_KEY,
 MAT_SORT_ROWS) = range(17)


class MaterializeStats(C.Structure):
    """evql_materialize_stats_t"""
    _fields_ = [("rows", C.c_uint64), ("string_bytes", C.c_uint64),
                ("presorted", C.c_uint32), ("passes", C.c_uint32),
                ("n_kernel_launches", C.c_uint32), ("n_host_waits", C.c_uint32),
                ("gather_ms", C.c_float), ("sort_ms", C.c_float), ("encode_ms", C.c_float)]


def bind_materialize(lib):
    """declares evql_table_from_query and evql_plan_materialize on the loaded library"""
    lib.evql_table_from_query.restype = C.c_int
    lib.evql_table_from_query.argtypes = [
        C.c_void_p, C.POINTER(ColumnSpec), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
        C.POINTER(MaterializeStats)]
    lib.evql_plan_materialize.restype = C.c_int
    lib.evql_plan_materialize.argtypes = [
        C.POINTER(PlanDesc), C.POINTER(ColumnInfo), C.c_int, C.POINTER(ColumnSpec), C.c_int,
        C.c_int, C.c_int, C.POINTER(C.c_int)]


FLOAT_SUM_FAST = 0
FLOAT_SUM_EXACT = 1
