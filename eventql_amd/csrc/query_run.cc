// query_run.cc -- life cycle of a query: prepare (decode, JIT), launch, finish, and the
// maintenance of its group table (recount, rebuild, import, reset).
#include <algorithm>
#include <cmath>
#include <cstring>
#include "runtime.h"

evql_query::~evql_query() {
  if (d_gtab) hipFree(d_gtab);
  if (d_status) hipFree(d_status);
  if (d_counters) hipFree(d_counters);
  if (d_small_rec) hipFree(d_small_rec);
  if (h_tail && tail_pool) {
    // (an epilogue that is still in flight stores to the block: it goes back idle)
    if (launched) hipDeviceSynchronize();
    tail_pool->give(h_tail);
  }
  for (auto* p : d_pairset) {
    if (p) hipFree(p);
  }
  for (auto* p : d_mset) {
    if (p) hipFree(p);
  }
  if (d_row_filter && row_filter_owned) hipFree(d_row_filter);
  for (auto* c : chain) delete c;
  if (d_part_counts) hipFree(d_part_counts);
  if (d_bucket_start) hipFree(d_bucket_start);
  if (d_tuples) hipFree(d_tuples);
  if (d_tuples_tmp) hipFree(d_tuples_tmp);
  if (d_part_cursors) hipFree(d_part_cursors);
  if (d_dense) hipFree(d_dense);
  if (d_mtab) hipFree(d_mtab);
  if (d_mdense) hipFree(d_mdense);
  if (d_conv) hipFree(d_conv);
  for (auto* p : demit.col) {
    if (p) hipHostFree(p);
  }
  for (auto* p : demit.off) {
    if (p) hipHostFree(p);
  }
  for (auto* p : nested_owned) hipFree(p);
  if (ev0) hipEventDestroy(ev0);
  if (ev1) hipEventDestroy(ev1);
}

namespace evql {

// ---------------------------------------------------------------------------
// query execution
// ---------------------------------------------------------------------------
// an empty group table: every word of every slot at its operation's identity
// (step_prologue: the same launch zeroes the query's status words and counters)
static hipError_t init_gtab(const evql_query* q, hipStream_t s, bool step_prologue = false) {
  const KernelPlan& kp = q->kp;
  TableInitArgs ia{};
  ia.words = q->d_gtab;
  ia.stride = q->gcap + 8;
  ia.nwords = uint32_t(kp.words_per_slot());
  slot_identities(kp, ia.nwords, ia.identity);
  if (step_prologue) {
    ia.status = q->d_status;
    ia.counters = q->d_counters;
  }
  return launch_table_init(ia, s);
}

// The eager step tail: which launches leave their groups in the pinned block, and how many.
// Evaluated by every launch (a relaunch after a grown table asks again); everything it
// refuses takes the lazy tail, which is what ran for every plan before.
static const uint32_t kEagerMaxRecords = 4096;    // far below results.cc kDeviceEmitMinGroups
static const uint64_t kEagerMaxSlots = 1u << 18;  // the epilogue scans block-wise: small tables only
uint32_t eager_tail_records(const evql_query* q) {
  const KernelPlan& kp = q->kp;
  // EVQL_EAGER_TAIL=0
  if (q->eager_tail == evql_query::EAGER_OFF) return 0;
  // the cardinality probe aggregates several launches into one table and reads only counts
  if (q->keep_table) return 0;
  // a partition's file chain: the groups leave through chain_merge, not through next_batch
  if (q->in_chain) return 0;
  // no group table
  if (kp.bare_scan) return 0;
  // most groups leave the LDS tables as dense records, and there are many of them
  if (kp.partitioned) return 0;
  // the records are translated from dictionary codes first (query_records_view)
  if (q->dict_key) return 0;
  // PARTIAL rows read the pair sets; a full set is regrown and the scan re-run
  if (kp.n_distinct > 0) return 0;
  // first-row values are gathered from the table once the records are known (lazy path)
  if (kp.need_first_row) return 0;
  // ORDER BY .. LIMIT: select_top_records picks the records on the device
  if (!q->order.empty() && q->has_limit) return 0;
  // large tables with few groups: the count-only pass is the cheaper one there
  if (q->gcap > kEagerMaxSlots) return 0;
  const uint64_t rw = uint64_t(kp.words_per_slot()) + 1;
  const uint64_t fit = (kTailBlockBytes / 8 - kTailRecords) / rw;
  return uint32_t(std::min<uint64_t>(fit, kEagerMaxRecords));
}

static Status alloc_gtab(evql_query* q, uint64_t gcap) {
  if (q->d_gtab) {
    hipFree(q->d_gtab);
    q->d_gtab = nullptr;
  }
  q->gcap = gcap;
  const uint64_t stride = gcap + 8;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_gtab),
                    stride * uint64_t(q->kp.words_per_slot()) * 8));
  return Status();
}

// (re)compiles the fused kernel(s) of q->kp and sizes the persistent grid
static Status compile_plan_kernels(evql_query* q) {
  evql_ctx* ctx = q->ctx;
  if (q->kp.partitioned) {
    Status stw = choose_tuple_widths(q);
    if (!stw.ok()) return stw;
    // two partition levels: without the count pass, unless a coarse bucket overflowed its
    // slack before (skewed keys) or the tuple buffers have to be sized by an exact count
    // (very large scans with a selective predicate, query_launch)
    evql_table* t = q->table;
    const uint64_t nrows = q->nested ? q->nested_rows : t->layout.num_rows;
    const uint64_t begin = std::min(q->row_begin, nrows);
    const uint64_t end = q->row_end ? std::min(q->row_end, nrows) : nrows;
    q->kp.part_fused = false;
    const uint64_t tw = uint64_t(partition_tuple_u32_words(q->kp)) / 2;
    q->kp.part_fused = q->kp.part_bits > 8 && !q->part_fused_off &&
                       (end - begin) * tw * 8 <= (16ull << 30);
  }
  q->source = generate_kernel_source(&q->kp);
  Status st = compile_kernel(ctx, q->source, &q->module, true);
  if (!st.ok()) return st;
  if (q->kp.stage) {
    // The staging loop adds a tuple and its ring address to what the prefetching loop holds.
    // Where that does not fit the registers, the plan keeps the prefetching loop.
    int sc = 0;
    if (q->module.fn &&
        hipFuncGetAttribute(&sc, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, q->module.fn) == hipSuccess && sc != 0) {
      q->kp.stage = false;
      q->kp.stage_allowed = false;
      q->source = generate_kernel_source(&q->kp);
      st = compile_kernel(ctx, q->source, &q->module, true);
      if (!st.ok()) return st;
    }
  }
  if (q->kp.prefetch) {
    // The prefetching tile loop holds two raw tiles.  Where that does not fit the registers,
    // the plan keeps the plain loop at its unroll (and keeps it when it is re-shaped) rather
    // than prefetching half a tile.
    int sc = 0;
    if (q->module.fn &&
        hipFuncGetAttribute(&sc, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, q->module.fn) == hipSuccess && sc != 0) {
      q->kp.prefetch = false;
      q->kp.prefetch_allowed = false;
      q->source = generate_kernel_source(&q->kp);
      st = compile_kernel(ctx, q->source, &q->module, true);
      if (!st.ok()) return st;
    }
  }
  // A plan with many columns / state words can outgrow the 128 VGPRs a 1024-thread
  // workgroup leaves each wave: the scan kernel then keeps part of a tile in scratch
  // memory.  Fewer unroll steps per tile (fewer loads in flight, no scratch) are tried
  // until the kernel fits.
  while (q->kp.unroll > 1) {
    // (the kernels that hold a tile in registers: the fused scan and, for partitioned
    // plans, count and scatter -- only the latter run then)
    // (a bare scan: its count and emit kernels)
    int scratch = 0;
    hipFunction_t fns[5] = {q->kp.partitioned ? nullptr : q->module.fn, q->module.fn_count,
                            q->module.fn_scatter, q->module.fn_scan_count, q->module.fn_scan_emit};
    for (hipFunction_t f : fns) {
      int sc = 0;
      if (f && hipFuncGetAttribute(&sc, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, f) == hipSuccess) {
        scratch = std::max(scratch, sc);
      }
    }
    if (scratch == 0) break;
    q->kp.unroll /= 2;
    q->source = generate_kernel_source(&q->kp);
    st = compile_kernel(ctx, q->source, &q->module, true);
    if (!st.ok()) return st;
  }
  // persistent grid: one wave of workgroups per CU slot
  int per_cu = 1;
  hipError_t oe = hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(
      &per_cu, q->kp.bare_scan ? q->module.fn_scan_emit : q->module.fn, q->kp.block, 0);
  if (oe != hipSuccess || per_cu < 1) per_cu = 1;
  if (per_cu > 8) per_cu = 8;
  q->grid = ctx->num_cus * per_cu;
  return Status();
}

Status query_prepare(evql_query* q) {
  evql_table* t = q->table;
  const LeafLevels* where_leaf = nullptr;
  // a row filter on a nested scan holds one bit per RECORD (setFilter, CSTableScan.cc:
  // 203-204): its expansion to flattened rows needs the leaf's levels as well
  const bool record_filter = q->nested && (q->d_row_filter || !q->row_filter_host.empty());
  if (q->within_record) {
    Status st = materialize_within_record(q);
    if (!st.ok()) return st;
  } else if (q->nested) {
    Status st;
    if (!q->nested_siblings) {
      st = materialize_nested(q, q->kp.cols, &q->nested_flat, &q->nested_rows,
                              q->nested_where_mixed || record_filter ? &where_leaf : nullptr,
                              &q->nested_strpos);
      // (the planner's chain check reads names only: groups that merely look like one
      // chain are caught by the slot counts)
      if (!st.ok() && st.code == EVQL_ENOTSUP && !q->nested_where_mixed &&
          st.msg.find("different repeated groups") != std::string::npos) {
        q->nested_siblings = true;
      } else if (!st.ok()) {
        return st;
      }
    }
    if (q->nested_siblings && record_filter) {
      // (the rows of a record come from k_zip_rows' row offsets, which are not kept)
      return Status::error(EVQL_ENOTSUP, "record filter over sibling repeated groups is not lowered");
    }
    if (q->nested_siblings) {
      st = materialize_nested_zip(q, q->kp.cols, &q->nested_flat, &q->nested_rows, &q->nested_strpos);
      if (!st.ok()) return st;
    }
  }
  // resolve bit widths and materialise SoA columns
  bool repacked = false;
  q->nested_packed.assign(q->kp.cols.size(), evql_query::PackedSource{});
  if (q->nested && !q->within_record && !q->nested_where_mixed && q->nested_leaf >= 0) {
    // The fused kernel streams the flattened columns; like required LEB128 columns they
    // are kept once more as flat arrays of 8 / 16 / 32 bits per value where their maximum
    // fits (config 5: 1 + 4 bytes per row instead of 8 + 8).  Not for string hashes,
    // nor when WHERE resets rewrite the columns per query (apply_where_resets).
    for (size_t i = 0; i < q->kp.cols.size(); ++i) {
      ColAccess& c = q->kp.cols[i];
      if (c.string_hash || c.stype == EVQL_T_FLOAT64) continue;
      auto hit = t->nested_cache.find({c.layout_index, q->nested_leaf});
      if (hit == t->nested_cache.end()) continue;
      evql_table::NestedFlat& e = hit->second;
      if (!e.pack_tried) {
        e.pack_tried = true;
        Status stp = pack_narrow(q->ctx->stream, e.d_values, e.nflat, &e.d_packed, &e.packed_bits);
        if (!stp.ok()) return stp;
      }
      if (!e.packed_bits) continue;
      c.mode = ColAccess::NARROW;
      c.bits = e.packed_bits;
      c.packed = true;
      q->nested_packed[i].base = e.d_packed;
      repacked = true;
    }
  }
  for (size_t i = 0; i < q->kp.cols.size(); ++i) {
    if (q->nested) break;
    ColAccess& c = q->kp.cols[i];
    const ColumnLayout& cl = t->layout.columns[c.layout_index];
    if (c.mode == ColAccess::PLAIN64 && cl.storage_type == ColumnEncoding::UINT64_PLAIN &&
        cl.dlevel_max == 0 && (c.stype != EVQL_T_FLOAT64 || c.from_uint_to_float) &&
        t->layout.num_rows >= t->narrow_min_rows) {
      // A required UINT64_PLAIN column of a table that stays resident: kept once more as
      // a flat array of 8 / 16 / 32 bits per value where its maximum fits, like a LEB128 column
      // (DESIGN.md 3.3).  The maximum comes from the cached statistics pass; the copy is
      // made by the first operator that references the column.
      auto hit = t->materialized.find(c.name);
      if (hit == t->materialized.end()) {
        double mx = 0;
        Status st = column_abs_max(q, i, &mx);
        if (!st.ok()) return st;
        if (mx <= 4294967295.0) {
          st = narrow_plain_column(t, c.layout_index, uint64_t(mx));
          if (!st.ok()) return st;
          hit = t->materialized.find(c.name);
        }
      }
      if (hit != t->materialized.end() && hit->second.packed_bits && !hit->second.packed_f32) {
        c.mode = ColAccess::NARROW;
        c.bits = hit->second.packed_bits;
        c.packed = true;
        repacked = true;
      }
    } else if (c.mode == ColAccess::PLAIN64 && cl.storage_type == ColumnEncoding::FLOAT_IEEE754 &&
               cl.dlevel_max == 0 && cl.rlevel_max == 0 && c.stype == EVQL_T_FLOAT64 &&
               !c.from_uint_to_float && t->layout.num_rows >= t->narrow_float_min_rows) {
      // A required FLOAT_IEEE754 column whose every value is exactly float32: kept once more
      // as a flat float32 array that the tile loads widen back -- 4 bytes per
      // row for the same 64 bits.  The first operator that references the column runs the
      // pass; a refusal is remembered on the table.
      auto hit = t->materialized.find(c.name);
      if (hit == t->materialized.end()) {
        Status st = narrow_float_column(t, c.layout_index);
        if (!st.ok()) return st;
        hit = t->materialized.find(c.name);
      }
      if (hit != t->materialized.end() && hit->second.packed_f32) {
        c.mode = ColAccess::NARROW_F32;
        c.bits = 32;
        c.packed = true;
        repacked = true;
      }
    } else if (c.mode == ColAccess::BITPACKED) {
      Status st = stream_bits(t, cl.data_pages, &c.bits);
      if (!st.ok()) return st;
    } else if (c.mode == ColAccess::SOA) {
      Status st = materialize_column(t, c);
      if (!st.ok()) return st;
      const MaterializedColumn& m = t->materialized[c.name];
      if (m.packed_bits) {  // LEB128 kept as a flat narrow array
        c.mode = ColAccess::NARROW;
        c.bits = m.packed_bits;
        c.packed = true;
        repacked = true;
      }
    }
  }
  {
    // zone maps: statistics of the pruning columns (cached on the table), then the bitmap
    // of the zones this query's literals exclude; every later execute reuses it
    Status stz = query_zone_select(q);
    if (!stz.ok()) return stz;
  }
  if (q->dict_candidate >= 0 && !q->nested) {
    // a STRING key with a usable dictionary: the kernels group by its 32-bit codes.
    // (Here, behind the loop above: the record-level copy of the plan must know the
    // resolved access modes of the other columns -- first-row gathers read them.)
    KernelPlan& kp = q->kp;
    const int ki = q->dict_candidate;
    StringDict* dict = nullptr;
    Status std_ = table_string_dict(t, kp.cols[ki].layout_index, &dict);
    if (!std_.ok()) return std_;
    if (dict->usable) {
      q->rkp = kp;  // what the group records look like outside the scan
      ColAccess code = kp.cols[ki];
      code.stype = EVQL_T_UINT64;
      code.mode = ColAccess::PLAIN32;
      code.has_tags = false;
      code.string_hash = code.string_bytes = false;
      code.dict_code = true;
      kp.cols[ki] = code;
      auto in = std::make_shared<Expr>();
      in->kind = Expr::INPUT;
      in->type = EVQL_T_UINT64;
      in->input = uint32_t(ki);
      kp.group[0] = in;
      kp.key_mode = KEY_EXACT;
      kp.need_first_row = false;
      q->dict_key = true;
      choose_launch_shape(&kp, q->groups_hint);
    }
  }
  if (repacked && !q->kp.partitioned) {
    // the access modes changed: block / unroll / LDS table are chosen again
    choose_launch_shape(&q->kp, q->groups_hint);
  }
  if (q->kp.n_exact > 0) {
    Status stb = choose_exact_sum_scales(q);
    if (!stb.ok()) return stb;
  }
  Status st = compile_plan_kernels(q);
  if (!st.ok()) return st;
  if (q->kp.bare_scan) bare_configure(q);
  // (two allocations on purpose: with the status words and the counters in one 128-byte
  // line -- tried, to read both back with one copy -- the scan kernel's per-tile poll of
  // status[0] shared its line with the counter atomics: config 3 over 16-bit pages
  // 0.36 -> 0.58 ms)
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_status), 16));
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_counters), 64));
  if (!q->row_filter_host.empty()) {
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_row_filter), q->row_filter_host.size() + 16));
    HIP_TRY(hipMemcpy(q->d_row_filter, q->row_filter_host.data(), q->row_filter_host.size(),
                      hipMemcpyHostToDevice));
  }
  if (record_filter) {
    st = expand_record_filter(q, where_leaf);
    if (!st.ok()) return st;
  }
  if (q->nested_where_mixed) {
    // (evql_where_rows reads the row filter: the expanded one must be in place)
    st = apply_where_resets(q, where_leaf);
    if (!st.ok()) return st;
  }
  HIP_TRY(hipEventCreate(&q->ev0));
  HIP_TRY(hipEventCreate(&q->ev1));
  return Status();
}

// Plans without a cardinality hint (the reference's planner has none): before the
// first full run the fused kernel aggregates a prefix of the scan range, and the
// number of groups it finds among the passing rows gives the total by the occupancy
// formula d = G (1 - exp(-p / G)).  A plan whose groups will not fit the LDS tables
// is re-shaped for the partitioned path (choose_launch_shape) in the same execute.
static const uint64_t kProbeMinRows = 8ull << 20;  // below this the probe cannot pay
static const uint64_t kProbeRows = 256ull << 10;
static const uint64_t kProbeSegments = 16;  // row ranges spread evenly over the scan range

static void beat(evql_query* q) {
  if (q->hb && q->hb(q->hb_user) != 0) q->hb_abort = true;
}

static Status probe_cardinality(evql_query* q) {
  evql_table* t = q->table;
  const uint64_t nrows = q->nested ? q->nested_rows : t->layout.num_rows;
  const uint64_t begin = std::min(q->row_begin, nrows);
  const uint64_t end = q->row_end ? std::min(q->row_end, nrows) : nrows;
  if (end - begin < kProbeMinRows) return Status();
  const uint64_t saved_begin = q->row_begin, saved_end = q->row_end;
  // room for one group per sampled row
  Status st = alloc_gtab(q, 4 * kProbeRows);
  if (!st.ok()) return st;
  // The sample is kProbeSegments row ranges spread over the whole scan range, all
  // aggregated into one table: a prefix alone misjudges tables whose keys follow the
  // row order (time-ordered partitions: a prefix of a sorted key column holds one group).
  const uint64_t seg_rows = kProbeRows / kProbeSegments;
  const uint64_t stride = (end - begin) / kProbeSegments;
  for (uint64_t sg = 0; sg < kProbeSegments && st.ok(); ++sg) {
    q->row_begin = begin + sg * stride;
    q->row_end = q->row_begin + seg_rows;
    q->keep_table = sg > 0;
    st = query_launch(q);
    if (st.ok()) st = query_finish(q);
    beat(q);
  }
  q->keep_table = false;
  q->row_begin = saved_begin;
  q->row_end = saved_end;
  if (!st.ok()) return st;  // (a division by zero in the sample is one in the whole scan)
  const double p = double(q->stats.rows_passed), d = double(q->stats.num_groups);
  // the group table is rebuilt for the real run
  hipFree(q->d_gtab);
  q->d_gtab = nullptr;
  q->gcap = 0;
  q->executed = false;
  if (p < 1 || d < 1) return Status();
  const double p_total = p * double(end - begin) / double(kProbeRows);
  double g_est;
  if (d >= 0.999 * p) {
    g_est = p_total;  // (nearly) every sampled row its own group
  } else {
    // solve d = G (1 - exp(-p / G)) for G >= d by bisection (monotone in G)
    double lo = d, hi = std::max(p_total, d) * 4 + 16;
    for (int i = 0; i < 80; ++i) {
      const double mid = 0.5 * (lo + hi);
      const double dm = mid * (1.0 - std::exp(-p / mid));
      if (dm < d) lo = mid; else hi = mid;
    }
    g_est = std::min(0.5 * (lo + hi), p_total);
  }
  const uint64_t hint = uint64_t(g_est * 1.25) + 16;  // headroom for the estimate's error
  q->groups_hint = hint;
  q->stats.estimated_groups = hint;
  if (hint > kPartitionAboveSlots * lds_table_max_slots(q->kp) && partitioned_path_possible(q->kp)) {
    choose_launch_shape(&q->kp, hint);
    return compile_plan_kernels(q);
  }
  if (d >= 2 && d <= 4 && p >= 4096) {
    // a handful of groups among thousands of sampled rows: the shape for 2 .. 4 groups
    // (four lane-private accumulators, choose_launch_shape)
    choose_launch_shape(&q->kp, uint64_t(d));
    if (q->kp.lane_cache > 1) return compile_plan_kernels(q);
  }
  return Status();
}

// the kernel arguments that do not change between launches of one operator
void fill_host_args(evql_query* q, HostArgs* ap) {
  HostArgs& a = *ap;
  evql_table* t = q->table;
  const KernelPlan& kp = q->kp;
  a.image = t->d_image;
  const uint64_t nrows = q->nested ? q->nested_rows : t->layout.num_rows;
  a.row_begin = std::min(q->row_begin, nrows);
  a.row_end = q->row_end ? std::min(q->row_end, nrows) : nrows;
  const uint64_t T = uint64_t(kp.tile_rows());
  a.tile0 = a.row_begin / T;
  a.ntiles = a.row_end > a.row_begin ? (a.row_end + T - 1) / T - a.tile0 : 0;
  a.row_filter = q->d_row_filter;
  a.row_filter_len = q->row_filter_len;
  a.gtab = q->d_gtab;
  a.gcap = q->gcap;
  a.status = q->d_status;
  a.counters = q->d_counters;
  a.tile_skip = q->tile_skip;
  for (int k = 0; k < kp.n_exact; ++k) {
    a.fscale[k] = std::ldexp(1.0, -q->fsum_exp[k]);
    a.fbound[k] = q->fsum_bound[k];
  }
  for (size_t i = 0; i < kp.lit_pool.size() && i < size_t(kMaxLits); ++i) a.lit[i] = kp.lit_pool[i];
  for (size_t i = 0; i < kp.cols.size(); ++i) {
    const ColAccess& c = kp.cols[i];
    a.col[i].base = t->d_image;
    if (c.layout_index >= 0) {
      a.col[i].pages = t->d_pages[c.layout_index][0];
      a.col[i].npages = t->layout.columns[c.layout_index].data_pages.size();
    }
    if (c.dict_code) {
      const StringDict& d = t->dicts[c.name];
      a.col[i].pages = d.d_code_pages;
      a.col[i].base = reinterpret_cast<const uint8_t*>(d.d_codes);
    } else if (c.packed && q->nested) {
      a.col[i].pages = nullptr;  // (ColAccess::NARROW: a flat array)
      a.col[i].base = q->nested_packed[i].base;
    } else if (c.packed) {
      const MaterializedColumn& m = t->materialized[c.name];
      a.col[i].pages = nullptr;
      a.col[i].base = m.d_packed;
    }
    if (q->nested) {
      a.col[i].soa = q->nested_flat[i];
      if (i < q->nested_strpos.size()) a.col[i].strpos = q->nested_strpos[i];
    } else if (c.mode == ColAccess::SOA) {
      const MaterializedColumn& m = t->materialized[c.name];
      a.col[i].soa = m.d_values;
      a.col[i].tags = m.d_tags;
      a.col[i].strpos = m.d_strpos;
    }
  }
}

Status query_launch(evql_query* q) {
  evql_ctx* ctx = q->ctx;
  if (q->kp.bare_scan) return bare_launch(q);
  if (!q->probed && q->groups_hint == 0 && q->kp.key_mode != KEY_NONE && !q->within_record) {
    q->probed = true;
    Status st = probe_cardinality(q);
    if (!st.ok()) return st;
  }
  q->probed = true;
  q->merged = false;
  q->chain_merged = false;
  q->merged_dense = false;
  q->conv_valid = false;
  const KernelPlan& kp = q->kp;
  hipStream_t s = ctx->stream;
  if (!q->d_gtab) {
    // load factor <= 1/4 for small tables; very large ones (>= 1M groups) are kept
    // at <= 1/2: initialising and scanning the table is then a visible part of a
    // step (2.7 GB of slots for 1e7 groups at 1/4)
    const uint64_t slack = q->groups_hint >= (1ull << 20) ? 2 : 4;
    uint64_t want = kp.key_mode == KEY_NONE ? 8 : std::max<uint64_t>(q->groups_hint * slack, 1 << 16);
    // partitioned path: groups leave the LDS tables as dense records; the HBM table
    // only takes the groups of buckets that overflowed theirs (regrown on demand)
    if (kp.partitioned) want = 1 << 16;
    uint64_t cap = 8;
    while (cap < want) cap <<= 1;
    Status st = alloc_gtab(q, cap);
    if (!st.ok()) return st;
  }
  q->tail_valid = false;
  q->tail_armed = 0;
  uint32_t n_launches = 0;
  if (!q->keep_table) {
    // one prologue: empty table, status words and counters
    HIP_TRY(init_gtab(q, s, true));
    ++n_launches;
  } else {
    HIP_TRY(hipMemsetAsync(q->d_counters + kFreshGroupCounter, 0, 8, s));  // (the group count is recounted)
  }

  HostArgs a{};
  fill_host_args(q, &a);
  zone_stats_after_run(q, a.ntiles, 0);
  if (kp.n_distinct > 0 && !q->keep_table) {
    // count_distinct pair sets: emptied before every launch
    if (q->pairset_cap == 0) {
      const uint64_t span = a.row_end > a.row_begin ? a.row_end - a.row_begin : 0;
      // starts at <= 2^20 triples; a full set is regrown x4 and the query re-run
      uint64_t cap = 1 << 16;
      while (cap < 2 * span && cap < (1ull << 20)) cap <<= 1;
      q->pairset_cap = cap;
    }
    for (int i = 0; i < kp.n_distinct; ++i) {
      if (!q->d_pairset[i]) {
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_pairset[i]), q->pairset_cap * 3 * 8));
      }
      HIP_TRY(hipMemsetAsync(q->d_pairset[i], 0xff, q->pairset_cap * 3 * 8, s));
    }
  }
  for (int i = 0; i < kp.n_distinct; ++i) {
    a.pairset[i] = q->d_pairset[i];
    a.pairset_cap[i] = q->pairset_cap;
  }
  if (kp.partitioned && a.ntiles > 0) {
    // count -> per-bucket prefix -> scatter -> per-bucket LDS aggregation
    const uint64_t npart = 1ull << kp.part_bits;
    const uint64_t nwg = std::min<uint64_t>(uint64_t(q->grid), a.ntiles);
    HostArgsWithPart ap{};
    ap.a = a;
    ap.p.tiles_per_wg = (a.ntiles + nwg - 1) / nwg;
    ap.p.nwg = nwg;
    const bool two_level = q->module.fn_refine != nullptr;
    const uint64_t ncursors = 256 + npart;  // [coarse] + [fine]
    if (!q->d_part_counts) {
      HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_part_counts),
                        npart * uint64_t(q->grid) * sizeof(uint32_t)));
      HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_bucket_start), (npart + 2) * 8));
      HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_part_cursors), ncursors * 4));
    }
    ap.p.counts = q->d_part_counts;
    ap.p.bucket_start = q->d_bucket_start;
    ap.p.tuples = q->d_tuples;
    ap.p.tuples_tmp = q->d_tuples_tmp;
    ap.p.cursors = q->d_part_cursors;
    if (!q->d_dense) {
      q->dense_cap = std::max<uint64_t>(q->groups_hint, 1) * 2 + 4096;
      HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_dense),
                        q->dense_cap * uint64_t(kp.words_per_slot() + 1) * 8));
    }
    ap.p.dense = q->d_dense;
    ap.p.dense_cap = q->dense_cap;
    q->dense_n = 0;
    HIP_TRY(hipMemsetAsync(q->d_part_cursors, 0, ncursors * 4, s));
    size_t psz = sizeof(HostArgsWithPart);
    void* pconfig[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ap, HIP_LAUNCH_PARAM_BUFFER_SIZE, &psz,
                       HIP_LAUNCH_PARAM_END};
    const uint64_t tw = uint64_t(partition_tuple_u32_words(kp)) / 2;  // 8-byte words
    const uint64_t span = a.row_end - a.row_begin;
    uint64_t* d_total = q->d_bucket_start + npart + 1;
    const bool fused = kp.part_fused && two_level;
    HIP_TRY(hipEventRecord(q->ev0, s));
    HIP_TRY(hipMemsetAsync(q->d_bucket_start, 0, (npart + 2) * 8, s));
    uint64_t ntuples = span;  // upper bound: every row passes
    if (!fused) {
      HIP_TRY(hipModuleLaunchKernel(q->module.fn_count, unsigned(nwg), 1, 1, kp.block, 1, 1, 0, s,
                                    nullptr, pconfig));
      HIP_TRY(launch_part_scan(q->d_part_counts, npart, nwg, q->d_bucket_start, s));
      HIP_TRY(launch_exclusive_scan(q->d_bucket_start, npart + 1, d_total, s));
      if (q->tuples_cap < span && span * tw * 8 > (16ull << 30)) {
        // large scans with a selective predicate: size the buffers by the count pass
        HIP_TRY(hipMemcpyAsync(&ntuples, d_total, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
      }
    }
    if (ntuples > q->tuples_cap) {
      if (q->d_tuples) hipFree(q->d_tuples);
      q->d_tuples = nullptr;
      const uint64_t cap = ntuples + ntuples / 16 + 1024;
      HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_tuples), cap * tw * 8));
      q->tuples_cap = cap;
    }
    if (two_level) {
      // coarse-bucket order.  Fused form: every coarse bucket owns a fixed range with 5 %
      // slack over an even share of the rows (+ one tile's worth); the hash spreads the
      // tuples evenly (64 buckets of ~2e6 tuples deviate by ~0.1 %), a bucket that
      // overflows anyway (one dominant key) voids the launch: exact offsets then
      const uint64_t ncoarse = 64;
      ap.p.coarse_cap = span / ncoarse + span / (ncoarse * 20) + 16384;
      const uint64_t want = fused ? ap.p.coarse_cap * ncoarse : q->tuples_cap;
      if (want > q->tuples_tmp_cap) {
        if (q->d_tuples_tmp) hipFree(q->d_tuples_tmp);
        q->d_tuples_tmp = nullptr;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_tuples_tmp), want * tw * 8));
        q->tuples_tmp_cap = want;
      }
    }
    ap.p.tuples = q->d_tuples;
    ap.p.tuples_tmp = q->d_tuples_tmp;
    HIP_TRY(hipModuleLaunchKernel(q->module.fn_scatter, unsigned(nwg), 1, 1, kp.block, 1, 1, 0, s,
                                  nullptr, pconfig));
    if (fused) {
      // the fine-bucket sizes the scatter counted -> bucket_start[]
      HIP_TRY(launch_exclusive_scan(q->d_bucket_start, npart + 1, d_total, s));
    }
    // two workgroups per CU where the resources allow it: both passes wait on
    // dependent loads (tuple -> slot) and hide each other's latency
    const uint64_t wide = std::max<uint64_t>(uint64_t(q->grid), uint64_t(ctx->num_cus) * 2);
    if (two_level) {
      HIP_TRY(hipModuleLaunchKernel(q->module.fn_refine, unsigned(wide), 1, 1, kp.block, 1, 1, 0, s,
                                    nullptr, pconfig));
    }
    const unsigned agrid = unsigned(std::min<uint64_t>(npart, wide));
    HIP_TRY(hipModuleLaunchKernel(q->module.fn_aggregate, agrid, 1, 1, kp.block, 1, 1, 0, s, nullptr,
                                  pconfig));
    HIP_TRY(hipEventRecord(q->ev1, s));
    // group count into counter word 4 (read back by finish together with the rest)
    HIP_TRY(launch_table_compact(q->d_gtab, q->gcap, q->gcap + 8, uint32_t(kp.words_per_slot()),
                                 nullptr, 0, q->d_counters + kFreshGroupCounter, s));
    q->launched = true;
    q->stats.n_kernel_launches = 7;
    q->stats.rows_scanned = a.row_end - a.row_begin;
    return Status();
  }
  size_t sz = sizeof(HostArgs);
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz,
                    HIP_LAUNCH_PARAM_END};
  HIP_TRY(hipEventRecord(q->ev0, s));
  if (a.ntiles > 0) {
    int grid = q->grid;
    if (uint64_t(grid) > a.ntiles) grid = int(a.ntiles);
    HIP_TRY(hipModuleLaunchKernel(q->module.fn, grid, 1, 1, kp.block, 1, 1, 0, s, nullptr, config));
    ++n_launches;
  }
  HIP_TRY(hipEventRecord(q->ev1, s));
  const uint32_t eager = eager_tail_records(q);
  if (eager) {
    // one epilogue: group count, status words, counters and the records of a small result
    // into the pinned block finish reads after its one wait
    if (!q->h_tail) {
      void* p = nullptr;
      HIP_TRY(ctx->pinned->take(&p));
      q->tail_pool = ctx->pinned;
      q->h_tail = static_cast<uint64_t*>(p);
      void* dp = nullptr;
      HIP_TRY(hipHostGetDevicePointer(&dp, p, 0));
      q->d_tail = static_cast<uint64_t*>(dp);
    }
    TableTailArgs ta{};
    ta.words = q->d_gtab;
    ta.gcap = q->gcap;
    ta.nwords = uint32_t(kp.words_per_slot());
    ta.max_records = eager;
    ta.status = q->d_status;
    ta.counters = q->d_counters;
    ta.block = q->d_tail;
    ta.seq = ++q->tail_seq;
    HIP_TRY(launch_table_tail(ta, s));
    q->tail_armed = eager;
  } else {
    // group count into counter word 4 (read back by finish together with the rest)
    HIP_TRY(launch_table_compact(q->d_gtab, q->gcap, q->gcap + 8, uint32_t(kp.words_per_slot()),
                                 nullptr, 0, q->d_counters + kFreshGroupCounter, s));
  }
  ++n_launches;
  q->launched = true;
  q->stats.n_kernel_launches = n_launches;
  q->stats.rows_scanned = a.row_end - a.row_begin;
  return Status();
}

// The groups of `q` as dense records of rplan()'s layout.  Plans that ran on dictionary
// codes are translated here, once per execute and only when somebody asks: code ->
// the hashed identity words of the string + its first row (k_dict_records).
Status query_records_view(evql_query* q, RecordsView* v) {
  if (!q->dict_key) {
    v->dense = q->d_dense;
    v->nd = std::min(q->dense_n, q->ngroups);
    return Status();
  }
  hipStream_t s = q->ctx->stream;
  const uint64_t n = q->ngroups;
  if (!q->conv_valid && n) {
    const uint32_t in_words = uint32_t(q->kp.words_per_slot()) + 1;
    const uint64_t nd = std::min(q->dense_n, n);
    DevBuf<uint64_t> tmp;
    const uint64_t* src = q->d_dense;
    if (n > nd) {  // groups of overflowed buckets / of the LDS path sit in the HBM table
      HIP_TRY(tmp.alloc(n * in_words * 8));
      if (nd) HIP_TRY(hipMemcpyAsync(tmp, q->d_dense, nd * in_words * 8, hipMemcpyDeviceToDevice, s));
      uint64_t* d_cnt = q->d_counters + kScratchCounter;
      HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, s));
      HIP_TRY(launch_table_compact(q->d_gtab, q->gcap, q->gcap + 8, in_words - 1,
                                   tmp.p + nd * in_words, n - nd, d_cnt, s));
      src = tmp;
    }
    if (q->conv_cap < n) {
      if (q->d_conv) hipFree(q->d_conv);
      q->d_conv = nullptr;
      q->conv_cap = n + n / 8 + 1024;
      HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_conv), q->conv_cap * uint64_t(in_words + 2) * 8));
    }
    const StringDict& d = q->table->dicts[q->rkp.cols[q->dict_candidate].name];
    HIP_TRY(launch_dict_records(src, n, in_words, d.d_entries, q->d_conv, s));
    HIP_TRY(hipStreamSynchronize(s));  // (tmp lives until here)
    q->conv_valid = true;
  }
  v->dense = q->d_conv;
  v->nd = n;
  return Status();
}

Status query_finish(evql_query* q) {
  if (!q->launched) return Status::error(EVQL_EARG, "query was not launched");
  if (q->kp.bare_scan) return bare_finish(q);
  evql_ctx* ctx = q->ctx;
  for (int attempt = 0; attempt < 12; ++attempt) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    uint32_t status[4] = {0, 0, 0, 0};
    uint64_t counters[8];
    // the eager tail: everything is in the pinned block once the stream has drained.  (A
    // relaunch below enqueues its own epilogue or count pass; `eager` follows it.)
    const bool eager = q->tail_armed != 0;
    if (eager) {
      const uint64_t* blk = q->h_tail;
      if (blk[kTailSeq] != q->tail_seq) {
        return Status::error(EVQL_ERUNTIME, "step epilogue did not write its result block");
      }
      memcpy(status, blk + kTailStatus, 16);
      memcpy(counters, blk + kTailCounters, 64);
      counters[kFreshGroupCounter] = blk[kTailCount];
    } else {
      HIP_TRY(hipMemcpy(status, q->d_status, 16, hipMemcpyDeviceToHost));
    }
    if (status[0] & 1u) return Status::error(EVQL_ERUNTIME, "division by zero");
    if (status[0] & 4u) return Status::error(EVQL_ERUNTIME, "modulo by zero");
    if (status[0] & 32u) {
      return Status::error(EVQL_ERUNTIME, "exact float sum: a value is not finite or exceeds the bound");
    }
    if (status[0] & 64u) {
      // a coarse bucket outgrew its slack (skewed keys): exact offsets from the count pass
      q->part_fused_off = true;
      Status stc = compile_plan_kernels(q);
      if (!stc.ok()) return stc;
      beat(q);
      Status st = query_launch(q);
      if (!st.ok()) return st;
      continue;
    }
    if (status[0] & (2u | 8u | 16u)) {
      // group table / count_distinct pair set / dense record buffer too small: grow
      // and run again
      Status st;
      beat(q);
      if (status[0] & 16u) {
        hipFree(q->d_dense);
        q->d_dense = nullptr;
        q->groups_hint = std::max<uint64_t>(q->groups_hint, 1024) * 4;
        if (q->kp.partitioned && !q->keep_table) {
          // the estimate was off by more than the headroom: bucket bits and launch shape
          // follow the corrected group count (too few buckets overflow every LDS table)
          const int old_bits = q->kp.part_bits;
          choose_launch_shape(&q->kp, q->groups_hint);
          if (q->kp.part_bits != old_bits || !q->kp.partitioned) {
            for (void* p : {(void*) q->d_part_counts, (void*) q->d_bucket_start, (void*) q->d_part_cursors}) {
              if (p) hipFree(p);
            }
            q->d_part_counts = nullptr;
            q->d_bucket_start = nullptr;
            q->d_part_cursors = nullptr;
            Status stc = compile_plan_kernels(q);
            if (!stc.ok()) return stc;
          }
        }
      }
      if (status[0] & 2u) {
        st = alloc_gtab(q, q->gcap * 4);
        if (!st.ok()) return st;
      }
      if (status[0] & 8u) {
        for (auto& p : q->d_pairset) {
          if (p) hipFree(p);
          p = nullptr;
        }
        q->pairset_cap *= 4;
      }
      st = query_launch(q);
      if (!st.ok()) return st;
      continue;
    }
    float ms = 0;
    hipEventElapsedTime(&ms, q->ev0, q->ev1);
    q->stats.kernel_ms = ms;
    // (a record scan's per-record reduction ran when the operator was built)
    q->stats.total_ms = ms + q->within_record_ms;
    if (!eager) HIP_TRY(hipMemcpy(counters, q->d_counters, 64, hipMemcpyDeviceToHost));
    q->stats.rows_passed = counters[0];
    q->zstats.tiles_skipped = counters[5];
    if (q->reported_rows_scanned != ~0ull) q->stats.rows_scanned = q->reported_rows_scanned;
    q->stats.used_lds_table = q->kp.lds_slots > 0;
    q->launched = false;
    // the groups stay in HBM; they are compacted and copied to the host only
    // when the first nextBatch asks for them (a partial aggregate that is merged
    // on the device never leaves it).  Only the group count is read back: the
    // count pass was enqueued behind the kernels by launch (counter word 4).
    q->dense_n = q->kp.partitioned ? counters[3] : 0;
    q->ngroups = counters[4] + q->dense_n;
    q->stats.num_groups = q->ngroups;
    q->executed = true;
    q->fetched = false;
    q->order_applied = false;
    q->emit_pos = 0;
    // more groups than the block takes: its records are ignored, the first next_batch
    // compacts the table (results.cc collect_records)
    q->tail_valid = eager && q->dense_n == 0 && q->ngroups <= q->tail_armed;
    return Status();
  }
  return Status::error(EVQL_ENOMEM, "group table kept overflowing");
}

// number of occupied slots after the table was changed behind the host's back
// (import of another partition's groups)
Status query_recount(evql_query* q) {
  evql_ctx* ctx = q->ctx;
  uint64_t* d_cnt = q->d_counters + kFreshGroupCounter;
  HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, ctx->stream));
  HIP_TRY(launch_table_compact(q->d_gtab, q->gcap, q->gcap + 8, uint32_t(q->kp.words_per_slot()),
                               nullptr, 0, d_cnt, ctx->stream));
  uint64_t n = 0;
  HIP_TRY(hipMemcpyAsync(&n, d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  q->ngroups = n + q->dense_n;
  q->stats.num_groups = q->ngroups;
  q->fetched = false;
  q->order_applied = false;
  q->tail_valid = false;  // (the block holds the table as finish saw it)
  q->executed = true;
  q->emit_pos = 0;
  return Status();
}

// Moves every group of the query -- slots of the HBM hash table and the dense records of
// the partitioned path -- into a fresh hash table with room for `total` groups at load
// factor <= 1/2.
static Status rebuild_table(evql_query* q, uint64_t total) {
  evql_ctx* ctx = q->ctx;
  hipStream_t s = ctx->stream;
  const KernelPlan& kp = q->kp;
  const uint32_t nwords = uint32_t(kp.words_per_slot());
  q->tail_valid = false;
  // groups already in the table (overflowed buckets of the partitioned path, or all)
  uint64_t in_table = q->ngroups - q->dense_n;
  DevBuf<uint64_t> old_rec;
  if (in_table) {
    HIP_TRY(old_rec.alloc(in_table * (nwords + 1) * 8));
    uint64_t* d_cnt = q->d_counters + kScratchCounter;
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, s));
    HIP_TRY(launch_table_compact(q->d_gtab, q->gcap, q->gcap + 8, nwords, old_rec, in_table, d_cnt, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  uint64_t cap = 1 << 16;
  while (cap < total * 2) cap <<= 1;
  Status st = alloc_gtab(q, cap);
  if (!st.ok()) return st;
  HIP_TRY(init_gtab(q, s));
  MergeArgs a{};
  a.words = q->d_gtab;
  a.gcap = q->gcap;
  a.stride = q->gcap + 8;
  merge_ops(kp, false, &a);
  a.status = q->d_status;
  HIP_TRY(hipMemsetAsync(q->d_status, 0, 16, s));
  if (in_table) HIP_TRY(launch_table_merge(a, old_rec, in_table, s));
  if (q->dense_n) HIP_TRY(launch_table_merge(a, q->d_dense, q->dense_n, s));
  uint32_t status[4] = {0};
  HIP_TRY(hipMemcpyAsync(status, q->d_status, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (status[0] & 2u) return merge_status_error(2u, "");
  q->dense_n = 0;
  return Status();
}

// the dense records of the partitioned path moved into the (regrown) HBM hash table:
// what merging another partition's groups into this query needs
Status query_dense_into_table(evql_query* q) {
  if (q->dense_n == 0) return Status();
  return rebuild_table(q, q->ngroups);
}

// room for `extra` more groups: the table is rebuilt BEFORE a merge could fill it, so a
// merge never stops half way (GroupByMergeExpression's map simply grows, groupby.cc:528-637)
Status query_reserve_groups(evql_query* q, uint64_t extra) {
  if (q->dense_n == 0 && (q->ngroups + extra) * 2 <= q->gcap) return Status();
  return rebuild_table(q, q->ngroups + extra);
}

// count_distinct pairs of another partition into this query's set (aggregate.cc:119-137:
// mergeInstance inserts the other set's values); every pair that is new adds 1 to its
// group's aggregate.  The set is regrown first when the pairs might not fit.
Status query_import_pairs(evql_query* q, int which, const uint64_t* d_triples, uint64_t n) {
  hipStream_t s = q->ctx->stream;
  const KernelPlan& kp = q->kp;
  if (q->dense_n) {
    Status st = query_dense_into_table(q);
    if (!st.ok()) return st;
  }
  // pairs held today (all sets share one capacity: the scan kernel takes one)
  uint64_t held_max = 0;
  std::vector<uint64_t> held(kp.n_distinct, 0);
  for (int d = 0; d < kp.n_distinct; ++d) {
    if (!q->d_pairset[d]) continue;
    Status stc = pairset_count(q, q->d_pairset[d], q->pairset_cap, &held[d]);
    if (!stc.ok()) return stc;
    held_max = std::max(held_max, held[d]);
  }
  const uint64_t need = std::max(held_max, held[which] + n);
  uint64_t cap = q->pairset_cap ? q->pairset_cap : (1 << 16);
  while (cap < need * 2) cap <<= 1;
  if (cap != q->pairset_cap) {
    // regrow every set: stored triples re-inserted as they are, nothing counted again
    for (int d = 0; d < kp.n_distinct; ++d) {
      DevBuf<uint64_t> d_new, d_tr;
      HIP_TRY(d_new.alloc(cap * 24));
      HIP_TRY(hipMemsetAsync(d_new, 0xff, cap * 24, s));
      if (q->d_pairset[d] && held[d]) {
        HIP_TRY(d_tr.alloc(held[d] * 24));
        uint64_t* d_cnt = q->d_counters + kScratchCounter;
        HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, s));
        HIP_TRY(launch_pairset_export(q->d_pairset[d], q->pairset_cap, d_tr, held[d], d_cnt, s));
        PairsetMergeArgs pa{};
        pa.set = d_new;
        pa.set_cap = cap;
        pa.words = nullptr;
        pa.status = q->d_status;
        HIP_TRY(launch_pairset_merge(pa, d_tr, held[d], s));
        HIP_TRY(hipStreamSynchronize(s));
      }
      if (q->d_pairset[d]) hipFree(q->d_pairset[d]);
      q->d_pairset[d] = d_new.release();
    }
    q->pairset_cap = cap;
  }
  for (int d = 0; d < kp.n_distinct; ++d) {
    if (q->d_pairset[d]) continue;  // (an empty merge target: evql_query_reset)
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_pairset[d]), q->pairset_cap * 24));
    HIP_TRY(hipMemsetAsync(q->d_pairset[d], 0xff, q->pairset_cap * 24, s));
  }
  if (n == 0) return Status();
  int word = -1;
  for (const auto& ag : kp.aggs) {
    if (ag.distinct_index == which) word = kp.state_word_base() + ag.first_word;
  }
  PairsetMergeArgs pa{};
  pa.set = q->d_pairset[which];
  pa.set_cap = q->pairset_cap;
  pa.words = q->d_gtab;
  pa.gcap = q->gcap;
  pa.nwords = uint32_t(kp.words_per_slot());
  pa.word = uint32_t(word);
  pa.key_mode = uint32_t(kp.key_mode);
  pa.status = q->d_status;
  HIP_TRY(hipMemsetAsync(q->d_status, 0, 16, s));
  HIP_TRY(launch_pairset_merge(pa, d_triples, n, s));
  uint32_t status[4] = {0};
  HIP_TRY(hipMemcpyAsync(status, q->d_status, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (status[0] & 8u) return merge_status_error(8u, "");
  if (status[0] & 2u) {  // (here: the kernel found no slot with the pair's identity)
    return Status::error(EVQL_EARG, "a pair's group is not in the table: import the group records first");
  }
  q->fetched = false;
  q->order_applied = false;
  q->tail_valid = false;
  return Status();
}

// (re)creates an empty group table without scanning: the merge target of
// GroupByMergeExpression (groupby.cc:528-637)
Status query_reset(evql_query* q) {
  evql_ctx* ctx = q->ctx;
  if (q->kp.bare_scan) return bare_reset(q);
  const KernelPlan& kp = q->kp;
  if (!q->d_gtab) {
    uint64_t want = kp.key_mode == KEY_NONE ? 8 : std::max<uint64_t>(q->groups_hint * 4, 1 << 16);
    uint64_t cap = 8;
    while (cap < want) cap <<= 1;
    Status st = alloc_gtab(q, cap);
    if (!st.ok()) return st;
  }
  HIP_TRY(init_gtab(q, ctx->stream));
  HIP_TRY(hipMemsetAsync(q->d_status, 0, 16, ctx->stream));
  HIP_TRY(hipMemsetAsync(q->d_counters, 0, 64, ctx->stream));
  HIP_TRY(hipEventRecord(q->ev0, ctx->stream));
  HIP_TRY(hipEventRecord(q->ev1, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  q->ngroups = 0;
  q->dense_n = 0;
  q->merged = false;
  q->chain_merged = false;
  q->merged_dense = false;
  q->stats.num_groups = 0;
  q->stats.rows_scanned = 0;
  q->stats.rows_passed = 0;
  q->executed = true;
  q->fetched = false;
  q->order_applied = false;
  q->tail_valid = false;
  q->tail_armed = 0;
  q->launched = false;
  q->emit_pos = 0;
  return Status();
}

}  // namespace evql
