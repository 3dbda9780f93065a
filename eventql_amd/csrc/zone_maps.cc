// zone_maps.cc -- zone maps: per-column minimum / maximum of every
// kZoneRows rows, cached on the table, and the per-query bitmap of the zones that the
// pruning conjuncts of WHERE exclude.
#include <algorithm>
#include "runtime.h"

namespace evql {

bool zone_column_qualifies(const ColumnLayout& cl) {
  return cl.dlevel_max == 0 && cl.rlevel_max == 0 &&
         (cl.logical_type == ColumnType::UNSIGNED_INT || cl.logical_type == ColumnType::DATETIME);
}

Status table_zone_map(evql_table* t, const std::string& name, const evql_table::ZoneMap** out) {
  auto hit = t->zone_maps.find(name);
  if (hit != t->zone_maps.end()) {
    *out = &hit->second;
    return Status();
  }
  const ColumnLayout* cl = nullptr;
  for (const auto& c : t->layout.columns) {
    if (c.name == name) cl = &c;
  }
  if (!cl) return Status::error(EVQL_EARG, "column not found: " + name);
  if (!zone_column_qualifies(*cl)) {
    return Status::error(EVQL_EARG, "no zone map for column " + name +
                                        ": not a required unsigned-integer / datetime column");
  }
  RtColumn rc{};
  Status st = table_rt_column(t, name, &rc, nullptr);
  if (!st.ok()) return st;
  if (rc.mode == uint32_t(ColAccess::PLAIN64)) {
    // a PLAIN column the table keeps a narrow copy of is read from the copy
    auto m = t->materialized.find(name);
    if (m != t->materialized.end() && m->second.packed_bits && !m->second.packed_f32) {
      rc.mode = uint32_t(ColAccess::NARROW);
      rc.bits = m->second.packed_bits;
      rc.pages = nullptr;
      rc.base = m->second.d_packed;
    }
  }
  hipStream_t s = t->ctx->stream;
  const uint64_t n = t->layout.num_rows;
  evql_table::ZoneMap zm;
  zm.n_zones = (n + kZoneRows - 1) / kZoneRows;
  HIP_TRY(zm.zmin.alloc(zm.n_zones * 8));
  HIP_TRY(zm.zmax.alloc(zm.n_zones * 8));
  HIP_TRY(launch_zone_minmax(t->d_image, rc, n, zm.zmin, zm.zmax, s));
  HIP_TRY(hipStreamSynchronize(s));
  // (only a complete entry enters the cache)
  *out = &(t->zone_maps[name] = std::move(zm));
  return Status();
}

Status query_zone_select(evql_query* q) {
  const KernelPlan& kp = q->kp;
  q->tile_skip = nullptr;
  q->zstats = evql_zone_stats_t{};
  q->zstats.zone_rows = uint32_t(kZoneRows);
  if (kp.zone_conjuncts.empty() || q->nested) return Status();
  evql_table* t = q->table;
  hipStream_t s = q->ctx->stream;
  ZoneSelectArgs a{};
  for (const ZoneConjunct& z : kp.zone_conjuncts) {
    const evql_table::ZoneMap* zm = nullptr;
    Status st = table_zone_map(t, kp.cols[z.col].name, &zm);
    if (!st.ok()) return st;
    const uint32_t k = a.n_conjuncts++;
    a.zmin[k] = zm->zmin;
    a.zmax[k] = zm->zmax;
    a.op[k] = z.op;
    a.lit[k] = z.lit;
    a.n_zones = zm->n_zones;
  }
  q->zstats.conjuncts_used = a.n_conjuncts;
  q->zstats.zones_total = a.n_zones;
  if (a.n_zones == 0) return Status();
  // whole words, with room for the zones of a tile (at most 8) that reaches behind the table
  a.n_words = (a.n_zones + 8 + 31) / 32;
  DevBuf<uint64_t> d_excluded;
  HIP_TRY(q->d_zone_bits.alloc(a.n_words * 4));
  HIP_TRY(d_excluded.alloc(8));
  HIP_TRY(hipMemsetAsync(d_excluded, 0, 8, s));
  a.bits = q->d_zone_bits;
  a.excluded = d_excluded;
  HIP_TRY(launch_zone_select(a, s));
  uint64_t excluded = 0;
  HIP_TRY(hipMemcpyAsync(&excluded, d_excluded, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  q->zstats.zones_excluded = excluded;
  if (excluded) q->tile_skip = q->d_zone_bits;
  else q->d_zone_bits.reset();
  return Status();
}

void zone_stats_after_run(evql_query* q, uint64_t ntiles, uint64_t skipped) {
  q->zstats.zone_rows = uint32_t(kZoneRows);
  q->zstats.tile_rows = uint64_t(q->kp.tile_rows());
  q->zstats.tiles_total = ntiles;
  q->zstats.tiles_skipped = skipped;
}

}  // namespace evql
