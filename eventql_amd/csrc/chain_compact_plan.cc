// chain_compact_plan.cc -- see chain_compact_plan.h
#include "chain_compact_plan.h"

namespace evql {

std::string plan_chain_compact(const std::vector<const TableLayout*>& tables,
                               const std::vector<uint64_t>& rows_kept,
                               const std::vector<ColumnSpec>& specs, bool reverse_order,
                               CompactPlan* out) {
  *out = CompactPlan();
  const size_t nt = tables.size();
  if (nt == 0 || rows_kept.size() != nt) return "chain without tables";
  if (specs.empty()) return "no output columns";
  for (size_t i = 0; i < specs.size(); ++i) {
    const ColumnSpec& c = specs[i];
    for (size_t j = 0; j < i; ++j) {
      if (specs[j].name == c.name) return "output column named twice: " + c.name;
    }
    CompactColumn cc;
    cc.nested = c.rlevel_max > 0 || c.dlevel_max > 1;
    cc.is_string = c.logical_type == ColumnType::STRING;
    cc.source.assign(nt, -1);
    if (c.name == "__lsm_skip") return "a compacted table has no skiplist: __lsm_skip";
    if (c.name == "__lsm_is_update") {
      if (cc.nested || cc.is_string) return "__lsm_is_update is a flat boolean column";
      cc.constant_false = true;
      out->columns.push_back(cc);
      continue;
    }
    for (size_t k = 0; k < nt; ++k) {
      const TableLayout& tl = *tables[k];
      for (size_t li = 0; li < tl.columns.size(); ++li) {
        if (tl.columns[li].name == c.name) cc.source[k] = int(li);
      }
      if (cc.source[k] < 0) {
        if (c.dlevel_max == 0) {
          return "can't merge CSTables after a new required column was added: " + c.name;
        }
        continue;
      }
      const ColumnLayout& cl = tl.columns[cc.source[k]];
      if (cl.logical_type != c.logical_type || cl.rlevel_max != c.rlevel_max ||
          cl.dlevel_max != c.dlevel_max) {
        return "column type or levels differ from the output's: " + c.name;
      }
    }
    out->columns.push_back(cc);
  }
  out->position.assign(nt, 0);
  out->row_base.assign(nt, 0);
  out->tile_base.assign(nt, 0);
  for (size_t p = 0; p < nt; ++p) {
    const size_t k = reverse_order ? nt - 1 - p : p;
    const uint64_t n = tables[k]->num_rows;
    if (rows_kept[k] > n) return "more rows kept than a table holds";
    out->position[k] = uint32_t(p);
    out->row_base[k] = out->rows_out;
    out->tile_base[k] = out->tiles;
    out->rows_in += n;
    out->rows_out += rows_kept[k];
    out->tiles += (n + kCompactTile - 1) / kCompactTile;
  }
  return std::string();
}

}  // namespace evql
