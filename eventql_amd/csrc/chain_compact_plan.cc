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

std::string plan_compact_sort_key(const std::vector<ColumnSpec>& specs, const char* key_column,
                                  size_t* key_index, bool* not_supported) {
  *not_supported = false;
  *key_index = 0;
  if (!key_column) return "no key column";
  const std::string key(key_column);
  size_t k = specs.size();
  for (size_t i = 0; i < specs.size(); ++i) {
    if (specs[i].name == key) k = i;
  }
  if (k == specs.size()) return "the key is not among the output columns: " + key;
  const ColumnSpec& c = specs[k];
  if (c.rlevel_max > 0 || c.dlevel_max > 1) return "the key is a repeated / nested column: " + key;
  *not_supported = true;
  if (c.dlevel_max > 0) return "sort key is an optional column (NULLs have no place in the order): " + key;
  switch (c.logical_type) {
    case ColumnType::UNSIGNED_INT:
    case ColumnType::DATETIME: break;
    case ColumnType::FLOAT: return "sort key is a float column: " + key;
    case ColumnType::BOOLEAN: return "sort key is a boolean column: " + key;
    case ColumnType::SIGNED_INT: return "sort key is a signed column: " + key;
    case ColumnType::STRING: return "sort key is a string column: " + key;
    default: return "sort key has no value words: " + key;
  }
  for (const ColumnSpec& o : specs) {
    if (o.rlevel_max > 0 || o.dlevel_max > 1) {
      return "sorted compaction of a repeated / nested column: " + o.name;
    }
  }
  *not_supported = false;
  *key_index = k;
  return std::string();
}

std::string plan_compact_sort_rows(uint64_t rows_out, bool* not_supported) {
  *not_supported = rows_out > 0xffffffffull;
  return *not_supported ? "sorted compaction of more than 2^32 - 1 rows" : std::string();
}

}  // namespace evql
