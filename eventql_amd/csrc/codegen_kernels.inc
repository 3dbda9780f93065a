// codegen_kernels.inc -- part of codegen.cc: the generated translation unit.
//
// Everything plan-specific is emitted once into `evql_eval_row` (predicate,
// group identity, aggregate arguments); three kernel skeletons consume it:
//
//   evql_scan_agg        fused scan -> filter -> GROUP BY (LDS table -> HBM table)
//   evql_scan_count /    bare scans (no GROUP BY, no aggregate): the passing rows' select
//   evql_scan_emit       values in row order, window by window
//   evql_part_count /    high-cardinality plans: radix-partition the passing
//   evql_part_scatter /  rows by 12 hash bits into 4096 buckets of (identity,
//   evql_part_aggregate  update words) tuples with streaming traffic, then
//                        aggregate every bucket in LDS -- instead of one random
//                        HBM atomic per state word per row

namespace {

struct UpdWord {
  int word;  // state word index
  int op;    // EVQL_OP_*
  // position among the update words of a partition tuple, or -1: the update is the
  // same for every row (count: 1) and does not travel
  int tslot = -1;
  const char* constant = nullptr;
  // ... as 32 bits (values below 2^32 - 1; the all-ones identity of a minimum maps to
  // 32 ones and back), at 32-bit word `toff` of the tuple
  bool narrow = false;
  int toff = -1;
};

struct Gen {
  const KernelPlan& kp;
  std::ostringstream s;
  const int NC, NW, S, W, SB;
  const bool grouped;
  std::vector<UpdWord> updw;

  explicit Gen(const KernelPlan& p)
      : kp(p), NC(int(p.cols.size())), NW(int(p.states.size())), S(p.lds_slots),
        W(p.words_per_slot()), SB(p.state_word_base()), grouped(p.key_mode != KEY_NONE) {
    for (const auto& a : kp.aggs) {
      switch (a.fn) {
        case EVQL_AGG_COUNT:
          updw.push_back({a.first_word, 0});
          updw.back().constant = "1ull";  // count(x) counts NULLs too (aggregate.cc:35-71)
          break;
        case EVQL_AGG_SUM_UINT64:
          updw.push_back({a.first_word, 0});
          updw.back().narrow = a.narrow_arg;
          break;
        case EVQL_AGG_SUM_INT64:
        case EVQL_AGG_COUNT_DISTINCT_UINT64:
          updw.push_back({a.first_word, 0});
          break;
        case EVQL_AGG_SUM_FLOAT64:
          if (a.exact_index >= 0) {  // exact: integer high / low parts
            updw.push_back({a.first_word, 0});
            updw.push_back({a.first_word + 1, 0});
            updw.back().narrow = true;  // low 31 bits (evql_fix)
          } else {
            updw.push_back({a.first_word, 1});
          }
          break;
        case EVQL_AGG_MEAN_UINT64:
        case EVQL_AGG_MEAN_INT64:
        case EVQL_AGG_MEAN_FLOAT64:
          updw.push_back({a.first_word, 1});
          updw.push_back({a.first_word + 1, 0});
          updw.back().narrow = true;  // 0 / 1
          break;
        default:
          updw.push_back({a.first_word, kp.states[a.first_word].op});
          updw.back().narrow =
              a.narrow_arg && (a.fn == EVQL_AGG_MIN_UINT64 || a.fn == EVQL_AGG_MAX_UINT64);
          updw.push_back({a.first_word + 1, 0});
          updw.back().narrow = true;  // 0 / 1
      }
    }
    for (auto& u : updw) {
      if (!u.constant) u.tslot = n_tuple_upd++;
    }
    // tuple layout: 64-bit members first (8-byte aligned), 32-bit members behind them
    int o = 0;
    for (int pass = 0; pass < 2; ++pass) {
      const bool nar = pass == 1;
      if (kp.narrow_ident == nar) { off_ident = o; o += nar ? 1 : 2; }
      if (kp.has_ident2() && !nar) { off_ident2 = o; o += 2; }
      if (kp.need_first_row && kp.narrow_first_row == nar) { off_row = o; o += nar ? 1 : 2; }
      for (auto& u : updw) {
        if (u.tslot < 0 || u.narrow != nar) continue;
        u.toff = o;
        o += nar ? 1 : 2;
      }
    }
    tuple_u32 = (o + 1) & ~1;
  }

  int n_tuple_upd = 0;
  int off_ident = 0, off_ident2 = -1, off_row = -1;
  // 32-bit words of one tuple of the partitioned path: identity, [identity 2], [row],
  // the update words that differ from row to row; even (tuples are 8-byte aligned)
  int tuple_u32 = 0;
  int U() const { return int(updw.size()); }

  // member at 32-bit word `off` of the tuple held in the u32 array `arr`
  static std::string t64(const std::string& arr, int off) {
    return "(((u64) " + arr + "[" + std::to_string(off + 1) + "] << 32) | (u64) " + arr + "[" +
           std::to_string(off) + "])";
  }
  static std::string t32(const std::string& arr, int off) {
    return "((u64) " + arr + "[" + std::to_string(off) + "])";
  }
  std::string tuple_ident(const std::string& arr) const {
    return kp.narrow_ident ? t32(arr, off_ident) : t64(arr, off_ident);
  }
  std::string tuple_row(const std::string& arr) const {
    return kp.narrow_first_row ? t32(arr, off_row) : t64(arr, off_row);
  }
  std::string tuple_upd(const std::string& arr, const UpdWord& u) const {
    if (!u.narrow) return t64(arr, u.toff);
    if (u.op == 2) {  // EVQL_OP_MIN_U64: the identity of a skipped update
      const std::string w = arr + "[" + std::to_string(u.toff) + "]";
      return "(" + w + " == 0xffffffffu ? 0xFFFFFFFFFFFFFFFFull : (u64) " + w + ")";
    }
    return t32(arr, u.toff);
  }
  // tv[off..] = value
  void tuple_put(const char* ind, int off, bool narrow, const std::string& value) {
    s << ind << "{ const u64 tx = " << value << "; tv[" << off << "] = (u32) tx;";
    if (!narrow) s << " tv[" << (off + 1) << "] = (u32) (tx >> 32);";
    s << " }\n";
  }

  std::string lds_word(int w, const std::string& slot) const {
    char b[96];
    snprintf(b, sizeof(b), "lds[%d * EVQL_LSTRIDE + %s]", w, slot.c_str());
    return b;
  }
  std::string gtab_word(int w, const std::string& slot) const {
    char b[96];
    snprintf(b, sizeof(b), "A.gtab[(u64) %s * EVQL_WORDS + %d]", slot.c_str(), w);
    return b;
  }

  // ---- defines + row evaluation ----------------------------------------------------
  void prologue() {
    s << "// generated by eventql_amd codegen\n";
    s << "#define EVQL_BLOCK " << kp.block << "\n";
    s << "#define EVQL_UNROLL " << kp.unroll << "\n";
    s << "#define EVQL_TILE_ROWS " << kp.tile_rows() << "\n";
    s << "#define EVQL_LDS_SLOTS " << S << "\n";
    s << "#define EVQL_LSTRIDE " << (S + 2) << "\n";
    s << "#define EVQL_WORDS " << W << "\n";
    s << "#define EVQL_NSTATE " << NW << "\n";
    s << "#define EVQL_NUPD " << (U() > 0 ? U() : 1) << "\n";
    s << "#define EVQL_LCACHE " << kp.lane_cache << "\n";
    s << "#define EVQL_TUPLE_U32 " << tuple_u32 << "\n";
    // tuples a thread of refine / aggregate holds in flight (~32 registers of tuple data)
    // (8 in flight for 16-byte tuples measured no faster in refine, 10 % slower in aggregate)
    s << "#define EVQL_TIF " << (tuple_u32 <= 10 ? 4 : 2) << "\n\n";
    s << "struct EvqlRowOut {\n  bool live;\n  bool knull;\n  u64 ident;\n  u64 ident2;\n"
         "  u64 ub[EVQL_NUPD];\n  bool uc[EVQL_NUPD];\n};\n\n";
  }

  // emits one row function through `body`; the string literals it uses are declared in
  // front of it as evql_slit<lit_base + i>.  Returns their number.
  template <typename Body>
  size_t row_function(size_t lit_base, Body body) {
    const std::string before = s.str();
    s.str("");
    Emitter em;
    em.lit_base = lit_base;
    em.pool = &pool;
    em.cols = &kp.cols;
    body(em);
    const std::string fn = s.str();
    s.str("");
    s << before;
    if (em.uses_strfn && !strfn_emitted) {
      s << strfn_library_source();
      strfn_emitted = true;
    }
    for (size_t i = 0; i < em.string_literals.size(); ++i) {
      const std::string& l = em.string_literals[i];
      s << "__device__ const u8 evql_slit" << (lit_base + i) << "[" << (l.empty() ? 1 : l.size())
        << "] = {";
      for (size_t k = 0; k < l.size(); ++k) s << (k ? "," : "") << unsigned((unsigned char) l[k]);
      if (l.empty()) s << "0";
      s << "};\n";
    }
    s << fn;
    return em.string_literals.size();
  }

  bool strfn_emitted = false;  // evql_strfn.h is in the text
  size_t n_literals = 0;  // of evql_eval_row
  // numeric literals are numbered once per plan, across its row functions (A.lit[i])
  std::vector<uint64_t> pool;
  // (a staging plan: the staging loop of its scan kernel, prefetch_tile_loop)
  bool staged() const { return kp.stage && kp.prefetch; }
  void eval_row() {
    if (!staged()) {
      n_literals = row_function(0, [&](Emitter& em) { eval_row_body(em); });
      return;
    }
    // A staging plan evaluates a row in two places: WHERE for every row (evql_where_row), the
    // group identity and the update operands for the rows taken out of the ring
    // (evql_eval_post).  evql_eval_row, for the loop with zone test, is the two in a row.
    n_literals = row_function(0, [&](Emitter& em) {
      row_signature("bool", "evql_where_row", "valid", false);
      where_part(em);
      s << "  return live;\n}\n\n";
    });
    n_literals += row_function(n_literals, [&](Emitter& em) {
      row_signature("void", "evql_eval_post", "live", true);
      col_decls();
      post_part(em);
      s << "}\n\n";
    });
    row_signature("void", "evql_eval_row", "valid", true);
    for (int pass = 0; pass < 2; ++pass) {
      s << (pass ? "), " : "  evql_eval_post(A, row, evql_where_row(A, row, valid, ");
      for (int i = 0; i < NC; ++i) s << (i ? ", " : "") << "r" << i << ", g" << i;
    }
    s << ", o);\n}\n\n";
  }

  // c<i>: scan column i of the row as the VM types it, from its loaded word r<i>
  void col_decls() {
    for (int i = 0; i < NC; ++i) {
      const ColAccess& c = kp.cols[i];
      s << "  const " << ctype(c.stype) << " c" << i << " = ";
      if (c.stype == EVQL_T_FLOAT64) {
        s << (c.from_uint_to_float ? "(double) r" : "evql_as_f64(r") << i
          << (c.from_uint_to_float ? "" : ")") << ";\n";
      } else if (c.stype == EVQL_T_BOOL) {
        s << "(r" << i << " != 0);\n";
      } else if (c.stype == EVQL_T_INT64) {
        s << "(i64) r" << i << ";\n";
      } else {
        s << "r" << i << ";\n";
      }
      s << "  (void) c" << i << "; (void) g" << i << ";\n";
    }
  }

  // `flag`: the name of the bool behind `row` (is the row in the window / did it pass WHERE)
  void row_signature(const char* ret, const char* name, const char* flag, bool out) {
    s << "__device__ __forceinline__ " << ret << " " << name << "(const EvqlArgs& A, const u64 row, "
         "const bool " << flag;
    for (int i = 0; i < NC; ++i) s << ", const u64 r" << i << ", const u32 g" << i;
    s << (out ? ", EvqlRowOut& o) {\n" : ") {\n");
  }
  // `live`: is the row in the window, in the row filter and does it pass WHERE
  void where_part(Emitter& em) {
    s << "  bool live = valid;\n";
    if (kp.has_row_filter) {
      s << "  live = live && evql_row_filter(A.row_filter, A.row_filter_len, row);\n";
    }
    col_decls();
    em.ind = "    ";
    if (kp.where) {
      s << "  if (live) {\n";
      Val p = em.emit(kp.where);
      s << em.o.str();
      em.o.str("");
      s << "    live = " << p.v << ";\n  }\n";
    }
  }
  void eval_row_body(Emitter& em) {
    row_signature("void", "evql_eval_row", "valid", true);
    where_part(em);
    post_part(em);
    s << "}\n\n";
  }
  // the group identity and the update operands of a row that is `live`
  void post_part(Emitter& em) {
    em.ind = "    ";
    s << "  o.live = live;\n  o.knull = false;\n  o.ident = 0;\n  o.ident2 = 0;\n";
    for (int i = 0; i < U(); ++i) {
      s << "  o.ub[" << i << "] = evql_op_identity<" << op_name(updw[i].op) << ">(); o.uc[" << i
        << "] = false;\n";
    }
    s << "  if (live) {\n";
    if (kp.key_mode == KEY_EXACT) {
      Val k = em.emit(kp.group[0]);
      s << em.o.str();
      em.o.str("");
      s << "    o.ident = " << Emitter::as_bits(k) << ";\n";
      s << "    o.knull = (" << k.g << " & 1u) != 0;\n";
    } else if (kp.key_mode == KEY_HASHED) {
      s << "    u64 ident = EVQL_IDENT_SEED1, ident2 = EVQL_IDENT_SEED2;\n";
      for (const auto& g : kp.group) {
        Val k = em.emit(g);
        s << em.o.str();
        em.o.str("");
        s << "    evql_ident_add(ident, ident2, " << Emitter::as_bits(k) << ", " << k.g << ");\n";
      }
      s << "    o.ident = evql_ident_word(ident);\n";
      s << "    o.ident2 = evql_ident_word(ident2);\n";
    }
    int ui = 0;
    auto push = [&](const std::string& bits, const std::string& cond) {
      // a skipped update carries the identity of its op, so that the tuple of
      // the partitioned path needs no condition bits
      if (cond.empty()) {
        s << "    o.ub[" << ui << "] = " << bits << "; o.uc[" << ui << "] = true;\n";
      } else {
        s << "    o.uc[" << ui << "] = " << cond << ";\n";
        s << "    if (o.uc[" << ui << "]) o.ub[" << ui << "] = " << bits << ";\n";
      }
      ++ui;
    };
    for (const auto& a : kp.aggs) {
      Val v{"0", "0u", EVQL_T_NIL};
      if (a.arg) {
        v = em.emit(a.arg);
        s << em.o.str();
        em.o.str("");
      }
      const std::string notnull = "((" + v.g + " & 1u) == 0)";
      switch (a.fn) {
        case EVQL_AGG_COUNT:
          push("1ull", "");
          break;
        case EVQL_AGG_SUM_UINT64:
        case EVQL_AGG_SUM_INT64:
          push(Emitter::as_bits(v), "");
          break;
        case EVQL_AGG_SUM_FLOAT64:
          if (a.exact_index >= 0) {
            s << "    u64 fxh" << a.exact_index << ", fxl" << a.exact_index << ";\n";
            s << "    evql_fix(A, " << a.exact_index << ", " << v.v << ", fxh" << a.exact_index
              << ", fxl" << a.exact_index << ");\n";
            push("fxh" + std::to_string(a.exact_index), "");
            push("fxl" + std::to_string(a.exact_index), "");
          } else {
            push(Emitter::as_bits(v), "");
          }
          break;
        case EVQL_AGG_COUNT_DISTINCT_UINT64: {
          // +1 iff this row is the first to put (group, value) into the pair set
          const char* flags = kp.key_mode == KEY_HASHED ? "o.ident2"
                              : (kp.key_mode == KEY_EXACT ? "(o.knull ? 1ull : 0ull)" : "0ull");
          char b[64];
          snprintf(b, sizeof(b), "evql_pairset_insert(A, %d, o.ident, ", a.distinct_index);
          push(std::string(b) + Emitter::as_bits(v) + ", " + flags + ", " +
                   (kp.key_mode == KEY_HASHED ? "false" : "true") + ")",
               "");
          break;
        }
        case EVQL_AGG_MEAN_UINT64:
        case EVQL_AGG_MEAN_INT64:
        case EVQL_AGG_MEAN_FLOAT64: {
          std::string d = a.fn == EVQL_AGG_MEAN_FLOAT64 ? v.v : "((double) " + v.v + ")";
          push("evql_f64_bits(" + d + ")", notnull);
          push("1ull", notnull);
          break;
        }
        default: {  // min / max; NaN inputs are skipped like NULLs (order-free)
          const bool is_f = a.fn == EVQL_AGG_MIN_FLOAT64 || a.fn == EVQL_AGG_MAX_FLOAT64;
          const std::string ok = is_f ? "(" + notnull + " && (" + v.v + " == " + v.v + "))" : notnull;
          push(Emitter::as_bits(v), ok);
          push("1ull", ok);
        }
      }
    }
    s << "  }\n";
  }

  // loads of one tile into x<i>[u][j] / y<i>[u][j]; `only`: of these columns alone
  void tile_loads(const char* ind, const std::vector<bool>* only = nullptr) {
    for (int i = 0; i < NC; ++i) {
      if (only && !(*only)[i]) continue;
      s << ind << "u64 x" << i << "[EVQL_UNROLL][2]; u32 y" << i << "[EVQL_UNROLL][2];\n";
    }
    s << "#pragma unroll\n" << ind << "for (int u = 0; u < EVQL_UNROLL; ++u) {\n";
    s << ind << "  const u64 r = base + ((u64) (u * EVQL_BLOCK) + tid) * 2;\n";
    for (int i = 0; i < NC; ++i) {
      if (only && !(*only)[i]) continue;
      const ColAccess& c = kp.cols[i];
      switch (c.mode) {
        case ColAccess::PLAIN64:
          s << ind << "  evql_plain64_x2(A.col[" << i << "].base, A.col[" << i << "].pages, r, x" << i << "[u][0], x"
            << i << "[u][1]);\n";
          break;
        case ColAccess::PLAIN32:
          s << ind << "  evql_plain32_x2(A.col[" << i << "].base, A.col[" << i << "].pages, r, x" << i << "[u][0], x"
            << i << "[u][1]);\n";
          break;
        case ColAccess::BITPACKED:
          s << ind << "  evql_bitpacked_x2<" << c.bits << ">(A.col[" << i << "].base, A.col[" << i << "].pages, r, x"
            << i << "[u][0], x" << i << "[u][1]);\n";
          break;
        case ColAccess::NARROW:
          // (the page-less overload of the width's accessor: evql_narrow_x2)
          s << ind << "  evql_bitpacked_x2<" << c.bits << ">(A.col[" << i << "].base, r, x" << i
            << "[u][0], x" << i << "[u][1]);\n";
          break;
        case ColAccess::NARROW_F32:
          s << ind << "  evql_f32_x2(A.col[" << i << "].base, r, x" << i << "[u][0], x" << i
            << "[u][1]);\n";
          break;
        case ColAccess::SOA:
          s << ind << "  evql_soa_x2(A.col[" << i << "].soa, r, x" << i << "[u][0], x" << i
            << "[u][1]);\n";
          break;
      }
      if (c.has_tags) {
        s << ind << "  { const unsigned short tt = *reinterpret_cast<const unsigned short*>(A.col["
          << i << "].tags + r); y" << i << "[u][0] = tt & 0xffu; y" << i << "[u][1] = tt >> 8; }\n";
      } else {
        s << ind << "  y" << i << "[u][0] = 0; y" << i << "[u][1] = 0;\n";
      }
    }
    s << ind << "}\n";
  }

  // Zone maps (plans with pruning conjuncts): the first statement of a tile loop's body.  A
  // tile whose zones are all excluded is left without a load: `on_skip`, then `continue`.
  // The decision depends on t alone -- every thread of the workgroup takes the same branch,
  // none has entered a barrier of this iteration -- and the bitmap word comes from one
  // scalar load (evql_zones_excluded).  A tile is a whole number of aligned zones or a
  // divisor of one: both forms are constants of the shape.
  bool prunes() const { return !kp.zone_conjuncts.empty(); }
  // A pruning plan carries every tile loop twice, chosen once per launch by the (uniform)
  // null test of the bitmap: without a bitmap -- nothing is excluded, every benchmark table --
  // the loop is the one a plan without zone maps has, statement for statement; a test inside
  // one shared loop changed how the compiler versions and schedules it (measured on an
  // ungrouped two-column plan with an empty bitmap: 0.285 -> 0.323 ms per 1e8 rows).
  bool zone_test = false;
  template <typename Loop>
  void tile_loop_twice(const char* ind, Loop emit_loop) {
    zone_test = false;
    if (!prunes()) {
      emit_loop();
      return;
    }
    s << ind << "if (!A.tile_skip) {\n";
    emit_loop();
    s << ind << "} else {\n";
    zone_test = true;
    emit_loop();
    zone_test = false;
    s << ind << "}\n";
  }
  void zone_skip(const char* ind, const char* on_skip, bool count = true) {
    if (!zone_test) return;
    const uint64_t T = uint64_t(kp.tile_rows());
    const uint64_t zones = T >= kZoneRows ? T / kZoneRows : 1;
    s << ind << "{\n";
    if (T >= kZoneRows) {
      s << ind << "  const u64 zi = (A.tile0 + t) * " << zones << "ull;\n";
    } else {
      s << ind << "  const u64 zi = ((A.tile0 + t) * (u64) EVQL_TILE_ROWS) / EVQL_ZONE_ROWS;\n";
    }
    s << ind << "  if (evql_zones_excluded<" << zones << ">(A.tile_skip, zi)) { " << on_skip
      << (count ? " ++zskipped;" : "") << " continue; }\n";
    s << ind << "}\n";
  }
  void zone_skip_decl(const char* ind) {
    if (prunes()) s << ind << "u32 zskipped = 0;  // tiles this workgroup skipped\n";
  }
  void zone_skip_flush(const char* ind) {
    if (prunes()) s << ind << "if (tid == 0 && zskipped) atomicAdd(&A.counters[5], (u64) zskipped);\n";
  }

  // evaluates row (u, j) of the loaded tile into `o` (columns outside `only` were not
  // loaded and read as 0: the caller knows that the row function does not use them)
  //
  // Whether the row lies in the plan's window [A.row_begin, A.row_end) is decided in 32 bits.
  // Once per tile, on uniform values (tile_window, after `base`): the window clipped to the
  // tile as offsets wlo <= whi into it, its length `wlen`, and per lane `wrel` = the offset of
  // the lane's first row of step 0, minus wlo.  Row (u, j) has the offset
  // (u * BLOCK + tid) * 2 + j, so per row one add of a constant and one unsigned compare
  // remain: offsets below wlo wrap to >= 2^32 - TILE_ROWS > wlen.  (The two 64-bit compares
  // of r + j against the window cost 8 .. 15 VGPRs in the narrow shapes.)  Every tile loop
  // numbers its rows this way.
  // Loops that hold few values per lane keep the 64-bit compares (window32 = false): the
  // predicate-only passes evql_scan_count and evql_part_count and the ungrouped scan came out
  // 1 .. 5 VGPRs FATTER in the 32-bit form over plain pages, against their pins.
  bool window32 = true;
  void tile_window(const char* ind) {
    if (!window32) return;
    s << ind << "const u64 wb = A.row_begin > base ? A.row_begin - base : 0ull;\n";
    s << ind << "const u64 we = A.row_end > base ? A.row_end - base : 0ull;\n";
    s << ind << "const u32 wlo = (u32) (wb < (u64) EVQL_TILE_ROWS ? wb : (u64) EVQL_TILE_ROWS);\n";
    s << ind << "const u32 whi = (u32) (we < (u64) EVQL_TILE_ROWS ? we : (u64) EVQL_TILE_ROWS);\n";
    s << ind << "const u32 wlen = whi > wlo ? whi - wlo : 0u;\n";
    s << ind << "const u32 wrel = 2u * tid - wlo;\n";
  }
  // (step_local: the row's values are x<i>s[j], decoded in the step from a raw tile, no tags)
  void eval_call(const char* ind, int j, const std::vector<bool>* only = nullptr,
                 const char* out = "o", bool step_local = false) {
    if (window32) {
      s << ind << "evql_eval_row(A, r + " << j << ", wrel + (u32) (u * EVQL_BLOCK * 2 + " << j
        << ") < wlen";
    } else {
      s << ind << "evql_eval_row(A, r + " << j << ", (r + " << j << " >= A.row_begin) && (r + " << j
        << " < A.row_end)";
    }
    for (int i = 0; i < NC; ++i) {
      if (only && !(*only)[i]) {
        s << ", 0ull, 0u";
        continue;
      }
      if (step_local) {
        s << ", x" << i << "s[" << j << "], 0u";
        continue;
      }
      s << ", x" << i << "[u][" << j << "], y" << i << "[u][" << j << "]";
    }
    s << ", " << out << ");\n";
  }

  // ---- the prefetching tile loop of evql_scan_agg (KernelPlan::prefetch) ------------------
  // Two tiles are held RAW, as the words the loads returned: N, the tile being loaded, and C,
  // the tile being evaluated.  One body: load N = next tile -> evaluate C -> C = N.  The loads
  // of a tile then have a whole tile's evaluation to arrive in, where the plain loop waits for
  // them with nothing else to issue.  All columns are flat narrow / float32 copies without
  // tags (choose_launch_shape): one word per step and column for 8 / 16 bits, two for 32.
  static int raw_words(const ColAccess& c) { return c.bits == 32 ? 2 : 1; }
  void raw_tile_decls(const char* ind, const char* name, bool zero) {
    for (int i = 0; i < NC; ++i) {
      s << ind << "u32 " << name << i << "[EVQL_UNROLL][" << raw_words(kp.cols[i]) << "]"
        << (zero ? " = {}" : "") << ";\n";
    }
  }
  void raw_tile_loads(const char* ind) {
    s << "#pragma unroll\n" << ind << "for (int u = 0; u < EVQL_UNROLL; ++u) {\n";
    s << ind << "  const u64 r = lbase + ((u64) (u * EVQL_BLOCK) + tid) * 2;\n";
    for (int i = 0; i < NC; ++i) {
      const ColAccess& c = kp.cols[i];
      const int hi = raw_words(c) - 1;
      // (the accessors' names of tile_loads; their u32 overloads return the words as loaded:
      // evql_f32_ld, evql_narrow_ld)
      if (c.mode == ColAccess::NARROW_F32) {
        s << ind << "  evql_f32_x2(A.col[" << i << "].base, r, n" << i << "[u][0], n" << i << "[u][" << hi
          << "]);\n";
      } else {
        s << ind << "  evql_bitpacked_x2<" << c.bits << ">(A.col[" << i << "].base, r, n" << i << "[u][0], n"
          << i << "[u][" << hi << "]);\n";
      }
    }
    s << ind << "}\n";
  }
  // the head of a step: its raw words are touched, for every row, then decoded into x<i>s[2]
  void raw_step_decode(const char* ind) {
    s << ind << "asm(\"\" : ";
    bool first = true;
    for (int i = 0; i < NC; ++i) {
      for (int w = 0; w < raw_words(kp.cols[i]); ++w) {
        s << (first ? "" : ", ") << "\"+v\"(c" << i << "[u][" << w << "])";
        first = false;
      }
    }
    s << ");\n";
    for (int i = 0; i < NC; ++i) {
      const ColAccess& c = kp.cols[i];
      const int hi = raw_words(c) - 1;
      s << ind << "u64 x" << i << "s[2]; ";
      if (c.mode == ColAccess::NARROW_F32) {
        s << "evql_f32_dec(c" << i << "[u][0], c" << i << "[u][" << hi << "], x" << i << "s[0], x" << i
          << "s[1]);\n";
      } else {
        s << "evql_narrow_dec<" << c.bits << ">(c" << i << "[u][0], c" << i << "[u][" << hi << "], x" << i
          << "s[0], x" << i << "s[1]);\n";
      }
    }
  }
  void raw_tile_copy(const char* ind) {
    s << "#pragma unroll\n" << ind << "for (int u = 0; u < EVQL_UNROLL; ++u) {\n" << ind << " ";
    for (int i = 0; i < NC; ++i) {
      for (int w = 0; w < raw_words(kp.cols[i]); ++w) {
        s << " c" << i << "[u][" << w << "] = n" << i << "[u][" << w << "];";
      }
    }
    s << "\n" << ind << "}\n";
  }

  // ---- the staging form of the prefetching loop (KernelPlan::stage) ------------------------
  // The evaluation of a tile in two halves.  STAGE, for every row: WHERE on the row's values
  // (evql_where_row); the lanes whose row passes put a tuple into the wave's ring in LDS
  // (evql_device.h evql_stage_put).  DRAIN, whenever 64 tuples are pending: every lane takes
  // one, evaluates the group identity and the update operands from it (evql_eval_post) and
  // updates the group table with evql_update, as the other loops do -- with all 64 lanes at
  // work, where the row's own exec mask has as many as WHERE lets pass.
  //
  // The tuple holds the columns that the group key and the aggregate arguments read, each as
  // the bits of its copy (stage_tuple_layout): what a row function computes from them it
  // computes behind the ring, so a tuple is never wider than the row's loaded words, a float32
  // copy travels as its raw word (widened by evql_f32_dec as in the other loops, bit for bit)
  // and tags, NULL keys and skipped updates need no bits of their own.
  std::vector<StageField> sfields;
  int stage_words = 0;
  // field `f` of row j of the step, from the raw words of tile C
  static std::string stage_raw_field(const StageField& f, int j) {
    const std::string c = "c" + std::to_string(f.col) + "[u]";
    if (f.bits == 32) return c + "[" + std::to_string(j) + "]";
    const std::string m = f.bits == 16 ? "0xffffu" : "0xffu";
    return "((" + c + "[0] >> " + std::to_string(f.bits * j) + ") & " + m + ")";
  }
  // EvqlStaged, its pack (one argument per field, in the layout's order) and, per staged
  // column, the value the row function takes
  void stage_tuple_text() {
    stage_words = stage_tuple_layout(kp, &sfields);
    s << "struct alignas(" << (stage_words % 2 == 0 ? 8 : 4) << ") EvqlStaged { u32 w[" << stage_words
      << "]; };\n";
    s << "__device__ __forceinline__ EvqlStaged evql_stage_pack(";
    for (size_t k = 0; k < sfields.size(); ++k) s << (k ? ", " : "") << "const u32 f" << k;
    s << ") {\n  EvqlStaged t;\n";
    for (int w = 0; w < stage_words; ++w) {
      s << "  t.w[" << w << "] = ";
      bool first = true;
      for (size_t k = 0; k < sfields.size(); ++k) {
        if (sfields[k].word != w) continue;
        s << (first ? "" : " | ");
        if (sfields[k].shift) s << "(f" << k << " << " << sfields[k].shift << ")";
        else s << "f" << k;
        first = false;
      }
      s << ";\n";
    }
    s << "  return t;\n}\n";
    for (const StageField& f : sfields) {
      s << "__device__ __forceinline__ u64 evql_stage_col" << f.col << "(const EvqlStaged& t) {\n";
      if (f.f32) {
        s << "  u64 v0, v1;\n  evql_f32_dec(t.w[" << f.word << "], t.w[" << f.word << "], v0, v1);\n  return v0;\n";
      } else if (f.bits == 32) {
        s << "  return (u64) evql_opaque(t.w[" << f.word << "]);\n";
      } else {
        s << "  return (u64) evql_opaque((t.w[" << f.word << "] >> " << f.shift << ") & 0xffffu);\n";
      }
      s << "}\n";
    }
    s << "\n";
  }
  // 64 tuples, or the `live` lanes' at the end of the kernel, out of the ring and into the table
  void stage_drain_function() {
    s << "__device__ __forceinline__ void evql_stage_drain(const EvqlArgs& A, u64* lds, const EvqlStaged* ring,\n"
         "                                                 EvqlAcc& acc, const bool bypass, u32& head, "
         "const u32 lane, const bool live) {\n";
    s << "  const EvqlStaged t = evql_stage_take(ring, head, lane);\n";
    s << "  EvqlRowOut o;\n  evql_eval_post(A, 0ull, live";
    for (int i = 0; i < NC; ++i) {
      bool in = false;
      for (const StageField& f : sfields) in = in || f.col == i;
      if (in) s << ", evql_stage_col" << i << "(t), 0u";
      else s << ", 0ull, 0u";
    }
    s << ", o);\n";
    s << "  const u64 k = evql_lds_peek(&lds[(u32) o.ident & (EVQL_LDS_SLOTS - 1)]);\n";
    s << "  evql_update(A, lds, acc, bypass, 0ull, o, k);\n}\n\n";
  }
  // rows (u, 0) and (u, 1) of the tile held raw in C.  Drain first, then stage: at most 63
  // tuples are pending when a row puts its own, at most 64, into EVQL_STAGE_RING = 128 entries
  // (and the copy's wait for the next tile then follows a row's few staging instructions, not
  // the cold block of a drain's HBM updates).
  void stage_step(const std::string& ind) {
    const char* in = ind.c_str();
    for (int j = 0; j < 2; ++j) {
      s << in << "if (tail - head >= 64u) evql_stage_drain(A, lds, ring, acc, bypass, head, lane, true);\n";
      s << in << "const bool l" << j << " = evql_where_row(A, r + " << j << ", wrel + (u32) (u * EVQL_BLOCK * 2 + "
        << j << ") < wlen";
      for (int i = 0; i < NC; ++i) s << ", x" << i << "s[" << j << "], 0u";
      s << ");\n";
      s << in << "evql_stage_put(ring, tail, l" << j << ", evql_stage_pack(";
      for (size_t k = 0; k < sfields.size(); ++k) s << (k ? ", " : "") << stage_raw_field(sfields[k], j);
      s << "));\n";
    }
  }

  // ---- the fused scan kernel --------------------------------------------------------
  // (the tile loop reads the identity slots of a step's two rows ahead of their updates)
  bool probe_ahead() const { return grouped && S > 0 && !kp.has_ident2(); }
  // rows (u, 0) and (u, 1) of a tile: evaluate, update
  void scan_step(const std::string& ind, bool step_local) {
    const char* in = ind.c_str();
    if (probe_ahead()) {
      // both rows of the step are evaluated and their identity slots read before either is
      // consumed: one exposed LDS round trip per step instead of one per row.  A slot that
      // row 0 claims after row 1's read is seen by row 1's compare-and-swap (evql_lds_find_from)
      s << in << "EvqlRowOut o0, o1;\n";
      for (int j = 0; j < 2; ++j) eval_call(in, j, nullptr, j ? "o1" : "o0", step_local);
      for (int j = 0; j < 2; ++j) {
        s << in << "const u64 k" << j << " = evql_lds_peek(&lds[(u32) o" << j
          << ".ident & (EVQL_LDS_SLOTS - 1)]);\n";
      }
      for (int j = 0; j < 2; ++j) {
        s << in << "evql_update(A, lds, acc, bypass, r + " << j << ", o" << j << ", k" << j << ");\n";
      }
    } else {
      s << in << "EvqlRowOut o;\n";
      for (int j = 0; j < 2; ++j) {
        eval_call(in, j, nullptr, "o", step_local);
        s << in << "evql_update(A, lds, acc, bypass, r + " << j << ", o);\n";
      }
    }
  }
  // The prefetching form of the tile loop without zone test (grouped, LDS table).  `tc` is the
  // tile held in C, `have` whether there is one.  Past a workgroup's last tile the load is
  // clamped to the tile it holds -- a tile of this launch, whatever lies behind the arrays --
  // and its values are dropped.  The poll of TABLE_FULL is issued AHEAD of the cluster and
  // tested behind the copy, where the loads are waited for anyway: every global load counts on
  // the same in-order vmcnt, and a value tested between the cluster and the copy would wait
  // for the whole prefetch.  (A launch that ends this way is void: the host grows the table
  // and runs it again, so the one more tile it evaluates does not matter.)  The scheduling
  // barriers keep the cluster in front of the evaluation and the copy behind it.
  void prefetch_tile_loop() {
    s << "  u32 tile_no = 0;  // tiles evaluated\n";
    raw_tile_decls("  ", "c", false);
    s << "  bool have = false;\n  u64 tc = 0;\n";
    if (staged()) {
      s << "  EvqlStaged* const ring = evql_stage_ring + (tid >> 6) * EVQL_STAGE_RING;\n";
      s << "  const u32 lane = tid & 63u;\n";
      s << "  u32 head = 0, tail = 0;  // tuples this wave has taken out of its ring / put into it\n";
    }
    s << "  for (u64 t = blockIdx.x; have || t < A.ntiles; t += gridDim.x) {\n";
    s << "    const bool more = t < A.ntiles;\n";
    s << "    const u64 tl = more ? t : tc;\n";
    s << "    u32 st = 0;\n";
    s << "    if ((tile_no & 15u) == 0) st = __hip_atomic_load(&A.status[0], __ATOMIC_RELAXED, "
         "__HIP_MEMORY_SCOPE_AGENT);\n";
    s << "    const u64 lbase = (A.tile0 + tl) * (u64) EVQL_TILE_ROWS;\n";
    raw_tile_decls("    ", "n", false);
    raw_tile_loads("    ");
    s << "    __builtin_amdgcn_sched_barrier(0);\n";
    s << "    if (have) {\n";
    s << "      const bool bypass = evql_lds_peek32(reinterpret_cast<const u32*>(&lds[EVQL_WORDS * "
         "EVQL_LSTRIDE])) >= 4u * EVQL_BLOCK;\n";
    s << "      const u64 base = (A.tile0 + tc) * (u64) EVQL_TILE_ROWS;\n";
    tile_window("      ");
    s << "#pragma unroll\n      for (int u = 0; u < EVQL_UNROLL; ++u) {\n";
    s << "        const u64 r = base + ((u64) (u * EVQL_BLOCK) + tid) * 2;\n";
    raw_step_decode("        ");
    if (staged()) stage_step("        ");
    else scan_step("        ", true);
    s << "      }\n      ++tile_no;\n    }\n";
    s << "    __builtin_amdgcn_sched_barrier(0);\n";
    raw_tile_copy("    ");
    // (the volatile statement stays where it is written: the copy and its waits are not
    // sunk behind the test of the poll, and the polled word stays in its VGPR until here)
    s << "    asm volatile(\"\" : \"+v\"(st)";
    for (int i = 0; i < NC; ++i) {
      for (int w = 0; w < raw_words(kp.cols[i]); ++w) s << ", \"+v\"(c" << i << "[EVQL_UNROLL - 1][" << w << "])";
    }
    s << ");\n";
    s << "    tc = tl;\n    have = more;\n";
    s << "    if (__builtin_amdgcn_readfirstlane(st) & EVQL_ST_TABLE_FULL) break;\n";
    s << "  }\n";
    if (staged()) {
      // what is still pending behind the last tile: up to 63 + 64 tuples.  (Behind a
      // TABLE_FULL break too: that launch is void either way.)
      s << "  {\n";
      s << "    const bool bypass = evql_lds_peek32(reinterpret_cast<const u32*>(&lds[EVQL_WORDS * "
           "EVQL_LSTRIDE])) >= 4u * EVQL_BLOCK;\n";
      s << "    if (tail - head >= 64u) evql_stage_drain(A, lds, ring, acc, bypass, head, lane, true);\n";
      s << "    const u32 left = tail - head;\n";
      s << "    if (left) evql_stage_drain(A, lds, ring, acc, bypass, head, lane, lane < left);\n";
      s << "  }\n";
    }
  }
  void scan_kernel() {
    // (passed / spilled: rows of this lane.  A plan with the prefetching loop counts them in 32
    // bits, widened at the wave reduction -- one v_addc per row instead of a select and a 64-bit
    // add; a lane sees 8 rows of a tile, 2^32 of them are beyond any table.  The other plans
    // keep their text.)
    const char* ctr = kp.prefetch ? "u32" : "u64";
    s << "struct EvqlAcc {\n  " << ctr << " passed;\n  " << ctr << " spilled;\n";
    if (!grouped) s << "  u64 w[" << (NW > 0 ? NW : 1) << "];\n";
    // (the one global group's first passing row, for select expressions over its values:
    // `select s, count(1) from t`)
    if (!grouped && kp.need_first_row) s << "  u64 first;\n";
    if (grouped && S > 0) {
      s << "  int cs[EVQL_LCACHE];\n  u64 cfirst[EVQL_LCACHE];\n  u64 cw[EVQL_LCACHE][EVQL_NUPD];\n"
           "  u32 cv;\n";
    }
    s << "};\n\n";
    if (grouped && S > 0) {
      // entry J of a lane's accumulator cache into the LDS table (one atomic per word)
      s << "template <int J>\n";
      s << "__device__ __forceinline__ void evql_flush_entry(u64* lds, EvqlAcc& acc) {\n";
      s << "  const int cs = acc.cs[J];\n";
      if (kp.need_first_row) {
        s << "  evql_atomic<EVQL_OP_MIN_U64>(&" << lds_word(kp.first_row_word(), "cs") << ", acc.cfirst[J]);\n";
        s << "  acc.cfirst[J] = 0xFFFFFFFFFFFFFFFFull;\n";
      }
      for (int i = 0; i < U(); ++i) {
        s << "  evql_atomic<" << op_name(updw[i].op) << ">(&" << lds_word(SB + updw[i].word, "cs")
          << ", acc.cw[J][" << i << "]);\n";
        s << "  acc.cw[J][" << i << "] = evql_op_identity<" << op_name(updw[i].op) << ">();\n";
      }
      s << "}\n";
      s << "__device__ __forceinline__ void evql_flush_private(u64* lds, EvqlAcc& acc) {\n";
      for (int j = 0; j < kp.lane_cache; ++j) {
        s << "  if (acc.cs[" << j << "] >= 0) { evql_flush_entry<" << j << ">(lds, acc); acc.cs[" << j
          << "] = -1; }\n";
      }
      s << "}\n\n";
    }

    // update of the group table with one evaluated row.  No early returns: every
    // lane of the wave reaches the cooperative part together.
    s << "__device__ __forceinline__ void evql_update(const EvqlArgs& A, u64* lds, EvqlAcc& acc,\n"
         "                                            const bool bypass, const u64 row, "
         "const EvqlRowOut& o"
      << (probe_ahead() ? ", const u64 slot0" : "") << ") {\n";
    s << "  acc.passed += o.live ? 1 : 0;\n";
    if (!grouped) {
      if (kp.need_first_row) s << "  if (o.live && row < acc.first) acc.first = row;\n";
      for (int i = 0; i < U(); ++i) {
        s << "  if (o.uc[" << i << "]) acc.w[" << updw[i].word << "] = evql_combine<"
          << op_name(updw[i].op) << ">(acc.w[" << updw[i].word << "], o.ub[" << i << "]);\n";
      }
      s << "}\n\n";
    } else {
      auto updates = [&](bool global, const char* slot, const char* ind) {
        if (kp.need_first_row) {
          s << ind << "evql_atomic<EVQL_OP_MIN_U64>(&"
            << (global ? gtab_word(kp.first_row_word(), slot) : lds_word(kp.first_row_word(), slot))
            << ", row);\n";
        }
        for (int i = 0; i < U(); ++i) {
          s << ind << "if (o.uc[" << i << "]) evql_atomic<" << op_name(updw[i].op) << ">(&"
            << (global ? gtab_word(SB + updw[i].word, slot) : lds_word(SB + updw[i].word, slot))
            << ", o.ub[" << i << "]);\n";
        }
      };
      if (S > 0) {
        // `bypass`: this workgroup has seen so many rows that found no LDS slot
        // that the table is evidently too small for the data: stop probing it
        s << "  int s = -1;\n";
        s << "  if (o.live && !bypass) {\n";
        s << "    if (o.knull) { s = EVQL_LDS_SLOTS + 1; lds[s] = 0; }\n";
        s << "    else if (o.ident == EVQL_EMPTY) { s = EVQL_LDS_SLOTS; lds[s] = 0; }\n";
        if (kp.has_ident2()) {
          s << "    else s = evql_lds_find2<16>(lds, lds + EVQL_LSTRIDE, EVQL_LDS_SLOTS - 1, o.ident, "
               "o.ident2, (u32) evql_mix64(o.ident));\n";
        } else {
          s << "    else s = evql_lds_find" << (probe_ahead() ? "_from" : "")
            << "<16>(lds, EVQL_LDS_SLOTS - 1, o.ident, (u32) evql_mix64(o.ident)"
            << (probe_ahead() ? ", slot0" : "") << ");\n";
        }
        s << "    if (s < 0) atomicAdd(reinterpret_cast<u32*>(&lds[EVQL_WORDS * EVQL_LSTRIDE]), 1u);\n";
        s << "  }\n";
        // Lane-private accumulator cache.  Rows that hit the slot a lane updated last (one
        // group, a dominant key, input clustered by key) are combined in registers and
        // reach the LDS table only when the lane moves on to another slot: 64 same-address
        // LDS atomics would serialise (~1.8 cycles per lane; one group ran 3.3x slower than
        // 1000).  Round 2 detected WAVE-uniform runs with ballot / readlane / ballot; the
        // per-lane form needs no wave-wide agreement -- it also halves the atomics of a
        // two-group plan -- and no scalar round trips in front of every row.  Plans with
        // 2 .. 4 expected groups keep EVQL_LCACHE = 4 entries, enough to hold every group
        // (predicated updates: no dynamic register indexing).
        //
        // One entry (every plan but those with 2 .. 4 expected groups): the same policy and
        // the same LDS atomics, as two branches.  The select form ran both halves for every
        // row -- combines and selects that picked nothing, the entry refilled with
        // identities and overwritten at once -- and with 1000 spread groups, where a lane's
        // entry practically never hits, that was 40 % of the vector instructions of a passing
        // row.  The miss block holds atomics and stays a branch; its install is plain moves
        // under the exec mask.  The hit block is five instructions, which the back end would
        // rather run with an empty exec mask than jump over: the empty asm statement makes it
        // keep the s_cbranch_execz.
        if (kp.lane_cache == 1) {
          s << "  const bool hit = s >= 0 && acc.cs[0] == s;\n";
          s << "  const bool miss = s >= 0 && !hit;\n";
          s << "  if (hit) {\n    asm volatile(\"\");\n";
          if (kp.need_first_row) s << "    if (row < acc.cfirst[0]) acc.cfirst[0] = row;\n";
          for (int i = 0; i < U(); ++i) {
            s << "    if (o.uc[" << i << "]) acc.cw[0][" << i << "] = evql_combine<" << op_name(updw[i].op)
              << ">(acc.cw[0][" << i << "], o.ub[" << i << "]);\n";
          }
          s << "  }\n";
          s << "  if (miss) {\n";
          s << "    if (acc.cs[0] >= 0) evql_flush_entry<0>(lds, acc);\n";
          s << "    acc.cs[0] = s;\n";
          if (kp.need_first_row) s << "    acc.cfirst[0] = row;\n";
          // (a skipped update carries the identity of its op in o.ub[])
          for (int i = 0; i < U(); ++i) s << "    acc.cw[0][" << i << "] = o.ub[" << i << "];\n";
          s << "  }\n";
        } else {
          s << "  if (s >= 0) {\n";
          s << "    bool hit = false;\n";
          for (int j = 0; j < kp.lane_cache; ++j) {
            s << "    {\n      const bool h = acc.cs[" << j << "] == s;\n      hit = hit || h;\n";
            if (kp.need_first_row) {
              s << "      acc.cfirst[" << j << "] = (h && row < acc.cfirst[" << j << "]) ? row : acc.cfirst["
                << j << "];\n";
            }
            for (int i = 0; i < U(); ++i) {
              s << "      if (h && o.uc[" << i << "]) acc.cw[" << j << "][" << i << "] = evql_combine<"
                << op_name(updw[i].op) << ">(acc.cw[" << j << "][" << i << "], o.ub[" << i << "]);\n";
            }
            s << "    }\n";
          }
          // (the victim is chosen with selects, entry by entry: an if / else-if chain over
          // acc.cv is turned into an indexed access by the optimiser, which puts the
          // accumulators into scratch memory)
          s << "    if (!hit) {\n";
          for (int j = 0; j < kp.lane_cache; ++j) {
            s << "      {\n        const bool v = acc.cv == " << j << "u;\n";
            s << "        if (v && acc.cs[" << j << "] >= 0) evql_flush_entry<" << j << ">(lds, acc);\n";
            s << "        acc.cs[" << j << "] = v ? s : acc.cs[" << j << "];\n";
            if (kp.need_first_row) {
              s << "        acc.cfirst[" << j << "] = v ? row : acc.cfirst[" << j << "];\n";
            }
            for (int i = 0; i < U(); ++i) {
              s << "        acc.cw[" << j << "][" << i << "] = (v && o.uc[" << i << "]) ? o.ub[" << i
                << "] : acc.cw[" << j << "][" << i << "];\n";
            }
            s << "      }\n";
          }
          if (kp.lane_cache > 1) {
            s << "      acc.cv = (acc.cv + 1u) & " << (kp.lane_cache - 1) << "u;\n";
          }
          s << "    }\n  }\n";
        }
        s << "  const bool spill = o.live && s < 0;\n";
        s << "  acc.spilled += spill ? 1 : 0;\n";
      } else {
        s << "  const bool spill = o.live;\n";
      }
      s << "  if (spill) {\n";
      s << "    i64 gs;\n";
      s << "    if (o.knull) { gs = (i64) A.gcap + 1; A.gtab[(u64) gs * EVQL_WORDS] = 0; }\n";
      s << "    else if (o.ident == EVQL_EMPTY) { gs = (i64) A.gcap; A.gtab[(u64) gs * EVQL_WORDS] = 0; }\n";
      if (kp.has_ident2()) {
        s << "    else gs = evql_gtab_find2(A.gtab, EVQL_WORDS, A.gcap, o.ident, o.ident2, "
             "evql_mix64(o.ident));\n";
      } else {
        s << "    else gs = evql_gtab_find(A.gtab, EVQL_WORDS, A.gcap, o.ident, evql_mix64(o.ident));\n";
      }
      s << "    if (gs < 0) { atomicOr(&A.status[0], EVQL_ST_TABLE_FULL); }\n";
      s << "    else {\n";
      updates(true, "gs", "      ");
      s << "    }\n  }\n}\n\n";
    }

    // LDS table init / flush helpers shared with the partition-aggregate kernel
    if (grouped && S > 0) {
      s << "__device__ __forceinline__ void evql_lds_init(u64* lds) {\n";
      s << "  if (threadIdx.x == 0) lds[EVQL_WORDS * EVQL_LSTRIDE] = 0;\n";
      s << "  for (u32 i = threadIdx.x; i < EVQL_LSTRIDE; i += blockDim.x) {\n";
      s << "    lds[i] = EVQL_EMPTY;\n";
      if (kp.has_ident2()) s << "    lds[1 * EVQL_LSTRIDE + i] = EVQL_EMPTY;\n";
      if (kp.need_first_row) {
        s << "    " << lds_word(kp.first_row_word(), "i") << " = 0xFFFFFFFFFFFFFFFFull;\n";
      }
      for (int w = 0; w < NW; ++w) {
        s << "    " << lds_word(SB + w, "i") << " = evql_op_identity<" << op_name(kp.states[w].op)
          << ">();\n";
      }
      s << "  }\n}\n\n";
      // EXCL: the caller owns every group it flushes (a partition bucket: a group
      // lives in exactly one bucket) and nothing of this bucket went to the HBM
      // table directly -- the states are then stored, not combined with atomics
      // (1e7 groups x 4 random HBM atomics cost ~1 ms of the aggregate pass)
      s << "template <bool EXCL>\n";
      s << "__device__ __forceinline__ void evql_lds_flush(const EvqlArgs& A, u64* lds) {\n";
      s << "  const bool excl = EXCL && evql_lds_peek32(reinterpret_cast<const u32*>(&lds[EVQL_WORDS * EVQL_LSTRIDE])) "
           "== 0;\n";
      s << "  for (u32 s = threadIdx.x; s < EVQL_LSTRIDE; s += blockDim.x) {\n";
      s << "    const u64 k = lds[s];\n    if (k == EVQL_EMPTY) continue;\n";
      s << "    i64 gs;\n";
      s << "    if (s == EVQL_LDS_SLOTS) gs = (i64) A.gcap;\n";
      s << "    else if (s == EVQL_LDS_SLOTS + 1) gs = (i64) A.gcap + 1;\n";
      if (kp.has_ident2()) {
        s << "    else gs = evql_gtab_find2(A.gtab, EVQL_WORDS, A.gcap, k, lds[EVQL_LSTRIDE + s], "
             "evql_mix64(k));\n";
      } else {
        s << "    else gs = evql_gtab_find(A.gtab, EVQL_WORDS, A.gcap, k, evql_mix64(k));\n";
      }
      s << "    if (gs < 0) { atomicOr(&A.status[0], EVQL_ST_TABLE_FULL); continue; }\n";
      s << "    if (s >= EVQL_LDS_SLOTS) A.gtab[(u64) gs * EVQL_WORDS] = 0;\n";
      s << "    if (excl) {\n";
      if (kp.need_first_row) {
        s << "      " << gtab_word(kp.first_row_word(), "gs") << " = " << lds_word(kp.first_row_word(), "s")
          << ";\n";
      }
      for (int w = 0; w < NW; ++w) {
        s << "      " << gtab_word(SB + w, "gs") << " = " << lds_word(SB + w, "s") << ";\n";
      }
      s << "      continue;\n    }\n";
      if (kp.need_first_row) {
        s << "    evql_atomic<EVQL_OP_MIN_U64>(&" << gtab_word(kp.first_row_word(), "gs") << ", "
          << lds_word(kp.first_row_word(), "s") << ");\n";
      }
      for (int w = 0; w < NW; ++w) {
        s << "    evql_atomic<" << op_name(kp.states[w].op) << ">(&" << gtab_word(SB + w, "gs") << ", "
          << lds_word(SB + w, "s") << ");\n";
      }
      s << "  }\n}\n\n";
    }

    if (staged()) {
      stage_tuple_text();
      stage_drain_function();
    }

    s << "extern \"C\" __global__ void __launch_bounds__(EVQL_BLOCK) evql_scan_agg(const EvqlArgs A) {\n";
    s << "  const u32 tid = threadIdx.x;\n";
    if (grouped && S > 0) {
      s << "  __shared__ u64 lds[EVQL_WORDS * EVQL_LSTRIDE + 1];\n";
      // (a ring of tuples per wave, behind the table: the staging loop)
      if (staged()) s << "  __shared__ EvqlStaged evql_stage_ring[(EVQL_BLOCK / 64) * EVQL_STAGE_RING];\n";
      s << "  evql_lds_init(lds);\n  __syncthreads();\n";
    } else {
      s << "  u64* lds = nullptr;\n";
    }
    s << "  EvqlAcc acc;\n  acc.passed = 0;\n  acc.spilled = 0;\n";
    if (grouped && S > 0) {
      s << "  acc.cv = 0;\n";
      for (int j = 0; j < kp.lane_cache; ++j) {
        s << "  acc.cs[" << j << "] = -1;\n  acc.cfirst[" << j << "] = 0xFFFFFFFFFFFFFFFFull;\n";
        for (int i = 0; i < U(); ++i) {
          s << "  acc.cw[" << j << "][" << i << "] = evql_op_identity<" << op_name(updw[i].op) << ">();\n";
        }
      }
    }
    if (!grouped) {
      for (int w = 0; w < NW; ++w) {
        s << "  acc.w[" << w << "] = evql_op_identity<" << op_name(kp.states[w].op) << ">();\n";
      }
      if (kp.need_first_row) s << "  acc.first = 0xFFFFFFFFFFFFFFFFull;\n";
    }
    zone_skip_decl("  ");
    window32 = grouped;
    tile_loop_twice("  ", [&] {
    if (kp.prefetch && !zone_test && grouped && S > 0) {
      prefetch_tile_loop();
      return;
    }
    s << "  u32 tile_no = 0;\n";
    s << "  for (u64 t = blockIdx.x; t < A.ntiles; t += gridDim.x, ++tile_no) {\n";
    zone_skip("    ", "");
    if (grouped) {
      // a full HBM table makes the whole launch void (the host grows it and runs
      // again): stop scanning soon after any workgroup has reported it.  Polled every
      // 16th tile only: the agent-scope load is a round trip past the L2 in front of
      // the tile's column loads (an 8192-row tile of narrow columns lasts ~8 us)
      s << "    if ((tile_no & 15u) == 0 && (__hip_atomic_load(&A.status[0], __ATOMIC_RELAXED, "
           "__HIP_MEMORY_SCOPE_AGENT) & EVQL_ST_TABLE_FULL)) break;\n";
    }
    if (grouped && S > 0) {
      s << "    const bool bypass = evql_lds_peek32(reinterpret_cast<const u32*>(&lds[EVQL_WORDS * EVQL_LSTRIDE])) "
           ">= 4u * EVQL_BLOCK;\n";
    } else {
      s << "    const bool bypass = false;\n";
    }
    s << "    const u64 base = (A.tile0 + t) * (u64) EVQL_TILE_ROWS;\n";
    tile_window("    ");
    // (SQ counters, round 2: 55-62 % of the wave cycles of every variant of this kernel are
    // s_waitcnt stalls, VALU 6-11 %, LDS <= 14 % -- each wave drains its memory pipeline at
    // the tile border.  These are shares of WAVE cycles, summed over the four waves that
    // share a SIMD here (one 1024-thread workgroup per CU): a SIMD's VALU issue is busy four
    // times that share of its time -- 71 % for today's config 3 at 18 %, DESIGN.md 6m -- so
    // the instructions per row behind the loads do count.
    // Overlapping a tile's loads with the tile in front of them, by form:
    //  - a RING over the unroll steps (a step's registers refilled with the next tile's rows
    //    right after the step is evaluated) ran 1.2-2.7x SLOWER, conditional or not: with
    //    loads spread over the body, the compiler's waitcnt insertion no longer knows across
    //    the back edge how many are outstanding and emits s_waitcnt vmcnt(0) / vmcnt(1) in
    //    front of every step (76 + 8 of them against vmcnt(14), (13), ... here), i.e. it
    //    serialises the loads.  A ring with hand-placed waits around inline-asm loads (and
    //    scalar page-table loads): config 3 over 16-bit pages 0.360 -> 0.327 ms, but 10-bit
    //    config 2 1.87 -> 3.02 ms and plain config 2 2.42 -> 2.68 ms -- dropped.
    //  - the ROTATING form (prefetch_tile_loop: one cluster for the NEXT tile at the head of
    //    the body, the tile held raw from the iteration before evaluated behind it, one copy
    //    at the end) compiles as written: no vmcnt wait between the cluster and the copy but
    //    in the cold HBM blocks, one vmcnt(0) at the copy.  It needs the tile raw (two tiles
    //    in the registers of one decoded tile), so it serves the plans whose columns are all
    //    narrow / float32 copies (choose_launch_shape); the others keep this loop, one burst
    //    per tile.  DESIGN.md 6o has the measurement.
    tile_loads("    ");
    s << "#pragma unroll\n    for (int u = 0; u < EVQL_UNROLL; ++u) {\n";
    s << "      const u64 r = base + ((u64) (u * EVQL_BLOCK) + tid) * 2;\n";
    scan_step("      ", false);
    s << "    }\n  }\n";
    });
    window32 = true;

    // epilogue
    zone_skip_flush("  ");
    s << "  {\n    const u64 p = evql_wave_reduce<EVQL_OP_ADD_U64>(" << (kp.prefetch ? "(u64) " : "") << "acc.passed);\n";
    s << "    if ((tid & 63u) == 0 && p) atomicAdd(&A.counters[0], p);\n";
    s << "    const u64 sp = evql_wave_reduce<EVQL_OP_ADD_U64>(" << (kp.prefetch ? "(u64) " : "") << "acc.spilled);\n";
    s << "    if ((tid & 63u) == 0 && sp) atomicAdd(&A.counters[1], sp);\n  }\n";
    if (!grouped) {
      // block reduction of the register accumulators, one atomic per word per block
      s << "  __shared__ u64 red[(EVQL_BLOCK / 64) * " << (NW + 1) << "];\n";
      s << "  const u32 wave = tid >> 6;\n";
      for (int w = 0; w < NW; ++w) {
        s << "  { const u64 v = evql_wave_reduce<" << op_name(kp.states[w].op) << ">(acc.w[" << w
          << "]); if ((tid & 63u) == 0) red[wave * " << (NW + 1) << " + " << w << "] = v; }\n";
      }
      s << "  { const u64 v = evql_wave_reduce<EVQL_OP_ADD_U64>(acc.passed); if ((tid & 63u) == 0) "
           "red[wave * "
        << (NW + 1) << " + " << NW << "] = v; }\n";
      if (kp.need_first_row) {
        s << "  { const u64 v = evql_wave_reduce<EVQL_OP_MIN_U64>(acc.first); if ((tid & 63u) == 0 && "
             "v != 0xFFFFFFFFFFFFFFFFull) evql_atomic<EVQL_OP_MIN_U64>(&A.gtab["
          << kp.first_row_word() << "], v); }\n";
      }
      s << "  __syncthreads();\n";
      s << "  if (tid == 0) {\n";
      s << "    u64 any = 0;\n";
      s << "    for (u32 k = 0; k < EVQL_BLOCK / 64; ++k) any += red[k * " << (NW + 1) << " + " << NW
        << "];\n";
      s << "    if (any) {\n      A.gtab[0] = 0;\n";
      for (int w = 0; w < NW; ++w) {
        s << "      { u64 v = red[" << w << "]; for (u32 k = 1; k < EVQL_BLOCK / 64; ++k) v = evql_combine<"
          << op_name(kp.states[w].op) << ">(v, red[k * " << (NW + 1) << " + " << w
          << "]); evql_atomic<" << op_name(kp.states[w].op) << ">(&A.gtab[" << (SB + w)
          << "], v); }\n";
      }
      s << "    }\n  }\n";
    } else if (S > 0) {
      s << "  evql_flush_private(lds, acc);\n";
      s << "  __syncthreads();\n";
      s << "  evql_lds_flush<false>(A, lds);\n";
    }
    s << "}\n\n";
  }

  // ---- bare scans: SELECT .. WHERE without GROUP BY / aggregates ---------------------------
  //
  // The passing rows leave the device in ROW ORDER (a LIMIT above the scan depends on it),
  // so the hash-ordered scatter machinery above does not apply.  Two passes over the tiles,
  // no waiting between workgroups (no look-back, no spinning on another workgroup's flag):
  //
  //   evql_scan_count  predicate of every row (only the columns WHERE reads are loaded),
  //                    passing rows per tile -> tile_count[t]; the host scans the counts
  //   evql_scan_emit   over a contiguous tile range (a window): predicate again, rank of
  //                    every passing row inside its tile (row order is (u, tid, j): one
  //                    ballot per (u, j), mbcnt for the lanes below, wave totals through
  //                    LDS), select expressions of the passing rows staged in LDS in rank
  //                    order, then the tile's run stored at tile_offset[t] - window_base:
  //                    consecutive lanes store consecutive elements, 16 bytes per lane
  //
  // Output per select expression: one u64 word (strings: length << 40 | position) and, for
  // expressions that can be NULL, one tag byte per passing row.
  void bare_scan_kernels() {
    const int NOUT = int(kp.scan_out.size());
    std::vector<bool> where_cols(size_t(NC), false);
    if (kp.where) {
      std::vector<uint32_t> used;
      expr_inputs(kp.where, &used);
      for (uint32_t u : used) {
        if (u < uint32_t(NC)) where_cols[u] = true;
      }
    }
    int n_nullable = 0;
    for (int k = 0; k < NOUT; ++k) n_nullable += kp.scan_out_nullable[k] ? 1 : 0;
    // how many unroll steps are staged in LDS at once: the whole tile when its values fit
    // 48 KiB (runs of up to a tile per store phase, two barriers per tile), else one step
    const int stage_steps =
        uint64_t(kp.tile_rows()) * uint64_t(8 * NOUT + n_nullable) <= 48 * 1024 ? kp.unroll : 1;
    s << "#define EVQL_NOUT " << NOUT << "\n";
    s << "#define EVQL_NWAVE (EVQL_BLOCK / 64)\n";
    s << "#define EVQL_STAGE_STEPS " << stage_steps << "\n";
    s << "#define EVQL_STAGE_ROWS (EVQL_STAGE_STEPS * EVQL_BLOCK * 2)\n";
    s << "static_assert(EVQL_UNROLL * EVQL_NWAVE <= 64, \"one wave scans the wave totals of a tile\");\n";
    // (host mirror: HostScanArgs in bare_scan.cc)
    s << "struct EvqlScanArgs {\n"
         "  const u64* tile_offset;  // [ntiles + 1]: passing rows in front of tile t of the scan\n"
         "  u64 t0, t1;              // the window: tiles [t0, t1)\n"
         "  u64 window_base;         // tile_offset[t0]\n"
         "  u64 window_rows;         // tile_offset[t1] - window_base: rows of every output array\n"
         "  u64* words;              // [EVQL_NOUT][window_rows]\n"
         "  u8* tags;                // [EVQL_NOUT][window_rows], written for nullable outputs only\n"
         "};\n\n";
    // values of the select list for one passing row
    row_function(n_literals, [&](Emitter& em) {
      s << "__device__ __forceinline__ void evql_scan_select(const EvqlArgs& A, const u64 row";
      for (int i = 0; i < NC; ++i) s << ", const u64 r" << i << ", const u32 g" << i;
      s << ", u64 (&w)[EVQL_NOUT], u32 (&q)[EVQL_NOUT]) {\n";
      col_decls();
      em.ind = "  ";
      for (int k = 0; k < NOUT; ++k) {
        const ExprPtr& e = kp.scan_out[k];
        if (e->kind == Expr::INPUT && e->type == EVQL_T_STRING) {
          // a string travels as the (length << 40 | position) word of its bytes
          s << "  w[" << k << "] = A.col[" << e->input << "].strpos[row]; q[" << k << "] = g" << e->input
            << ";\n";
          continue;
        }
        Val v = em.emit(e);
        s << em.o.str();
        em.o.str("");
        s << "  w[" << k << "] = " << Emitter::as_bits(v) << "; q[" << k << "] = " << v.g << ";\n";
      }
      s << "}\n\n";
    });
    // n elements of 8 bytes from LDS to out[at, at + n): an element in front of the first
    // 16-byte boundary and one behind the last go alone, the pairs between them as 16 bytes
    // per lane.  Nothing is stored at or behind out[cap].
    s << "__device__ __forceinline__ void evql_run_store(u64* out, const u64 at, const u64 cap, const u64* src, "
         "u32 n) {\n"
         "  typedef u64 evql_u64x2 __attribute__((ext_vector_type(2)));\n"
         "  if (at >= cap) return;\n"
         "  if ((u64) n > cap - at) n = (u32) (cap - at);\n"
         "  u64* const dst = out + at;\n"
         "  const u32 head = (n > 0 && ((u64) dst & 8ull)) ? 1u : 0u;\n"
         "  const u32 pairs = (n - head) >> 1;\n"
         "  if (threadIdx.x == 0 && head) dst[0] = src[0];\n"
         "  for (u32 i = threadIdx.x; i < pairs; i += EVQL_BLOCK) {\n"
         "    evql_u64x2 v;\n    v.x = src[head + 2 * i];\n    v.y = src[head + 2 * i + 1];\n"
         "    *reinterpret_cast<evql_u64x2*>(dst + head + 2 * i) = v;\n  }\n"
         "  if (threadIdx.x == 0 && ((n - head) & 1u)) dst[n - 1] = src[n - 1];\n"
         "}\n\n";

    // pass 1
    s << "extern \"C\" __global__ void __launch_bounds__(EVQL_BLOCK) evql_scan_count(const EvqlArgs A, "
         "u32* tile_count) {\n";
    s << "  const u32 tid = threadIdx.x;\n";
    s << "  __shared__ u32 wsum[EVQL_NWAVE];\n";
    zone_skip_decl("  ");
    window32 = false;
    tile_loop_twice("  ", [&] {
    s << "  for (u64 t = blockIdx.x; t < A.ntiles; t += gridDim.x) {\n";
    // (the host does not clear tile_count: a skipped tile still stores its 0)
    zone_skip("    ", "if (tid == 0) tile_count[t] = 0;");
    s << "    const u64 base = (A.tile0 + t) * (u64) EVQL_TILE_ROWS;\n";
    tile_window("    ");
    tile_loads("    ", &where_cols);
    s << "    u32 cnt = 0;\n";
    s << "#pragma unroll\n    for (int u = 0; u < EVQL_UNROLL; ++u) {\n";
    s << "      const u64 r = base + ((u64) (u * EVQL_BLOCK) + tid) * 2;\n";
    s << "      EvqlRowOut o;\n";
    for (int j = 0; j < 2; ++j) {
      eval_call("      ", j, &where_cols);
      s << "      cnt += (u32) __popcll(__ballot(o.live));\n";
    }
    s << "    }\n";
    s << "    if ((tid & 63u) == 0) wsum[tid >> 6] = cnt;\n";
    s << "    __syncthreads();\n";
    s << "    if (tid == 0) {\n      u32 total = 0;\n";
    s << "      for (u32 k = 0; k < EVQL_NWAVE; ++k) total += wsum[k];\n";
    s << "      tile_count[t] = total;\n    }\n";
    s << "    __syncthreads();\n";
    s << "  }\n";
    });
    window32 = true;
    zone_skip_flush("  ");
    s << "}\n\n";

    // pass 2
    s << "extern \"C\" __global__ void __launch_bounds__(EVQL_BLOCK) evql_scan_emit(const EvqlArgs A, "
         "const EvqlScanArgs S) {\n";
    s << "  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;\n";
    s << "  __shared__ u64 sw[EVQL_NOUT * EVQL_STAGE_ROWS];\n";
    if (n_nullable) s << "  __shared__ u8 sq[" << n_nullable << " * EVQL_STAGE_ROWS];\n";
    // exclusive prefix of the passing rows of (step u, wave) in row order; [last] = the tile's
    s << "  __shared__ u32 wpre[EVQL_UNROLL * EVQL_NWAVE + 1];\n";
    s << "  for (u64 t = S.t0 + blockIdx.x; t < S.t1; t += gridDim.x) {\n";
    // (a tile without passing rows -- selective predicates -- is not read again)
    s << "    const u64 dst0 = S.tile_offset[t] - S.window_base;\n";
    s << "    if (S.tile_offset[t + 1] == S.tile_offset[t]) continue;\n";
    s << "    const u64 base = (A.tile0 + t) * (u64) EVQL_TILE_ROWS;\n";
    tile_window("    ");
    tile_loads("    ");
    s << "    u32 live = 0;  // bit 2u + j: row (u, j) of this lane passes\n";
    s << "#pragma unroll\n    for (int u = 0; u < EVQL_UNROLL; ++u) {\n";
    s << "      const u64 r = base + ((u64) (u * EVQL_BLOCK) + tid) * 2;\n";
    s << "      EvqlRowOut o;\n";
    s << "      u32 wcnt = 0;\n";
    for (int j = 0; j < 2; ++j) {
      eval_call("      ", j);
      s << "      live |= o.live ? (1u << (2 * u + " << j << ")) : 0u;\n";
      s << "      wcnt += (u32) __popcll(__ballot(o.live));\n";
    }
    s << "      if (lane == 0) wpre[u * EVQL_NWAVE + wave] = wcnt;\n";
    s << "    }\n    __syncthreads();\n";
    s << "    if (wave == 0) {\n";
    s << "      const u32 v = lane < EVQL_UNROLL * EVQL_NWAVE ? wpre[lane] : 0u;\n";
    s << "      u32 incl = v;\n";
    s << "#pragma unroll\n      for (int d = 1; d < 64; d <<= 1) { const u32 x = __shfl_up(incl, d, 64); "
         "if ((int) lane >= d) incl += x; }\n";
    s << "      if (lane < EVQL_UNROLL * EVQL_NWAVE) wpre[lane] = incl - v;\n";
    s << "      if (lane == EVQL_UNROLL * EVQL_NWAVE - 1) wpre[EVQL_UNROLL * EVQL_NWAVE] = incl;\n";
    s << "    }\n    __syncthreads();\n";
    s << "#pragma unroll\n    for (int u0 = 0; u0 < EVQL_UNROLL; u0 += EVQL_STAGE_STEPS) {\n";
    s << "      const u32 g0 = wpre[u0 * EVQL_NWAVE], g1 = wpre[(u0 + EVQL_STAGE_STEPS) * EVQL_NWAVE];\n";
    s << "#pragma unroll\n      for (int u = u0; u < u0 + EVQL_STAGE_STEPS; ++u) {\n";
    s << "        const u64 r = base + ((u64) (u * EVQL_BLOCK) + tid) * 2;\n";
    s << "        const bool l0 = (live >> (2 * u)) & 1u, l1 = (live >> (2 * u + 1)) & 1u;\n";
    s << "        const u64 b0 = __ballot(l0), b1 = __ballot(l1);\n";
    s << "        u32 rank = wpre[u * EVQL_NWAVE + wave] - g0;\n";
    s << "        rank = __builtin_amdgcn_mbcnt_hi((u32) (b0 >> 32), __builtin_amdgcn_mbcnt_lo((u32) b0, rank));\n";
    s << "        rank = __builtin_amdgcn_mbcnt_hi((u32) (b1 >> 32), __builtin_amdgcn_mbcnt_lo((u32) b1, rank));\n";
    for (int j = 0; j < 2; ++j) {
      s << "        if (l" << j << ") {\n";
      s << "          u64 w[EVQL_NOUT]; u32 q[EVQL_NOUT];\n";
      s << "          evql_scan_select(A, r + " << j;
      for (int i = 0; i < NC; ++i) s << ", x" << i << "[u][" << j << "], y" << i << "[u][" << j << "]";
      s << ", w, q);\n";
      int nk = 0;
      for (int k = 0; k < NOUT; ++k) {
        s << "          sw[" << k << " * EVQL_STAGE_ROWS + rank] = w[" << k << "];\n";
        if (kp.scan_out_nullable[k]) {
          s << "          sq[" << nk++ << " * EVQL_STAGE_ROWS + rank] = (u8) (q[" << k << "] & 1u);\n";
        }
      }
      s << "          rank += 1;\n        }\n";
    }
    s << "      }\n      __syncthreads();\n";
    s << "      const u32 n = g1 - g0;\n";
    s << "      const u64 at = dst0 + g0;\n";
    {
      int nk = 0;
      for (int k = 0; k < NOUT; ++k) {
        s << "      evql_run_store(S.words + " << k << " * S.window_rows, at, S.window_rows, sw + " << k
          << " * EVQL_STAGE_ROWS, n);\n";
        if (kp.scan_out_nullable[k]) {
          s << "      for (u32 i = tid; i < n && at + i < S.window_rows; i += EVQL_BLOCK) S.tags[" << k
            << " * S.window_rows + at + i] = sq[" << nk++ << " * EVQL_STAGE_ROWS + i];\n";
        }
      }
    }
    s << "      __syncthreads();\n";
    s << "    }\n  }\n}\n\n";
  }

  // ---- predicate of every row (nested scans, see KernelPlan::where_rows_kernel) -------------
  void where_rows_kernel() {
    s << "extern \"C\" __global__ void __launch_bounds__(EVQL_BLOCK) evql_where_rows(const EvqlArgs A, "
         "u8* acc) {\n";
    s << "  const u32 tid = threadIdx.x;\n";
    s << "  for (u64 t = blockIdx.x; t < A.ntiles; t += gridDim.x) {\n";
    s << "    const u64 base = (A.tile0 + t) * (u64) EVQL_TILE_ROWS;\n";
    tile_window("    ");
    tile_loads("    ");
    s << "#pragma unroll\n    for (int u = 0; u < EVQL_UNROLL; ++u) {\n";
    s << "      const u64 r = base + ((u64) (u * EVQL_BLOCK) + tid) * 2;\n";
    s << "      EvqlRowOut o;\n";
    for (int j = 0; j < 2; ++j) {
      eval_call("      ", j);
      s << "      if (r + " << j << " < A.row_end) acc[r + " << j << "] = o.live ? 1 : 0;\n";
    }
    s << "    }\n  }\n}\n\n";
  }

  // ---- partitioned high-cardinality path ----------------------------------------------
  //
  // workgroup w owns the contiguous tile range [w*tpw, (w+1)*tpw) in BOTH passes,
  // so the per-(bucket, workgroup) counts of the first pass give every workgroup
  // exact, disjoint output positions in the second: no global atomics, only an
  // LDS cursor per bucket.
  void partition_kernels() {
    const int frw = kp.first_row_word();
    s << "#define EVQL_PBITS " << kp.part_bits << "\n#define EVQL_NPART " << (1 << kp.part_bits)
      << "\n";
    s << "__device__ __forceinline__ u32 evql_bucket(u64 ident) { return (u32) (evql_mix64(ident ^ "
         "0x5851f42d4c957f2dull) >> (64 - EVQL_PBITS)); }\n\n";
    // arguments shared by the three kernels (host mirror: PartArgs in runtime.h)
    // Two-level scatter.  Writing tuples straight into 4096 buckets leaves every
    // (workgroup, bucket) stream advancing by ~2 tuples per tile: lines linger half
    // written in L2 and the scatter ran at 2 TB/s.  Instead tuples first go into
    // NCOARSE = 64 coarse buckets (the top bits of the bucket id, so a coarse
    // bucket is a contiguous run of fine buckets), each tile reserving one
    // contiguous range per coarse bucket with a single global atomic (~128 tuples
    // = 4 KB written at once), and a second pass (evql_part_refine) moves every
    // coarse bucket's tuples into its fine buckets the same way.
    const int cbits = kp.part_bits <= 8 ? kp.part_bits : 6;
    const int fbits = kp.part_bits - cbits;
    s << "#define EVQL_CBITS " << cbits << "\n#define EVQL_FBITS " << fbits << "\n";
    s << "#define EVQL_NCOARSE " << (1 << cbits) << "\n#define EVQL_NFINE " << (1 << fbits) << "\n";
    s << "struct EvqlPartArgs {\n  u64 tiles_per_wg;\n  u32* counts;      // [bucket][workgroup]\n"
         "  const u64* bucket_start;  // [NPART + 1] tuple index\n  u64* tuples;\n  u64 nwg;\n"
         "  u64* tuples_tmp;  // coarse-bucket order (two-level only)\n"
         "  u32* cursors;     // [NCOARSE] + [NPART] reservation cursors, zeroed per launch\n"
         "  u64* dense;       // dense group records [kind, identity, ...] of the buckets\n"
         "  u64 dense_cap;    // ... whose groups all fitted the LDS table (records)\n"
         "  u64 coarse_cap;   // fused form: capacity (tuples) of every coarse bucket of tuples_tmp\n};\n\n";
    // Fused form (kp.part_fused): no count pass.  The count pass re-read every column only
    // to give the scatter exact offsets (1.09 GB / 0.18 ms of config 4's 2.85 ms).  Instead
    // every coarse bucket owns a fixed, slack-allocated range of tuples_tmp -- the hash
    // spreads the tuples evenly, a range that overflows anyway (one dominant key) voids the
    // launch and the host falls back to exact offsets -- and the FINE bucket sizes, which
    // refine and aggregate need exactly, are counted in LDS while the tuples are scattered
    // and added up in bucket_start[], which the host scans before refine runs.
    const bool fused = kp.part_fused && fbits > 0;
    s << "#define EVQL_ST_PART_OVERFLOW 64u\n";
    if (fused) {
      s << "#define EVQL_CSTART(c_) ((u64) (c_) * P.coarse_cap)\n";
      // (a bucket that overflowed its slack voided the launch: its cursor ran past the range)
      s << "#define EVQL_CEND(c_) ((u64) (c_) * P.coarse_cap + ((u64) P.cursors[c_] < P.coarse_cap ? "
           "(u64) P.cursors[c_] : P.coarse_cap))\n";
    } else {
      s << "#define EVQL_CSTART(c_) (P.bucket_start[(u64) (c_) << EVQL_FBITS])\n";
      s << "#define EVQL_CEND(c_) (P.bucket_start[(u64) ((c_) + 1) << EVQL_FBITS])\n";
    }
    // a tuple is EVQL_TUPLE_U32 32-bit words, moved with the widest aligned vector
    // access (16 bytes when the tuple size is a multiple of 16)
    s << "__device__ __forceinline__ void evql_tuple_store(u32* p, const u32* v) {\n"
         "#pragma unroll\n"
         "  for (int x = 0; x < EVQL_TUPLE_U32; x += (EVQL_TUPLE_U32 % 4 == 0 ? 4 : 2)) {\n"
         "    if (EVQL_TUPLE_U32 % 4 == 0) *reinterpret_cast<uint4*>(p + x) = make_uint4(v[x], v[x + 1], "
         "v[x + 2], v[x + 3]);\n"
         "    else *reinterpret_cast<uint2*>(p + x) = make_uint2(v[x], v[x + 1]);\n  }\n}\n";
    s << "__device__ __forceinline__ void evql_tuple_load(const u32* p, u32* v) {\n"
         "#pragma unroll\n"
         "  for (int x = 0; x < EVQL_TUPLE_U32; x += (EVQL_TUPLE_U32 % 4 == 0 ? 4 : 2)) {\n"
         "    if (EVQL_TUPLE_U32 % 4 == 0) { const uint4 t = *reinterpret_cast<const uint4*>(p + x); "
         "v[x] = t.x; v[x + 1] = t.y; v[x + 2] = t.z; v[x + 3] = t.w; }\n"
         "    else { const uint2 t = *reinterpret_cast<const uint2*>(p + x); v[x] = t.x; v[x + 1] = "
         "t.y; }\n  }\n}\n\n";

    // pass 1: histogram
    if (!fused) {
    s << "extern \"C\" __global__ void __launch_bounds__(EVQL_BLOCK) evql_part_count(const EvqlArgs A, "
         "const EvqlPartArgs P) {\n";
    s << "  const u32 tid = threadIdx.x;\n";
    s << "  __shared__ u32 hist[EVQL_NPART];\n";
    s << "  for (u32 i = tid; i < EVQL_NPART; i += EVQL_BLOCK) hist[i] = 0;\n  __syncthreads();\n";
    s << "  const u64 t0 = (u64) blockIdx.x * P.tiles_per_wg;\n";
    s << "  const u64 t1 = t0 + P.tiles_per_wg < A.ntiles ? t0 + P.tiles_per_wg : A.ntiles;\n";
    window32 = false;
    tile_loop_twice("  ", [&] {
    s << "  for (u64 t = t0; t < t1; ++t) {\n";
    zone_skip("    ", "", false);  // (counted by the scatter pass)
    s << "    const u64 base = (A.tile0 + t) * (u64) EVQL_TILE_ROWS;\n";
    tile_window("    ");
    tile_loads("    ");
    s << "#pragma unroll\n    for (int u = 0; u < EVQL_UNROLL; ++u) {\n";
    s << "      const u64 r = base + ((u64) (u * EVQL_BLOCK) + tid) * 2;\n";
    s << "      EvqlRowOut o;\n";
    for (int j = 0; j < 2; ++j) {
      eval_call("      ", j);
      s << "      if (o.live) atomicAdd(&hist[evql_bucket(o.ident)], 1u);\n";
    }
    s << "    }\n  }\n";
    });
    window32 = true;
    s << "  __syncthreads();\n";
    s << "  for (u32 i = tid; i < EVQL_NPART; i += EVQL_BLOCK) P.counts[(u64) i * P.nwg + blockIdx.x] = "
         "hist[i];\n";
    s << "}\n\n";
    }

    // pass 2: scatter tuples.  counts[b][w] now holds the exclusive prefix of
    // workgroup w inside bucket b
    // (tried: sorting a sub-tile's tuples by coarse bucket in 128 KB of LDS and storing
    // the runs coalesced, as refine does -- 0.99-1.00 ms against 0.99-1.05 ms: the runs
    // of this pass are 2 KB already and the gain is within the run-to-run spread)
    s << "extern \"C\" __global__ void __launch_bounds__(EVQL_BLOCK) evql_part_scatter(const EvqlArgs A, "
         "const EvqlPartArgs P) {\n";
    s << "  const u32 tid = threadIdx.x;\n";
    s << "  __shared__ u32 hist[EVQL_NCOARSE];\n";
    s << "  __shared__ u64 gbase[EVQL_NCOARSE];\n";
    if (fused) {
      s << "  __shared__ u32 fhist[EVQL_NPART];\n";
      s << "  for (u32 i = tid; i < EVQL_NPART; i += EVQL_BLOCK) fhist[i] = 0;\n";
    }
    s << "  u32* const dst = reinterpret_cast<u32*>(EVQL_FBITS ? P.tuples_tmp : P.tuples);\n";
    s << "  u64 passed = 0;\n";
    s << "  const u64 t0 = (u64) blockIdx.x * P.tiles_per_wg;\n";
    s << "  const u64 t1 = t0 + P.tiles_per_wg < A.ntiles ? t0 + P.tiles_per_wg : A.ntiles;\n";
    zone_skip_decl("  ");
    tile_loop_twice("  ", [&] {
    s << "  for (u64 t = t0; t < t1; ++t) {\n";
    zone_skip("    ", "");
    s << "    const u64 base = (A.tile0 + t) * (u64) EVQL_TILE_ROWS;\n";
    tile_window("    ");
    tile_loads("    ");
    // sweep 1: how many tuples of this tile go to each coarse bucket
    s << "    for (u32 i = tid; i < EVQL_NCOARSE; i += EVQL_BLOCK) hist[i] = 0;\n";
    s << "    __syncthreads();\n";
    s << "#pragma unroll\n    for (int u = 0; u < EVQL_UNROLL; ++u) {\n";
    s << "      const u64 r = base + ((u64) (u * EVQL_BLOCK) + tid) * 2;\n";
    s << "      EvqlRowOut o;\n";
    for (int j = 0; j < 2; ++j) {
      eval_call("      ", j);
      s << "      if (o.live) atomicAdd(&hist[evql_bucket(o.ident) >> EVQL_FBITS], 1u);\n";
    }
    s << "    }\n    __syncthreads();\n";
    // one contiguous range per coarse bucket for the whole tile
    s << "    for (u32 i = tid; i < EVQL_NCOARSE; i += EVQL_BLOCK) {\n";
    s << "      const u32 c = hist[i];\n";
    if (fused) {
      s << "      u64 gb = EVQL_EMPTY;\n";
      s << "      if (c) {\n";
      s << "        const u64 at = (u64) atomicAdd(&P.cursors[i], c);\n";
      s << "        if (at + c <= P.coarse_cap) gb = (u64) i * P.coarse_cap + at;\n";
      s << "        else atomicOr(&A.status[0], EVQL_ST_PART_OVERFLOW);\n";
      s << "      }\n";
      s << "      gbase[i] = gb;\n";
    } else {
      s << "      gbase[i] = P.bucket_start[(u64) i << EVQL_FBITS] + (c ? (u64) atomicAdd(&P.cursors[i], c) "
           ": 0ull);\n";
    }
    s << "      hist[i] = 0;\n    }\n    __syncthreads();\n";
    // sweep 2: write
    s << "#pragma unroll\n    for (int u = 0; u < EVQL_UNROLL; ++u) {\n";
    s << "      const u64 r = base + ((u64) (u * EVQL_BLOCK) + tid) * 2;\n";
    s << "      EvqlRowOut o;\n";
    for (int j = 0; j < 2; ++j) {
      eval_call("      ", j);
      s << "      if (o.live) {\n";
      s << "        passed += 1;\n";
      if (fused) {
        s << "        const u32 fb = evql_bucket(o.ident);\n";
        s << "        const u32 b = fb >> EVQL_FBITS;\n";
        s << "        atomicAdd(&fhist[fb], 1u);\n";
      } else {
        s << "        const u32 b = evql_bucket(o.ident) >> EVQL_FBITS;\n";
      }
      s << "        const u64 pos = gbase[b] + atomicAdd(&hist[b], 1u);\n";
      s << "        u32 tv[EVQL_TUPLE_U32];\n";
      s << "        tv[EVQL_TUPLE_U32 - 1] = 0;\n";  // (the padding word of an odd layout)
      tuple_put("        ", off_ident, kp.narrow_ident, "o.ident");
      if (kp.has_ident2()) tuple_put("        ", off_ident2, false, "o.ident2");
      if (kp.need_first_row) {
        tuple_put("        ", off_row, kp.narrow_first_row, "r + " + std::to_string(j));
      }
      for (int i = 0; i < U(); ++i) {
        if (updw[i].tslot < 0) continue;
        tuple_put("        ", updw[i].toff, updw[i].narrow, "o.ub[" + std::to_string(i) + "]");
      }
      if (fused) {
        // (a coarse bucket beyond its slack: the launch is void, nothing may be written)
        s << "        if (gbase[b] != EVQL_EMPTY) evql_tuple_store(dst + pos * EVQL_TUPLE_U32, tv);\n";
      } else {
        s << "        evql_tuple_store(dst + pos * EVQL_TUPLE_U32, tv);\n";
      }
      s << "      }\n";
    }
    s << "    }\n    __syncthreads();\n  }\n";
    });
    if (fused) {
      // this workgroup's fine-bucket counts -> the global sizes (scanned by the host's
      // launch_exclusive_scan into bucket_start[] before refine runs)
      s << "  __syncthreads();\n";
      s << "  for (u32 i = tid; i < EVQL_NPART; i += EVQL_BLOCK) {\n";
      s << "    const u32 c = fhist[i];\n";
      s << "    if (c) atomicAdd(const_cast<u64*>(&P.bucket_start[i]), (u64) c);\n  }\n";
    }
    zone_skip_flush("  ");
    s << "  { const u64 p = evql_wave_reduce<EVQL_OP_ADD_U64>(passed);\n";
    s << "    if ((tid & 63u) == 0 && p) atomicAdd(&A.counters[0], p); }\n";
    s << "}\n\n";

    // pass 2b: coarse bucket -> its fine buckets, chunk by chunk
    if (fbits > 0) {
      const int TWn = tuple_u32;
      // tuples per thread and chunk: the chunk is staged in LDS (<= 64 KB, two workgroups
      // per CU)
      const int rtif = TWn <= 4 ? 4 : (TWn <= 8 ? 2 : 1);
      s << "#define EVQL_RTIF " << rtif << "\n";
      s << "extern \"C\" __global__ void __launch_bounds__(EVQL_BLOCK) evql_part_refine(const EvqlArgs "
           "A, const EvqlPartArgs P) {\n";
      s << "  const u32 tid = threadIdx.x;\n";
      if (fused) {
        // A coarse bucket outgrew its slack (skewed keys): some tuples were never written,
        // the fine-bucket sizes no longer describe what the ranges hold, and sorting that
        // into P.tuples could leave the buffer.  The host runs the plan again with exact
        // offsets (query_finish); nothing of this launch is read.
        s << "  if (__hip_atomic_load(&A.status[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & "
             "EVQL_ST_PART_OVERFLOW) return;\n";
      }
      s << "  __shared__ u32 hist[EVQL_NFINE];\n";
      s << "  __shared__ u32 lpos[EVQL_NFINE + 1];\n";
      s << "  __shared__ u64 gbase[EVQL_NFINE];\n";
      s << "  __shared__ u32 stage[EVQL_BLOCK * EVQL_RTIF * " << TWn << "];\n";
      s << "  const u64 CH = (u64) EVQL_BLOCK * EVQL_RTIF;\n";
      // The chunks of a workgroup -- chunk blockIdx, blockIdx + grid, ... of every coarse
      // bucket in turn -- are software-pipelined: the tuples of the next chunk are
      // requested before the current one is processed.  A chunk is sorted by fine bucket
      // in LDS and written out in that order, so that consecutive lanes store consecutive
      // tuples of one bucket's run: the 16-byte stores of a wave coalesce into whole
      // lines instead of reaching L2 as 64 separate partial-line writes (the L2 request
      // rate, not the bytes, bounded the unsorted version).
      s << "#define EVQL_REFINE_SEEK(c_, n1_, ch_) while (c_ < EVQL_NCOARSE && ch_ >= n1_) { ++c_; if (c_ < "
           "EVQL_NCOARSE) { ch_ = EVQL_CSTART(c_) + (u64) blockIdx.x * CH; n1_ = EVQL_CEND(c_); } }\n";
      s << "#define EVQL_REFINE_LOAD(dst_, ch_, n1_) _Pragma(\"unroll\") for (int k = 0; k < EVQL_RTIF; ++k) { "
           "const u64 i = ch_ + tid + (u64) k * EVQL_BLOCK; if (i < n1_) evql_tuple_load(reinterpret_cast<const "
           "u32*>(P.tuples_tmp) + i * " << TWn << ", dst_[k]); }\n";
      s << "  u32 c = 0;\n";
      s << "  u64 n1 = EVQL_CEND(0);\n";
      s << "  u64 ch = EVQL_CSTART(0) + (u64) blockIdx.x * CH;\n";
      s << "  EVQL_REFINE_SEEK(c, n1, ch)\n";
      s << "  u32 w[EVQL_RTIF][" << TWn << "];\n";
      s << "  if (c < EVQL_NCOARSE) { EVQL_REFINE_LOAD(w, ch, n1) }\n";
      s << "  while (c < EVQL_NCOARSE) {\n";
      s << "    u32 c2 = c;\n    u64 m1 = n1;\n    u64 ch2 = ch + (u64) gridDim.x * CH;\n";
      s << "    EVQL_REFINE_SEEK(c2, m1, ch2)\n";
      s << "    u32 w2[EVQL_RTIF][" << TWn << "];\n";
      s << "    if (c2 < EVQL_NCOARSE) { EVQL_REFINE_LOAD(w2, ch2, m1) }\n";
      s << "    {\n";
      s << "      const u32 cnt = (u32) (n1 - ch < CH ? n1 - ch : CH);\n";
      s << "      for (u32 i = tid; i < EVQL_NFINE; i += EVQL_BLOCK) hist[i] = 0;\n";
      s << "      __syncthreads();\n";
      s << "      u32 f[EVQL_RTIF];\n";
      s << "#pragma unroll\n      for (int k = 0; k < EVQL_RTIF; ++k) {\n";
      s << "        f[k] = 0xffffffffu;\n";
      s << "        if (tid + (u32) k * EVQL_BLOCK < cnt) {\n";
      s << "          f[k] = evql_bucket(" << tuple_ident("w[k]") << ") & (EVQL_NFINE - 1);\n";
      s << "          atomicAdd(&hist[f[k]], 1u);\n        }\n      }\n";
      s << "      __syncthreads();\n";
      // reservation in the fine buckets + positions of the buckets' runs inside the chunk
      s << "      for (u32 i = tid; i < EVQL_NFINE; i += EVQL_BLOCK) {\n";
      s << "        const u32 n = hist[i];\n";
      s << "        const u64 fb = ((u64) c << EVQL_FBITS) + i;\n";
      s << "        gbase[i] = P.bucket_start[fb] + (n ? (u64) atomicAdd(&P.cursors[EVQL_NCOARSE + fb], n) "
           ": 0ull);\n      }\n";
      s << "      if (tid < 64) {\n";  // one wave scans the (<= 256) bucket counts
      s << "        u32 run = 0;\n";
      s << "        for (u32 b0 = 0; b0 < EVQL_NFINE; b0 += 64) {\n";
      s << "          const u32 v = b0 + tid < EVQL_NFINE ? hist[b0 + tid] : 0u;\n";
      s << "          u32 incl = v;\n";
      s << "#pragma unroll\n          for (int d = 1; d < 64; d <<= 1) { const u32 t = __shfl_up(incl, d, 64); "
           "if ((int) tid >= d) incl += t; }\n";
      s << "          if (b0 + tid < EVQL_NFINE) lpos[b0 + tid] = run + incl - v;\n";
      s << "          run += __shfl(incl, 63, 64);\n        }\n      }\n";
      s << "      __syncthreads();\n";
      s << "      for (u32 i = tid; i < EVQL_NFINE; i += EVQL_BLOCK) hist[i] = 0;\n";
      s << "      __syncthreads();\n";
      s << "#pragma unroll\n      for (int k = 0; k < EVQL_RTIF; ++k) {\n";
      s << "        if (f[k] != 0xffffffffu) {\n";
      s << "          const u32 sl = lpos[f[k]] + atomicAdd(&hist[f[k]], 1u);\n";
      s << "#pragma unroll\n          for (int x = 0; x < " << TWn << "; ++x) stage[sl * " << TWn
        << " + x] = w[k][x];\n";
      s << "        }\n      }\n      __syncthreads();\n";
      s << "#pragma unroll\n      for (int k = 0; k < EVQL_RTIF; ++k) {\n";
      s << "        const u32 sl = tid + (u32) k * EVQL_BLOCK;\n";
      s << "        if (sl < cnt) {\n";
      s << "          u32 tv[" << TWn << "];\n";
      s << "#pragma unroll\n          for (int x = 0; x < " << TWn << "; ++x) tv[x] = stage[sl * " << TWn
        << " + x];\n";
      s << "          const u32 fb = evql_bucket(" << tuple_ident("tv") << ") & (EVQL_NFINE - 1);\n";
      s << "          evql_tuple_store(reinterpret_cast<u32*>(P.tuples) + (gbase[fb] + (sl - lpos[fb])) * "
        << TWn << ", tv);\n";
      s << "        }\n      }\n      __syncthreads();\n";
      s << "    }\n";
      s << "#pragma unroll\n    for (int k = 0; k < EVQL_RTIF; ++k) {\n";
      s << "#pragma unroll\n      for (int x = 0; x < " << TWn << "; ++x) w[k][x] = w2[k][x];\n    }\n";
      s << "    c = c2;\n    n1 = m1;\n    ch = ch2;\n";
      s << "  }\n}\n\n";
    }

    // A bucket whose groups all fitted the LDS table owns them exclusively (a group
    // lives in exactly one bucket): its table is written out as dense group records
    // -- the form compaction would produce -- at a range reserved with one atomic per
    // bucket.  No probing of, and no scattered 32-byte writes into, a sparse HBM table
    // (measured: 1.35 GB of probe reads + 0.96 GB of writes per 1e7 groups).
    s << "#define EVQL_ST_DENSE_FULL 16u\n";
    s << "__device__ __forceinline__ void evql_lds_emit_dense(const EvqlArgs& A, const EvqlPartArgs& P, "
         "u64* lds) {\n";
    s << "  __shared__ u32 wsum[EVQL_BLOCK / 64];\n  __shared__ u64 base_s;\n";
    s << "  u32 cnt = 0;\n";
    s << "  for (u32 sl = threadIdx.x; sl < EVQL_LSTRIDE; sl += EVQL_BLOCK) cnt += lds[sl] != EVQL_EMPTY ? 1u : 0u;\n";
    s << "  u32 incl = cnt;\n";
    s << "#pragma unroll\n  for (int d = 1; d < 64; d <<= 1) { const u32 t = __shfl_up(incl, d, 64); "
         "if ((int) (threadIdx.x & 63u) >= d) incl += t; }\n";
    s << "  if ((threadIdx.x & 63u) == 63u) wsum[threadIdx.x >> 6] = incl;\n  __syncthreads();\n";
    s << "  u32 off = 0, total = 0;\n";
    s << "  for (u32 w = 0; w < EVQL_BLOCK / 64; ++w) { if (w < (threadIdx.x >> 6)) off += wsum[w]; total += "
         "wsum[w]; }\n";
    s << "  if (threadIdx.x == 0) base_s = total ? atomicAdd(&A.counters[3], (u64) total) : 0ull;\n";
    s << "  __syncthreads();\n";
    s << "  u64 idx = base_s + off + incl - cnt;\n";
    s << "  if (threadIdx.x == 0 && base_s + total > P.dense_cap) atomicOr(&A.status[0], EVQL_ST_DENSE_FULL);\n";
    s << "  for (u32 sl = threadIdx.x; sl < EVQL_LSTRIDE; sl += EVQL_BLOCK) {\n";
    s << "    const u64 k = lds[sl];\n    if (k == EVQL_EMPTY) continue;\n";
    s << "    if (idx < P.dense_cap) {\n";
    s << "      u64* rec = P.dense + idx * (EVQL_WORDS + 1);\n";
    s << "      rec[0] = sl == EVQL_LDS_SLOTS ? 1ull : (sl == EVQL_LDS_SLOTS + 1 ? 2ull : 0ull);\n";
    s << "      rec[1] = sl == EVQL_LDS_SLOTS ? EVQL_EMPTY : k;\n";
    for (int w = 1; w < W; ++w) {
      s << "      rec[" << (1 + w) << "] = " << lds_word(w, "sl") << ";\n";
    }
    s << "    }\n    ++idx;\n  }\n  __syncthreads();\n}\n\n";

    // pass 3: one workgroup per bucket, LDS table, flush into the HBM table
    // (tried: 256-thread workgroups, several per CU, so that the per-bucket phases
    // of different buckets overlap -- 2.7x slower on MI355X, 1024 threads stay)
    s << "#define EVQL_ABLOCK EVQL_BLOCK\n";
    // one batch of tuples (EVQL_TIF per thread, loaded before any is processed: with one
    // load in flight per thread the pass was latency-bound, 32 us per 244 KB bucket)
    s << "#define EVQL_AGG_LOAD(dst_, i0_, n1_) _Pragma(\"unroll\") for (int k = 0; k < EVQL_TIF; ++k) { "
         "const u64 i = i0_ + threadIdx.x + (u64) k * EVQL_ABLOCK; if (i < n1_) evql_tuple_load("
         "reinterpret_cast<const u32*>(P.tuples) + i * EVQL_TUPLE_U32, dst_[k]); }\n";
    s << "__device__ __forceinline__ void evql_agg_batch(const EvqlArgs& A, u64* lds, const u32 "
         "(&tw)[EVQL_TIF][EVQL_TUPLE_U32], const u64 i0, const u64 n1) {\n";
    s << "  const u32 tid = threadIdx.x;\n";
    s << "#pragma unroll\n      for (int k = 0; k < EVQL_TIF; ++k) {\n";
    s << "      if (i0 + tid + (u64) k * EVQL_ABLOCK >= n1) continue;\n";
    s << "      const u64 ident = " << tuple_ident("tw[k]") << ";\n";
    if (kp.has_ident2()) s << "      const u64 ident2 = " << t64("tw[k]", off_ident2) << ";\n";
    if (kp.need_first_row) s << "      const u64 row = " << tuple_row("tw[k]") << ";\n";
    if (kp.has_ident2()) {
      s << "      int s = evql_lds_find2<32>(lds, lds + EVQL_LSTRIDE, EVQL_LDS_SLOTS - 1, ident, ident2, "
           "(u32) evql_mix64(ident));\n";
    } else {
      s << "      int s = ident == EVQL_EMPTY ? (int) EVQL_LDS_SLOTS : evql_lds_find<32>(lds, "
           "EVQL_LDS_SLOTS - 1, ident, (u32) evql_mix64(ident));\n";
      s << "      if (ident == EVQL_EMPTY) lds[s] = 0;\n";
    }
    s << "      if (s >= 0) {\n";
    if (kp.need_first_row) {
      s << "        evql_atomic<EVQL_OP_MIN_U64>(&" << lds_word(frw, "s") << ", row);\n";
    }
    auto upd_value = [&](int i) {
      return updw[i].tslot < 0 ? std::string(updw[i].constant) : tuple_upd("tw[k]", updw[i]);
    };
    for (int i = 0; i < U(); ++i) {
      s << "        evql_atomic<" << op_name(updw[i].op) << ">(&" << lds_word(SB + updw[i].word, "s")
        << ", " << upd_value(i) << ");\n";
    }
    s << "      } else {\n";
    // the bucket holds more groups than the LDS table: straight to the HBM table
    // (and the flush of this bucket has to combine, not store)
    s << "        atomicAdd(reinterpret_cast<u32*>(&lds[EVQL_WORDS * EVQL_LSTRIDE]), 1u);\n";
    s << "        i64 gs;\n";
    if (kp.has_ident2()) {
      s << "        gs = evql_gtab_find2(A.gtab, EVQL_WORDS, A.gcap, ident, ident2, evql_mix64(ident));\n";
    } else {
      s << "        gs = evql_gtab_find(A.gtab, EVQL_WORDS, A.gcap, ident, evql_mix64(ident));\n";
    }
    s << "        if (gs < 0) { atomicOr(&A.status[0], EVQL_ST_TABLE_FULL); }\n        else {\n";
    if (kp.need_first_row) {
      s << "          evql_atomic<EVQL_OP_MIN_U64>(&" << gtab_word(frw, "gs") << ", row);\n";
    }
    for (int i = 0; i < U(); ++i) {
      s << "          evql_atomic<" << op_name(updw[i].op) << ">(&" << gtab_word(SB + updw[i].word, "gs")
        << ", " << upd_value(i) << ");\n";
    }
    s << "        }\n      }\n      }\n}\n\n";
    // pass 3 proper.  The first batch of the NEXT bucket is requested before this
    // bucket's table is written out, so that its latency hides behind the emit phase
    // (measured: 0.741 -> 0.735 ms -- the pass is bound by the LDS table itself: with
    // the updates compiled out it takes 0.20 ms, without the emit 0.62, without the
    // table initialisation 0.73.  SQ counters: 65 % s_waitcnt stalls, LDS busy 9 %, bank
    // conflicts 4 % -- dependent LDS round trips at 16 waves per CU.  Reading the
    // identity-slot keys of all four tuples of a batch up front, to overlap those round
    // trips, ran 5 % slower (0.773 ms) and was dropped).
    s << "extern \"C\" __global__ void __launch_bounds__(EVQL_ABLOCK) evql_part_aggregate(const EvqlArgs A, "
         "const EvqlPartArgs P) {\n";
    s << "  __shared__ u64 lds[EVQL_WORDS * EVQL_LSTRIDE + 1];\n";
    if (fused) {
      s << "  if (__hip_atomic_load(&A.status[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & "
           "EVQL_ST_PART_OVERFLOW) return;  // (void launch, see evql_part_refine)\n";
    }
    s << "#define EVQL_AGG_SEEK(b_) while (b_ < EVQL_NPART && P.bucket_start[b_] == P.bucket_start[b_ + 1]) "
         "b_ += gridDim.x;\n";
    // (the second buffer costs EVQL_TIF * EVQL_TUPLE_U32 registers: with 32-byte tuples it
    // pushed the kernel into 37 spilled VGPRs, so wide tuples go without the prefetch)
    const bool prefetch = tuple_u32 <= 4;
    s << "  u32 b = blockIdx.x;\n";
    s << "  EVQL_AGG_SEEK(b)\n";
    if (prefetch) {
      s << "  u32 pf[EVQL_TIF][EVQL_TUPLE_U32];\n";
      s << "  if (b < EVQL_NPART) { EVQL_AGG_LOAD(pf, P.bucket_start[b], P.bucket_start[b + 1]) }\n";
    }
    s << "  while (b < EVQL_NPART) {\n";
    s << "    const u64 n0 = P.bucket_start[b], n1 = P.bucket_start[b + 1];\n";
    s << "    evql_lds_init(lds);\n    __syncthreads();\n";
    if (prefetch) {
      s << "    evql_agg_batch(A, lds, pf, n0, n1);\n";
      s << "    for (u64 i0 = n0 + (u64) EVQL_ABLOCK * EVQL_TIF; i0 < n1; i0 += (u64) EVQL_ABLOCK * EVQL_TIF) {\n";
    } else {
      s << "    for (u64 i0 = n0; i0 < n1; i0 += (u64) EVQL_ABLOCK * EVQL_TIF) {\n";
    }
    s << "      u32 tw[EVQL_TIF][EVQL_TUPLE_U32];\n";
    s << "      EVQL_AGG_LOAD(tw, i0, n1)\n";
    s << "      evql_agg_batch(A, lds, tw, i0, n1);\n    }\n";
    // (the word behind the table counts the tuples that found no LDS slot and went
    // to the HBM table: such a bucket is combined into that table instead)
    s << "    __syncthreads();\n";
    s << "    u32 b2 = b + gridDim.x;\n";
    s << "    EVQL_AGG_SEEK(b2)\n";
    if (prefetch) {
      s << "    if (b2 < EVQL_NPART) { EVQL_AGG_LOAD(pf, P.bucket_start[b2], P.bucket_start[b2 + 1]) }\n";
    }
    s << "    if (evql_lds_peek32(reinterpret_cast<const u32*>(&lds[EVQL_WORDS * EVQL_LSTRIDE])) == 0) {\n";
    s << "      evql_lds_emit_dense(A, P, lds);\n";
    s << "    } else {\n";
    s << "      if (threadIdx.x == 0) atomicAdd(&A.counters[2], 1ull);\n";
    s << "      evql_lds_flush<false>(A, lds);\n    }\n    __syncthreads();\n";
    s << "    b = b2;\n";
    s << "  }\n}\n";
  }
};

}  // namespace

int partition_tuple_u32_words(const KernelPlan& kp) { return Gen(kp).tuple_u32; }

std::string generate_kernel_source(KernelPlan* kp) {
  Gen g(*kp);
  g.prologue();
  g.eval_row();
  if (kp->bare_scan) {
    g.bare_scan_kernels();
  } else {
    g.scan_kernel();
    if (kp->partitioned) g.partition_kernels();
  }
  if (kp->where_rows_kernel) g.where_rows_kernel();
  kp->lit_pool = g.pool;
  return g.s.str();
}
