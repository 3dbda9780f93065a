#include "codegen.h"
#include <cstdio>
#include <sstream>

namespace evql {

const char* device_library_source() {
  static const char* src =
#include "evql_device.inc"
      ;
  return src;
}

namespace {

// string functions per row: part of the generated text of the plans that use one
const char* strfn_library_source() {
  static const char* src =
#include "evql_strfn.inc"
      ;
  return src;
}

const char* ctype(uint32_t t) {
  switch (t) {
    case EVQL_T_INT64: return "i64";
    case EVQL_T_FLOAT64: return "double";
    case EVQL_T_BOOL: return "bool";
    default: return "u64";
  }
}

std::string hex64(uint64_t v) {
  char b[32];
  snprintf(b, sizeof(b), "0x%016llxull", (unsigned long long) v);
  return b;
}

const char* op_name(int op) {
  static const char* n[] = {"EVQL_OP_ADD_U64", "EVQL_OP_ADD_F64", "EVQL_OP_MIN_U64",
                            "EVQL_OP_MAX_U64", "EVQL_OP_MIN_I64", "EVQL_OP_MAX_I64",
                            "EVQL_OP_MIN_F64", "EVQL_OP_MAX_F64"};
  return n[op];
}

// An integer div / mod gets a zero-divisor check unless its divisor is a non-zero integer
// literal (which stays a constant of the text, Emitter::emit `bake`).
bool needs_zero_check(const ExprPtr& e) {
  if (e->kind != Expr::CALL || (e->family != EVQL_FAM_DIV && e->family != EVQL_FAM_MOD)) return false;
  if (e->type_slot == EVQL_TS_FLOAT64 || e->args.size() != 2) return false;
  const ExprPtr& d = e->args[1];
  const bool int_lit = d->kind == Expr::LITERAL && !d->lit_tag &&
                       (d->type == EVQL_T_UINT64 || d->type == EVQL_T_INT64 || d->type == EVQL_T_TIMESTAMP64);
  return !(int_lit && d->lit_bits != 0);
}

struct Val {
  std::string v;  // payload expression (already typed)
  std::string g;  // tag expression (u32)
  uint32_t type;
};

struct Emitter {
  std::ostringstream o;
  int tmp = 0;
  std::string ind = "  ";

  std::string fresh(const char* p) {
    char b[32];
    snprintf(b, sizeof(b), "%s%d", p, tmp++);
    return b;
  }

  // string literals referenced by compares; declared at file scope by the caller
  std::vector<std::string> string_literals;
  // index of this emitter's first literal among the translation unit's `evql_slit<i>`
  size_t lit_base = 0;
  // the plan's numeric literal pool (KernelPlan::lit_pool), one per translation unit and
  // shared by its row functions: slot i is read as A.lit[i]
  std::vector<uint64_t>* pool = nullptr;

  // the plan's scan columns (how each is read bounds its values)
  const std::vector<ColAccess>* cols = nullptr;

  static bool poolable(const ExprPtr& e) {
    return e->kind == Expr::LITERAL && !e->lit_tag &&
           (e->type == EVQL_T_UINT64 || e->type == EVQL_T_INT64 || e->type == EVQL_T_FLOAT64 ||
            e->type == EVQL_T_TIMESTAMP64);
  }
  // an unsigned column whose values are read from 32 bits or fewer
  bool narrow_input(const ExprPtr& e) const {
    if (!cols || e->kind != Expr::INPUT || e->input >= cols->size()) return false;
    if (e->type != EVQL_T_UINT64 && e->type != EVQL_T_TIMESTAMP64) return false;
    const ColAccess& c = (*cols)[e->input];
    if (c.stype != e->type) return false;
    return c.mode == ColAccess::PLAIN32 || c.mode == ColAccess::NARROW ||
           (c.mode == ColAccess::BITPACKED && c.bits >= 1 && c.bits <= 32);
  }
  // Compare of a narrow unsigned column with a pooled literal.  With the constant in the
  // text the compiler knew both operands to fit 32 bits and compared 32 bits; against an
  // unknown 64-bit word it would widen every value of the tile to a register pair (config
  // 3 over 16-bit pages: 98 -> 114 VGPRs).  So the text splits the literal itself: its
  // high half is tested once per wave on the scalar unit, the lanes compare 32 bits.
  bool narrow_compare(const ExprPtr& e, std::string* rhs) {
    const int fam = e->family;
    if (fam < EVQL_FAM_EQ || fam > EVQL_FAM_GTE || e->args.size() != 2) return false;
    if (e->type_slot != EVQL_TS_UINT64 && e->type_slot != EVQL_TS_TIMESTAMP64) return false;
    if (!pool || pool->size() >= size_t(kMaxLits)) return false;
    int ci = -1;
    if (narrow_input(e->args[0]) && poolable(e->args[1])) ci = 0;
    if (narrow_input(e->args[1]) && poolable(e->args[0])) ci = 1;
    if (ci < 0) return false;
    const Val c = emit(e->args[ci]), l = emit(e->args[1 - ci]);
    // the relation as seen from the column: c OP l
    const char* opr = nullptr;
    bool when_high = false;  // the result when the literal does not fit 32 bits
    switch (fam) {
      case EVQL_FAM_EQ: opr = "=="; break;
      case EVQL_FAM_NEQ: opr = "!="; when_high = true; break;
      case EVQL_FAM_LT: opr = ci == 0 ? "<" : ">"; when_high = ci == 0; break;
      case EVQL_FAM_LTE: opr = ci == 0 ? "<=" : ">="; when_high = ci == 0; break;
      case EVQL_FAM_GT: opr = ci == 0 ? ">" : "<"; when_high = ci != 0; break;
      case EVQL_FAM_GTE: opr = ci == 0 ? ">=" : "<="; when_high = ci != 0; break;
      default: return false;
    }
    const std::string lo = "((u32) " + c.v + " " + opr + " (u32) " + l.v + ")";
    const std::string hi = "((u32) (" + l.v + " >> 32) " + (when_high ? "!=" : "==") + " 0u)";
    *rhs = "(" + hi + (when_high ? " | " : " & ") + lo + ")";
    return true;
  }

  // the 64 bits of a numeric literal: a slot of the pool, or the constant itself
  std::string lit_word(const ExprPtr& e, bool bake) {
    if (bake || !pool || pool->size() >= size_t(kMaxLits)) return hex64(e->lit_bits);
    pool->push_back(e->lit_bits);
    return "A.lit[" + std::to_string(pool->size() - 1) + "]";
  }

  std::string str_operand(const ExprPtr& x) {
    char b[96];
    if (x->kind == Expr::INPUT) {
      snprintf(b, sizeof(b), "evql_col_str(A, A.col[%u], row)", x->input);
      return b;
    }
    snprintf(b, sizeof(b), "evql_lit_str(evql_slit%zu, %zuu)", lit_base + string_literals.size(),
             x->lit_str.size());
    string_literals.push_back(x->lit_str);
    return b;
  }

  // set once the text uses a helper of evql_strfn.h (Gen::row_function puts it in front)
  bool uses_strfn = false;

  // A string value (planner.cc string_value_refusal) as a lazy value object of evql_strfn.h:
  // the factory calls nest the way the tree nests, every function node becomes a `const
  // auto` local, a column or literal the leaf over str_operand.  Returns the expression
  // that names the value.
  std::string str_value(const ExprPtr& x) {
    uses_strfn = true;
    if (x->kind != Expr::CALL) return "evql_sx_leaf(" + str_operand(x) + ")";
    std::string rhs;
    switch (x->family) {
      case EVQL_FAM_LCASE: rhs = "evql_sx_lcase(" + str_value(x->args[0]) + ")"; break;
      case EVQL_FAM_UCASE: rhs = "evql_sx_ucase(" + str_value(x->args[0]) + ")"; break;
      case EVQL_FAM_LTRIM: rhs = "evql_sx_ltrim(" + str_value(x->args[0]) + ")"; break;
      case EVQL_FAM_RTRIM: rhs = "evql_sx_rtrim(" + str_value(x->args[0]) + ")"; break;
      case EVQL_FAM_CONCAT: {
        const std::string a = str_value(x->args[0]), b = str_value(x->args[1]);
        rhs = "evql_sx_concat(" + a + ", " + b + ")";
        break;
      }
      case EVQL_FAM_SUBSTRING: {
        // (a literal position is a pooled kernel argument like any numeric literal)
        const std::string a = str_value(x->args[0]);
        const Val p = emit(x->args[1]);
        rhs = "evql_sx_substring(" + a + ", (i64) " + p.v + ")";
        break;
      }
      default: {  // EVQL_FAM_TO_STRING
        const Val v = emit(x->args[0]);
        const std::string null = "((" + v.g + " & 1u) != 0)";
        if (x->type_slot == EVQL_TS_BOOL) rhs = "evql_sx_bool(" + v.v + ", " + null + ")";
        else if (x->type_slot == EVQL_TS_INT64) rhs = "evql_sx_i64((i64) " + v.v + ", " + null + ")";
        else rhs = "evql_sx_u64((u64) " + v.v + ", " + null + ")";
      }
    }
    const std::string t = fresh("s");
    o << ind << "const auto " << t << " = " << rhs << ";\n";
    return t;
  }

  // payload reinterpreted as raw 64 bits
  static std::string as_bits(const Val& x) {
    switch (x.type) {
      case EVQL_T_FLOAT64: return "evql_f64_bits(" + x.v + ")";
      case EVQL_T_BOOL: return "((u64) (" + x.v + " ? 1 : 0))";
      default: return "((u64) " + x.v + ")";
    }
  }

  // `bake`: a literal at `e` stays a constant of the text
  Val emit(const ExprPtr& e, bool bake = false) {
    switch (e->kind) {
      case Expr::INPUT: {
        char v[16], g[16];
        snprintf(v, sizeof(v), "c%u", e->input);
        snprintf(g, sizeof(g), "g%u", e->input);
        return {v, g, e->type};
      }
      case Expr::LITERAL: {
        // A numeric literal (UINT64, INT64, FLOAT64, TIMESTAMP64; not NULL) is data of the
        // launch: the text reads its 64 bits from the kernel arguments (A.lit[i], a
        // wave-uniform read at a constant index) and keeps only its type, so plans that
        // differ in such values share one code object.  What stays in the text:
        //   - BOOL literals and literals with a NULL tag: they decide control flow and tags;
        //   - string literals (evql_slit<i>, str_operand);
        //   - the right operand of div / mod / pow (`bake`): the compiler strength-reduces
        //     a constant divisor and folds the zero-divisor check away;
        //   - literals beyond the kMaxLits-th of a plan.
        const std::string w = poolable(e) ? lit_word(e, bake) : hex64(e->lit_bits);
        std::string v;
        switch (e->type) {
          case EVQL_T_FLOAT64: v = "evql_as_f64(" + w + ")"; break;
          case EVQL_T_INT64: v = "((i64) " + w + ")"; break;
          case EVQL_T_BOOL: v = e->lit_bits ? "true" : "false"; break;
          default: v = w;
        }
        return {v, e->lit_tag ? "1u" : "0u", e->type};
      }
      case Expr::AGG_GET:
        return {"0", "0u", e->type};  // never reached on the device
      case Expr::IF: {
        Val c = emit(e->args[0]);
        std::string t = fresh("t"), g = fresh("q");
        o << ind << ctype(e->type) << " " << t << "; u32 " << g << ";\n";
        o << ind << "if (" << c.v << ") {\n";
        std::string save = ind;
        ind += "  ";
        Val a = emit(e->args[1]);
        o << ind << t << " = " << a.v << "; " << g << " = " << a.g << ";\n";
        ind = save;
        o << ind << "} else {\n";
        ind += "  ";
        Val b = emit(e->args[2]);
        o << ind << t << " = " << b.v << "; " << g << " = " << b.g << ";\n";
        ind = save;
        o << ind << "}\n";
        return {t, g, e->type};
      }
      case Expr::CALL:
        break;
    }
    const int fam = e->family, ts = e->type_slot;
    if (ts == EVQL_TS_STRING && ((fam >= EVQL_FAM_CMP && fam <= EVQL_FAM_GTE) ||
                                 fam == EVQL_FAM_STARTSWITH || fam == EVQL_FAM_ENDSWITH)) {
      // operands are string values (planner.cc strings_refusal): two columns / literals go
      // through evql_device.h's compares, a computed operand takes both through evql_strfn.h
      const bool lazy = e->args[0]->kind == Expr::CALL || e->args[1]->kind == Expr::CALL;
      const std::string fn = lazy ? "evql_sx_" : "evql_str_";
      std::string l, r;
      if (lazy) {
        l = str_value(e->args[0]);
        r = str_value(e->args[1]);
      } else {
        l = str_operand(e->args[0]);
        r = str_operand(e->args[1]);
      }
      const std::string c = fn + "cmp(" + l + ", " + r + ")";
      std::string rhs;
      switch (fam) {
        case EVQL_FAM_EQ: rhs = fn + "eq(" + l + ", " + r + ")"; break;
        case EVQL_FAM_NEQ: rhs = "(!" + fn + "eq(" + l + ", " + r + "))"; break;
        case EVQL_FAM_LT: rhs = "(" + c + " < 0)"; break;
        case EVQL_FAM_LTE: rhs = "(" + c + " <= 0)"; break;
        case EVQL_FAM_GT: rhs = "(" + c + " > 0)"; break;
        case EVQL_FAM_GTE: rhs = "(" + c + " >= 0)"; break;
        case EVQL_FAM_STARTSWITH: rhs = fn + "affix(" + l + ", " + r + ", false)"; break;
        case EVQL_FAM_ENDSWITH: rhs = fn + "affix(" + l + ", " + r + ", true)"; break;
        default: rhs = "((i64) " + c + ")";
      }
      std::string t = fresh("t");
      o << ind << "const " << ctype(e->type) << " " << t << " = " << rhs << ";\n";
      return {t, "0u", e->type};
    }
    if (e->type == EVQL_T_STRING) {
      // a computed string as a VALUE (a group key): the hash of its bytes, tag 0 like the
      // result of every pure function
      const std::string sv = str_value(e);
      std::string t = fresh("t");
      o << ind << "const u64 " << t << " = evql_sx_hash(" << sv << ");\n";
      return {t, "0u", e->type};
    }
    {
      std::string narrow;
      if (narrow_compare(e, &narrow)) {
        std::string t = fresh("t");
        o << ind << "const bool " << t << " = " << narrow << ";\n";
        return {t, "0u", e->type};
      }
    }
    std::vector<Val> a;
    const bool const_rhs = fam == EVQL_FAM_DIV || fam == EVQL_FAM_MOD || fam == EVQL_FAM_POW;
    for (size_t i = 0; i < e->args.size(); ++i) a.push_back(emit(e->args[i], const_rhs && i == 1));
    std::string t = fresh("t");
    std::string rhs;
    auto bin = [&](const char* opr) { return "(" + a[0].v + " " + opr + " " + a[1].v + ")"; };
    switch (fam) {
      case EVQL_FAM_LOGICAL_AND: rhs = "(" + a[0].v + " & " + a[1].v + ")"; break;  // eager
      case EVQL_FAM_LOGICAL_OR: rhs = "(" + a[0].v + " | " + a[1].v + ")"; break;
      case EVQL_FAM_NEG: rhs = "(!" + a[0].v + ")"; break;
      case EVQL_FAM_EQ: rhs = bin("=="); break;
      case EVQL_FAM_NEQ: rhs = bin("!="); break;
      case EVQL_FAM_LT: rhs = bin("<"); break;
      case EVQL_FAM_LTE: rhs = bin("<="); break;
      case EVQL_FAM_GT: rhs = bin(">"); break;
      case EVQL_FAM_GTE: rhs = bin(">="); break;
      case EVQL_FAM_CMP:
        rhs = "((i64) (" + a[0].v + " < " + a[1].v + " ? -1 : (" + a[0].v + " > " + a[1].v +
              " ? 1 : 0)))";
        break;
      case EVQL_FAM_ADD: rhs = bin("+"); break;
      case EVQL_FAM_SUB: rhs = bin("-"); break;
      case EVQL_FAM_MUL: rhs = bin("*"); break;
      case EVQL_FAM_DIV:
      case EVQL_FAM_MOD: {
        const bool is_div = fam == EVQL_FAM_DIV;
        if (ts == EVQL_TS_FLOAT64) {
          rhs = is_div ? bin("/") : "fmod(" + a[0].v + ", " + a[1].v + ")";
        } else {
          // integer division by zero raises in the reference (math.cc:136-164):
          // flag it and keep going with 0; the host turns the flag into ERUNTIME
          o << ind << ctype(e->type) << " " << t << " = 0;\n";
          if (needs_zero_check(e)) {
            o << ind << "if (" << a[1].v << " == 0) { atomicOr(&A.status[0], "
              << (is_div ? "EVQL_ST_DIV_BY_ZERO" : "EVQL_ST_MOD_BY_ZERO") << "); } else {\n";
          } else {
            o << ind << "{\n";
          }
          if (ts == EVQL_TS_INT64) {
            if (is_div) {
              o << ind << "  " << t << " = (" << a[0].v
                << " == (i64) 0x8000000000000000ull && " << a[1].v << " == -1) ? " << a[0].v
                << " : " << a[0].v << " / " << a[1].v << ";\n";
            } else {
              o << ind << "  " << t << " = (" << a[1].v << " == -1) ? 0 : " << a[0].v << " % "
                << a[1].v << ";\n";
            }
          } else {
            o << ind << "  " << t << " = " << a[0].v << (is_div ? " / " : " % ") << a[1].v
              << ";\n";
          }
          o << ind << "}\n";
          return {t, "0u", e->type};
        }
        break;
      }
      case EVQL_FAM_POW:
        if (ts == EVQL_TS_FLOAT64) rhs = "pow(" + a[0].v + ", " + a[1].v + ")";
        else
          rhs = std::string("((") + ctype(e->type) + ") pow((double) " + a[0].v + ", (double) " +
                a[1].v + "))";
        break;
      case EVQL_FAM_TO_NIL: rhs = "0ull"; break;
      case EVQL_FAM_TO_INT64:
        rhs = "((i64) " + a[0].v + ")";
        break;
      case EVQL_FAM_TO_TIMESTAMP64:
        rhs = "((u64) " + a[0].v + ")";
        break;
      default: rhs = "0";
    }
    if (ts == EVQL_TS_INT64 && (fam == EVQL_FAM_ADD || fam == EVQL_FAM_SUB || fam == EVQL_FAM_MUL)) {
      // wrap-around like the reference's two's complement arithmetic, without UB
      const char* opr = fam == EVQL_FAM_ADD ? "+" : (fam == EVQL_FAM_SUB ? "-" : "*");
      rhs = "((i64) ((u64) " + a[0].v + " " + opr + " (u64) " + a[1].v + "))";
    }
    o << ind << "const " << ctype(e->type) << " " << t << " = " << rhs << ";\n";
    return {t, "0u", e->type};
  }
};

}  // namespace

bool expr_prints_zero_check(const ExprPtr& e) {
  if (!e) return false;
  if (needs_zero_check(e)) return true;
  for (const auto& a : e->args) {
    if (expr_prints_zero_check(a)) return true;
  }
  return false;
}

// kernel skeletons (scan, partition count / scatter / aggregate)
#include "codegen_kernels.inc"

}  // namespace evql
