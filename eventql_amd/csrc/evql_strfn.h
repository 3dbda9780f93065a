// evql_strfn.h -- string functions evaluated per row.  NOT part of
// evql_device.h: this text is put in front of the row function of the plans that use a
// string function, and of no other plan, so every other plan keeps its cache digest.
//
// A computed string is never materialised.  It is a VALUE OBJECT: a length and a byte
// accessor `at(i)` (0 <= i < len), composed at compile time from its operands -- the
// generated text nests the factory calls below the way the expression tree nests, and
// every type is a template over its operand types.  Nothing here indexes an array held
// by a lane: a dynamically indexed private array would live in scratch memory.
//
//   leaf        a column value (bytes through the page table) or a literal: EvqlStr
//   case map    a function of the inner byte
//   window      ltrim / rtrim / substring: offset and length found by scanning / clamping
//   concat      a select on i < a.len
//   text        to_string of an integer / bool / NULL: up to 20 bytes in three registers
//
// Compare, affix and hash are written once over any two such values and read one byte of
// each side per step, so they stop at the first byte that decides.

struct EvqlSxLeaf {
  EvqlStr s;
  u32 len;
  __device__ __forceinline__ u32 at(u32 i) const { return evql_str_byte(s, i); }
};
__device__ __forceinline__ EvqlSxLeaf evql_sx_leaf(const EvqlStr& s) { return EvqlSxLeaf{s, s.len}; }

// ASCII only: bytes first .. first + 25 flip bit 5, every other byte (NUL included) stays
template <class A>
struct EvqlSxCase {
  A a;
  u32 first;
  u32 len;
  __device__ __forceinline__ u32 at(u32 i) const {
    const u32 b = a.at(i);
    return (b - first) < 26u ? (b ^ 0x20u) : b;
  }
};
template <class A>
__device__ __forceinline__ EvqlSxCase<A> evql_sx_lcase(const A& a) { return EvqlSxCase<A>{a, 'A', a.len}; }
template <class A>
__device__ __forceinline__ EvqlSxCase<A> evql_sx_ucase(const A& a) { return EvqlSxCase<A>{a, 'a', a.len}; }

template <class A>
struct EvqlSxWin {
  A a;
  u32 off;
  u32 len;  // off + len <= a.len
  __device__ __forceinline__ u32 at(u32 i) const { return a.at(off + i); }
};
// leading / trailing ' ' only
template <class A>
__device__ __forceinline__ EvqlSxWin<A> evql_sx_ltrim(const A& a) {
  u32 off = 0;
  while (off < a.len && a.at(off) == ' ') ++off;
  return EvqlSxWin<A>{a, off, a.len - off};
}
template <class A>
__device__ __forceinline__ EvqlSxWin<A> evql_sx_rtrim(const A& a) {
  u32 n = a.len;
  while (n > 0 && a.at(n - 1) == ' ') --n;
  return EvqlSxWin<A>{a, 0, n};
}
// substring(s, pos): a SUFFIX (string.cc substring_call).  pos == 0 or an empty s: "";
// pos < 0 counts from the end, beyond the start: ""; pos > 0 starts at min(pos - 1, len - 1)
template <class A>
__device__ __forceinline__ EvqlSxWin<A> evql_sx_substring(const A& a, i64 pos) {
  const i64 len = (i64) a.len;
  i64 off = len;
  if (pos != 0 && len != 0) {
    if (pos < 0) {
      if (pos + len >= 0) off = pos + len;
    } else {
      off = pos - 1 < len - 1 ? pos - 1 : len - 1;
    }
  }
  return EvqlSxWin<A>{a, (u32) off, (u32) (len - off)};
}

template <class A, class B>
struct EvqlSxCat {
  A a;
  B b;
  u32 len;
  __device__ __forceinline__ u32 at(u32 i) const { return i < a.len ? a.at(i) : b.at(i - a.len); }
};
template <class A, class B>
__device__ __forceinline__ EvqlSxCat<A, B> evql_sx_concat(const A& a, const B& b) {
  return EvqlSxCat<A, B>{a, b, a.len + b.len};
}

// up to 24 bytes, byte i in bits 8 (i & 7) .. of word i >> 3
struct EvqlSxText {
  u64 w0, w1, w2;
  u32 len;
  __device__ __forceinline__ u32 at(u32 i) const {
    // (the select is over three shifted VALUES: a select over the words themselves is
    // turned into an indexed load by the optimiser, which puts the struct into scratch)
    const u32 sh = (i & 7u) * 8u;
    const u32 b0 = (u32) (w0 >> sh) & 0xffu, b1 = (u32) (w1 >> sh) & 0xffu, b2 = (u32) (w2 >> sh) & 0xffu;
    return i < 8u ? b0 : (i < 16u ? b1 : b2);
  }
};
#define EVQL_SX_NULL 0x4c4c554eull /* "NULL" */
__device__ __forceinline__ void evql_sx_push_front(EvqlSxText& t, u32 byte) {
  t.w2 = (t.w2 << 8) | (t.w1 >> 56);
  t.w1 = (t.w1 << 8) | (t.w0 >> 56);
  t.w0 = (t.w0 << 8) | (u64) byte;
  ++t.len;
}
// to_string (svalue.cc sql_tostring): decimal digits; a NULL tag reads "NULL"
__device__ __forceinline__ EvqlSxText evql_sx_digits(u64 v, bool minus, bool null) {
  if (null) return EvqlSxText{EVQL_SX_NULL, 0, 0, 4};
  EvqlSxText t{0, 0, 0, 0};
  do {
    evql_sx_push_front(t, '0' + (u32) (v % 10));
    v /= 10;
  } while (v != 0);
  if (minus) evql_sx_push_front(t, '-');
  return t;
}
__device__ __forceinline__ EvqlSxText evql_sx_u64(u64 v, bool null) { return evql_sx_digits(v, false, null); }
__device__ __forceinline__ EvqlSxText evql_sx_i64(i64 v, bool null) {
  return evql_sx_digits(v < 0 ? 0ull - (u64) v : (u64) v, v < 0, null);
}
__device__ __forceinline__ EvqlSxText evql_sx_bool(bool v, bool null) {
  if (null) return EvqlSxText{EVQL_SX_NULL, 0, 0, 4};
  return v ? EvqlSxText{0x65757274ull, 0, 0, 4} : EvqlSxText{0x65736c6166ull, 0, 0, 5};
}

// ---- consumers (the semantics of evql_str_eq / _cmp / _affix, evql_device.h) --------------
template <class A, class B>
__device__ __forceinline__ bool evql_sx_eq(const A& a, const B& b) {
  // (requesting the bytes of step i + 1 before those of step i are compared was measured
  // slower: `where lcase(s) = 'g17'` 0.827 ms against 0.785 ms)
  if (a.len != b.len) return false;
  for (u32 i = 0; i < a.len; ++i) {
    if (a.at(i) != b.at(i)) return false;
  }
  return true;
}
template <class A, class B>
__device__ __forceinline__ bool evql_sx_affix(const A& s, const B& affix, bool at_end) {
  if (s.len < affix.len) return false;
  const u32 off = at_end ? s.len - affix.len : 0;
  for (u32 i = 0; i < affix.len; ++i) {
    if (s.at(off + i) != affix.at(i)) return false;
  }
  return true;
}
template <class A, class B>
__device__ __forceinline__ int evql_sx_cmp(const A& a, const B& b) {
  const u32 n = a.len < b.len ? a.len : b.len;
  for (u32 i = 0; i < n; ++i) {
    const u32 x = a.at(i), y = b.at(i);
    if (x != y) return x < y ? -1 : 1;
    if (x == 0) break;
  }
  return a.len < b.len ? -1 : (a.len > b.len ? 1 : 0);
}
// identity of a computed group key: the hash k_string_hash keeps per row of a string
// column (aot_kernels.hip), so a computed value equal to a column value hashes like it
template <class A>
__device__ __forceinline__ u64 evql_sx_hash(const A& a) {
  u64 h = 0xcbf29ce484222325ull ^ ((u64) a.len * 0x9e3779b97f4a7c15ull);
  for (u32 k = 0; k < a.len; ++k) {
    h ^= (u64) a.at(k);
    h *= 0x100000001b3ull;
  }
  return evql_mix64(h);
}

