// neo_wave.hpp -- the cross-lane layer of the kernels (gfx950, 64-lane wavefronts): lane predicates, DPP moves, lane
// reads, scans, wave reductions and neighbour shifts, each written ONCE for the value types int, float and double.
// Includes nothing else of the project: a unit that needs only these does not pull in the MINCO machinery of
// neo_device.hpp (which includes this header and builds the lane-group policies on it).
#pragma once
#include <type_traits>
#include <hip/hip_runtime.h>

namespace neo {

constexpr int kWave = 64;

__device__ __forceinline__ int lane_id() { return (int)__lane_id(); }

// Ordering of LDS traffic inside ONE wavefront (every workgroup of these kernels is a single wavefront): the LDS
// executes a wavefront's DS instructions in issue order, so a read issued after a write sees it -- whichever lanes
// wrote and read.  All that is needed is that the compiler keeps the order: a wavefront-scope fence and a scheduling
// barrier, no s_barrier and no wait for every outstanding LDS operation as __syncthreads() would add.
__device__ __forceinline__ void lds_wave_sync() {
#ifdef NEO_STRONG_SYNC  // (diagnostic builds: a workgroup barrier with its full waits)
  __syncthreads();
#else
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
#endif
}

// reciprocal to working precision: v_rcp_f64 (4.6e-8 raw on gfx950) with two Newton steps, v_rcp_f32 (1 ulp) as it is
__device__ __forceinline__ double precise_rcp(double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = fma(fma(-d, r, 1.0), r, r);
  r = fma(fma(-d, r, 1.0), r, r);
  return r;
}
__device__ __forceinline__ float precise_rcp(float d) { return __builtin_amdgcn_rcpf(d); }
// position markers in the assembly listing (tools/probe/mark_counts.py prices the phases between them); no code
#ifdef NEO_MARKS
#define NEO_MARK(name) asm volatile("; NEOMARK " name)
#else
#define NEO_MARK(name)
#endif
// the value, hidden from loop-invariant code motion and common-subexpression elimination: what is computed from it is
// computed where it is written (no instruction; used where a hoisted address costs a register across a whole loop)
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ float opaque(float v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ double opaque(double v) {
  asm volatile("" : "+v"(v));
  return v;
}
// the same for a wave-uniform value (it stays in a scalar register)
__device__ __forceinline__ int opaque_uniform(int v) {
  asm volatile("" : "+s"(v));
  return v;
}
// lane predicates compared WHERE THEY ARE USED: the bound goes through an opaque scalar copy, so the compare cannot be
// hoisted out of the optimiser loop -- where it would be a scalar register pair that lives across the whole loop, is
// spilled to a lane of a vector register and costs two v_readlane at every use instead of one v_cmp (DevBackend::eval)
__device__ __forceinline__ bool lane_lt(int bound) { return (int)__lane_id() < opaque_uniform(bound); }
__device__ __forceinline__ bool lane_ge(int bound) { return (int)__lane_id() >= opaque_uniform(bound); }
__device__ __forceinline__ bool lane_eq(int which) { return (int)__lane_id() == opaque_uniform(which); }

// ------------------------------------------------------------------ the typed layer
// Every cross-lane instruction moves 32-bit words.  NEO_MAP_WORDS returns the value v of type T with the word operation
// WORD_OP -- an expression in the int `w` -- applied to each of its words: an int as it is, a float through its bits, a
// double as its low word, then its high word.  Exactly these three types: the 8-byte path goes through __double2loint,
// which would quietly CONVERT a long long or a size_t to double first.
// A macro, not a function taking a functor: the optimiser simplifies every function on its own before it inlines it, and a
// level more between a primitive and its builtin changes what it makes of the word pair of a double (a 64-bit lane read
// in one place, two 32-bit ones in another) and, through that, the register allocation of the kernels around it.
template <class T>
constexpr bool is_lane_type = std::is_same<T, int>::value || std::is_same<T, float>::value || std::is_same<T, double>::value;
#define NEO_MAP_WORDS(T, v, WORD_OP)                                                              \
  static_assert(is_lane_type<T>, "cross-lane primitives take exactly int, float or double");      \
  if constexpr (std::is_same<T, int>::value) {                                                    \
    const int w = v;                                                                              \
    return WORD_OP;                                                                               \
  } else if constexpr (std::is_same<T, float>::value) {                                           \
    const int w = __float_as_int(v);                                                              \
    return __int_as_float(WORD_OP);                                                               \
  } else {                                                                                        \
    int w = __double2loint(v);                                                                    \
    const int lo = WORD_OP;                                                                       \
    w = __double2hiint(v);                                                                        \
    const int hi = WORD_OP;                                                                       \
    return __hiloint2double(hi, lo);                                                              \
  }

// value of lane src (v_readlane; two for a double)
template <class T>
__device__ __forceinline__ T rdlane(T v, int src /*wave-uniform*/) {
  NEO_MAP_WORDS(T, v, __builtin_amdgcn_readlane(w, src))
}
// a wave-uniform value back into scalar registers (v_readfirstlane)
template <class T>
__device__ __forceinline__ T uniform(T v) {
  NEO_MAP_WORDS(T, v, __builtin_amdgcn_readfirstlane(w))
}

// ---- DPP cross-lane moves (no LDS round trip).  ctrl: 0x110+n = row_shr:n (lane i <- lane i-n inside
// its row of 16), 0x142 / 0x143 = row_bcast:15 / row_bcast:31, 0x130 / 0x138 = wave_shl:1 / wave_shr:1.
// Lanes without a valid source (or masked off by row_mask) receive 0.  With every row enabled that is the
// instruction's own bound_ctrl zero fill: no register has to be preset to 0 ahead of each move (two v_mov_b32 per
// fp64 step, 8 of the 34 instructions of a wave_sum); with a row mask the masked rows keep `old`, which must be the 0.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, ROW_MASK == 0xf);
}
template <int CTRL, int ROW_MASK = 0xf, class T>
__device__ __forceinline__ T dpp(T v) {
  NEO_MAP_WORDS(T, v, (dpp_i<CTRL, ROW_MASK>(w)))
}
// The two row broadcasts of a reduction that is read at lane 63 only: rows masked off by row_mask are left UNDEFINED
// (no preset register, v_mov_dpp with an undefined `old`).  Lane 63 depends only on written rows: row_bcast:15 (rows 1,
// 3) gives lane 31 = S1 + S0 and lane 63 = S3 + S2, row_bcast:31 (rows 2, 3) adds lane 31 to lane 63.  Not for scans.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_any_i(int v) {
  return __builtin_amdgcn_mov_dpp(v, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK, class T>
__device__ __forceinline__ T dpp_any(T v) {
  NEO_MAP_WORDS(T, v, (dpp_any_i<CTRL, ROW_MASK>(w)))
}
// the lane's OWN value where it has no source (bound_ctrl off, old = the value): neutral for a minimum, whatever the
// values are
template <int CTRL, int ROW_MASK = 0xf, class T>
__device__ __forceinline__ T dpp_keep(T v) {
  NEO_MAP_WORDS(T, v, __builtin_amdgcn_update_dpp(w, w, CTRL, ROW_MASK, 0xf, false))
}
// what a lane without a source receives in a scan step: the first two moves as policies
struct FillZero {
  template <int CTRL, int ROW_MASK, class T>
  static __device__ __forceinline__ T move(T v) { return dpp<CTRL, ROW_MASK>(v); }
};
struct FillAny {
  template <int CTRL, int ROW_MASK, class T>
  static __device__ __forceinline__ T move(T v) { return dpp_any<CTRL, ROW_MASK>(v); }
};

// ---- scans with a fixed association order.  row_scan: inclusive scan inside each row of 16 (row_shr 1, 2, 4, 8; lane 15
// of a row ends with the row's total).  wave_scan: that, then the two row broadcasts -- an inclusive scan over the 64 lanes
// when the broadcasts fill like the row steps, a reduction valid at lane 63 alone with FillAny.  op(own, moved).
template <class Fill = FillZero, class T, class Op>
__device__ __forceinline__ T row_scan(T v, Op op) {
  v = op(v, Fill::template move<0x111, 0xf>(v));
  v = op(v, Fill::template move<0x112, 0xf>(v));
  v = op(v, Fill::template move<0x114, 0xf>(v));
  v = op(v, Fill::template move<0x118, 0xf>(v));
  return v;
}
template <class Fill = FillZero, class BcastFill = Fill, class T, class Op>
__device__ __forceinline__ T wave_scan(T v, Op op) {
  v = row_scan<Fill>(v, op);
  v = op(v, BcastFill::template move<0x142, 0xa>(v));
  v = op(v, BcastFill::template move<0x143, 0xc>(v));
  return v;
}
// the wave-wide result, returned wave-uniform (taken from lane 63 through v_readlane)
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
  return rdlane(wave_scan<FillZero, FillAny>(v, op), kWave - 1);
}
struct OpAdd {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct OpMax {
  __device__ __forceinline__ int operator()(int a, int b) const { return max(a, b); }
  __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
  __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
};
// wave-wide sum / max; maxima of NON-NEGATIVE values (the 0 fill of the DPP moves is then neutral)
template <class T>
__device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, OpAdd()); }
template <class T>
__device__ __forceinline__ T wave_max_nonneg(T v) { return wave_reduce(v, OpMax()); }
// (the two int sums keep a body of their own: written through op(v, moved) the compiler commutes their additions and
//  folds the prefix sum's last move into a v_add_u32_dpp -- the same values from other instructions than before)
__device__ __forceinline__ int wave_sum(int v) {
  v += dpp<0x111>(v);
  v += dpp<0x112>(v);
  v += dpp<0x114>(v);
  v += dpp<0x118>(v);
  v += dpp_any<0x142, 0xa>(v);
  v += dpp_any<0x143, 0xc>(v);
  return rdlane(v, kWave - 1);
}
// inclusive prefix sum / prefix maximum over the lanes of the wavefront (non-negative ints; the same DPP sequence as
// wave_sum, which is that scan read at lane 63)
__device__ __forceinline__ int wave_scan_add(int v) {
  v += dpp<0x111>(v);
  v += dpp<0x112>(v);
  v += dpp<0x114>(v);
  v += dpp<0x118>(v);
  v += dpp<0x142, 0xa>(v);
  v += dpp<0x143, 0xc>(v);
  return v;
}
__device__ __forceinline__ int wave_scan_max_nonneg(int v) { return wave_scan(v, OpMax()); }

// Four wave-wide sums for little more than the price of one: the four per-lane values are first folded onto one
// register -- v_permlane32_swap / v_permlane16_swap (gfx950) exchange half-waves and odd/even rows of two registers, so
// two adds leave the 64 partials of value k on the 16 lanes of row k -- then ONE row-wise DPP scan finishes all four
// (lane 15 of row k holds the total of value k).  One dependent chain of 7 additions instead of four of 6, 37
// instructions instead of 80 (fp64); for fp32: 2 + 1 register swaps, 3 adds, one row-wise DPP scan, 4 v_readlane -- the
// price of about one and a half wave_sum(float) for four sums on ONE dependent chain (the paired two-loop recursion
// batches its dots).  Fixed association order: half-waves first, then odd / even rows, then the 16 lanes of a row left
// to right.
template <class T, class F>
__device__ __forceinline__ void swap_words(T &x, T &y, F f) {  // f(unsigned, unsigned): the two exchanged words
  static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value, "float or double");
  if constexpr (std::is_same<T, float>::value) {
    const auto r = f(__float_as_uint(x), __float_as_uint(y));
    x = __uint_as_float(r[0]);
    y = __uint_as_float(r[1]);
  } else {
    const auto lo = f((unsigned)__double2loint(x), (unsigned)__double2loint(y));
    const auto hi = f((unsigned)__double2hiint(x), (unsigned)__double2hiint(y));
    x = __hiloint2double((int)hi[0], (int)lo[0]);
    y = __hiloint2double((int)hi[1], (int)lo[1]);
  }
}
template <class T>
__device__ __forceinline__ void swap_half_waves(T &x, T &y) {  // lanes 32..63 of x <-> lanes 0..31 of y
  swap_words(x, y, [](unsigned a, unsigned b) { return __builtin_amdgcn_permlane32_swap(a, b, false, false); });
}
template <class T>
__device__ __forceinline__ void swap_odd_even_rows(T &x, T &y) {  // odd rows of x <-> even rows of y
  swap_words(x, y, [](unsigned a, unsigned b) { return __builtin_amdgcn_permlane16_swap(a, b, false, false); });
}
template <class T>
__device__ __forceinline__ void wave_sum4(T a, T b, T c, T d, T &ta, T &tb, T &tc, T &td) {
  swap_half_waves(a, c);
  T x = a + c;  // lanes 0..31: a folded to 32 values, lanes 32..63: c
  swap_half_waves(b, d);
  T y = b + d;
  swap_odd_even_rows(x, y);
  T z = x + y;  // row 0: a, row 1: b, row 2: c, row 3: d (16 partials each)
  z = row_scan(z, OpAdd());
  ta = rdlane(z, 15);
  tb = rdlane(z, 31);
  tc = rdlane(z, 47);
  td = rdlane(z, 63);
}

// value of lane (l-1) / (l+1); lanes without such a neighbour get `fill`
template <class T>
__device__ __forceinline__ T from_prev(T v, T fill) {
  const T o = dpp<0x138>(v);  // wave_shr:1
  return lane_eq(0) ? fill : o;
}
template <class T>
__device__ __forceinline__ T from_next(T v, T fill) {
  const T o = dpp<0x130>(v);  // wave_shl:1
  return lane_eq(kWave - 1) ? fill : o;
}

#undef NEO_MAP_WORDS

}  // namespace neo
