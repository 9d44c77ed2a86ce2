// kdev.h -- device-side building blocks shared by the kernel files (kernels.hip, sched.hip): element / packet
// arithmetic, cache-policy loads and stores, and the rendezvous of the device-synchronised collectives.
// Included by HIP translation units only.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

// ---- the few constructs a host compiler cannot take, behind names ------------------------------------------------------
// tests/devsim/ compiles THESE kernel sources for the CPU (lanes as threads, under ThreadSanitizer) to race the flag protocols
// of the code that ships instead of a model of them; it defines XMPI_DEVSIM and supplies its own versions of the four macros
// and of the system-scope packet accessors further down.  Nothing else in the kernels knows about it.
#ifndef XMPI_DEVSIM
#define XMPI_SHARED(T, name) __shared__ T name
// this wave's memory operations have completed (stores: acknowledged by where they were written to)
#define XMPI_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define XMPI_REGS_DEFINED4(a, b, c, d) asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d))
#define XMPI_REG_DEFINED(a) asm volatile("" : "+v"(a)::"memory")
#endif

namespace xmpi {
namespace {

constexpr int kBlock = 256;      // 4 waves: one per SIMD
constexpr int kUnroll = 4;       // 16-byte packets per lane per operand in flight

enum { DT_U8 = 0, DT_I32 = 1, DT_I64 = 2, DT_F16 = 3, DT_F32 = 4, DT_F64 = 5, DT_BF16 = 6, DT_F8E4M3 = 7, DT_F8E5M2 = 8 };
// OP_SUM_WIDE (XMPI_SUM_WIDE): _Float16 / bf16_t / f8e4m3_t / f8e5m2_t only, and only in the kernels that see all N contributions to
// an element in one lane (FoldAcc below); the launchers hand it to nothing else (launch.h with_fold_op)
// The two 8-bit float types exist in those kernels only, under every operator: the stepped kernels and reduce2* pass partial results
// between ranks in T, and two or three mantissa bits are not something to pass round a ring (launch.h keeps them out)
// OP_BAND / OP_BOR / OP_BXOR (XMPI_BAND / _BOR / _BXOR): uint8_t, int32_t and int64_t only, in every kernel that has an operator
// (launch.h with_op hands them on for those three types and for no other)
enum { OP_SUM = 0, OP_PROD = 1, OP_MIN = 2, OP_MAX = 3, OP_SUM_WIDE = 4, OP_BAND = 5, OP_BOR = 6, OP_BXOR = 7 };
template <int OP>
constexpr bool kBitOp = OP == OP_BAND || OP == OP_BOR || OP == OP_BXOR;

struct bf16_t {
  uint16_t bits;
};
// OCP 8-bit floating point v1.0.  E4M3: S.EEEE.MMM, bias 7, no infinities, S.1111.111 is NaN, largest finite 448 (0x7E), smallest
// subnormal 2^-9.  E5M2: S.EEEEE.MM, bias 15, IEEE-like: 0x7C +-inf, 0x7D..0x7F NaN, largest finite 57344 (0x7B), smallest subnormal 2^-16.
struct f8e4m3_t {
  uint8_t bits;
};
struct f8e5m2_t {
  uint8_t bits;
};
template <typename T>
constexpr bool kF8Elem = __is_same(T, f8e4m3_t) || __is_same(T, f8e5m2_t);

typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
// 16-byte packet: a native vector (not HIP's pack_t struct) so it always lives in 4 VGPRs
typedef unsigned int pack_t __attribute__((ext_vector_type(4)));

template <typename T>
constexpr bool kIntegerElem = __is_same(T, uint8_t) || __is_same(T, int32_t) || __is_same(T, int64_t);

// ---- the bitwise operators: on W itself, whatever it holds -- an element, the 8 payload bytes of an LL line (uint64_t), a 16-byte
// packet (four 32-bit VALU operations: the element width plays no part, nor does signedness)
template <int OP, typename W>
__device__ __forceinline__ W bitop(W a, W b) {
  static_assert(kBitOp<OP>, "AND, OR or XOR");
  if constexpr (OP == OP_BAND) return (W)(a & b);
  else if constexpr (OP == OP_BOR) return (W)(a | b);
  else return (W)(a ^ b);
}

// ---- scalar combine: one rounding per operation, min/max spelled as in oracle/xmpi_oracle.c ---

template <typename T, int OP>
__device__ __forceinline__ T combine(T a, T b) {
  static_assert((OP >= OP_SUM && OP <= OP_MAX) || kBitOp<OP>, "a two-operand combine has the four arithmetic operators and the three bitwise ones: every branch below names its own");
  static_assert(!kBitOp<OP> || kIntegerElem<T>, "a bitwise operator is never instantiated with a floating-point type or bf16_t (launch.h with_op)");
  if constexpr (OP == OP_SUM) return a + b;
  else if constexpr (OP == OP_PROD) return a * b;
  else if constexpr (OP == OP_MIN) return (b < a) ? b : a;
  else if constexpr (OP == OP_MAX) return (a < b) ? b : a;
  else return bitop<OP>(a, b);
}

__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

template <int OP>
__device__ __forceinline__ bf16_t combine_bf16(bf16_t a, bf16_t b) {
  static_assert(OP >= OP_SUM && OP <= OP_MAX, "bf16_t has the four arithmetic operators (the bitwise ones are for integer types)");
  float x = bf16_to_f32(a.bits), y = bf16_to_f32(b.bits);
  if constexpr (OP == OP_SUM) return bf16_t{f32_to_bf16(x + y)};
  else if constexpr (OP == OP_PROD) return bf16_t{f32_to_bf16(x * y)};
  else if constexpr (OP == OP_MIN) return (y < x) ? b : a;
  else if constexpr (OP == OP_MAX) return (x < y) ? b : a;
}

// ---- the 8-bit floats: f32(x) is exact; narrow(f) rounds to nearest, ties to even, with gradual underflow, and SATURATES -------------
// A NaN gives a NaN of the type (which one is not specified); +-inf gives +-inf (E5M2; E4M3 has none and no fold reaches one); any
// other value whose rounded magnitude exceeds the largest finite one becomes +-448 / +-57344 (the default of HIP's __hip_fp8 types): a
// sum of finite inputs never turns into inf or NaN.  Written once in plain C++ -- the definition, what the host pass and tests/devsim
// compile, and what tests/f8_ref.py restates -- and, on gfx950, as the packed conversion instructions further down, which are
// held to it bit for bit by the tests on the card.
template <bool E5>
__device__ __forceinline__ float f8_to_f32_soft(uint8_t b) {
  constexpr int MB = E5 ? 2 : 3, BIAS = E5 ? 15 : 7;
  const uint32_t sign = (uint32_t)(b & 0x80u) << 24, e = (uint32_t)(b & 0x7Fu) >> MB, m = b & ((1u << MB) - 1u);
  if constexpr (E5) {
    if (e == 31u) return __uint_as_float(sign | 0x7F800000u | (m << 21));  // +-inf, NaN
  } else {
    if ((b & 0x7Fu) == 0x7Fu) return __uint_as_float(sign | 0x7FC00000u);
  }
  if (e == 0u) return __uint_as_float(sign | __float_as_uint((float)m * (E5 ? 0x1p-16f : 0x1p-9f)));  // +-0 and the subnormals
  return __uint_as_float(sign | ((e + 127u - (uint32_t)BIAS) << 23) | (m << (23 - MB)));
}
template <bool E5>
__device__ __forceinline__ uint8_t f32_to_f8_soft(float f) {
  constexpr int MB = E5 ? 2 : 3, BIAS = E5 ? 15 : 7, EMIN = 1 - BIAS;
  constexpr uint32_t MAXFIN = E5 ? 0x7Bu : 0x7Eu;
  const uint32_t u = __float_as_uint(f), a = u & 0x7FFFFFFFu;
  const uint8_t sign = (uint8_t)((u >> 24) & 0x80u);
  if (a > 0x7F800000u) return (uint8_t)(sign | 0x7Fu);                     // NaN
  if (a == 0x7F800000u) return (uint8_t)(sign | (E5 ? 0x7Cu : MAXFIN));    // inf (E4M3: never reached; saturates)
  const int e = (int)(a >> 23) - 127;
  const uint32_t sig = (a & 0x7FFFFFu) | 0x800000u;  // 1.m, 24 bits (an f32 subnormal has e = -127: far below half the smallest subnormal)
  uint32_t q = 0;
  // the bits below the type's last place: `sh` of them -- 23 - MB for a normal result, one more per binade below the smallest normal
  const int sh = 23 - MB + (e >= EMIN ? 0 : EMIN - e);
  if (sh <= 24) {
    q = sig >> sh;
    const uint32_t rem = sig & ((1u << sh) - 1u), half = 1u << (sh - 1);
    if (rem > half || (rem == half && (q & 1u))) q++;
    // normal: the leading 1 of q counts as exponent 1 + ...; a carry out of the mantissa runs into the exponent field as it should
    if (e >= EMIN) q += (uint32_t)(e + BIAS - 1) << MB;
  }
  if (q > MAXFIN) q = MAXFIN;  // saturate (E5M2: this is also what keeps a rounded 0x7C from reading as inf)
  return (uint8_t)(sign | q);
}
template <typename T>
__device__ __forceinline__ float f8_to_f32(T v) {
  static_assert(kF8Elem<T>, "f8e4m3_t or f8e5m2_t");
#if defined(__gfx950__)
  if constexpr (__is_same(T, f8e4m3_t)) return __builtin_amdgcn_cvt_f32_fp8((int)v.bits, 0);
  else return __builtin_amdgcn_cvt_f32_bf8((int)v.bits, 0);
#else
  return f8_to_f32_soft<__is_same(T, f8e5m2_t)>(v.bits);
#endif
}
#if defined(__gfx950__)
// the saturation, before the instruction: it is not relied on for anything past the largest finite value (NaN and inf pass as they are)
template <typename T>
__device__ __forceinline__ float f8_clamp(float f) {
  constexpr float M = __is_same(T, f8e4m3_t) ? 448.0f : 57344.0f;
  return __builtin_amdgcn_classf(f, 0x207) ? f : __builtin_amdgcn_fmed3f(f, M, -M);  // 0x207: sNaN | qNaN | -inf | +inf
}
// two floats -> the low (HI = false) or high half of `old`
template <typename T, bool HI>
__device__ __forceinline__ int f8_pack2(float a, float b, int old) {
  if constexpr (__is_same(T, f8e4m3_t)) return __builtin_amdgcn_cvt_pk_fp8_f32(f8_clamp<T>(a), f8_clamp<T>(b), old, HI);
  else return __builtin_amdgcn_cvt_pk_bf8_f32(f8_clamp<T>(a), f8_clamp<T>(b), old, HI);
}
#endif
template <typename T>
__device__ __forceinline__ T f32_to_f8(float f) {
  static_assert(kF8Elem<T>, "f8e4m3_t or f8e5m2_t");
#if defined(__gfx950__)
  return T{(uint8_t)f8_pack2<T, false>(f, f, 0)};
#else
  return T{f32_to_f8_soft<__is_same(T, f8e5m2_t)>(f)};
#endif
}
// the 4 elements of a 32-bit word <-> 4 floats: v_cvt_pk_f32_fp8 / _bf8 (two elements per instruction, the half word selected) and
// v_cvt_pk_fp8_f32 / _bf8_f32 on gfx950
template <typename T>
__device__ __forceinline__ void f8_widen4(uint32_t w, float* f) {
#if defined(__gfx950__)
  typedef float float2_t __attribute__((ext_vector_type(2)));
  float2_t lo, hi;
  if constexpr (__is_same(T, f8e4m3_t)) {
    lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  } else {
    lo = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, false);
    hi = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, true);
  }
  f[0] = lo[0]; f[1] = lo[1]; f[2] = hi[0]; f[3] = hi[1];
#else
#pragma unroll
  for (int i = 0; i < 4; i++) f[i] = f8_to_f32_soft<__is_same(T, f8e5m2_t)>((uint8_t)(w >> (8 * i)));
#endif
}
template <typename T>
__device__ __forceinline__ uint32_t f8_narrow4(const float* f) {
#if defined(__gfx950__)
  return (uint32_t)f8_pack2<T, true>(f[2], f[3], f8_pack2<T, false>(f[0], f[1], 0));
#else
  uint32_t w = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) w |= (uint32_t)f32_to_f8_soft<__is_same(T, f8e5m2_t)>(f[i]) << (8 * i);
  return w;
#endif
}

// min / max compare the widened values with combine_bf16's expressions and return the chosen operand's own byte
template <typename T, int OP>
__device__ __forceinline__ T combine_f8(T a, T b) {
  static_assert(OP >= OP_SUM && OP <= OP_MAX, "an 8-bit float has the four arithmetic operators (the bitwise ones are for integer types)");
  const float x = f8_to_f32(a), y = f8_to_f32(b);
  if constexpr (OP == OP_SUM) return f32_to_f8<T>(x + y);
  else if constexpr (OP == OP_PROD) return f32_to_f8<T>(x * y);
  else if constexpr (OP == OP_MIN) return (y < x) ? b : a;
  else if constexpr (OP == OP_MAX) return (x < y) ? b : a;
}

// wrapping integer arithmetic (Go semantics) without signed-overflow UB
template <int OP>
__device__ __forceinline__ int32_t combine_i32(int32_t a, int32_t b) {
  if constexpr (OP == OP_SUM) return (int32_t)((uint32_t)a + (uint32_t)b);
  else if constexpr (OP == OP_PROD) return (int32_t)((uint32_t)a * (uint32_t)b);
  else return combine<int32_t, OP>(a, b);
}
template <int OP>
__device__ __forceinline__ int64_t combine_i64(int64_t a, int64_t b) {
  if constexpr (OP == OP_SUM) return (int64_t)((uint64_t)a + (uint64_t)b);
  else if constexpr (OP == OP_PROD) return (int64_t)((uint64_t)a * (uint64_t)b);
  else return combine<int64_t, OP>(a, b);
}

template <typename T, int OP>
__device__ __forceinline__ T combine_any(T a, T b) {
  if constexpr (kF8Elem<T>) return combine_f8<T, OP>(a, b);
  else if constexpr (sizeof(T) == 2 && !__is_same(T, _Float16)) return combine_bf16<OP>(a, b);
  else if constexpr (__is_same(T, int32_t)) return combine_i32<OP>(a, b);
  else if constexpr (__is_same(T, int64_t)) return combine_i64<OP>(a, b);
  else if constexpr (__is_same(T, uint8_t)) {
    if constexpr (OP == OP_SUM) return (uint8_t)(a + b);
    else if constexpr (OP == OP_PROD) return (uint8_t)(a * b);
    else return combine<uint8_t, OP>(a, b);
  } else return combine<T, OP>(a, b);
}

// ---- a word of 8-bit floats (a 16-byte packet: 16 elements; the 8 payload bytes of an LL line: 8) ------------------------------
// Both operands are widened ONCE with the packed conversions (a packet: 8 instructions each), combined as floats and narrowed with
// the packed conversions -- not sixteen scalar round trips.  min / max pick whole bytes of the operands by the widened comparison.
template <typename T, typename W>
__device__ __forceinline__ void f8_widen_word(W w, float (&f)[sizeof(W)]) {
  union { W u; uint32_t d[sizeof(W) / 4]; } x;
  x.u = w;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(W) / 4); i++) f8_widen4<T>(x.d[i], &f[4 * i]);
}
template <typename T, typename W>
__device__ __forceinline__ W f8_narrow_word(const float (&f)[sizeof(W)]) {
  union { W u; uint32_t d[sizeof(W) / 4]; } r;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(W) / 4); i++) r.d[i] = f8_narrow4<T>(&f[4 * i]);
  return r.u;
}
template <typename T, int OP, typename W>
__device__ __forceinline__ W combine_f8_word(W a, W b) {
  static_assert(OP >= OP_SUM && OP <= OP_MAX, "an 8-bit float has the four arithmetic operators");
  constexpr int N = sizeof(W);
  float x[N], y[N];
  f8_widen_word<T, W>(a, x);
  f8_widen_word<T, W>(b, y);
  if constexpr (OP == OP_SUM || OP == OP_PROD) {
#pragma unroll
    for (int i = 0; i < N; i++) x[i] = (OP == OP_SUM) ? (x[i] + y[i]) : (x[i] * y[i]);
    return f8_narrow_word<T, W>(x);
  } else {
    union { W u; uint32_t d[N / 4]; } p, q, r;
    p.u = a; q.u = b;
#pragma unroll
    for (int i = 0; i < N / 4; i++) {
      uint32_t take_b = 0;  // 0xFF in every byte whose element comes from b
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const bool t = (OP == OP_MIN) ? (y[4 * i + k] < x[4 * i + k]) : (x[4 * i + k] < y[4 * i + k]);
        take_b |= t ? (0xFFu << (8 * k)) : 0u;
      }
      r.d[i] = (q.d[i] & take_b) | (p.d[i] & ~take_b);
    }
    return r.u;
  }
}

// ---- 16-byte packet combine ------------------------------------------------------------------

template <typename T, int OP>
__device__ __forceinline__ pack_t combine16(pack_t a, pack_t b) {
  constexpr int N = 16 / sizeof(T);
  if constexpr (kBitOp<OP>) {
    static_assert(kIntegerElem<T>, "a bitwise operator is never instantiated with a floating-point type or bf16_t (launch.h with_op)");
    return bitop<OP>(a, b);  // the packet itself: v_and_b32 / v_or_b32 / v_xor_b32 x 4, no per-element loop
  } else if constexpr (__is_same(T, _Float16) && (OP == OP_SUM || OP == OP_PROD)) {
    // packed halves: v_pk_add_f16 / v_pk_mul_f16, 2 elements per VALU lane-op
    union { pack_t u; half2_t h[4]; } x, y, r;
    x.u = a; y.u = b;
#pragma unroll
    for (int i = 0; i < 4; i++) r.h[i] = (OP == OP_SUM) ? (x.h[i] + y.h[i]) : (x.h[i] * y.h[i]);
    return r.u;
  } else if constexpr (kF8Elem<T>) {
    return combine_f8_word<T, OP, pack_t>(a, b);
  } else {
    union { pack_t u; T e[N]; } x, y, r;
    x.u = a; y.u = b;
#pragma unroll
    for (int i = 0; i < N; i++) r.e[i] = combine_any<T, OP>(x.e[i], y.e[i]);
    return r.u;
  }
}

// 8-byte line (ll.hip: the payload of a {data, flag} line)
template <typename T, int OP>
__device__ __forceinline__ uint64_t combine8(uint64_t a, uint64_t b) {
  if constexpr (kBitOp<OP>) {
    static_assert(kIntegerElem<T>, "a bitwise operator is never instantiated with a floating-point type or bf16_t (launch.h with_op)");
    return bitop<OP>(a, b);
  } else if constexpr (kF8Elem<T>) {
    return combine_f8_word<T, OP, uint64_t>(a, b);
  } else {
    constexpr int N = 8 / sizeof(T);
    union {
      uint64_t u;
      T e[N];
    } x, y, r;
    x.u = a;
    y.u = b;
#pragma unroll
    for (int i = 0; i < N; i++) r.e[i] = combine_any<T, OP>(x.e[i], y.e[i]);
    return r.u;
  }
}

// ---- the accumulator of a fold: first source, N-1 times add(), result() ----------------------------------------------------
// W is what a lane holds of every source: a 16-byte packet (pack_t), the 8 payload bytes of an LL line (uint64_t) or one element (T).
// Every operator but OP_SUM_WIDE accumulates in W itself -- combine16 / combine8 / combine_any per source, one rounding each, which
// is "bit-identical to a host sum in rank order" (the 8-bit floats: acc = narrow(f32(acc) op f32(x)), a packet widened and narrowed by
// the packed conversions, the accumulator in its four VGPRs between sources).  OP_SUM_WIDE (_Float16, bf16_t, f8e4m3_t, f8e5m2_t)
// holds the sizeof(W) / sizeof(T) elements as floats:
//   narrow( ((f32(x0) + f32(x1)) + f32(x2)) + ... )      f32() exact, IEEE f32 additions in source order, narrow() ONCE --
// bf16: f32_to_bf16 above (round to nearest even, its NaN rule); f16: the conversion (_Float16)f, round to nearest even; the 8-bit
// floats: f32_to_f8 (nearest even, saturating).  Plain C++ conversions wherever this is not compiled for gfx950: tests/devsim
// compiles it for the host.
// (the 8-bit floats: f8_to_f32 / f32_to_f8 above -- a word of them by the packed conversions, an element alone by itself)
template <typename T>
__device__ __forceinline__ float widen1(T v) {
  static_assert(sizeof(T) < 4, "_Float16, bf16_t, f8e4m3_t or f8e5m2_t");
  if constexpr (kF8Elem<T>) return f8_to_f32(v);
  else if constexpr (__is_same(T, _Float16)) return (float)v;
  else return bf16_to_f32(v.bits);
}
template <typename T>
__device__ __forceinline__ T narrow1(float f) {
  static_assert(sizeof(T) < 4, "_Float16, bf16_t, f8e4m3_t or f8e5m2_t");
  if constexpr (kF8Elem<T>) return f32_to_f8<T>(f);
  else if constexpr (__is_same(T, _Float16)) return (_Float16)f;
  else return bf16_t{f32_to_bf16(f)};
}
template <typename T, typename W>
__device__ __forceinline__ void widen_word(W w, float (&f)[sizeof(W) / sizeof(T)]) {
  if constexpr (kF8Elem<T> && sizeof(W) >= 4) f8_widen_word<T, W>(w, f);
  else {
    union { W u; T e[sizeof(W) / sizeof(T)]; } x;
    x.u = w;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(W) / sizeof(T)); i++) f[i] = widen1<T>(x.e[i]);
  }
}
template <typename T, typename W>
__device__ __forceinline__ W narrow_word(const float (&f)[sizeof(W) / sizeof(T)]) {
  if constexpr (kF8Elem<T> && sizeof(W) >= 4) return f8_narrow_word<T, W>(f);
  else {
    union { W u; T e[sizeof(W) / sizeof(T)]; } r;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(W) / sizeof(T)); i++) r.e[i] = narrow1<T>(f[i]);
    return r.u;
  }
}
// a 16-byte packet of 8 halves / bfloat16s or 16 8-bit floats <-> as many floats
template <typename T>
__device__ __forceinline__ void widen16(pack_t p, float (&f)[16 / sizeof(T)]) { widen_word<T, pack_t>(p, f); }
template <typename T>
__device__ __forceinline__ pack_t narrow16(const float (&f)[16 / sizeof(T)]) { return narrow_word<T, pack_t>(f); }

template <typename T, int OP>
constexpr bool kWideFold = OP == OP_SUM_WIDE && (__is_same(T, _Float16) || __is_same(T, bf16_t) || kF8Elem<T>);

template <typename T, int OP, typename W, bool WIDE = kWideFold<T, OP>>
struct FoldAcc {
  static_assert(OP != OP_SUM_WIDE, "OP_SUM_WIDE is OP_SUM for every type but _Float16 / bf16_t / the 8-bit floats: the launcher says so (with_fold_op)");
  W v;
  __device__ __forceinline__ explicit FoldAcc(W first) : v(first) {}
  __device__ __forceinline__ void add(W x) {
    if constexpr (__is_same(W, pack_t)) v = combine16<T, OP>(v, x);
    else if constexpr (__is_same(W, T)) v = combine_any<T, OP>(v, x);
    else v = combine8<T, OP>(v, x);
  }
  __device__ __forceinline__ W result() const { return v; }
};
template <typename T, int OP, typename W>
struct FoldAcc<T, OP, W, true> {
  static constexpr int N = sizeof(W) / sizeof(T);  // an element narrower than f32: 8 or 16 of a packet, 4 or 8 of an LL line, 1
  float f[N];
  __device__ __forceinline__ explicit FoldAcc(W first) { widen_word<T, W>(first, f); }
  __device__ __forceinline__ void add(W x) {
    float g[N];
    widen_word<T, W>(x, g);
#pragma unroll
    for (int i = 0; i < N; i++) f[i] += g[i];
  }
  __device__ __forceinline__ W result() const { return narrow_word<T, W>(f); }
};
template <typename T, int OP>
using Acc16 = FoldAcc<T, OP, pack_t>;  // a packet
template <typename T, int OP>
using Acc1 = FoldAcc<T, OP, T>;        // one element (ragged tails, buffers at odd alignments)

// ---- cache policy of the streaming accesses ----------------------------------------------------
// MODE 0: plain loads and stores.  MODE 1: non-temporal loads and stores.  MODE 2: non-temporal
// loads, plain stores.  Data that is touched once should not displace lines in L2 / the Infinity
// Cache: measured on MI355X at 256 MiB operands (beyond the 256 MiB Infinity Cache) nt loads take
// reduce2<f32> from 5.45 to 6.6-6.8 TB/s; which mode wins at a given size is a launch-time choice
// (set_kernel_mode / XMPI_KERNEL_MODE), the arithmetic is identical in all three.
template <int MODE>
__device__ __forceinline__ pack_t ldp(const pack_t* p) {
  if constexpr (MODE != 0) return __builtin_nontemporal_load(p);
  else return *p;
}
template <int MODE>
__device__ __forceinline__ void stp(pack_t* p, pack_t v) {
  if constexpr (MODE == 1) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// ---- device-synchronised collectives: system-scope flag words, rendezvous, completion --------------------
__device__ __forceinline__ uint64_t ld_sys64(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void st_sys64(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {  // the value is the same in every lane: keep it in SGPRs
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

// the XCD (accelerator complex die) this wave runs on: HW_REG_XCC_ID (hardware register 20), bits 3..0
__device__ __forceinline__ uint32_t xcc_id() { return __builtin_amdgcn_s_getreg(20 | (0 << 6) | ((4 - 1) << 11)) & 15u; }

// Wait until *p >= want.  0 = it did; otherwise why not (the job was aborted / the wait outlasted spin_limit).
__device__ uint32_t spin_until(const uint64_t* p, uint64_t want, const int32_t* abort_word, uint64_t spin_limit) {
  if (ld_sys64(p) >= want) return DSYNC_OK;
  const uint64_t t0 = wall_clock64();
  for (uint32_t k = 1;; k++) {
    __builtin_amdgcn_s_sleep(1);
    if (ld_sys64(p) >= want) return DSYNC_OK;
    if ((k & 127u) == 0) {  // the expensive checks (a load over PCIe, the clock) now and then only
      if (abort_word && __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) return DSYNC_ABORTED;
      if (spin_limit && wall_clock64() - t0 > spin_limit) return DSYNC_TIMEOUT;
    }
  }
}
__device__ __forceinline__ uint32_t dsync_spin(const uint64_t* p, uint64_t want, const DsyncArgs& a) {
  return spin_until(p, want, a.abort_word, a.spin_limit);
}

struct DsyncShared {
  uint64_t epoch;                                 // of this kernel
  uint64_t send[kDsyncRanks], recv[kDsyncRanks];  // every rank's buffers as addressable from here
  uint64_t land[kDsyncRanks];                     // ... and its landing block (push forms of the stepped kernels); 0 = it lends none
  uint64_t src[kDsyncRanks], dst[kDsyncRanks];    // this block's segment: sources in rank order, destinations local first
  int nsrc, ndst;
  uint32_t fail, last;
};

// Where this process mapped registration `gen` (table slot `slot`) of `peer`: from the cache in this rank's page, or
// -- the first time, and after the peer re-used the slot -- from the host's table (a few loads over PCIe).
__device__ uint64_t translate(uint64_t comm_tag, const DsyncEntry* table, DsyncPage* mine, int peer, uint64_t slot, uint64_t gen, uint64_t off) {
  if (gen == 0 || slot >= (uint64_t)kDsyncArenas) return 0;
  DsyncEntry* c = &mine->cache[peer][slot];
  uint64_t base, bytes;
  if (__hip_atomic_load(&c->gen, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == gen &&
      __hip_atomic_load(&c->tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == comm_tag) {
    base = __hip_atomic_load(&c->base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bytes = __hip_atomic_load(&c->bytes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    const DsyncEntry* h = &table[peer * kDsyncArenas + (int)slot];
    if (__hip_atomic_load(&h->gen, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != gen) return 0;
    base = __hip_atomic_load(&h->base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    bytes = __hip_atomic_load(&h->bytes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // several blocks may do this at once: they all write the same values, the number last
    __hip_atomic_store(&c->gen, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __hip_atomic_store(&c->base, base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&c->bytes, bytes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&c->tag, comm_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&c->gen, gen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
  return (off <= bytes) ? base + off : 0;
}

__device__ __forceinline__ uint64_t dsync_translate(const DsyncArgs& a, DsyncPage* mine, int peer, uint64_t slot, uint64_t gen, uint64_t off) {
  return translate(a.tag, a.table, mine, peer, slot, gen, off);
}

__device__ void dsync_begin(const DsyncArgs& a, DsyncShared& sh) {
  const int t = threadIdx.x, me = a.me, n = a.n;
  DsyncPage* mine = a.page[me];
  if (t == 0) {
    sh.fail = DSYNC_OK;
    sh.send[me] = (uint64_t)(uintptr_t)a.my_send;
    sh.recv[me] = (uint64_t)(uintptr_t)a.my_recv;
    sh.land[me] = (uint64_t)(uintptr_t)a.my_land;
    // the epoch is counted on the device (every block reads the same value: only the closing block of a kernel
    // advances it, after all the others have finished), so replaying a captured launch counts on
    const uint64_t seen = ld_sys64(&mine->epoch_now);
    sh.epoch = (seen > a.epoch_floor ? seen : a.epoch_floor) + 1;
  }
  __syncthreads();
  const uint64_t epoch = sh.epoch;
  if (t < n && t != me) {
    if (blockIdx.x == 0 && blockIdx.y == 0) {  // one block announces this rank
      DsyncSlot* out = &a.page[t]->ready[me];
      st_sys64(&out->send_gen, a.send_gen);
      st_sys64(&out->send_off, a.send_off);
      st_sys64(&out->recv_gen, a.recv_gen);
      st_sys64(&out->recv_off, a.recv_off);
      st_sys64(&out->slots, a.send_slot | (a.recv_slot << 8) | (a.land_slot << 16) | (a.land_gen ? 1ull << 24 : 0) | (a.sig << 32));
      if (a.land_gen) {  // (bit 24 of `slots` says whether these two mean anything)
        st_sys64(&out->land_gen, a.land_gen);
        st_sys64(&out->land_off, a.land_off);
      }
      __hip_atomic_store(&out->epoch, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const DsyncSlot* in = &mine->ready[t];
    uint32_t why = dsync_spin(&in->epoch, epoch, a);
    if (why == DSYNC_OK) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
      const uint64_t slots = ld_sys64(&in->slots), lgen = (slots >> 24 & 1u) ? ld_sys64(&in->land_gen) : 0;
      const uint64_t s = dsync_translate(a, mine, t, slots & 0xffu, ld_sys64(&in->send_gen), ld_sys64(&in->send_off));
      const uint64_t r = dsync_translate(a, mine, t, (slots >> 8) & 0xffu, ld_sys64(&in->recv_gen), ld_sys64(&in->recv_off));
      const uint64_t l = lgen ? dsync_translate(a, mine, t, (slots >> 16) & 0xffu, lgen, ld_sys64(&in->land_off)) : 0;
      sh.send[t] = s;
      sh.recv[t] = r;
      sh.land[t] = l;
      if (!s || !r || (lgen && !l)) why = DSYNC_UNMAPPED;
      // the peer is in another call (another collective, schedule, length, type, operation or root): nobody moves anything
      if ((uint32_t)a.sig && (uint32_t)(slots >> 32) && (uint32_t)(slots >> 32) != (uint32_t)a.sig) why = DSYNC_MISMATCH;
    }
    if (why != DSYNC_OK) atomicMax(&sh.fail, why);
  }
  // every lane acquires: what the peers wrote before they announced themselves (their inputs) must not be
  // served from a stale line of this CU's L1 / this XCD's L2
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  __syncthreads();
}

// The block that finishes last exchanges "done" with every peer.  xcd_guard (the done kernel of the split form): the masks of
// XCDs the meet and the done kernel's blocks ran on are collected, reported (status[6], status[7]) and -- xcc_need -- checked.
__device__ void dsync_end(const DsyncArgs& a, DsyncShared& sh, bool xcd_guard = false) {
  const int t = threadIdx.x, me = a.me, n = a.n;
  DsyncPage* mine = a.page[me];
  XMPI_DRAIN();  // this wave's stores have left
  __syncthreads();
  if (t == 0) {
    // a block that gave up (its own wait timed out, the job was aborted) says so where the closing block looks:
    // a kernel whose closing block happened to see nothing wrong must not report success for it
    if (sh.fail != DSYNC_OK) __hip_atomic_fetch_max(&mine->failword, sh.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // ... and are visible system-wide (writes back this XCD's L2)
    const uint32_t total = gridDim.x * gridDim.y;
    sh.last = (__hip_atomic_fetch_add(&mine->ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == total - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (!sh.last) return;
  if (t == 0) {
    __hip_atomic_store(&mine->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t f = __hip_atomic_exchange(&mine->failword, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (f > sh.fail) sh.fail = f;
    if (xcd_guard) {
      const uint32_t m = __hip_atomic_exchange(&mine->xcc_meet, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t d = __hip_atomic_exchange(&mine->xcc_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a.status) {
        __hip_atomic_store(a.status + 6, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(a.status + 7, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      if (a.xcc_need > 0 && (__builtin_popcount(m) < a.xcc_need || __builtin_popcount(d) < a.xcc_need) && sh.fail == DSYNC_OK)
        sh.fail = DSYNC_XCD;
    }
  }
  __syncthreads();
  uint32_t why = DSYNC_OK;
  if (t < n && t != me) {
    __hip_atomic_store(&a.page[t]->done[me][0], sh.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (sh.fail == DSYNC_OK) why = dsync_spin(&mine->done[t][0], sh.epoch, a);
    if (why != DSYNC_OK) atomicMax(&sh.fail, why);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  __syncthreads();
  if (t == 0) {
    st_sys64(&mine->epoch_now, sh.epoch);  // this kernel is over: the next one (an ordinary launch or a graph replay) counts from here
    if (a.host_epoch) st_sys64(a.host_epoch, sh.epoch);
    if (sh.fail != DSYNC_OK && a.status) __hip_atomic_store(a.status, sh.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // the blocking caller's word, last: every rank's stores into this rank's buffers were released before its "done"
    if (a.host_done) __hip_atomic_store(a.host_done, a.done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}


// ---- data that another rank's kernel writes WHILE this kernel runs (the steps of ring / halving / tree) -------------
// 16 bytes straight from / to memory at system scope (sc0 sc1): a load is never served from a line of this XCD's L2 (or
// this CU's L1) that predates the peer's store, a store is written through -- so a step needs no cache maintenance at all:
// the writer waits for its stores' acknowledgements (s_waitcnt vmcnt(0)) and raises the flag, the reader sees the flag and
// loads.  (The alternative -- ordinary accesses bracketed by release / acquire fences -- writes back and invalidates a
// whole L2 per block per step: 2.64 ms for the 8 x 256 MiB ring where the data alone needs 1.7, r03 session 1.)
// The loads are asynchronous inline assembly: sys128_wait() is what makes their results usable.
#ifndef XMPI_DEVSIM
__device__ __forceinline__ void ld_sys128_issue(pack_t& v, const pack_t* p) {
  asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=&v"(v) : "v"(p) : "memory");
}
__device__ __forceinline__ void st_sys128(pack_t* p, pack_t v) {
  // (s_nop: the two wait states the hardware needs before the data registers of a store of more than 8 bytes may be
  // overwritten -- the compiler inserts them for its own stores, it cannot see into this one)
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
template <int U>
__device__ __forceinline__ void sys128_wait(pack_t (&v)[U]) {
  static_assert(U == 1 || U == 2 || U == 4, "unroll");
  if constexpr (U == 1) asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0])::"memory");
  else if constexpr (U == 2) asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0]), "+v"(v[1])::"memory");
  else asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3])::"memory");
}
#else
#include <devsim/sys128.h>  // tests/devsim: the same three accessors for a host compiler
#endif
// any number of packets: one wait, then every register passes through an (empty) volatile statement behind it
template <int U>
__device__ __forceinline__ void sys128_wait_n(pack_t* v) {
  XMPI_DRAIN();
#pragma unroll
  for (int k = 0; k < U; k++) XMPI_REG_DEFINED(v[k]);
  (void)v;
}
// one element, same scope (the ragged ends of a tile, buffers at odd alignments)
template <typename T>
__device__ __forceinline__ T ld_sys_elem(const T* p) {
  T out;
  if constexpr (sizeof(T) == 1) {
    const uint8_t u = __hip_atomic_load(reinterpret_cast<const uint8_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __builtin_memcpy(&out, &u, 1);
  } else if constexpr (sizeof(T) == 2) {
    const uint16_t u = __hip_atomic_load(reinterpret_cast<const uint16_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __builtin_memcpy(&out, &u, 2);
  } else if constexpr (sizeof(T) == 4) {
    const uint32_t u = __hip_atomic_load(reinterpret_cast<const uint32_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __builtin_memcpy(&out, &u, 4);
  } else {
    const uint64_t u = __hip_atomic_load(reinterpret_cast<const uint64_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __builtin_memcpy(&out, &u, 8);
  }
  return out;
}
template <typename T>
__device__ __forceinline__ void st_sys_elem(T* p, T v) {
  if constexpr (sizeof(T) == 1) {
    uint8_t u;
    __builtin_memcpy(&u, &v, 1);
    __hip_atomic_store(reinterpret_cast<uint8_t*>(p), u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  } else if constexpr (sizeof(T) == 2) {
    uint16_t u;
    __builtin_memcpy(&u, &v, 2);
    __hip_atomic_store(reinterpret_cast<uint16_t*>(p), u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  } else if constexpr (sizeof(T) == 4) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    __hip_atomic_store(reinterpret_cast<uint32_t*>(p), u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  } else {
    uint64_t u;
    __builtin_memcpy(&u, &v, 8);
    __hip_atomic_store(reinterpret_cast<uint64_t*>(p), u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// dst = src, all blocks of the grid together: 16 KiB tiles, four 16-byte loads per lane in flight (a message is pulled
// over a link: round trips), bytes at odd alignments one by one
__device__ __forceinline__ void copy_span(char* dst, const char* src, size_t bytes, unsigned bid = blockIdx.x, unsigned nb = gridDim.x) {
  const int t = threadIdx.x;
  if ((((uintptr_t)src | (uintptr_t)dst) & 15u) == 0) {
    const size_t npack = bytes / 16;
    constexpr size_t kTile = (size_t)kBlock * 4;
    const pack_t* ps = reinterpret_cast<const pack_t*>(src);
    pack_t* pd = reinterpret_cast<pack_t*>(dst);
    for (size_t base = (size_t)bid * kTile; base < npack; base += (size_t)nb * kTile) {
      if (base + kTile <= npack) {
        pack_t v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = ldp<2>(ps + base + (size_t)u * kBlock + t);
#pragma unroll
        for (int u = 0; u < 4; u++) pd[base + (size_t)u * kBlock + t] = v[u];
      } else {
        for (size_t i = base + t; i < npack; i += kBlock) pd[i] = ldp<2>(ps + i);
      }
    }
    if (bid == 0 && npack * 16 + t < bytes) dst[npack * 16 + t] = src[npack * 16 + t];
  } else {
    for (size_t i = (size_t)bid * kBlock + t; i < bytes; i += (size_t)nb * kBlock) dst[i] = src[i];
  }
}

__device__ __forceinline__ uint64_t* step_flags(DsyncPage* page) {
  return reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(page) + kStepOff);
}

__device__ __forceinline__ VBox* vbox_of(DsyncPage* page) {
  return reinterpret_cast<VBox*>(reinterpret_cast<char*>(page) + kVBoxOff);
}

}  // namespace
}  // namespace xmpi
