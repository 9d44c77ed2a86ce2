// launch.h -- the host half of the kernel files (kernels.hip, sched.hip, ll.hip): how a launcher turns its run-time dtype,
// operator, source count and cache policy into ONE kernel instantiation.  The only ladder over the dtypes and the only one over
// the operators live here; a launcher nests the helpers and names its kernel in the innermost lambda:
//
//   return with_dtype(dtype, [&](auto t) {
//     using T = typename decltype(t)::type;
//     return with_op<T>(op, [&](auto o) {
//       XMPI_LAUNCH((some_kernel<T, decltype(o)::value>), grid, dim3(kBlock), s, es, ee, args);
//       return hipGetLastError();
//     });
//   });
//
// Only what a lambda names is instantiated: where a combination must not exist, `if constexpr` on the tag keeps it out.
// Host code only.  Include it AFTER kdev.h and kernels.h (DT_*, OP_*, bf16_t, get_kernel_mode): it names neither, so that a
// kernel file built from a copy of itself beside an edited kdev.h (tests/devsim's mutants) sees that one kdev.h and no second.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <type_traits>

// plain launch, or a launch that carries its own begin / end events.  `kern` is the kernel's own name, spelled at the launch
// site (never a pointer handed down: tests/devsim tells the kernels apart by this text)
#define XMPI_LAUNCH(kern, grid, block, stream, es, ee, ...)                                  \
  do {                                                                                       \
    if ((es) || (ee)) hipExtLaunchKernelGGL(kern, grid, block, 0, stream, es, ee, 0, __VA_ARGS__); \
    else hipLaunchKernelGGL(kern, grid, block, 0, stream, __VA_ARGS__);                      \
  } while (0)

namespace xmpi {
namespace {

// nothing to launch: still honour the events
inline void record_events(hipEvent_t es, hipEvent_t ee, hipStream_t s) {
  if (es) (void)hipEventRecord(es, s);
  if (ee) (void)hipEventRecord(ee, s);
}

// cache policy of a streaming launch: the forced one (set_kernel_mode), else by size
inline int kernel_mode_for(size_t traffic_bytes) {
  if (get_kernel_mode() >= 0) return get_kernel_mode();
  // a launch whose traffic exceeds what the caches can hold streams through them: keep its loads
  // from displacing anything (nt); small launches are served from L2 / Infinity Cache as they are
  return traffic_bytes >= (size_t)(48u << 20) ? 2 : 0;
}

// grid cap (set_grid_cap) 0 = one tile per block, the hardware dispatcher balances (measured better than a 2048-block
// grid-stride loop inside the collective: reduce_n 60 -> 56 us per 288 MiB); > 0 caps the grid
inline int grid_for(size_t work_items, size_t per_block) {
  size_t g = (work_items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (get_grid_cap() > 0 && g > (size_t)get_grid_cap()) g = (size_t)get_grid_cap();
  if (g > 0x7fffffffu) g = 0x7fffffffu;
  return (int)g;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- run-time value -> compile-time tag ------------------------------------------------------------------------------
// Each calls `f` with a tag for the value it was given and returns what `f` returns (a hipError_t).

template <typename T>
struct type_tag {
  using type = T;
};
template <int V>
using int_tag = std::integral_constant<int, V>;

template <typename F>
hipError_t with_dtype(int dtype, F&& f) {
  switch (dtype) {
    case DT_U8: return f(type_tag<uint8_t>{});
    case DT_I32: return f(type_tag<int32_t>{});
    case DT_I64: return f(type_tag<int64_t>{});
    case DT_F16: return f(type_tag<_Float16>{});
    case DT_F32: return f(type_tag<float>{});
    case DT_F64: return f(type_tag<double>{});
    case DT_BF16: return f(type_tag<bf16_t>{});
    case DT_F8E4M3: return f(type_tag<f8e4m3_t>{});
    case DT_F8E5M2: return f(type_tag<f8e5m2_t>{});
    default: return hipErrorInvalidValue;
  }
}

// The operators of every kernel that has one: the four arithmetic ones for every T, and the three bitwise ones for the integer
// types -- for any other T they answer hipErrorInvalidValue and nothing is instantiated (kdev.h would refuse to compile it).
// The two 8-bit float types exist in the fold family only (with_fold_op): a launcher of anything else -- the stepped kernels,
// reduce2* -- keeps them out with `if constexpr (kF8Elem<T>)` in front of this, so nothing of theirs is instantiated for them.
template <typename T, typename F>
hipError_t with_op(int op, F&& f) {
  switch (op) {
    case OP_SUM: return f(int_tag<OP_SUM>{});
    case OP_PROD: return f(int_tag<OP_PROD>{});
    case OP_MIN: return f(int_tag<OP_MIN>{});
    case OP_MAX: return f(int_tag<OP_MAX>{});
    case OP_BAND:
      if constexpr (kIntegerElem<T>) return f(int_tag<OP_BAND>{});
      else return hipErrorInvalidValue;
    case OP_BOR:
      if constexpr (kIntegerElem<T>) return f(int_tag<OP_BOR>{});
      else return hipErrorInvalidValue;
    case OP_BXOR:
      if constexpr (kIntegerElem<T>) return f(int_tag<OP_BXOR>{});
      else return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
  }
}

// The fold family's operators (kernels whose lane sees every contribution to an element: reduce_n*, dsync_fold, dsync_body, the LL
// folds): those of with_op and OP_SUM_WIDE -- handed through for the two 16-bit and the two 8-bit float types, OP_SUM for every
// other T, whose sum it is.  A launcher of anything else (the stepped kernels, reduce2*) keeps to with_op and answers hipErrorInvalidValue.
template <typename T, typename F>
hipError_t with_fold_op(int op, F&& f) {
  if (op != OP_SUM_WIDE) return with_op<T>(op, f);
  if constexpr (std::is_same_v<T, _Float16> || std::is_same_v<T, bf16_t> || kF8Elem<T>) return f(int_tag<OP_SUM_WIDE>{});
  else return f(int_tag<OP_SUM>{});
}

// `v` as a constant if it is one of Vs, else the constant 0 (a kernel's runtime-count / plain instantiation)
template <int... Vs, typename F>
hipError_t with_int(int v, F&& f) {
  hipError_t e = hipSuccess;
  if (((v == Vs ? (e = f(int_tag<Vs>{}), true) : false) || ...)) return e;
  return f(int_tag<0>{});
}

// the cache policies a kernel is compiled for: all of 0 / 1 / 2, or 0 / 2 only (a forced 1 then runs as 2)
template <typename F>
hipError_t with_mode012(int mode, F&& f) {
  return with_int<1, 2>(mode, f);
}
template <typename F>
hipError_t with_mode02(int mode, F&& f) {
  return with_int<2>(mode != 0 ? 2 : 0, f);
}

// a source count unrolled for NS among Vs under the policies 0 / 2, and the runtime-count kernel <0, 0> for any other count
template <int... Vs, typename F>
hipError_t with_nsrc_mode(int nsrc, int mode, F&& f) {
  return with_int<Vs...>(nsrc, [&](auto ns) {
    if constexpr (decltype(ns)::value == 0) return f(ns, int_tag<0>{});
    else return with_mode02(mode, [&](auto m) { return f(ns, m); });
  });
}

}  // namespace
}  // namespace xmpi
