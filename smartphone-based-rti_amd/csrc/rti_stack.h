// rti_stack.h -- the argument contract of the entry points that read a light-major stack and / or write
// coefficients (include/rti.h): the two views, their checks and the vector-path predicates, in one place.
//
// Every check takes the entry point's name, records "<entry>: ..." through fail() and returns its status
// (RTI_OK = 0 when the arguments pass), so an entry reads `if (int st = check_...(E, ...)) return st;` in the
// order it documents.  Nothing here allocates, synchronises or calls HIP.
#pragma once

#include <initializer_list>

#include "rti_internal.h"

namespace rti {

// I[c][n][p]: C channels of N light planes (a chunk's B) of P elements, strides in elements and resolved
struct StackView {
  const void* I;
  int in_dtype;
  size_t es;  // bytes per element
  int N;
  int64_t P;
  int C;
  int64_t lstride, cstride;
};

// coef[c][p][i] (RTI_COEF_PIXEL_MAJOR) or coef[c][i][p] (RTI_COEF_PLANAR), i < k; channel stride resolved.
// F = float where the entry writes coefficients, const float where it reads them (rti_fit_residual).
template <typename F>
struct CoefViewT {
  F* coef;
  int layout, k;
  int64_t ocstride;
};
using CoefView = CoefViewT<float>;
using CoefSource = CoefViewT<const float>;

// 0 strides mean dense: planes of P elements, channels of N planes
inline StackView stack_view(const void* I, int in_dtype, int N, int64_t P, int C, int64_t light_stride,
                            int64_t channel_stride) {
  const int64_t ls = light_stride ? light_stride : P;
  return {I, in_dtype, in_dtype == RTI_U8 ? (size_t)1 : (size_t)4, N, P, C, ls, channel_stride ? channel_stride : (int64_t)N * ls};
}

template <typename F>
inline CoefViewT<F> coef_view(F* coef, int layout, int k, int64_t P, int64_t coef_channel_stride) {
  return {coef, layout, k, coef_channel_stride ? coef_channel_stride : P * k};
}

// ---- checks ---------------------------------------------------------------------------------------------------
inline int check_pointers(const char* entry, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (!p) return fail(RTI_ERR_BAD_ARG, "%s: null pointer", entry);
  return RTI_OK;
}

// n planes (lights or a chunk's B), P pixels, C channels (a grid's y extent);
// `names` is how the entry spells them, e.g. "N/P/C"
inline bool extents_ok(int64_t n, int64_t P, int C) { return n > 0 && P > 0 && C > 0 && C <= 65535; }
inline int check_extents(const char* entry, const char* names, int64_t n, int64_t P, int C) {
  if (!extents_ok(n, P, C)) return fail(RTI_ERR_BAD_ARG, "%s: bad %s", entry, names);
  return RTI_OK;
}

inline int check_lights(const char* entry, int N, int k) {
  if (N < k) return fail(RTI_ERR_BAD_ARG, "%s: N=%d < k=%d", entry, N, k);
  return RTI_OK;
}

inline int check_in_dtype(const char* entry, int in_dtype) {
  if (in_dtype != RTI_F32 && in_dtype != RTI_U8 && in_dtype != RTI_I32)
    return fail(RTI_ERR_UNSUPPORTED, "%s: input dtype %d", entry, in_dtype);
  return RTI_OK;
}

inline int check_coef_layout(const char* entry, int layout) {
  if (layout != RTI_COEF_PIXEL_MAJOR && layout != RTI_COEF_PLANAR)
    return fail(RTI_ERR_BAD_ARG, "%s: coef layout %d", entry, layout);
  return RTI_OK;
}

// a single channel never uses its channel stride, so any value passes
inline int check_stack_strides(const char* entry, const StackView& s) {
  if (s.lstride < s.P) return fail(RTI_ERR_BAD_ARG, "%s: light_stride < P", entry);
  if (s.C > 1 && s.cstride < (int64_t)s.N * s.lstride) return fail(RTI_ERR_BAD_ARG, "%s: channel_stride", entry);
  return RTI_OK;
}

template <typename F>
inline int check_coef_stride(const char* entry, const CoefViewT<F>& o, int64_t P, int C) {
  if (C > 1 && o.ocstride < P * o.k) return fail(RTI_ERR_BAD_ARG, "%s: coef_channel_stride", entry);
  return RTI_OK;
}

// f(T{}) with T the stack's element type (after check_in_dtype): f is a generic lambda that calls a launcher
// template with decltype of its argument
template <typename F>
inline auto with_in_dtype(int in_dtype, F&& f) {
  switch (in_dtype) {
    case RTI_F32: return f(float{});
    case RTI_I32: return f(int32_t{});
    default: return f(uint8_t{});
  }
}

// ---- vector-path predicates -----------------------------------------------------------------------------------
// Which kernel instantiation a call gets hangs on these, so each family keeps the rule it shipped with.  The two
// families differ only at C == 1 with an explicit channel stride that is no multiple of the vector: the `_any_c`
// rules (fit, fit + residual, residual, q8, h16, apply_operator) then fall back to one element per lane although
// no kernel reads that stride; the `_used` rules (accumulate, solve) ignore a stride that is not used.

// lanes of `vec` consecutive stack elements (16 bytes for vec = 4 of fp32 / int32, vec = 16 of u8)
inline bool stack_vec_ok_any_c(const StackView& s, int vec) {
  return s.P % vec == 0 && s.lstride % vec == 0 && s.cstride % vec == 0 && aligned_to(s.I, vec * s.es);
}
inline bool stack_vec_ok_used(const StackView& s, int vec) {
  return s.P % vec == 0 && s.lstride % vec == 0 && (s.C == 1 || s.cstride % vec == 0) && aligned_to(s.I, vec * s.es);
}

// 16-byte stores of coefficient rows or planes
template <typename F>
inline bool coef_vec_ok_any_c(const CoefViewT<F>& o) { return aligned_to(o.coef, 16) && o.ocstride % 4 == 0; }
inline bool coef_vec_ok_used(const CoefView& o, int C) { return aligned_to(o.coef, 16) && (C == 1 || o.ocstride % 4 == 0); }

}  // namespace rti
