// rti_dispatch.h -- how the entries that read fitted maps (include/rti.h) turn (layout, output type, normal layout)
// into a kernel instantiation, and the argument checks and vector-path predicates they share.  Host code only.
//
// A dispatcher calls f with a tag for a checked value: f is a generic lambda that launches the kernel instantiated
// on decltype of its argument (`decltype(l)::value` for a layout, `decltype(t)` for an output type).  A check takes
// the entry point's name, records "<entry>: ..." through fail() and returns its status, as rti_stack.h's do.
#pragma once

#include <type_traits>

#include "rti_stack.h"

namespace rti {

template <int V>
using Tag = std::integral_constant<int, V>;

// RTI_COEF_PLANAR or RTI_COEF_PIXEL_MAJOR (after check_coef_layout, or the entry's own check of an LRGB layout)
template <typename F>
inline void with_layout(int layout, F&& f) {
  if (layout == RTI_COEF_PLANAR)
    f(Tag<RTI_COEF_PLANAR>{});
  else
    f(Tag<RTI_COEF_PIXEL_MAJOR>{});
}

// RTI_NORMAL_PLANAR or RTI_NORMAL_PIXEL_MAJOR (after check_normal_layout)
template <typename F>
inline void with_normal_layout(int normal_layout, F&& f) {
  if (normal_layout == RTI_NORMAL_PLANAR)
    f(Tag<RTI_NORMAL_PLANAR>{});
  else
    f(Tag<RTI_NORMAL_PIXEL_MAJOR>{});
}

// the terms of an HSH basis, 9 or 16 (after the entry's check of the basis)
template <typename F>
inline void with_hsh_terms(int k, F&& f) {
  if (k == 9)
    f(Tag<9>{});
  else
    f(Tag<16>{});
}

// one map or three (after the entry's check of C)
template <typename F>
inline void with_channels(int C, F&& f) {
  if (C == 1)
    f(Tag<1>{});
  else
    f(Tag<3>{});
}

// f(TO{}) with TO the output type (after check_out_dtype)
template <typename F>
inline void with_out(int out_dtype, F&& f) {
  switch (out_dtype) {
    case RTI_F32: f(float{}); break;
    case RTI_I32: f(int32_t{}); break;
    default: f(uint8_t{}); break;
  }
}

// f(TC{}) with TC the coefficients' type, RTI_F32 or RTI_F64 (after the entry's check of coef_dtype)
template <typename F>
inline void with_coef_dtype(int coef_dtype, F&& f) {
  if (coef_dtype == RTI_F64)
    f(double{});
  else
    f(float{});
}

// ---- checks ---------------------------------------------------------------------------------------------------

inline int check_normal_layout(const char* entry, int normal_layout) {
  if (normal_layout != RTI_NORMAL_PIXEL_MAJOR && normal_layout != RTI_NORMAL_PLANAR)
    return fail(RTI_ERR_BAD_ARG, "%s: normal layout %d", entry, normal_layout);
  return RTI_OK;
}

inline int check_out_dtype(const char* entry, int out_dtype) {
  if (out_dtype != RTI_F32 && out_dtype != RTI_I32 && out_dtype != RTI_U8)
    return fail(RTI_ERR_UNSUPPORTED, "%s: out dtype %d", entry, out_dtype);
  return RTI_OK;
}

// the doubles of an 8-bit PTM's header
inline int check_qparams_aligned(const char* entry, const double* qparams) {
  if (!aligned_to(qparams, 8)) return fail(RTI_ERR_BAD_ARG, "%s: qparams must be 8-byte aligned", entry);
  return RTI_OK;
}

// the layout and the channel stride of three maps of k terms, in the order include/rti.h lists them
inline int check_rgb_maps(const char* entry, int k, int layout, int64_t stride, int64_t P) {
  if (int st = check_coef_layout(entry, layout)) return st;
  return check_coef_stride(entry, coef_view(static_cast<const float*>(nullptr), layout, k, P, stride), P, 3);
}

// ---- vector-path predicates of the four-pixels-per-lane kernels (rti_lane4.h) -----------------------------------

// 16-byte loads of three maps cs elements apart: every wave's rows (or plane pieces) of every channel start on a
// 16-byte boundary
inline bool maps_vec(const float* coef, int64_t cs, int64_t P) {
  return P % 4 == 0 && aligned_to(coef, 16) && cs % 4 == 0;
}

// a lane's four outputs, or the wave's RGB rows: whole dwords of uint8, 16-byte pieces of fp32 / int32
inline bool rgb_out_vec(const void* out, int out_dtype) { return aligned_to(out, out_dtype == RTI_U8 ? 4 : 16); }

// rti_ptm_normals' three outputs: 16-byte pieces of normals and peak, a lane's dword of kind
inline bool normals_out_vec(const float* normals, const uint8_t* kind, const float* peak) {
  return aligned_to(normals, 16) && (!kind || aligned_to(kind, 4)) && (!peak || aligned_to(peak, 16));
}

}  // namespace rti
