// device_io_check.hpp -- host-only argument checks of gmg_solve_device (include/gravomg_hip.h): no HIP, no engine state, so that a small
// stand-alone program can run them under a sanitizer (tests/test_device_io_host.py builds one).
#pragma once

#include <stdint.h>

#include "../../include/gravomg_hip.h"

namespace gmg {

// Elements between the first and the last element of an n x d block with these strides (>= 0), i.e. the block occupies ptr[0 .. extent].
// false: a negative stride, or the extent does not fit 63 bits.
inline bool strided_extent(int64_t n, int64_t d, int64_t row_stride, int64_t col_stride, int64_t* extent) {
    if (n < 1 || d < 1 || row_stride < 0 || col_stride < 0) return false;
    int64_t a = 0, b = 0, e = 0;
    if (__builtin_mul_overflow(n - 1, row_stride, &a) || __builtin_mul_overflow(d - 1, col_stride, &b) || __builtin_add_overflow(a, b, &e)) return false;
    if (e > INT64_MAX / 8 - 1) return false;          // (byte offsets are formed from it)
    *extent = e;
    return true;
}

// What is wrong with the shape of a gmg_solve_device call, or nullptr.  n: rows of the system.  Looks at no memory behind the pointers.
inline const char* device_vectors_fault(const gmg_device_vectors* v, int64_t n, int d) {
    if (!v) return "gmg_solve_device: v is NULL";
    if (!v->rhs || !v->x) return "gmg_solve_device: rhs and x must not be NULL";
    if (d <= 0) return "gmg_solve_device: d must be positive";
    if (v->rhs_row_stride == 0 || v->x_row_stride == 0 || (v->x0 && v->x0_row_stride == 0)) return "gmg_solve_device: a row stride is zero";
    int64_t e;
    if (!strided_extent(n, d, v->rhs_row_stride, v->rhs_col_stride, &e) || !strided_extent(n, d, v->x_row_stride, v->x_col_stride, &e) ||
        (v->x0 && !strided_extent(n, d, v->x0_row_stride, v->x0_col_stride, &e)))
        return "gmg_solve_device: strides must be non-negative and the block must be addressable with 64-bit offsets";
    if (d > 1 && v->x_col_stride == 0) return "gmg_solve_device: the columns of x overlap (column stride zero)";
    return nullptr;
}

}  // namespace gmg
