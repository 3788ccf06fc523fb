// fl_ranged_math.h -- float square root, reciprocal and division for arguments of a STATED range (device code).
//
// hipcc's sqrtf(x), 1.0f / s and n / d are correctly rounded for every float: around the hardware estimate (v_sqrt_f32,
// v_rcp_f32) and its refinement they scale arguments near the ends of the exponent range (an input below 2^-96 by 2^32,
// v_div_scale_f32), pass zero, infinity and NaN through (v_cmp_class_f32, v_div_fixup_f32) and undo the scaling
// (v_div_fmas_f32).  The quantisers of fl_frontend.hip never hold such a value.  The functions below are the compiler's own
// refinement steps with every scale factor 1 and no special value looked for: on their domain they round correctly, so they
// give the bits of the compiler's operation (tests/test_gpu_ranged_math.py walks every float of each domain against it), and
// outside it they are simply not to be called.  The fused steps are explicit fmaf: the file is built with -ffp-contract=off.
#ifndef FL_RANGED_MATH_H
#define FL_RANGED_MATH_H

// sqrt(x), correctly rounded, for 2^-96 <= x <= FLT_MAX (finite, normal, positive).
// v_sqrt_f32 is within 1 ulp: the result is the estimate y or one of its neighbours.  The residual x - y- * y <= 0 says the
// root lies below y, x - y+ * y > 0 that it lies above.  (k_depth_quantize: x is a sum of squares of integers and > 0, so
// 1 <= x < 2^81.)
__device__ __forceinline__ float sqrt_rn(float x)
{
  const float y = __builtin_amdgcn_sqrtf(x);
  const float y_dn = __builtin_bit_cast(float, __builtin_bit_cast(int, y) - 1), y_up = __builtin_bit_cast(float, __builtin_bit_cast(int, y) + 1);
  const float r_dn = __builtin_fmaf(-y_dn, y, x), r_up = __builtin_fmaf(-y_up, y, x);
  float r = r_dn <= 0.0f ? y_dn : y;
  r = r_up > 0.0f ? y_up : r;
  return r;
}

// n / d, correctly rounded, for the operands of k_color_quantize's arctangent: n <= m are the smaller and the larger of |dx|
// and |dy| of one channel's Sobel sums, integers in 0 .. 1020 (a sum is (a0 - b0) + 2 (a1 - b1) + (a2 - b2) of bytes: at most
// 4 * 255), and d = (float)m + (float)DBL_EPSILON, which is m for m >= 1 and 2^-52 for m == 0, where n == 0 too.  So the
// domain is: n == 0 with d == 2^-52 or an integer 1 .. 1020, or integers 1 <= n <= d <= 1020.
// There v_div_scale_f32 scales nothing (d and 1 / d are normal, the quotient is 0 or in [2^-10, 1], n is 0 or >= 1) and
// v_div_fixup_f32 replaces nothing.  One Newton step on the reciprocal estimate, then the quotient and two residual
// corrections of it.
__device__ __forceinline__ float div_rn(float n, float d)
{
  const float r0 = __builtin_amdgcn_rcpf(d);
  const float r = __builtin_fmaf(__builtin_fmaf(-d, r0, 1.0f), r0, r0);
  const float q0 = n * r;
  const float q1 = __builtin_fmaf(__builtin_fmaf(-d, q0, n), r, q0);
  return __builtin_fmaf(__builtin_fmaf(-d, q1, n), r, q1);
}

// 1 / s, correctly rounded, for 1 <= s <= 2^64: div_rn(1, s), whose first product is the refined reciprocal itself.
// (k_depth_quantize: s is sqrt_rn of the sum above, 1 <= s < 2^41.)
__device__ __forceinline__ float rcp_rn(float s)
{
  const float r0 = __builtin_amdgcn_rcpf(s);
  const float r = __builtin_fmaf(__builtin_fmaf(-s, r0, 1.0f), r0, r0);
  const float q1 = __builtin_fmaf(__builtin_fmaf(-s, r, 1.0f), r, r);
  return __builtin_fmaf(__builtin_fmaf(-s, q1, 1.0f), r, q1);
}

#endif
