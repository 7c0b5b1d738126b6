/* yrt_sse_rcp.h — the reference's approximate reciprocals, bit for bit.
 *
 * The reference computes every rcp()/rsqrt() of its render path with the SSE estimate
 * instructions plus one Newton step (common/math/math.h:38-59; vector3f_sse.h:135-144 and
 * color_sse.h:142-149 per lane; color_sse.h:161-162 turns Color / float into a * rcp(b)):
 *
 *   rcp(x)   = (r + r) - (r * r) * x                     r = rcpps(x)
 *   rsqrt(x) = 1.5f * r + ((x * -0.5f) * r) * (r * r)    r = rsqrtps(x)
 *
 * (the reference build is x64 MSVC with SSE4.1 and no FMA, so each operation rounds).
 *
 * rcpps / rsqrtps are table lookups whose contents Intel does not document and AMD implements
 * differently. On Intel they are (measured on every input of this container's Xeon,
 * tests/golden/make_sse_tables.py -> tests/golden/sse_rcp_tables.json):
 *   rcpps(x)   = sign * 2^-(E+1) * (1 + m/4096),  m = RN(4096 * (2/mid - 1)),
 *                mid = 1 + (i + 1/2)/2048, i = the top 11 bits of x's mantissa;
 *   rsqrtps(x) = 2^-(k+1) * (1 + m/4096),          m = RN(4096 * (2/sqrt(mid) - 1)),
 *                E = 2k + p, mid = (1 + (j + 1/2)/1024) * 2^p, j = the top 10 mantissa bits
 * — the 12-bit round-to-nearest reciprocal (square root) of the midpoint of the input's
 * 11-bit (10-bit + exponent parity) interval, with no ties (|m - exact| <= 0.49994). Zero
 * and subnormal inputs give +-inf, results below 2^-126 flush to zero, rsqrtps of a negative
 * number is the default NaN.
 *
 * Both are computed here exactly, so the GPU and the host produce the same bits and neither
 * depends on the CPU vendor.
 *
 * Host (IEEE division and square root, correctly rounded):
 *   rcp:   RN(1/mid) in float, rounded to 12 bits, with the one entry where that double rounding
 *          differs corrected (see yrt_rcpps);
 *   rsqrt: RN(1 / RN(sqrt(mid))) in float, rounded to 12 bits: equal to the direct rounding on
 *          every entry (the closest call is 9e-5 of a unit from a tie).
 *
 * Device (gfx950): the hardware estimates v_rcp_f32 / v_rsq_f32 (within 1 ulp) taken directly at a
 * representative of the input's interval, its top mantissa bits with fixed low bits, so that the
 * instruction itself does the sign, the exponent, zero and subnormal inputs (flushed: +-inf),
 * huge inputs (a subnormal result, flushed: +-0), inf and NaN, and no select chain is left:
 *   rcpps:   v_rcp_f32 at low bits 0x7ff, the result rounded to 12 bits by adding 0x3ff and
 *            masking. At the midpoint 0x800 with the half unit 0x400, v_rcp_f32 gives the table on
 *            2047 entries and crosses the tie of entry 1984 as RN(1/mid) does; one ulp below the
 *            midpoint with ties broken downwards it gives all 2048 (the only such pair among the
 *            low bits 0 .. 0xfff and the addends 0x3f0 .. 0x410, enumerated on the GPU);
 *   rsqrtps: v_rsq_f32 at the midpoint 0x1000 of the 10-bit interval, rounded by adding 0x400
 *            and masking: the table on all 2048 entries.
 * An inf or NaN input (and for rsqrtps a negative one) goes through the instruction unchanged,
 * and its result is kept as it comes: the 12-bit rounding would disturb a NaN's payload, the
 * low bits would turn an inf into a NaN. v_rsq_f32's NaN of a negative input gets the input's
 * sign (the SSE default NaN is negative). These constants describe gfx950's estimate tables and
 * hold by the exhaustive checks alone: the GPU against the committed Intel tables over all 2^32
 * inputs (yrtDebugCheckMathTable, tests/test_gpu_parity.py) and on the special inputs
 * (tests/test_sse_rcp_special.py); the host against rcpps/rsqrtps themselves over all 2^32
 * inputs (tests/test_ref_pin.py, Intel hosts).
 *
 * C and HIP compatible (the oracle is C11).
 */
#ifndef YRT_SSE_RCP_H
#define YRT_SSE_RCP_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define YRT_SSE_FN __host__ __device__ static inline
#else
#define YRT_SSE_FN static inline
#endif

YRT_SSE_FN uint32_t yrt_sse_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
YRT_SSE_FN float yrt_sse_float(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

#if defined(__HIP_DEVICE_COMPILE__)

/* v_cmp_class_f32 masks: signalling and quiet NaN, -inf, +inf; negative normal */
#define YRT_SSE_CLASS_NAN_INF 0x207
#define YRT_SSE_CLASS_NEG_NORMAL 0x008

/* Intel rcpps (one lane) from v_rcp_f32, see above: 10 VALU (the estimate counts 4), no branch */
YRT_SSE_FN float yrt_rcpps(float x) {
  const uint32_t u = yrt_sse_bits(x);
  const bool pass = __builtin_amdgcn_classf(x, YRT_SSE_CLASS_NAN_INF);
  const uint32_t in = pass ? u : ((u & 0xfffff000u) | 0x7ffu);
  const uint32_t r = yrt_sse_bits(__builtin_amdgcn_rcpf(yrt_sse_float(in)));
  return yrt_sse_float(pass ? r : ((r + 0x3ffu) & 0xfffff800u));
}
/* Intel rsqrtps (one lane) from v_rsq_f32, see above */
YRT_SSE_FN float yrt_rsqrtps(float x) {
  const uint32_t u = yrt_sse_bits(x);
  const bool pass = __builtin_amdgcn_classf(x, YRT_SSE_CLASS_NAN_INF | YRT_SSE_CLASS_NEG_NORMAL);
  const uint32_t in = pass ? u : ((u & 0xffffe000u) | 0x1000u);
  const uint32_t r = yrt_sse_bits(__builtin_amdgcn_rsqf(yrt_sse_float(in)));
  return yrt_sse_float(pass ? (r | (u & 0x80000000u)) : ((r + 0x400u) & 0xfffff800u));
}

#else

/* Intel rcpps (one lane): RN(1/mid) rounded to 12 mantissa bits. mid = the input's top 11
 * mantissa bits + a half unit, exponent 0; 1/mid lies in (0.5, 1), so the 12-bit rounding is an
 * add of half a unit and a mask on its bits. That double rounding (24 then 12 bits) matches the
 * direct one on 2047 of the 2048 entries; entry 1984 rounds up across the tie-free midpoint and is
 * corrected (tests/test_sse_rcp.py, ref_check_sse_exhaustive). */
YRT_SSE_FN float yrt_rcpps(float x) {
  const uint32_t u = yrt_sse_bits(x), s = u & 0x80000000u, e = (u >> 23) & 0xffu;
  const uint32_t mid = (u & 0x7ff000u) | 0x3f800800u;
  uint32_t y = yrt_sse_bits(1.0f / yrt_sse_float(mid));             /* exponent 126 */
  y = (y + 0x400u) & 0x7ff800u;
  y -= (mid == 0x3ffc0800u) ? 0x800u : 0u;                            /* entry 1984 */
  uint32_t out = s | ((253u - e) << 23) | y;                          /* e in [1, 252] */
  if (e >= 253u) out = s;                                             /* below 2^-126: +-0 */
  if (e == 255u) out = (u & 0x7fffffu) ? (u | 0x400000u) : s;         /* NaN stays (quiet), inf -> 0 */
  if (e == 0u) out = s | 0x7f800000u;                                 /* +-0, subnormal -> +-inf */
  return yrt_sse_float(out);
}

/* Intel rsqrtps (one lane): RN(1 / RN(sqrt(mid))) rounded to 12 mantissa bits, mid = the input's
 * top 10 mantissa bits + a half unit, times 2^p (exponent parity); that double rounding matches
 * the direct one on all 2048 entries (tests/test_sse_rcp.py, exhaustive checks). */
YRT_SSE_FN float yrt_rsqrtps(float x) {
  const uint32_t u = yrt_sse_bits(x), e = (u >> 23) & 0xffu;
  const int E = (int)e - 127, p = E & 1, k = (E - p) / 2;
  const uint32_t mid = ((uint32_t)(127 + p) << 23) | (u & 0x7fe000u) | 0x1000u;
  const uint32_t y = (yrt_sse_bits(1.0f / __builtin_sqrtf(yrt_sse_float(mid))) + 0x400u) & 0x7ff800u;
  uint32_t out = ((uint32_t)(126 - k) << 23) | y;                     /* positive, e in [1, 254] */
  if (u & 0x80000000u) out = 0xffc00000u;                             /* negative: default NaN */
  if (e == 255u) out = (u & 0x7fffffu) ? (u | 0x400000u) : ((u & 0x80000000u) ? 0xffc00000u : 0u);
  if (e == 0u) out = (u & 0x80000000u) | 0x7f800000u;                 /* +-0, subnormal -> +-inf */
  return yrt_sse_float(out);
}

#endif

/* common/math/math.h:38-42 */
YRT_SSE_FN float yrt_ref_rcp(float x) {
  const float r = yrt_rcpps(x);
  return (r + r) - (r * r) * x;
}
/* common/math/math.h:53-58 */
YRT_SSE_FN float yrt_ref_rsqrt(float x) {
  const float r = yrt_rsqrtps(x);
  return 1.5f * r + ((x * -0.5f) * r) * (r * r);
}

#endif
