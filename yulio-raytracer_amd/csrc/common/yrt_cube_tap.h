// yrt_cube_tap.h — where a filter tap lands when it leaves a face of the stereo cube (DESIGN.md §9,
// "cube"): one integer rule shared by the cube form of k_atrous, the host's checks and
// yrtDebugCubeTap.
//
// Faces are W x W; pixel (x, y) of a face is the guides' pixel: its camera ray goes through
// ((x + .5) / W, (y + .5) / W). A tap (qx, qy) of face f (0..5 within its eye)
//   - with both coordinates in [0, W) stays on f;
//   - with both outside (the corner region) is skipped: its direction lies on the plane between
//     two neighbours and either choice would hang on rounding;
//   - with exactly one outside crosses edge e at depth k, lateral index j:
//         R  qx >= W   k = qx - W    j = qy          L  qx < 0   k = -1 - qx   j = qy
//         B  qy >= W   k = qy - W    j = qx          T  qy < 0   k = -1 - qy   j = qx
//     a = floor(W (2k + 1) / (2 (W + 2k + 1))),  b = floor(W (k + j + 1) / (W + 2k + 1)),
//     b := W - 1 - b where the table says "rev"; entered through edge e' of face g it lands on
//         L (a, b)    R (W - 1 - a, b)    T (b, a)    B (b, W - 1 - a).
// a and b are the floors of the exact rational images of the tap's direction on the ideal 90-degree
// cube (StereoCubeCamera hard-codes angle 90, aspect 1), so no float rounding enters; a < W / 2
// and b < W always.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define YRT_CUBE_HD __host__ __device__
#else
#define YRT_CUBE_HD
#endif

// The products stay inside 32 unsigned bits for W <= 16384 and taps within 2^17 pixels of the
// face (the filter's largest step is 2^15, two taps deep).
#define YRT_CUBE_MAX_WIDTH 16384
#define YRT_CUBE_MAX_REACH (1 << 17)

enum { YRT_CUBE_L = 0, YRT_CUBE_R = 1, YRT_CUBE_T = 2, YRT_CUBE_B = 3 };

// (f, e) -> (g, e', rev), fixed by how StereoCubeCamera rotates its six pixel2world frames (faces
// 1..3: face 0 turned about `up`; 4 / 5, up and down: turned about `right` and then by 180 degrees
// about `up`). One word per face, 6 bits per edge L, R, T, B: g | e' << 3 | rev << 5.
//
//   f |  L         R         T         B
//   0 |  3 R same  1 L same  4 T rev   5 B rev
//   1 |  0 R same  2 L same  4 L same  5 L rev
//   2 |  1 R same  3 L same  4 B same  5 T same
//   3 |  2 R same  0 L same  4 R rev   5 R same
//   4 |  1 T same  3 T rev   0 T rev   2 T same
//   5 |  1 B rev   3 B same  2 B same  0 B rev
#define YRT_CUBE_ENTRY(g, e, rev) ((uint32_t)((g) | (e) << 3 | (rev) << 5))
#define YRT_CUBE_ROW(l, r, t, b) ((l) | (r) << 6 | (t) << 12 | (b) << 18)
YRT_CUBE_HD inline uint32_t yrt_cube_neighbours(int face) {
  switch (face) {
    case 0:
      return YRT_CUBE_ROW(YRT_CUBE_ENTRY(3, YRT_CUBE_R, 0), YRT_CUBE_ENTRY(1, YRT_CUBE_L, 0),
                          YRT_CUBE_ENTRY(4, YRT_CUBE_T, 1), YRT_CUBE_ENTRY(5, YRT_CUBE_B, 1));
    case 1:
      return YRT_CUBE_ROW(YRT_CUBE_ENTRY(0, YRT_CUBE_R, 0), YRT_CUBE_ENTRY(2, YRT_CUBE_L, 0),
                          YRT_CUBE_ENTRY(4, YRT_CUBE_L, 0), YRT_CUBE_ENTRY(5, YRT_CUBE_L, 1));
    case 2:
      return YRT_CUBE_ROW(YRT_CUBE_ENTRY(1, YRT_CUBE_R, 0), YRT_CUBE_ENTRY(3, YRT_CUBE_L, 0),
                          YRT_CUBE_ENTRY(4, YRT_CUBE_B, 0), YRT_CUBE_ENTRY(5, YRT_CUBE_T, 0));
    case 3:
      return YRT_CUBE_ROW(YRT_CUBE_ENTRY(2, YRT_CUBE_R, 0), YRT_CUBE_ENTRY(0, YRT_CUBE_L, 0),
                          YRT_CUBE_ENTRY(4, YRT_CUBE_R, 1), YRT_CUBE_ENTRY(5, YRT_CUBE_R, 0));
    case 4:
      return YRT_CUBE_ROW(YRT_CUBE_ENTRY(1, YRT_CUBE_T, 0), YRT_CUBE_ENTRY(3, YRT_CUBE_T, 1),
                          YRT_CUBE_ENTRY(0, YRT_CUBE_T, 1), YRT_CUBE_ENTRY(2, YRT_CUBE_T, 0));
    default:
      return YRT_CUBE_ROW(YRT_CUBE_ENTRY(1, YRT_CUBE_B, 1), YRT_CUBE_ENTRY(3, YRT_CUBE_B, 0),
                          YRT_CUBE_ENTRY(2, YRT_CUBE_B, 0), YRT_CUBE_ENTRY(0, YRT_CUBE_B, 1));
  }
}
#undef YRT_CUBE_ROW
#undef YRT_CUBE_ENTRY

// The tap (qx, qy) of face `face` of a cube of W x W faces: 1 and the face and pixel it lands on,
// 0 for a skipped corner tap, -1 for arguments out of range (W outside 1..16384, face outside
// 0..5, a tap farther than 2^17 pixels from the face).
YRT_CUBE_HD inline int yrt_cube_tap(int W, int face, int qx, int qy, int* g, int* x, int* y) {
  if (W < 1 || W > YRT_CUBE_MAX_WIDTH || face < 0 || face > 5) return -1;
  if (qx < -YRT_CUBE_MAX_REACH || qy < -YRT_CUBE_MAX_REACH || qx >= W + YRT_CUBE_MAX_REACH ||
      qy >= W + YRT_CUBE_MAX_REACH)
    return -1;
  const bool outX = qx < 0 || qx >= W, outY = qy < 0 || qy >= W;
  if (!outX && !outY) {
    *g = face;
    *x = qx;
    *y = qy;
    return 1;
  }
  if (outX && outY) return 0;
  int e;
  uint32_t k, j;
  if (outX) {
    e = qx < 0 ? YRT_CUBE_L : YRT_CUBE_R;
    k = (uint32_t)(qx < 0 ? -1 - qx : qx - W);
    j = (uint32_t)qy;
  } else {
    e = qy < 0 ? YRT_CUBE_T : YRT_CUBE_B;
    k = (uint32_t)(qy < 0 ? -1 - qy : qy - W);
    j = (uint32_t)qx;
  }
  const uint32_t w = (uint32_t)W, n = w + 2u * k + 1u;
  const int a = (int)(w * (2u * k + 1u) / (2u * n));
  int b = (int)(w * (k + j + 1u) / n);
  const uint32_t t = yrt_cube_neighbours(face) >> (6 * e) & 63u;
  if (t & 32u) b = W - 1 - b;
  *g = (int)(t & 7u);
  switch (t >> 3 & 3u) {
    case YRT_CUBE_L:
      *x = a;
      *y = b;
      break;
    case YRT_CUBE_R:
      *x = W - 1 - a;
      *y = b;
      break;
    case YRT_CUBE_T:
      *x = b;
      *y = a;
      break;
    default:
      *x = b;
      *y = W - 1 - a;
      break;
  }
  return 1;
}
