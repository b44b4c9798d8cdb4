// orb_resize_tables.h -- the fixed-point tables of one pyramid level's resize
// (cv::resize INTER_LINEAR on 8U), as the planner
// builds them and the k_pyr_resize kernels read them.  Plain host C++ with
// internal linkage, no HIP: the runtime and the host tests include it.
#ifndef ORB_RESIZE_TABLES_H
#define ORB_RESIZE_TABLES_H

#include <math.h>
#include <stdint.h>

#include <algorithm>

static inline int cvRoundF(float v) { return (int)lrintf(v); }
static inline short satShort(int v) { return (short)std::min(std::max(v, -32768), 32767); }

// Columns: xofs[dx] is the first source column of output column dx, alpha[dx]
// packs its two 11-bit weights as (w1 << 16) | (w0 & 0xFFFF).  Returns xmax,
// the first output column whose second tap lies past the source row.
static inline int orb_resize_table_x(int dw, int sw, int32_t* xofs, int32_t* alpha) {
  const double scale_x = 1. / ((double)dw / sw);
  int xmax = dw;
  for (int dx = 0; dx < dw; ++dx) {
    float fx = (float)((dx + 0.5) * scale_x - 0.5);
    int sx = (int)floorf(fx);
    fx -= sx;
    if (sx < 0) { fx = 0; sx = 0; }
    if (sx + 1 >= sw) {
      xmax = std::min(xmax, dx);
      if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
    }
    const short a0 = satShort(cvRoundF((1.f - fx) * 2048)), a1 = satShort(cvRoundF(fx * 2048));
    xofs[dx] = sx;
    alpha[dx] = (int32_t)(((uint32_t)(uint16_t)a1 << 16) | (uint16_t)a0);
  }
  return xmax;
}

// Rows: yofs[dy] unclamped (the kernels clamp both source rows), beta as alpha.
static inline void orb_resize_table_y(int dh, int sh, int32_t* yofs, int32_t* beta) {
  const double scale_y = 1. / ((double)dh / sh);
  for (int dy = 0; dy < dh; ++dy) {
    float fy = (float)((dy + 0.5) * scale_y - 0.5);
    int sy = (int)floorf(fy);
    fy -= sy;
    const short b0 = satShort(cvRoundF((1.f - fy) * 2048)), b1 = satShort(cvRoundF(fy * 2048));
    yofs[dy] = sy;
    beta[dy] = (int32_t)(((uint32_t)(uint16_t)b1 << 16) | (uint16_t)b0);
  }
}

// The bound the tiled kernels' vertical stage rests on: read as unsigned 16-bit
// fields, the two weights of every entry sum to at most 2049.
//
// Why the tables above meet it.  f (fx or fy) is a float in [0, 1]: x - floorf(x)
// rounded to float, or 0 where a column is clamped.  f * 2048 is exact (a power
// of two), and 1.f - f is rounded to float with an error of at most 2^-25 (half
// an ulp of a value <= 1), so u = (1.f - f) * 2048 and v = f * 2048 are both in
// [0, 2048] and u + v is within 2^-14 of 2048.  Rounding to nearest moves each by
// at most 1/2, so w0 + w1 <= 2048 + 2^-14 + 1, and being an integer, <= 2049
// (2049 is reachable: for f just above 2^-12, 1.f - f rounds to 1 - 2^-12 and
// the weights are 2048 + 1; so the bound is not 2048).
//
// What follows from it.  A horizontal sum h = w0 S0 + w1 S1 of two bytes is at
// most 255 * 2049 < 2^20, and the vertical sum s = h0 b0 + h1 b1 + 2^21 at most
// 255 * 2049 * 2049 + 2^21 = 1,072,689,407 < 2^30.  So (s >> 22) <= 255 without a
// clamp, 4 s fits 32 bits, and the result byte is the top byte of 4 s.
// The planner checks the tables themselves rather than trusting the argument:
// a level that fails goes to k_pyr_resize_generic, which assumes nothing.
#define ORB_RESIZE_PAIR_MAX 2049
static inline bool orb_resize_weights_bounded(const int32_t* wts, int n) {
  for (int i = 0; i < n; ++i) {
    const uint32_t w = (uint32_t)wts[i];
    if ((w & 0xFFFFu) + (w >> 16) > ORB_RESIZE_PAIR_MAX) return false;
  }
  return true;
}

#endif
