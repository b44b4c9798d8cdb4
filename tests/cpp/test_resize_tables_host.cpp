// The weight-pair bound k_pyr_resize's vertical stage rests on, asserted on the
// planner's own tables (csrc/orb_resize_tables.h; plain host C++, no GPU):
// every (w0, w1) of every alpha and beta table sums to at most 2049, and with
// the largest pairs found the scaled vertical sum of an all-255 image stays
// below 2^32, so its top byte is the result.
// Usage: test_resize_tables_host W H scaleFactor nlevels [W H scaleFactor nlevels ...]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "orb_resize_tables.h"

static uint32_t pair_max(const std::vector<int32_t>& t) {
  uint32_t m = 0;
  for (int32_t v : t) m = std::max(m, ((uint32_t)v & 0xFFFFu) + ((uint32_t)v >> 16));
  return m;
}

int main(int argc, char** argv) {
  if (argc < 5 || (argc - 1) % 4) return 2;
  int levels = 0;
  uint32_t worst = 0;
  for (int a = 1; a + 3 < argc; a += 4) {
    const int W = atoi(argv[a]), H = atoi(argv[a + 1]), L = atoi(argv[a + 3]);
    const double sf = atof(argv[a + 2]);
    // level sizes as the extractor derives them (runtime.cpp: compute_tables, build_plan)
    float scale = 1.0f;
    int pw = W, ph = H;
    for (int l = 1; l < L; ++l) {
      scale = (float)((double)scale * sf);
      const float inv = 1.0f / scale;
      const int w = cvRoundF((float)W * inv), h = cvRoundF((float)H * inv);
      std::vector<int32_t> xo(w), al(w), yo(h), be(h);
      orb_resize_table_x(w, pw, xo.data(), al.data());
      orb_resize_table_y(h, ph, yo.data(), be.data());
      const uint32_t ma = pair_max(al), mb = pair_max(be);
      if (!orb_resize_weights_bounded(al.data(), w) || !orb_resize_weights_bounded(be.data(), h) ||
          ma > ORB_RESIZE_PAIR_MAX || mb > ORB_RESIZE_PAIR_MAX) {
        printf("FAIL %dx%d sf %g level %d (%dx%d from %dx%d): pair sums alpha %u beta %u > %d\n", W,
               H, sf, l, w, h, pw, ph, ma, mb, ORB_RESIZE_PAIR_MAX);
        return 1;
      }
      // what the kernel computes for an all-255 source under the largest pairs
      const unsigned long long s4 = 4ull * (255ull * ma * mb + (1ull << 21));
      if (s4 >> 32) {
        printf("FAIL %dx%d sf %g level %d: 4 s = %llu\n", W, H, sf, l, s4);
        return 1;
      }
      worst = std::max(worst, std::max(ma, mb));
      pw = w;
      ph = h;
      ++levels;
    }
  }
  printf("OK %d levels, largest pair sum %u\n", levels, worst);
  return 0;
}
