// The FAST cell class table (csrc/orb_plan.h; plain host C++, no GPU): for
// every cell of a plan, the class entry the planner files it under must equal
// what k_fast_cells used to derive per cell -- the float-reciprocal formulas,
// restated below as they stood -- for every lane, every tile byte and every
// window pixel the kernel divides; and the quotient multipliers must be exact
// over the whole ranges orb_cell_class_ok claims.
// Usage: test_cell_classes_host W H scaleFactor nlevels [W H scaleFactor nlevels ...]
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "orb_plan.h"
#include "orb_resize_tables.h"  // cvRoundF

#define CHECK(c, ...)                 \
  do {                                \
    if (!(c)) {                       \
      printf("FAIL " __VA_ARGS__);    \
      printf(" [%s]\n", #c);          \
      return 1;                       \
    }                                 \
  } while (0)

// the old per-cell quotient: (int)((x + 0.5) * (1 / d)), in float
static int fquot(int x, int d) { return (int)(((float)x + 0.5f) * (1.0f / (float)d)); }

static int check_plan(int W, int H, double sf, int L, int* ncellsOut, int* nclsOut) {
  OrbPlanDesc P;
  memset(&P, 0, sizeof(P));
  P.nlevels = L;
  std::vector<OrbCellDesc> cells;
  float scale = 1.0f;
  long long arena = 0;
  for (int l = 0; l < L; ++l) {
    OrbLevelDesc& d = P.lv[l];
    if (l) scale = (float)((double)scale * sf);
    const float inv = 1.0f / scale;
    d.w = l ? cvRoundF((float)W * inv) : W;
    d.h = l ? cvRoundF((float)H * inv) : H;
    CHECK(d.w >= 33 && d.h >= 33, "%dx%d sf %g: level %d is %dx%d", W, H, sf, l, d.w, d.h);
    d.pitch = ((d.w + 127) & ~127) | 128;
    d.arenaOff = l ? arena : 0;
    if (l) arena += (long long)d.pitch * d.h;
    // the FAST cell grid of the reference (src/ORBextractor.cc:797-839)
    const int minBX = 16, minBY = 16, maxBX = d.w - 16, maxBY = d.h - 16;
    const float width = (float)(maxBX - minBX), height = (float)(maxBY - minBY);
    const int nCols = (int)(width / 30.f), nRows = (int)(height / 30.f);
    const int wCell = nCols > 0 ? (int)ceilf(width / nCols) : 0;
    const int hCell = nRows > 0 ? (int)ceilf(height / nRows) : 0;
    d.cellBeg = (int)cells.size();
    for (int i = 0; i < nRows && nCols > 0; ++i) {
      const float iniY = (float)(minBY + i * hCell);
      float maxY = iniY + hCell + 6;
      if (iniY >= maxBY - 3) continue;
      if (maxY > maxBY) maxY = (float)maxBY;
      for (int j = 0; j < nCols; ++j) {
        const float iniX = (float)(minBX + j * wCell);
        float maxX = iniX + wCell + 6;
        if (iniX >= maxBX - 6) continue;
        if (maxX > maxBX) maxX = (float)maxBX;
        OrbCellDesc c;
        c.level = (int16_t)l;
        c.y0 = (int16_t)(int)iniY;
        c.y1 = (int16_t)(int)maxY;
        c.x0 = (int16_t)(int)iniX;
        c.x1 = (int16_t)(int)maxX;
        c.cls = -1;
        cells.push_back(c);
      }
    }
    d.cellEnd = (int)cells.size();
  }
  P.ncells = (int)cells.size();
  std::vector<OrbCellClass> cls(ORB_MAX_CELL_CLASSES);
  const int n = orb_build_cell_classes(&P, cells.data(), P.ncells, cls.data(), ORB_MAX_CELL_CLASSES);
  CHECK(n > 0, "%dx%d sf %g: %d classes", W, H, sf, n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < i; ++j)
      CHECK(!(cls[i].level == cls[j].level && cls[i].R == cls[j].R && cls[i].C == cls[j].C),
            "%dx%d sf %g: classes %d and %d are one", W, H, sf, i, j);
  for (size_t ci = 0; ci < cells.size(); ++ci) {
    const OrbCellDesc& c = cells[ci];
    CHECK(c.cls >= 0 && c.cls < n, "cell %zu: class %d of %d", ci, c.cls, n);
    const OrbCellClass& k = cls[c.cls];
    const OrbLevelDesc& d = P.lv[c.level];
#define CELL "%dx%d sf %g cell %zu (level %d, class %d)", W, H, sf, ci, (int)c.level, (int)c.cls
    // the level, as issue() read it from plan.lv[]
    CHECK(k.level == c.level && k.w == d.w && k.h1 == d.h - 1, CELL);
    CHECK(k.pitch == (c.level ? d.pitch : 0), CELL);
    CHECK((((long long)k.arenaHi << 32) | k.arenaLo) == d.arenaOff, CELL);
    // the cell, by the old per-cell formulas
    const int R = c.y1 - c.y0, C = c.x1 - c.x0;
    CHECK(k.R == R && k.C == C, CELL);
    CHECK(k.tiny == (R < 7 || C < 7), CELL);
    if (k.tiny) continue;
    if (((C + 12) & ~7) > 56) {  // wider than k_fast_cells stages: the plan takes k_fast_band
      CHECK(!orb_cell_class_ok(&k), CELL);
      continue;
    }
    CHECK(orb_cell_class_ok(&k), CELL);
    const int iw = C - 6, ih = R - 6, nK = (iw + 7) >> 3, nvLast = iw - 8 * (nK - 1);
    CHECK(k.P == ((C + 12) & ~7) && k.iw == iw && k.ih == ih && k.nK == nK, CELL);
    CHECK(k.lastMask == (int)((1u << nvLast) - 1u) && k.nG == ih * nK, CELL);
    const float invK = 1.0f / (float)nK;
    const int rInc = (int)(64.5f * invK), kInc = 64 - rInc * nK;
    CHECK(rInc == 64 / nK && k.kInc == kInc, CELL);
    const int pitches[2] = {k.P, ORB_FC_CONST_PITCH};
    for (int v = 0; v < 2; ++v) {
      const int Pv = pitches[v];
      if (Pv < k.P) continue;  // the compile-time instance runs only cells that fit its pitch
      const int dOff = v ? k.dOff48 : k.dOff, wrapOff = v ? k.wrapOff48 : k.wrapOff;
      const uint32_t mP = v ? k.mP48 : k.mP;
      CHECK(dOff == rInc * Pv + 8 * kInc && wrapOff == Pv - 8 * nK, CELL);
      // every tile byte a corner can sit at: row and column from the byte
      for (int off = 0; off < R * Pv; ++off)
        CHECK((int)(((uint32_t)off * mP) >> ORB_QUOT_SHIFT) == fquot(off, Pv) &&
                  fquot(off, Pv) == off / Pv, CELL);
    }
    // every lane's first group
    for (int lane = 0; lane < 64; ++lane) {
      const int rr0 = fquot(lane, nK);
      CHECK((int)(((uint32_t)lane * k.mK) >> ORB_QUOT_SHIFT) == rr0 && rr0 == lane / nK, CELL);
    }
    // every window pixel of the dense NMS
    for (int j = 0; j < ih * iw; ++j)
      CHECK((int)(((uint32_t)j * k.mW) >> ORB_QUOT_SHIFT) == fquot(j, iw) && fquot(j, iw) == j / iw,
            CELL);
    // the 24-bit operands
    CHECK(k.mK < (1u << 24) && k.mP < (1u << 24) && k.mW < (1u << 24) && k.pitch < (1 << 24), CELL);
#undef CELL
  }
  *ncellsOut = P.ncells;
  *nclsOut = n;
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 5 || (argc - 1) % 4) return 2;
  // the multipliers over the widest ranges any cell k_fast_cells accepts can
  // reach (rows <= 64, pitch <= 56, window <= 58 x 50): divisor d, argument
  // below 64 * 56 -- exact, and within the 24-bit multiply
  for (int d = 1; d <= 56; ++d)
    CHECK(orb_quot_exact(orb_quot_magic(d), d, 64 * 56), "divisor %d", d);
  CHECK(!orb_quot_exact(orb_quot_magic(0), 0, 16), "divisor 0 accepted");
  CHECK(!orb_quot_exact(orb_quot_magic(3) - 1, 3, 64 * 56), "a wrong multiplier accepted");
  int cells = 0, classes = 0;
  for (int a = 1; a + 3 < argc; a += 4) {
    int nc = 0, nk = 0;
    if (check_plan(atoi(argv[a]), atoi(argv[a + 1]), atof(argv[a + 2]), atoi(argv[a + 3]), &nc, &nk))
      return 1;
    cells += nc;
    classes += nk;
  }
  printf("OK %d cells %d classes\n", cells, classes);
  return 0;
}
