// orb_plan.h -- per-image-size extraction plan shared by the host runtime and kernels.
//
// Everything that depends only on (width, height, nfeatures, scaleFactor,
// nlevels) is computed once on the host -- level sizes, resize coefficient
// tables, the FAST cell grid, octree root layout, output slot layout -- with
// the exact float/double expressions of the reference
// (src/ORBextractor.cc:428-489, 785-815, 558-582, 1172-1207), and handed to
// the kernels by value.  The kernels then do only per-pixel / per-key work.
#pragma once
#include <stdint.h>

#ifndef ORB_MAX_LEVELS
#define ORB_MAX_LEVELS 16
#endif

struct OrbLevelDesc {
  int w, h;          // level size (cvRound(W * invScale), src/ORBextractor.cc:1180)
  int pitch;         // row pitch of the level in the pyramid arena (level 0: caller stride)
  int blurPitch;     // row pitch of the level's blurred copy
  long long arenaOff;// byte offset of the level inside one image's pyramid arena (l >= 1)
  long long blurOff; // byte offset of the blurred level inside one image's blur arena
  int cellBeg, cellEnd;  // range of this level's cells in the cell table
  int quota;         // mnFeaturesPerLevel[l]
  int nodeCap;       // max alive octree nodes == max keypoints this level can emit
  int outOff;        // first output slot of this level inside one image's slot arena
  int nIni;          // octree root count (src/ORBextractor.cc:562)
  float hX;          // root width (src/ORBextractor.cc:564)
  int Wr, Hr;        // maxBorderX-minBorderX, maxBorderY-minBorderY
  float scale;       // mvScaleFactor[l]
  float sizeF;       // (float)(int)(31 * scale), src/ORBextractor.cc:874
  int rtabX, rtabY;  // offsets of this level's resize tables (x: xofs/alpha, y: yofs/beta)
  int xmax;          // first dx whose source tap sx+1 falls outside (resize)
  int resizeMode;    // ORB_RESIZE_NARROW / _WIDE / _GENERIC: k_pyr_resize variant for this level
  int tileBeg;       // first blur tile of this level
  int cellMaxRows, cellMaxCols;  // largest cell ROI of this level (k_fast_cells LDS per launch)
  int resize2;       // 1: levels l and l + 1 are built by one k_pyr_resize2 launch (from l - 1)
};

#define ORB_RESIZE_NARROW 0   // 44 x 44-dword source windows (downscale <= 1.25)
#define ORB_RESIZE_WIDE 1     // 64 x 64 dwords
#define ORB_RESIZE_GENERIC 2  // untiled: each thread reads its taps from the source level

struct OrbPlanDesc {
  int nlevels;
  int ncells;        // total FAST cells over all levels
  int keyCap;        // per-cell candidate capacity (max strict NMS maxima in a cell window)
  int slotsPerImage; // sum of nodeCap over levels
  int iniTh, minTh;
  int maxCellRows, maxCellCols;  // largest cell ROI (for LDS sizing)
  int srcW, srcH;
  int nBlurTiles;    // blur tiles over all levels of one image
  int nBands;        // FAST bands over all levels
  int maxBandBytes;  // largest FAST band in elements: rows x LDS pitch ((cols + 20) & ~7)
  int nCellClasses;  // entries of the cell class table (OrbCellClass)
  int cellClassesOk; // 1: every class passed orb_cell_class_ok (k_fast_cells may run)
  OrbLevelDesc lv[ORB_MAX_LEVELS];
};

// One FAST cell: ROI rows [y0,y1) x cols [x0,x1) of its level image
// (src/ORBextractor.cc:816-839).  Cells are ordered level-major, then
// row-major, i.e. the order in which the reference appends to vToDistributeKeys.
struct OrbCellDesc {
  int16_t level, y0, y1, x0, x1, cls;  // cls: the cell's entry in the class table below
};

// One class of FAST cells: the cells of one level with one ROI size (interior
// cells, the last column, the last row, the corner).  Everything k_fast_cells
// derived from (level, rows, cols) per cell is computed here once by the
// planner; the kernel reads a cell's entry with scalar loads (and keeps the
// level's buffer resource from cell to cell, rebuilding it only where the
// level changes).  Quotients by nK, P and iw are multiply-shifts
// x / d = (x * ceil(2^ORB_QUOT_SHIFT / d)) >> ORB_QUOT_SHIFT, a 24-bit multiply;
// orb_cell_class_ok() checks each exhaustively over the range the kernel uses.
#define ORB_QUOT_SHIFT 18
#define ORB_FC_PITCH(C) (((C) + 12) & ~7)  // k_fast_cells' LDS row pitch of a ROI C wide
#define ORB_FC_CONST_PITCH 48              // the launch pitch of k_fast_cells' compile-time instance
struct OrbCellClass {
  // the level (staging): pitch 0 = level 0, whose pitch is the caller's stride
  int32_t level, pitch, w, h1;  // h1 = h - 1: the level holds h1 * pitch + w bytes
  uint32_t arenaLo, arenaHi;    // the level's byte offset in one image's pyramid arena
  int32_t R, C;                 // ROI rows, cols
  // the window (tiny: R < 7 or C < 7, no window; the fields below are 0)
  int32_t tiny;
  int32_t P;          // ORB_FC_PITCH(C)
  int32_t iw, ih;     // interior (window) size C - 6, R - 6
  int32_t nK;         // 8-pixel groups per interior row
  int32_t lastMask;   // pass mask of a row's last group: its nvLast valid pixels
  int32_t nG;         // ih * nK groups
  int32_t kInc;       // 64 groups on = rInc = 64 / nK rows and kInc = 64 % nK groups on
  // the tile-byte step of those 64 groups, rInc * pitch + 8 * kInc, and of a
  // wrap into the next row, pitch - 8 * nK; the quotient multiplier of the
  // pitch: at the class's own pitch P and at ORB_FC_CONST_PITCH
  int32_t dOff, wrapOff;
  uint32_t mP;
  int32_t dOff48, wrapOff48;
  uint32_t mP48;
  uint32_t mK, mW;    // quotient multipliers of nK and iw
};

static inline uint32_t orb_quot_magic(int d) {
  return d > 0 ? (uint32_t)(((1u << ORB_QUOT_SHIFT) + (uint32_t)d - 1u) / (uint32_t)d) : 0u;
}

static inline void orb_cell_class_fill(OrbCellClass* k, const OrbLevelDesc* lv, int level, int R,
                                       int C) {
  *k = OrbCellClass();
  k->level = level;
  k->pitch = level ? lv->pitch : 0;
  k->w = lv->w;
  k->h1 = lv->h - 1;
  k->arenaLo = (uint32_t)((unsigned long long)lv->arenaOff & 0xFFFFFFFFull);
  k->arenaHi = (uint32_t)((unsigned long long)lv->arenaOff >> 32);
  k->R = R;
  k->C = C;
  k->tiny = R < 7 || C < 7;
  if (k->tiny) return;
  k->P = ORB_FC_PITCH(C);
  k->iw = C - 6;
  k->ih = R - 6;
  k->nK = (k->iw + 7) >> 3;
  k->lastMask = (1 << (k->iw - 8 * (k->nK - 1))) - 1;
  k->nG = k->ih * k->nK;
  const int rInc = 64 / k->nK;
  k->kInc = 64 - rInc * k->nK;
  k->dOff = rInc * k->P + 8 * k->kInc;
  k->wrapOff = k->P - 8 * k->nK;
  k->mP = orb_quot_magic(k->P);
  k->dOff48 = rInc * ORB_FC_CONST_PITCH + 8 * k->kInc;
  k->wrapOff48 = ORB_FC_CONST_PITCH - 8 * k->nK;
  k->mP48 = orb_quot_magic(ORB_FC_CONST_PITCH);
  k->mK = orb_quot_magic(k->nK);
  k->mW = orb_quot_magic(k->iw);
}

// x / d == (x * m) >> ORB_QUOT_SHIFT for every x < n, as a 24-bit multiply
// (both operands below 2^24, the product below 2^32)
static inline bool orb_quot_exact(uint32_t m, int d, int n) {
  if (d <= 0 || n <= 0 || m >= (1u << 24) || n > (1 << 24)) return false;
  if ((unsigned long long)(n - 1) * m >= (1ull << 32)) return false;
  for (int x = 0; x < n; ++x)
    if (((uint32_t)x * m) >> ORB_QUOT_SHIFT != (uint32_t)(x / d)) return false;
  return true;
}

// The ranges k_fast_cells divides over: a lane (< 64) by nK, a tile byte
// (< R * pitch) by the pitch, a window pixel (< ih * iw) by iw; and the 24-bit
// products lane * pitch, row * pitch it forms from the class.
static inline bool orb_cell_class_ok(const OrbCellClass* k) {
  if (k->pitch < 0 || k->pitch >= (1 << 24) || k->R > 64) return false;
  if (k->tiny) return true;
  if (k->P > 56) return false;
  if (!orb_quot_exact(k->mK, k->nK, 64)) return false;
  if (!orb_quot_exact(k->mP, k->P, k->R * k->P)) return false;
  if (k->P <= ORB_FC_CONST_PITCH &&
      !orb_quot_exact(k->mP48, ORB_FC_CONST_PITCH, k->R * ORB_FC_CONST_PITCH))
    return false;
  return orb_quot_exact(k->mW, k->iw, k->ih * k->iw);
}

// Group `ncells` cells by (level, rows, cols): writes each cell's class id and
// the class table; returns the number of classes, or -1 beyond `cap` entries.
static inline int orb_build_cell_classes(const OrbPlanDesc* plan, OrbCellDesc* cells, int ncells,
                                         OrbCellClass* out, int cap) {
  int n = 0;
  for (int i = 0; i < ncells; ++i) {
    OrbCellDesc& c = cells[i];
    const int R = c.y1 - c.y0, C = c.x1 - c.x0;
    int j = n - 1;  // cells are level-major: a class met before is among the last few
    while (j >= 0 && !(out[j].level == c.level && out[j].R == R && out[j].C == C)) --j;
    if (j < 0) {
      if (n == cap) return -1;
      orb_cell_class_fill(&out[n], &plan->lv[c.level], c.level, R, C);
      j = n++;
    }
    c.cls = (int16_t)j;
  }
  return n;
}
#define ORB_MAX_CELL_CLASSES (8 * ORB_MAX_LEVELS)

// One FAST band: cells [cellBeg, cellBeg + nCells) of one cell row of one
// level (consecutive in the cell table); rows [y0,y1) x cols [x0,x1) is the
// union of their ROIs.
struct OrbBandDesc {
  int16_t level, y0, y1, x0, x1, nCells;
  int32_t cellBeg;
};
#ifndef ORB_OCTREE_LDS_KB
#define ORB_OCTREE_LDS_KB 52  // k_octree node tables + keys per workgroup (swept 24-64)
#endif
#define ORB_BAND_BYTES 6656  // elements (rows x LDS pitch) of one FAST band: f16 pixels + strengths; 5 workgroups per CU (swept 4-10 K)

// One ORB_BLUR_TW x ORB_BLUR_TH output tile of the 7x7 Gaussian pass over level `level`.
struct OrbTileDesc {
  int16_t level, x0, y0, _pad;
};
#define ORB_BLUR_TW 128
#define ORB_BLUR_TH 32

