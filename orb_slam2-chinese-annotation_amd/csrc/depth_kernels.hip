// depth_kernels.hip -- gfx950 kernels for what a stereo / RGB-D frame does
// with its depth:
//   k_stereo_from_rgbd   Frame::ComputeStereoFromRGBD (src/Frame.cc:707-728)
//                        with Tracking::GrabImageRGBD's convertTo
//                        (src/Tracking.cc:229-230) applied to the sampled
//                        element only
//   k_unproject_stereo   Frame::UnprojectStereo (src/Frame.cc:730-744) for
//                        every keypoint of a frame
//   k_close_points       the sorted closest-point selection of
//                        Tracking::UpdateLastFrame (src/Tracking.cc:969-1021)
//                        and CreateNewKeyFrame (:1263-1318) with the counts of
//                        NeedNewKeyFrame (:1181-1197)
//
// All float arithmetic is written in the reference's evaluation order; the
// library is built with -ffp-contract=off and correctly rounded divides, so
// every product, sum and quotient rounds separately as on the CPU.
//
// The first two are one thread per keypoint slot over n_frames x stride (the
// shape of k_undistort_keys): a gather of one depth element and five float
// operations, or eleven float operations and a 13-byte store; both are
// latency-bound epilogues.  k_close_points is one workgroup per frame.
#include <algorithm>

#include "orb_device.h"
#include "orb_kernels.h"

__global__ __launch_bounds__(256) void k_stereo_from_rgbd(
    RgbdParams P, const int32_t* __restrict__ counts, int nSingle,
    const orb_keypoint_t* __restrict__ keys, const orb_keypoint_t* __restrict__ keysUn,
    const uint8_t* __restrict__ depth, float* __restrict__ uRight, float* __restrict__ depthOut) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int f = (int)(g / P.stride), i = (int)(g - (long long)f * P.stride);
  if (f >= P.nFrames) return;
  const int n = counts ? counts[f] : nSingle;
  if (i >= n) return;
  // imDepth.at<float>(v, u): the float arguments convert to int, toward zero
  const float u = keys[g].x, v = keys[g].y;
  float ur = -1.0f, z = -1.0f;
  if (fabsf(u) < 2147483648.0f && fabsf(v) < 2147483648.0f) {  // (false for NaN)
    const int col = (int)u, row = (int)v;
    if (col >= 0 && col < P.cols && row >= 0 && row < P.rows) {
      const uint8_t* img = depth + (long long)f * P.imageBytes + (long long)row * P.rowBytes;
      float d;
      if (P.depthType == ORB_DEPTH_U16) {
        // cvtScale_<ushort, float, float>: (float)src * scale (+ 0.0f)
        d = (float)reinterpret_cast<const uint16_t*>(img)[col] * P.factor;
      } else {
        d = reinterpret_cast<const float*>(img)[col];
        if (P.convert) d = d * P.factor;
      }
      if (d > 0) {  // :722
        z = d;
        ur = keysUn[g].x - P.bf / d;  // :725
      }
    }
  }
  uRight[g] = ur;
  depthOut[g] = z;
}

__global__ __launch_bounds__(256) void k_unproject_stereo(
    UnprojectParams P, const int32_t* __restrict__ counts, int nSingle,
    const orb_keypoint_t* __restrict__ keysUn, const float* __restrict__ depth,
    const orb_pose_t* __restrict__ poses, float* __restrict__ x3d, uint8_t* __restrict__ valid) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int f = (int)(g / P.stride), i = (int)(g - (long long)f * P.stride);
  if (f >= P.nFrames) return;
  const int n = counts ? counts[f] : nSingle;
  if (i >= n) return;
  const float z = depth[g];
  float X = 0.0f, Y = 0.0f, Z = 0.0f;
  const bool ok = z > 0;  // :733
  if (ok) {
    const orb_pose_t& T = poses[f];
    const float x = (keysUn[g].x - P.cx) * z * P.invfx;  // :737
    const float y = (keysUn[g].y - P.cy) * z * P.invfy;  // :738
    // mRwc * x3Dc + mOw, mRwc = mRcw.t() (:298, :740)
    X = ((T.rcw[0] * x + T.rcw[3] * y) + T.rcw[6] * z) + T.ow[0];
    Y = ((T.rcw[1] * x + T.rcw[4] * y) + T.rcw[7] * z) + T.ow[1];
    Z = ((T.rcw[2] * x + T.rcw[5] * y) + T.rcw[8] * z) + T.ow[2];
  }
  x3d[3 * g] = X;
  x3d[3 * g + 1] = Y;
  x3d[3 * g + 2] = Z;
  valid[g] = ok;
}

// Bitonic sort of P (power of two) keys, ascending, by one workgroup: each
// work item owns one compare-exchange of a step.
__device__ __forceinline__ void cp_bitonic(unsigned long long* keys, int P) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += blockDim.x) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const unsigned long long a = keys[lo], b = keys[hi];
        if ((a > b) == ((lo & k) == 0)) {
          keys[lo] = b;
          keys[hi] = a;
        }
      }
      __syncthreads();
    }
  }
}

// One workgroup per frame.  vDepthIdx as keys (float bits of z) << 32 | index:
// positive floats (+inf included) order as unsigned integers and the index
// makes every key distinct, so an ascending sort of the keys is std::sort on
// the pairs.  The keys are compacted by ballot prefix (a wave reserves its
// run with one LDS atomic; the order inside the compacted list is irrelevant,
// the sort fixes it), padded with ~0 to the next power of two of their count
// and sorted by cp_bitonic: in dynamic LDS sized to the call's padded stride
// (GLOBAL = false, stride <= CP_LDS_KEYS), or in `gKeys`, `cap` keys of global
// scratch per frame (GLOBAL = true).  The visit bound, the create flags and
// NeedNewKeyFrame's counts follow in the same launch.
template <bool GLOBAL>
__global__ __launch_bounds__(1024) void k_close_points(
    const int32_t* __restrict__ counts, int nSingle, int stride, const float* __restrict__ depth,
    const uint8_t* __restrict__ mpState, const uint8_t* __restrict__ outlier, float thDepth,
    int32_t* __restrict__ order, uint8_t* __restrict__ create,
    orb_close_counts_t* __restrict__ out, unsigned long long* gKeys, int cap) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long cpKeys[];
  __shared__ int sCount, sTracked, sNon, sVisit;
  const int f = blockIdx.x, t = threadIdx.x, lane = t & 63;
  unsigned long long* keys = GLOBAL ? gKeys + (size_t)f * cap : cpKeys;
  const int n = min(max(counts ? counts[f] : nSingle, 0), stride);
  const size_t base = (size_t)f * stride;
  const float* Z = depth + base;
  const uint8_t* MS = mpState ? mpState + base : nullptr;
  const uint8_t* OL = outlier ? outlier + base : nullptr;
  if (t == 0) {
    sCount = 0;
    sTracked = 0;
    sNon = 0;
    sVisit = 0x7FFFFFFF;
  }
  __syncthreads();
  const unsigned long long ltMask = (1ull << lane) - 1ull;
  int tracked = 0, non = 0;
  for (int b0 = 0; b0 < n; b0 += blockDim.x) {  // (uniform trip count: whole waves ballot)
    const int i = b0 + t;
    float z = 0.0f;
    bool has = false;
    if (i < n) {
      z = Z[i];
      has = z > 0;  // :976, :1271
      if (has && z < thDepth) {  // :1187
        const bool tr = (MS && MS[i] != 0) && !(OL && OL[i]);  // :1189
        tracked += tr;
        non += !tr;
      }
    }
    const unsigned long long b = __ballot(has);
    int wbase = 0;
    if (lane == 0 && b) wbase = atomicAdd(&sCount, __popcll(b));
    wbase = __shfl(wbase, 0);
    if (has)
      keys[wbase + __popcll(b & ltMask)] =
          ((unsigned long long)__float_as_uint(z) << 32) | (uint32_t)i;
  }
  tracked = wave_sum(tracked);
  non = wave_sum(non);
  if (lane == 0) {
    if (tracked) atomicAdd(&sTracked, tracked);
    if (non) atomicAdd(&sNon, non);
  }
  __syncthreads();
  const int cnt = sCount;  // vDepthIdx.size(), <= n <= cap
  int P = 1;
  while (P < cnt) P <<= 1;
  for (int i = cnt + t; i < P; i += blockDim.x) keys[i] = ~0ull;
  __syncthreads();
  cp_bitonic(keys, P);
  // the loop of :990-1021 / :1282-1317 processes position j (nPoints = j + 1
  // in either branch) and breaks after it when z_j > mThDepth && nPoints > 100
  for (int j = t; j < cnt; j += blockDim.x) {
    const float z = __uint_as_float((uint32_t)(keys[j] >> 32));
    if (z > thDepth && j + 1 > 100) {
      atomicMin(&sVisit, j + 1);
      break;  // (this thread's later positions are larger)
    }
  }
  __syncthreads();
  const int nVisit = min(sVisit, cnt);
  for (int j = t; j < stride; j += blockDim.x) {
    int32_t idx = -1;
    uint8_t c = 0;
    if (j < cnt) {
      idx = (int32_t)(uint32_t)keys[j];
      c = j < nVisit && (!MS || MS[idx] < 2);  // bCreateNew (:997-1002, :1289-1295)
    }
    order[base + j] = idx;
    create[base + j] = c;
  }
  if (t == 0) {
    orb_close_counts_t r;
    r.n_sorted = cnt;
    r.n_visit = nVisit;
    r.n_tracked_close = sTracked;
    r.n_non_tracked_close = sNon;
    out[f] = r;
  }
}

extern "C" hipError_t orb_k_stereo_from_rgbd(const RgbdParams* params, const int32_t* counts,
                                             int nSingle, const orb_keypoint_t* keys,
                                             const orb_keypoint_t* keysUn, const void* depth,
                                             float* uRight, float* depthOut, hipStream_t s) {
  const long long total = (long long)params->nFrames * params->stride;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_stereo_from_rgbd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                     *params, counts, nSingle, keys, keysUn, (const uint8_t*)depth, uRight,
                     depthOut);
  return hipGetLastError();
}

extern "C" hipError_t orb_k_unproject_stereo(const UnprojectParams* params,
                                             const int32_t* counts, int nSingle,
                                             const orb_keypoint_t* keysUn, const float* depth,
                                             const orb_pose_t* poses, float* x3d, uint8_t* valid,
                                             hipStream_t s) {
  const long long total = (long long)params->nFrames * params->stride;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_unproject_stereo, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                     *params, counts, nSingle, keysUn, depth, poses, x3d, valid);
  return hipGetLastError();
}

// the power of two a frame of `stride` slots pads to (>= 2)
static int cp_cap(int stride) {
  int cap = 2;
  while (cap < stride) cap <<= 1;
  return cap;
}

extern "C" size_t orb_k_close_points_scratch(int nFrames, int stride) {
  if (stride <= CP_LDS_KEYS) return 0;
  return (size_t)nFrames * cp_cap(stride) * sizeof(unsigned long long);
}

extern "C" hipError_t orb_k_close_points(int nFrames, const int32_t* counts, int nSingle,
                                         int stride, const float* depth, const uint8_t* mpState,
                                         const uint8_t* outlier, float thDepth, int32_t* order,
                                         uint8_t* create, orb_close_counts_t* out, void* scratch,
                                         hipStream_t s) {
  if (nFrames <= 0 || stride <= 0) return hipSuccess;
  const int cap = cp_cap(stride);
  if (stride <= CP_LDS_KEYS) {
    // a thread per compare-exchange of a step, whole waves
    const int wg = std::min(1024, std::max(64, cap / 2));
    hipLaunchKernelGGL(k_close_points<false>, dim3(nFrames), dim3(wg),
                       (size_t)cap * sizeof(unsigned long long), s, counts, nSingle, stride, depth,
                       mpState, outlier, thDepth, order, create, out, nullptr, cap);
  } else {
    if (!scratch) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_close_points<true>, dim3(nFrames), dim3(1024), 0, s, counts, nSingle,
                       stride, depth, mpState, outlier, thDepth, order, create, out,
                       (unsigned long long*)scratch, cap);
  }
  return hipGetLastError();
}
