// What cdna.hip (the unfused transformation, M pieces in HBM) and cdna_composite.hip (the fused transform-and-composite)
// share, in its one copy: the tile geometry and its argument checks, the LDS staging of a sample's normalised kernels and
// of an image window at a channel pitch, and the two halves of the kernel gradient - the per-tile partials and the final
// pass through the normalisation and the relu.  The per-pixel correlation loops stay in the kernels.  The two composites
// (cdna_composite.hip, affine_composite.hip) also share the mask stage: the per-pixel softmax weight, the per-tile partial of
// the bias gradient and its final sum.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace acg_cdna {

constexpr int kTile = 16;       // pixels per tile side (256 threads = one per pixel)
constexpr int kMaxK = 7, kMaxM = 32, kMaxC = 4;

struct Geo {
  int B, H, W, C, M, K, pad;
  int tiles_x, tiles_y;
  int pitch;                    // channel pitch of the image (C: dense)
};

// odd_k: the entry runs kernels compiled per kernel size (3, 5 or 7); otherwise any 1 <= K <= kMaxK.  pitch 0 means dense.
inline int make_geo(const char* who, int B, int H, int W, int C, int M, int K, int pitch, bool odd_k, Geo* g) {
  ACG_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && M > 0 && K > 0, ACG_ERR_INVALID_ARG, "%s: non-positive size", who);
  ACG_REQUIRE(C <= kMaxC && M <= kMaxM, ACG_ERR_UNSUPPORTED, "%s: supports C <= %d, masks <= %d", who, kMaxC, kMaxM);
  ACG_REQUIRE(odd_k ? (K == 3 || K == 5 || K == 7) : K <= kMaxK, ACG_ERR_UNSUPPORTED, "%s: kernel size %d (%s)", who, K,
              odd_k ? "3, 5 or 7" : "1 to 7");
  ACG_REQUIRE(B <= 65535, ACG_ERR_UNSUPPORTED, "%s: batch too large", who);
  ACG_REQUIRE(pitch == 0 || (pitch >= C && pitch <= 64), ACG_ERR_INVALID_ARG, "%s: image pitch %d for %d channels", who, pitch, C);
  g->B = B; g->H = H; g->W = W; g->C = C; g->M = M; g->K = K;
  g->pad = (K - 1) / 2;                              // SAME, stride 1: pad_before = (k-1)//2
  g->tiles_x = (W + kTile - 1) / kTile; g->tiles_y = (H + kTile - 1) / kTile;
  g->pitch = pitch ? pitch : C;
  return ACG_OK;
}

constexpr int kPix = kTile * kTile;
constexpr int kMaxZ = kMaxM + 1;                                   // mask channels: the image, the M transforms and, for M < kMaxM, a canvas

// floats of the kernel-gradient partials in the workspace: [b][tile][(u*K+v)*M + m]
inline size_t partials(const Geo& g) { return (size_t)g.B * g.tiles_x * g.tiles_y * g.K * g.K * g.M; }

// normalised kernels of sample b into LDS: kn[(u*K+v)*M + m]; also the per-mask sums S[m]
__device__ __forceinline__ void stage_kernels(const float* __restrict__ params, int b, const Geo& g, float shift,
                                              float* kn, float* S) {
  const int kk = g.K * g.K, n = kk * g.M;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float p = params[(long long)b * n + i];
    kn[i] = fmaxf(p - shift, 0.f) + shift;
  }
  __syncthreads();
  if ((int)threadIdx.x < g.M) {
    float s = 0.f;
    for (int t = 0; t < kk; ++t) s += kn[t * g.M + threadIdx.x];
    S[threadIdx.x] = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) kn[i] /= S[i % g.M];
  __syncthreads();
}

// tile + halo of a [H,W,pitch] plane set (channels 0..Cs-1) into LDS as win[(y*ww + x)*Cs + c], zeros outside the image
__device__ __forceinline__ void stage_window(const float* __restrict__ src, int Cs, int pitch, int y0, int x0, const Geo& g,
                                             float* win) {
  const int ww = kTile + g.K - 1, n = ww * ww * Cs;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int c = i % Cs, p = i / Cs, x = p % ww, y = p / ww;
    const int gy = y0 + y - g.pad, gx = x0 + x - g.pad;
    win[i] = (gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) ? src[((long long)gy * g.W + gx) * pitch + c] : 0.f;
  }
}

// Kernel-gradient partials of one tile for the nm masks from m0 on: o[(u*K+v)*M + m0 + mm] = sum over the tile's pixels p
// and the colours of dd[(p*nm + mm)*C + c] * win(p + (u,v), c).  4 pixel groups x 64 tap slots: a thread sums its tap over
// 64 pixels, then the 4 groups are folded through red[256] in a fixed order.  win and dd must be complete (a barrier
// behind their last write) on entry.
__device__ __forceinline__ void tile_kernel_partials(const float* win, const float* dd, float* red, float* __restrict__ o,
                                                     int K, int C, int M, int m0, int nm) {
  static_assert(kMaxK * kMaxK <= 64, "one wave-slot per tap");
  const int kk = K * K, ww = kTile + K - 1, tid = threadIdx.x;
  const int t = tid & 63, pg = tid >> 6, u = t / K, v = t % K;
  for (int mm = 0; mm < nm; ++mm) {
    float acc = 0.f;
    if (t < kk) {
      for (int p = pg * 64; p < pg * 64 + 64; ++p) {
        const float* wsrc = win + ((p / kTile + u) * ww + p % kTile + v) * C;
        const float* dsrc = dd + (p * nm + mm) * C;
#pragma unroll
        for (int c = 0; c < kMaxC; ++c)
          if (c < C) acc += dsrc[c] * wsrc[c];
      }
    }
    __syncthreads();                                 // red[] of the previous mask has been consumed
    red[tid] = acc;
    __syncthreads();
    if (tid < kk) o[tid * M + m0 + mm] = red[tid] + red[64 + tid] + red[128 + tid] + red[192 + tid];
  }
}

// dparams of sample b by one block: dn = sum of the sample's tile partials in tile order; through the normalisation,
// dk = (dn - sum_uv(dn * n)) / S, and the relu, dp = dk * [p - shift > 0]
__device__ __forceinline__ void finish_dparams(const float* __restrict__ params, const float* __restrict__ kern_norm,
                                               const float* __restrict__ part, float* __restrict__ dparams, int b,
                                               const Geo& g, float shift) {
  __shared__ float dn[kMaxK * kMaxK * kMaxM];
  __shared__ float dot[kMaxM], S[kMaxM];
  const int kk = g.K * g.K, n = kk * g.M, ntile = g.tiles_x * g.tiles_y;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    double s = 0.0;
    for (int t = 0; t < ntile; ++t) s += part[((long long)b * ntile + t) * n + i];
    dn[i] = (float)s;
  }
  __syncthreads();
  if ((int)threadIdx.x < g.M) {
    const int m = threadIdx.x;
    float d = 0.f, s = 0.f;
    for (int t = 0; t < kk; ++t) {
      d += dn[t * g.M + m] * kern_norm[(long long)b * n + t * g.M + m];
      s += fmaxf(params[(long long)b * n + t * g.M + m] - shift, 0.f) + shift;
    }
    dot[m] = d; S[m] = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int m = i % g.M;
    const float dk = (dn[i] - dot[m]) / S[m];
    dparams[(long long)b * n + i] = params[(long long)b * n + i] - shift > 0.f ? dk : 0.f;
  }
}

// ---- the mask stage of the two composites ---------------------------------------------------------------------------
// softmax weight of channel j of a pixel (zp its logits, zb the bias in LDS) given its max and 1 / sum
__device__ __forceinline__ float weight(const float* zp, const float* zb, int j, float zmax, float inv) {
  return expf(zp[j] + zb[j] - zmax) * inv;
}

// max and 1 / sum of exp of a pixel's nz biased logits
__device__ __forceinline__ void softmax_stats(const float* zp, const float* zb, int nz, float* zmax_out, float* inv_out) {
  float zmax = -INFINITY, sum = 0.f;
  for (int j = 0; j < nz; ++j) zmax = fmaxf(zmax, zp[j] + zb[j]);
  for (int j = 0; j < nz; ++j) sum += expf(zp[j] + zb[j] - zmax);
  *zmax_out = zmax;
  *inv_out = 1.f / sum;
}

// bias-gradient partial of a tile from dz_j of pixel p at big[j * kPix + p] (complete: a barrier behind the last write):
// 4 lanes per channel, 64 pixels each, then the 4 in order.  o[j], j < nz.  red holds kPix floats.
__device__ __forceinline__ void tile_bias_partial(const float* big, float* red, float* __restrict__ o, int nz) {
  const int tid = threadIdx.x;
  if (tid < nz * 4) {
    const int j = tid >> 2, r = tid & 3;
    float s = 0.f;
    for (int p = r * 64; p < r * 64 + 64; ++p) s += big[j * kPix + p];
    red[tid] = s;
  }
  __syncthreads();
  if (tid < nz) o[tid] = red[tid * 4] + red[tid * 4 + 1] + red[tid * 4 + 2] + red[tid * 4 + 3];
}

// dbias[j] = (acc != 0 ? acc * dbias[j] : 0) + the sum of the `rows` tile partials, by one block.  scratch holds 16 doubles.
__device__ __forceinline__ void final_bias_sum(const float* __restrict__ part_b, float* __restrict__ dbias, float dbias_acc,
                                               int rows, int nz, double* scratch) {
  for (int j = 0; j < nz; ++j) {
    double s = 0.0;
    for (int r = threadIdx.x; r < rows; r += blockDim.x) s += part_b[(long long)r * nz + j];
    s = acg::block_sum(s, scratch);
    if (threadIdx.x == 0) dbias[j] = (dbias_acc != 0.f ? dbias_acc * dbias[j] : 0.f) + (float)s;
  }
}

}  // namespace acg_cdna
