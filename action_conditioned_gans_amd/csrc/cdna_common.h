// Tile geometry and LDS staging of cdna_composite.hip (the fused transform-and-composite): one sample's normalised
// kernels and an image window at a channel pitch.  The same arithmetic as cdna.hip's helpers, whose kernels keep their own
// copy (dense images only).
#pragma once
#include <hip/hip_runtime.h>

namespace acg_cdna {

constexpr int kTile = 16;       // pixels per tile side (256 threads = one per pixel)
constexpr int kMaxK = 7, kMaxM = 32, kMaxC = 4;

struct Geo {
  int B, H, W, C, M, K, pad;
  int tiles_x, tiles_y;
  int pitch;                    // channel pitch of the image (C: dense)
};

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

}  // namespace acg_cdna
