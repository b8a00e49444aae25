// CDNA transformation (reference ops.py:52-98): M per-sample k x k kernels, predicted as a vector per sample, are
// normalised ( k = relu(p - shift) + shift,  n = k / sum_uv k ) and applied as a depthwise SAME correlation to the
// previous image.  The reference then splits the depthwise output [B,H,W,C*M] (channel q = c*M + m) into M pieces of C
// channels along the channel axis; piece j, channel i is q = j*C + i, i.e. colour c = q / M with mask m = q % M.
// That indexing is reproduced as it is written.
//
// HBM-bound stencil, sibling of the DNA gather (dna.hip): a block owns a 16x16 pixel tile of one sample, stages the
// image window (tile + halo, zeros outside = SAME padding) and the sample's normalised kernels in LDS once, and every
// thread produces all C*M outputs of its pixel from registers.  Algorithmic bytes, forward: (1 + M) image-sized
// tensors; backward: (1 + M) read + 1 written, plus the k*k*M kernel gradients per sample.
#include <hip/hip_runtime.h>

#include "cdna_common.h"
#include "common.h"

namespace {

using namespace acg_cdna;

template <int K>
__global__ __launch_bounds__(256) void cdna_fwd_k(const float* __restrict__ params, const float* __restrict__ img,
                                                  float* __restrict__ out, float* __restrict__ kern_norm, Geo g,
                                                  float shift) {
  __shared__ float kn[kMaxK * kMaxK * kMaxM];
  __shared__ float S[kMaxM];
  __shared__ float win[(kTile + kMaxK - 1) * (kTile + kMaxK - 1) * kMaxC];
  const int b = blockIdx.z, ty = blockIdx.y, tx = blockIdx.x;
  constexpr int kk = K * K, ww = kTile + K - 1;
  const int y0 = ty * kTile, x0 = tx * kTile;
  stage_kernels(params, b, g, shift, kn, S);
  if (ty == 0 && tx == 0 && kern_norm)
    for (int i = threadIdx.x; i < kk * g.M; i += blockDim.x) kern_norm[(long long)b * kk * g.M + i] = kn[i];
  stage_window(img + (long long)b * g.H * g.W * g.C, g.C, g.C, y0, x0, g, win);       // dense: the pitch is C
  __syncthreads();
  const int ly = threadIdx.x / kTile, lx = threadIdx.x % kTile;
  const int y = y0 + ly, x = x0 + lx;
  if (y >= g.H || x >= g.W) return;
  const long long plane = (long long)g.B * g.H * g.W * g.C;               // one of the M output pieces
  const long long pix = (((long long)b * g.H + y) * g.W + x) * g.C;
  for (int c = 0; c < g.C; ++c) {
    float w[kk];                                                         // the pixel's window of colour c, in registers
#pragma unroll
    for (int u = 0; u < K; ++u)
#pragma unroll
      for (int v = 0; v < K; ++v) w[u * K + v] = win[((ly + u) * ww + lx + v) * g.C + c];
    for (int m = 0; m < g.M; ++m) {
      float acc = 0.f;
#pragma unroll
      for (int t = 0; t < kk; ++t) acc += w[t] * kn[t * g.M + m];       // LDS broadcast reads
      const int q = c * g.M + m;
      out[(q / g.C) * plane + pix + q % g.C] = acc;
    }
  }
}

// d img[b,y,x,c] = sum_{m,u,v} dout_q(c,m)[b, y-u+pad, x-v+pad] * n[b,u,v,m]
// The dout planes of as many masks as fit 48 KB of LDS (all 10 at k=5, C=3) are staged at once as a window with halo
// (K-1-pad before, pad after): one round of loads in flight instead of one memory round trip per mask.
constexpr int kWinFloats = 12288, kDdFloats = 8192;
__global__ __launch_bounds__(256) void cdna_bwd_img_k(const float* __restrict__ kern_norm, const float* __restrict__ dout,
                                                      float* __restrict__ dimg, Geo g) {
  __shared__ float kn[kMaxK * kMaxK * kMaxM];
  __shared__ float win[kWinFloats];                 // [window pixel][mask in chunk][colour]
  const int b = blockIdx.z, y0 = blockIdx.y * kTile, x0 = blockIdx.x * kTile, kk = g.K * g.K;
  const int ww = kTile + g.K - 1, before = g.K - 1 - g.pad;
  const int mc = min(g.M, kWinFloats / (ww * ww * g.C));           // masks per round (>= 1 for every supported shape)
  for (int i = threadIdx.x; i < kk * g.M; i += blockDim.x) kn[i] = kern_norm[(long long)b * kk * g.M + i];
  const int ly = threadIdx.x / kTile, lx = threadIdx.x % kTile;
  const int y = y0 + ly, x = x0 + lx;
  const long long plane = (long long)g.B * g.H * g.W * g.C;
  float acc[kMaxC] = {0.f, 0.f, 0.f, 0.f};
  for (int m0 = 0; m0 < g.M; m0 += mc) {
    const int nm = min(mc, g.M - m0);
    __syncthreads();
    for (int i = threadIdx.x; i < ww * ww * nm * g.C; i += blockDim.x) {
      const int c = i % g.C, r = i / g.C, mm = r % nm, p = r / nm, wx = p % ww, wy = p / ww, q = c * g.M + m0 + mm;
      const int gy = y0 + wy - before, gx = x0 + wx - before;
      win[i] = (gy >= 0 && gy < g.H && gx >= 0 && gx < g.W)
                   ? dout[(q / g.C) * plane + (((long long)b * g.H + gy) * g.W + gx) * g.C + q % g.C] : 0.f;
    }
    __syncthreads();
    for (int u = 0; u < g.K; ++u)
      for (int v = 0; v < g.K; ++v) {
        const float* src = win + ((ly + g.K - 1 - u) * ww + lx + g.K - 1 - v) * nm * g.C;
        for (int mm = 0; mm < nm; ++mm) {
          const float w = kn[(u * g.K + v) * g.M + m0 + mm];
#pragma unroll
          for (int c = 0; c < kMaxC; ++c)
            if (c < g.C) acc[c] += src[mm * g.C + c] * w;
        }
      }
  }
  if (y >= g.H || x >= g.W) return;
#pragma unroll
  for (int c = 0; c < kMaxC; ++c)
    if (c < g.C) dimg[(((long long)b * g.H + y) * g.W + x) * g.C + c] = acc[c];
}

// per-tile partial kernel gradients: part[b][tile][(u*K+v)*M + m] = sum_{pixels in tile, c} dout_q(c,m)[pix] * img[pix+(u,v)-pad, c]
// The tile's dout of as many masks as fit 32 KB is staged at once, then summed per tap (tile_kernel_partials).
__global__ __launch_bounds__(256) void cdna_bwd_kern_partial_k(const float* __restrict__ img, const float* __restrict__ dout,
                                                               float* __restrict__ part, Geo g) {
  __shared__ float win[(kTile + kMaxK - 1) * (kTile + kMaxK - 1) * kMaxC];
  __shared__ float dd[kDdFloats];                   // [pixel][mask in chunk][colour]
  __shared__ float red[256];
  const int b = blockIdx.z, ty = blockIdx.y, tx = blockIdx.x, y0 = ty * kTile, x0 = tx * kTile;
  const int mc = min(g.M, kDdFloats / (kTile * kTile * g.C));
  const long long plane = (long long)g.B * g.H * g.W * g.C;
  stage_window(img + (long long)b * g.H * g.W * g.C, g.C, g.C, y0, x0, g, win);
  float* o = part + (((long long)b * g.tiles_y + ty) * g.tiles_x + tx) * g.K * g.K * g.M;
  for (int m0 = 0; m0 < g.M; m0 += mc) {
    const int nm = min(mc, g.M - m0);
    __syncthreads();
    for (int i = threadIdx.x; i < kTile * kTile * nm * g.C; i += blockDim.x) {
      const int c = i % g.C, r = i / g.C, mm = r % nm, p = r / nm, y = y0 + p / kTile, x = x0 + p % kTile, q = c * g.M + m0 + mm;
      dd[i] = (y < g.H && x < g.W) ? dout[(q / g.C) * plane + (((long long)b * g.H + y) * g.W + x) * g.C + q % g.C] : 0.f;
    }
    __syncthreads();
    tile_kernel_partials(win, dd, red, o, g.K, g.C, g.M, m0, nm);
  }
}

// one block per sample: the tile partials summed and taken through the normalisation and the relu
__global__ __launch_bounds__(256) void cdna_bwd_kern_final_k(const float* __restrict__ params, const float* __restrict__ kern_norm,
                                                             const float* __restrict__ part, float* __restrict__ dparams,
                                                             Geo g, float shift) {
  finish_dparams(params, kern_norm, part, dparams, blockIdx.x, g, shift);
}

}  // namespace

extern "C" {

size_t acg_cdna_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t M, int32_t K) {
  Geo g;
  if (make_geo("cdna_workspace_bytes", B, H, W, C, M, K, C, false, &g) != ACG_OK) return 0;
  return partials(g) * sizeof(float);
}

int32_t acg_cdna_fwd(const void* params, const void* image, void* out, float* kern_norm, int32_t B, int32_t H, int32_t W,
                     int32_t C, int32_t M, int32_t K, float relu_shift, int32_t dtype, acg_stream_t stream) {
  ACG_REQUIRE_F32(dtype);
  Geo g;
  if (int rc = make_geo("cdna_fwd", B, H, W, C, M, K, C, false, &g)) return rc;
  ACG_REQUIRE(params && image && out, ACG_ERR_INVALID_ARG, "cdna_fwd: null pointer");
  ACG_REQUIRE(K == 3 || K == 5 || K == 7, ACG_ERR_UNSUPPORTED, "cdna_fwd: kernel size %d (3, 5 or 7)", K);
  const dim3 grid(g.tiles_x, g.tiles_y, B);
  hipStream_t st = acg::to_stream(stream);
  const float *pp = (const float*)params, *im = (const float*)image;
  if (K == 3) ACG_LAUNCH(cdna_fwd_k<3>, grid, dim3(256), 0, st, pp, im, (float*)out, kern_norm, g, relu_shift);
  else if (K == 5) ACG_LAUNCH(cdna_fwd_k<5>, grid, dim3(256), 0, st, pp, im, (float*)out, kern_norm, g, relu_shift);
  else ACG_LAUNCH(cdna_fwd_k<7>, grid, dim3(256), 0, st, pp, im, (float*)out, kern_norm, g, relu_shift);
  return acg::check_launch("cdna_fwd");
}

int32_t acg_cdna_bwd(const void* params, const float* kern_norm, const void* image, const void* dout, void* dparams,
                     void* dimage, int32_t B, int32_t H, int32_t W, int32_t C, int32_t M, int32_t K, float relu_shift,
                     int32_t dtype, void* ws, size_t wsb, acg_stream_t stream) {
  ACG_REQUIRE_F32(dtype);
  Geo g;
  if (int rc = make_geo("cdna_bwd", B, H, W, C, M, K, C, false, &g)) return rc;
  ACG_REQUIRE(params && kern_norm && image && dout && dparams, ACG_ERR_INVALID_ARG, "cdna_bwd: null pointer");
  ACG_REQUIRE(ws && wsb >= acg_cdna_workspace_bytes(B, H, W, C, M, K), ACG_ERR_WORKSPACE, "cdna_bwd: workspace too small");
  hipStream_t st = acg::to_stream(stream);
  const dim3 grid(g.tiles_x, g.tiles_y, B);
  if (dimage) {
    ACG_LAUNCH(cdna_bwd_img_k, grid, dim3(256), 0, st, kern_norm, (const float*)dout, (float*)dimage, g);
    if (int rc = acg::check_launch("cdna_bwd_img")) return rc;
  }
  ACG_LAUNCH(cdna_bwd_kern_partial_k, grid, dim3(256), 0, st, (const float*)image, (const float*)dout, (float*)ws, g);
  if (int rc = acg::check_launch("cdna_bwd_kern_partial")) return rc;
  ACG_LAUNCH(cdna_bwd_kern_final_k, dim3(B), dim3(256), 0, st, (const float*)params, kern_norm, (const float*)ws,
                     (float*)dparams, g, relu_shift);
  return acg::check_launch("cdna_bwd_kern_final");
}

}  // extern "C"
