// Fused CDNA transform-and-composite (include/acgan_cdna.h): the output stage of the CDNA generator.
//
// Forward, one launch: a block owns a 16x16 pixel tile of one sample and stages, as cdna_fwd_k does, the sample's
// normalised kernels and the image window (SAME zeros) in LDS.  Every thread computes the C*M transformed values of its
// pixel from registers and folds each one straight into the softmax-weighted composite (max-subtracted, the tconv4 bias
// folded in): the M transformed images never reach HBM.  Algorithmic bytes: the image, the M+1 mask logits and the frame.
//
// Backward: the transformed values are recomputed, not stored.  Per pixel g_0 = <dout, image>, g_{j+1} = <dout, T_j> and
// dz_j = s_j (g_j - sum_l s_l g_l); the kernel gradient takes dT_j = s_{j+1} dout.  The tile pass leaves per-(sample, tile)
// partials of the kernel gradient and of the bias gradient in the workspace (cdna_bwd_kern_partial_k's scheme); a final
// pass sums them in a fixed order and goes through the normalisation and the relu.  No atomics.
//
// kCanvas (the acg_cdna_composite_canvas_* entries): one more candidate behind the M transformed images, a canvas [B,H,W,C]
// under mask channel M+1.  Its value is read once per pixel and folded where s_0 * image is; backward, g_{M+1} = <dout,
// canvas> joins the other g_j and dcanvas = s_{M+1} dout is written by the pixel's thread.  The instantiations without it
// are the kernels as they were.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/acgan_cdna.h"
#include "cdna_common.h"
#include "common.h"

namespace {

using namespace acg_cdna;

constexpr int kWin = (kTile + kMaxK - 1) * (kTile + kMaxK - 1) * kMaxC;
constexpr int kBig = kMaxZ * kPix;                                 // bwd: g_j / dz_j per pixel, then the dd chunks

template <int K, bool kCanvas>
__global__ __launch_bounds__(256) void cdna_comp_fwd_k(const float* __restrict__ params, const float* __restrict__ z,
                                                       const float* __restrict__ zbias, const float* __restrict__ img,
                                                       const float* __restrict__ canvas, float* __restrict__ out,
                                                       float* __restrict__ kern_norm, Geo g, float shift) {
  __shared__ float kn[kMaxK * kMaxK * kMaxM];
  __shared__ float S[kMaxM];
  __shared__ float win[kWin];
  __shared__ float zb[kMaxZ];
  const int b = blockIdx.z, y0 = blockIdx.y * kTile, x0 = blockIdx.x * kTile, nz = g.M + 1 + kCanvas;
  constexpr int kk = K * K, ww = kTile + K - 1;
  if ((int)threadIdx.x < nz) zb[threadIdx.x] = zbias ? zbias[threadIdx.x] : 0.f;
  stage_kernels(params, b, g, shift, kn, S);
  if (blockIdx.x == 0 && blockIdx.y == 0 && kern_norm)
    for (int i = threadIdx.x; i < kk * g.M; i += blockDim.x) kern_norm[(long long)b * kk * g.M + i] = kn[i];
  stage_window(img + (long long)b * g.H * g.W * g.pitch, g.C, g.pitch, y0, x0, g, win);
  __syncthreads();
  const int ly = threadIdx.x / kTile, lx = threadIdx.x % kTile;
  const int y = y0 + ly, x = x0 + lx;
  if (y >= g.H || x >= g.W) return;
  const long long pix = ((long long)b * g.H + y) * g.W + x;
  const float* zp = z + pix * nz;
  float zmax, inv;
  softmax_stats(zp, zb, nz, &zmax, &inv);
  const float* centre = win + ((ly + g.pad) * ww + lx + g.pad) * g.C;           // the pixel itself
  const float s0 = weight(zp, zb, 0, zmax, inv);
  float f[kMaxC];
#pragma unroll
  for (int i = 0; i < kMaxC; ++i) f[i] = i < g.C ? s0 * centre[i] : 0.f;
  if (kCanvas) {
    const float sc = weight(zp, zb, g.M + 1, zmax, inv);
#pragma unroll
    for (int i = 0; i < kMaxC; ++i)
      if (i < g.C) f[i] += sc * canvas[pix * g.C + i];
  }
  for (int c = 0; c < g.C; ++c) {
    float w[kk];                                                                // the pixel's window of colour c, in registers
#pragma unroll
    for (int u = 0; u < K; ++u)
#pragma unroll
      for (int v = 0; v < K; ++v) w[u * K + v] = win[((ly + u) * ww + lx + v) * g.C + c];
    for (int m = 0; m < g.M; ++m) {
      float acc = 0.f;
#pragma unroll
      for (int t = 0; t < kk; ++t) acc += w[t] * kn[t * g.M + m];              // LDS broadcast reads
      const int q = c * g.M + m, j = q / g.C, i = q - j * g.C;                  // piece j, channel i
      const float v = weight(zp, zb, j + 1, zmax, inv) * acc;
#pragma unroll
      for (int ii = 0; ii < kMaxC; ++ii)                                         // (a select, not a dynamic register index)
        if (ii == i) f[ii] += v;
    }
  }
  float* o = out + pix * g.C;
#pragma unroll
  for (int i = 0; i < kMaxC; ++i)
    if (i < g.C) o[i] = f[i];
}

// The tile pass of the backward: dz for every pixel; part_n[b][tile][(u*K+v)*M + m] = sum over the tile's pixels and the
// colours of dT_q * image(pixel + (u,v) - pad, c) with q = c*M + m; part_b[b][tile][j] = sum over the tile's pixels of dz_j.
// kCanvas: nz = M + 2, g_{M+1} = <dout, canvas> and dcanvas = s_{M+1} dout, one thread per pixel.
template <int K, bool kCanvas>
__global__ __launch_bounds__(256) void cdna_comp_bwd_tile_k(const float* __restrict__ kern_norm, const float* __restrict__ z,
                                                            const float* __restrict__ zbias, const float* __restrict__ img,
                                                            const float* __restrict__ canvas, const float* __restrict__ dout,
                                                            float* __restrict__ dz, float* __restrict__ dcanvas,
                                                            float* __restrict__ part_n, float* __restrict__ part_b, Geo g) {
  __shared__ float kn[kMaxK * kMaxK * kMaxM];
  __shared__ float win[kWin];
  __shared__ float zb[kMaxZ];
  __shared__ float big[kBig];     // phase 1: g_j, then dz_j, of pixel p at big[j * kPix + p]; phase 2: dd[pixel][mask][colour]
  __shared__ float red[kPix];
  const int b = blockIdx.z, ty = blockIdx.y, tx = blockIdx.x, y0 = ty * kTile, x0 = tx * kTile;
  constexpr int kk = K * K, ww = kTile + K - 1;
  const int nz = g.M + 1 + kCanvas, n = kk * g.M, tid = threadIdx.x;
  if (tid < nz) zb[tid] = zbias ? zbias[tid] : 0.f;
  for (int i = tid; i < n; i += blockDim.x) kn[i] = kern_norm[(long long)b * n + i];
  stage_window(img + (long long)b * g.H * g.W * g.pitch, g.C, g.pitch, y0, x0, g, win);
  __syncthreads();
  const int ly = tid / kTile, lx = tid % kTile;
  const bool inside = y0 + ly < g.H && x0 + lx < g.W;
  // (a thread outside the image works on the last pixel of its row / column and contributes zeros)
  const long long pix = ((long long)b * g.H + min(y0 + ly, g.H - 1)) * g.W + min(x0 + lx, g.W - 1);
  const float* zp = z + pix * nz;
  float d[kMaxC];
#pragma unroll
  for (int i = 0; i < kMaxC; ++i) d[i] = (inside && i < g.C) ? dout[pix * g.C + i] : 0.f;
  float zmax, inv;
  softmax_stats(zp, zb, nz, &zmax, &inv);

  // ---- phase 1: g_j in big[j][pixel], then dz_j
  const float* centre = win + ((ly + g.pad) * ww + lx + g.pad) * g.C;
  float g0 = 0.f;
#pragma unroll
  for (int i = 0; i < kMaxC; ++i)
    if (i < g.C) g0 += d[i] * centre[i];
  big[tid] = g0;
  for (int j = 1; j <= g.M; ++j) big[j * kPix + tid] = 0.f;
  if (kCanvas) {
    const float sc = inside ? weight(zp, zb, g.M + 1, zmax, inv) : 0.f;
    float gc = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxC; ++i)
      if (i < g.C) {
        gc += d[i] * canvas[pix * g.C + i];
        if (inside) dcanvas[pix * g.C + i] = sc * d[i];
      }
    big[(g.M + 1) * kPix + tid] = gc;
  }
  for (int c = 0; c < g.C; ++c) {
    float w[kk];
#pragma unroll
    for (int u = 0; u < K; ++u)
#pragma unroll
      for (int v = 0; v < K; ++v) w[u * K + v] = win[((ly + u) * ww + lx + v) * g.C + c];
    for (int m = 0; m < g.M; ++m) {
      float acc = 0.f;
#pragma unroll
      for (int t = 0; t < kk; ++t) acc += w[t] * kn[t * g.M + m];
      const int q = c * g.M + m, j = q / g.C, i = q - j * g.C;
      float di = 0.f;
#pragma unroll
      for (int ii = 0; ii < kMaxC; ++ii)
        if (ii == i) di = d[ii];
      big[(j + 1) * kPix + tid] += di * acc;
    }
  }
  float gbar = 0.f;
  for (int j = 0; j < nz; ++j) gbar += weight(zp, zb, j, zmax, inv) * big[j * kPix + tid];
  float* dzp = dz + pix * nz;
  for (int j = 0; j < nz; ++j) {
    const float v = inside ? weight(zp, zb, j, zmax, inv) * (big[j * kPix + tid] - gbar) : 0.f;
    big[j * kPix + tid] = v;
    if (inside) dzp[j] = v;
  }
  __syncthreads();
  const long long tile = ((long long)b * g.tiles_y + ty) * g.tiles_x + tx;
  tile_bias_partial(big, red, part_b + tile * nz, nz);

  // ---- phase 2: kernel-gradient partials.  dd[(p*nm + mm)*C + c] = dT_q of pixel p, q = c*M + m0 + mm, for as many masks
  // as fit `big`, then the tap sums shared with cdna_bwd_kern_partial_k
  float* dd = big;
  float* o = part_n + tile * n;
  const int mc = min(g.M, kBig / (kPix * g.C));
  for (int m0 = 0; m0 < g.M; m0 += mc) {
    const int nm = min(mc, g.M - m0);
    __syncthreads();                                 // every read of big (dz sums, previous chunk) is done
    for (int mm = 0; mm < nm; ++mm)
      for (int c = 0; c < g.C; ++c) {
        const int q = c * g.M + m0 + mm, j = q / g.C, i = q - j * g.C;
        float di = 0.f;
#pragma unroll
        for (int ii = 0; ii < kMaxC; ++ii)
          if (ii == i) di = d[ii];                  // (zero outside the image)
        dd[(tid * nm + mm) * g.C + c] = di * weight(zp, zb, j + 1, zmax, inv);
      }
    __syncthreads();
    tile_kernel_partials(win, dd, red, o, K, g.C, g.M, m0, nm);
  }
}

// blocks 0..B-1: the sample's tile partials summed and taken through the normalisation and the relu.  Block B (when dbias
// is wanted): dbias over all the partials of the nz mask channels.
__global__ __launch_bounds__(256) void cdna_comp_bwd_final_k(const float* __restrict__ params, const float* __restrict__ kern_norm,
                                                             const float* __restrict__ part_n, const float* __restrict__ part_b,
                                                             float* __restrict__ dparams, float* __restrict__ dbias, float dbias_acc,
                                                             Geo g, float shift, int nz) {
  __shared__ double scratch[16];
  const int b = blockIdx.x;
  if (b == g.B) {
    final_bias_sum(part_b, dbias, dbias_acc, g.B * g.tiles_x * g.tiles_y, nz, scratch);
    return;
  }
  finish_dparams(params, kern_norm, part_n, dparams, b, g, shift);
}

// ---- the entries, with and without a canvas -------------------------------------------------------------------------
// a canvas takes one of the kMaxZ mask channels: M <= kMaxM - 1
template <bool kCanvas>
int comp_geo(const char* who, int B, int H, int W, int C, int M, int K, int pitch, Geo* g) {
  if (int rc = make_geo(who, B, H, W, C, M, K, pitch, true, g)) return rc;
  ACG_REQUIRE(!kCanvas || M + 2 <= kMaxZ, ACG_ERR_UNSUPPORTED, "%s: supports masks <= %d beside a canvas", who, kMaxZ - 2);
  return ACG_OK;
}

template <bool kCanvas>
size_t comp_workspace(const char* who, int B, int H, int W, int C, int M, int K) {
  Geo g;
  if (comp_geo<kCanvas>(who, B, H, W, C, M, K, 0, &g) != ACG_OK) return 0;
  return (partials(g) + (size_t)B * g.tiles_x * g.tiles_y * (M + 1 + kCanvas)) * sizeof(float);
}

template <bool kCanvas>
int comp_fwd(const char* who, const float* params, const float* z, const float* zbias, const float* image, int pitch,
             const float* canvas, float* out, float* kern_norm, int B, int H, int W, int C, int M, int K, float shift,
             acg_stream_t stream) {
  Geo g;
  if (int rc = comp_geo<kCanvas>(who, B, H, W, C, M, K, pitch, &g)) return rc;
  ACG_REQUIRE(params && z && image && out && (!kCanvas || canvas), ACG_ERR_INVALID_ARG, "%s: null pointer", who);
  const dim3 grid(g.tiles_x, g.tiles_y, B);
  hipStream_t st = acg::to_stream(stream);
  if (K == 3) ACG_LAUNCH((cdna_comp_fwd_k<3, kCanvas>), grid, dim3(256), 0, st, params, z, zbias, image, canvas, out, kern_norm, g, shift);
  else if (K == 5) ACG_LAUNCH((cdna_comp_fwd_k<5, kCanvas>), grid, dim3(256), 0, st, params, z, zbias, image, canvas, out, kern_norm, g, shift);
  else ACG_LAUNCH((cdna_comp_fwd_k<7, kCanvas>), grid, dim3(256), 0, st, params, z, zbias, image, canvas, out, kern_norm, g, shift);
  return acg::check_launch(who);
}

template <bool kCanvas>
int comp_bwd(const char* who, const float* params, const float* kern_norm, const float* z, const float* zbias, const float* image,
             int pitch, const float* canvas, const float* dout, float* dparams, float* dz, float* dbias, float dbias_acc,
             float* dcanvas, int B, int H, int W, int C, int M, int K, float shift, void* ws, size_t wsb, acg_stream_t stream) {
  Geo g;
  if (int rc = comp_geo<kCanvas>(who, B, H, W, C, M, K, pitch, &g)) return rc;
  ACG_REQUIRE(params && kern_norm && z && image && dout && dparams && dz && (!kCanvas || (canvas && dcanvas)), ACG_ERR_INVALID_ARG,
              "%s: null pointer", who);
  ACG_REQUIRE(ws && wsb >= comp_workspace<kCanvas>(who, B, H, W, C, M, K), ACG_ERR_WORKSPACE, "%s: workspace too small", who);
  hipStream_t st = acg::to_stream(stream);
  float* part_n = (float*)ws;
  float* part_b = part_n + partials(g);
  const dim3 grid(g.tiles_x, g.tiles_y, B);
  if (K == 3) ACG_LAUNCH((cdna_comp_bwd_tile_k<3, kCanvas>), grid, dim3(256), 0, st, kern_norm, z, zbias, image, canvas, dout, dz, dcanvas, part_n, part_b, g);
  else if (K == 5) ACG_LAUNCH((cdna_comp_bwd_tile_k<5, kCanvas>), grid, dim3(256), 0, st, kern_norm, z, zbias, image, canvas, dout, dz, dcanvas, part_n, part_b, g);
  else ACG_LAUNCH((cdna_comp_bwd_tile_k<7, kCanvas>), grid, dim3(256), 0, st, kern_norm, z, zbias, image, canvas, dout, dz, dcanvas, part_n, part_b, g);
  if (int rc = acg::check_launch((std::string(who) + " tile").c_str())) return rc;
  ACG_LAUNCH(cdna_comp_bwd_final_k, dim3(B + (dbias ? 1 : 0)), dim3(256), 0, st, params, kern_norm, (const float*)part_n,
             (const float*)part_b, dparams, dbias, dbias_acc, g, shift, M + 1 + kCanvas);
  return acg::check_launch((std::string(who) + " final").c_str());
}

}  // namespace

extern "C" {

size_t acg_cdna_composite_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t M, int32_t K) {
  return comp_workspace<false>("cdna_composite_workspace_bytes", B, H, W, C, M, K);
}

int32_t acg_cdna_composite_fwd(const float* params, const float* mask_logits, const float* mask_bias, const float* image,
                               int32_t image_pitch, float* out, float* kern_norm, int32_t B, int32_t H, int32_t W, int32_t C,
                               int32_t M, int32_t K, float relu_shift, acg_stream_t stream) {
  return comp_fwd<false>("cdna_composite_fwd", params, mask_logits, mask_bias, image, image_pitch, nullptr, out, kern_norm, B, H, W, C,
                         M, K, relu_shift, stream);
}

int32_t acg_cdna_composite_bwd(const float* params, const float* kern_norm, const float* mask_logits, const float* mask_bias,
                               const float* image, int32_t image_pitch, const float* dout, float* dparams, float* dmask_logits,
                               float* dmask_bias, float dmask_bias_accumulate, int32_t B, int32_t H, int32_t W, int32_t C,
                               int32_t M, int32_t K, float relu_shift, void* ws, size_t wsb, acg_stream_t stream) {
  return comp_bwd<false>("cdna_composite_bwd", params, kern_norm, mask_logits, mask_bias, image, image_pitch, nullptr, dout, dparams,
                         dmask_logits, dmask_bias, dmask_bias_accumulate, nullptr, B, H, W, C, M, K, relu_shift, ws, wsb, stream);
}

size_t acg_cdna_composite_canvas_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t M, int32_t K) {
  return comp_workspace<true>("cdna_composite_canvas_workspace_bytes", B, H, W, C, M, K);
}

int32_t acg_cdna_composite_canvas_fwd(const float* params, const float* mask_logits, const float* mask_bias, const float* image,
                                      int32_t image_pitch, const float* canvas, float* out, float* kern_norm, int32_t B, int32_t H,
                                      int32_t W, int32_t C, int32_t M, int32_t K, float relu_shift, acg_stream_t stream) {
  return comp_fwd<true>("cdna_composite_canvas_fwd", params, mask_logits, mask_bias, image, image_pitch, canvas, out, kern_norm, B, H, W,
                        C, M, K, relu_shift, stream);
}

int32_t acg_cdna_composite_canvas_bwd(const float* params, const float* kern_norm, const float* mask_logits, const float* mask_bias,
                                      const float* image, int32_t image_pitch, const float* canvas, const float* dout, float* dparams,
                                      float* dmask_logits, float* dmask_bias, float dmask_bias_accumulate, float* dcanvas, int32_t B,
                                      int32_t H, int32_t W, int32_t C, int32_t M, int32_t K, float relu_shift, void* ws, size_t wsb,
                                      acg_stream_t stream) {
  return comp_bwd<true>("cdna_composite_canvas_bwd", params, kern_norm, mask_logits, mask_bias, image, image_pitch, canvas, dout, dparams,
                        dmask_logits, dmask_bias, dmask_bias_accumulate, dcanvas, B, H, W, C, M, K, relu_shift, ws, wsb, stream);
}

}  // extern "C"
