// Fused affine warp-and-composite (include/acgan_cdna.h): the output stage of the affine (STP) generator.  Each of the M
// masks moves the image by a 2x3 affine transform sampled bilinearly with zeros outside; the M warped images are folded
// straight into the softmax-weighted composite and never reach HBM.
//
// Where the taps are read from: global memory, with a bounds check per tap, for every theta.  A sample image is 48 KiB
// (64x64) or 192 KiB (128x128) and is read by all M masks of all its tiles, so the taps hit L1 / L2; near the identity - the
// trained case - a wave's 64 pixels read 4 runs of 16 neighbouring pixels per tap.  Staging the source box of a (tile, mask)
// in LDS first (the bounding box of the tile's mapped corners, where it fits a 32x32 window) was built and measured: it was
// 1.3x to 1.6x slower forward and 1.15x to 1.25x slower backward at (32, 64x64) and (32, 128x128), M = 10 - the two barriers
// and the staging loads per mask cost more than the LDS reads save (DESIGN.md has the times) - and it needs a second path
// anyway, since any theta is legal.  One path, no LDS window.
//
// No index is formed from an unchecked coordinate: px, py are range-checked in float ((-1, W) x (-1, H), false for NaN)
// before the conversion to int, and every tap is checked against the image before its address is formed.
//
// Backward: the warps are recomputed.  The tile pass writes dmask_logits and leaves per-(sample, tile) partials of dparams
// (6 values per mask: wave shuffles, then the 4 waves in order) and of the bias gradient (cdna_common.h) in the workspace;
// the final pass sums them in tile order.  No atomics.
//
// kCanvas (the acg_affine_composite_canvas_* entries): one more candidate behind the M warped images, a canvas [B,H,W,C]
// under mask channel M+1, read once per pixel and folded where s_0 * image is; backward, g_{M+1} = <dout, canvas> and
// dcanvas = s_{M+1} dout by the pixel's thread.  The instantiations without it are the kernels as they were.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/acgan_cdna.h"
#include "cdna_common.h"
#include "common.h"

namespace {

using namespace acg_cdna;

constexpr int kTheta = 6;

// source coordinates, in pixels, of output pixel (x, y) under theta t[6]
__device__ __forceinline__ void affine_map(const float* t, float x, float y, int H, int W, float* px, float* py) {
  const float u = 2.f * x / (float)(W - 1) - 1.f, v = 2.f * y / (float)(H - 1) - 1.f;
  const float xs = t[0] * u + t[1] * v + t[2], ys = t[3] * u + t[4] * v + t[5];
  *px = (xs + 1.f) * (0.5f * (float)(W - 1));
  *py = (ys + 1.f) * (0.5f * (float)(H - 1));
}

// theta of sample b into LDS: th[m*6 + i] = params + (1, 0, 0, 0, 1, 0)
__device__ __forceinline__ void stage_theta(const float* __restrict__ params, int b, int M, float* th) {
  const int n = M * kTheta;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int k = i % kTheta;
    th[i] = params[(long long)b * n + i] + ((k == 0 || k == 4) ? 1.f : 0.f);
  }
}

// T[c] = the bilinear sample of the image at (px, py) and, with kGrad, its derivatives Tx, Ty with respect to px, py in the
// cell floor selects.  All zero unless -1 < px < W and -1 < py < H; a tap outside the image is 0.
template <bool kGrad>
__device__ __forceinline__ void sample(const float* __restrict__ src, const Geo& g, float px, float py, float (&T)[kMaxC],
                                       float (&Tx)[kMaxC], float (&Ty)[kMaxC]) {
#pragma unroll
  for (int c = 0; c < kMaxC; ++c) T[c] = Tx[c] = Ty[c] = 0.f;
  if (!(px > -1.f && px < (float)g.W && py > -1.f && py < (float)g.H)) return;
  const float fx0 = floorf(px), fy0 = floorf(py);
  const int xi = (int)fx0, yi = (int)fy0;                               // in [-1, W-1], [-1, H-1]
  const float fx = px - fx0, fy = py - fy0;
  float v[2][2][kMaxC];
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int X = xi + dx, Y = yi + dy;
      if (X >= 0 && X < g.W && Y >= 0 && Y < g.H) {
        const float* s = src + ((long long)Y * g.W + X) * g.pitch;
#pragma unroll
        for (int c = 0; c < kMaxC; ++c) v[dy][dx][c] = c < g.C ? s[c] : 0.f;
      } else {
#pragma unroll
        for (int c = 0; c < kMaxC; ++c) v[dy][dx][c] = 0.f;
      }
    }
  const float gx = 1.f - fx, gy = 1.f - fy;
#pragma unroll
  for (int c = 0; c < kMaxC; ++c) {
    T[c] = gy * (gx * v[0][0][c] + fx * v[0][1][c]) + fy * (gx * v[1][0][c] + fx * v[1][1][c]);
    if (kGrad) {
      Tx[c] = gy * (v[0][1][c] - v[0][0][c]) + fy * (v[1][1][c] - v[1][0][c]);
      Ty[c] = gx * (v[1][0][c] - v[0][0][c]) + fx * (v[1][1][c] - v[0][1][c]);
    }
  }
}

template <bool kCanvas>
__global__ __launch_bounds__(256) void affine_comp_fwd_k(const float* __restrict__ params, const float* __restrict__ z,
                                                         const float* __restrict__ zbias, const float* __restrict__ img,
                                                         const float* __restrict__ canvas, float* __restrict__ out, Geo g) {
  __shared__ float th[kMaxM * kTheta];
  __shared__ float zb[kMaxZ];
  const int b = blockIdx.z, y0 = blockIdx.y * kTile, x0 = blockIdx.x * kTile, nz = g.M + 1 + kCanvas, tid = threadIdx.x;
  if (tid < nz) zb[tid] = zbias ? zbias[tid] : 0.f;
  stage_theta(params, b, g.M, th);
  __syncthreads();
  const int ly = tid / kTile, lx = tid % kTile;
  const bool inside = y0 + ly < g.H && x0 + lx < g.W;
  // (a thread outside the image works on the last pixel of its row / column and writes nothing)
  const int y = min(y0 + ly, g.H - 1), x = min(x0 + lx, g.W - 1);
  const long long pix = ((long long)b * g.H + y) * g.W + x;
  const float* src = img + (long long)b * g.H * g.W * g.pitch;
  const float* zp = z + pix * nz;
  float zmax, inv;
  softmax_stats(zp, zb, nz, &zmax, &inv);
  const float s0 = weight(zp, zb, 0, zmax, inv);
  const float* centre = src + ((long long)y * g.W + x) * g.pitch;
  float f[kMaxC];
#pragma unroll
  for (int i = 0; i < kMaxC; ++i) f[i] = i < g.C ? s0 * centre[i] : 0.f;
  if (kCanvas) {
    const float sc = weight(zp, zb, g.M + 1, zmax, inv);
#pragma unroll
    for (int i = 0; i < kMaxC; ++i)
      if (i < g.C) f[i] += sc * canvas[pix * g.C + i];
  }
  for (int m = 0; m < g.M; ++m) {
    float px, py, T[kMaxC], Tx[kMaxC], Ty[kMaxC];
    affine_map(th + m * kTheta, (float)x, (float)y, g.H, g.W, &px, &py);
    sample<false>(src, g, px, py, T, Tx, Ty);
    const float s = weight(zp, zb, m + 1, zmax, inv);
#pragma unroll
    for (int i = 0; i < kMaxC; ++i) f[i] += s * T[i];
  }
  if (!inside) return;
  float* o = out + pix * g.C;
#pragma unroll
  for (int i = 0; i < kMaxC; ++i)
    if (i < g.C) o[i] = f[i];
}

// The tile pass of the backward: dz for every pixel; part_p[b][tile][m*6 + i] = the tile's sum of s_{m+1} * (a u, a v, a,
// b u, b v, b); part_b[b][tile][j] = the tile's sum of dz_j.  Dynamic LDS: big[nz * 256], nz = M + 1 mask channels.
// kCanvas: nz = M + 2, g_{M+1} = <dout, canvas> and dcanvas = s_{M+1} dout, one thread per pixel.
template <bool kCanvas>
__global__ __launch_bounds__(256) void affine_comp_bwd_tile_k(const float* __restrict__ params, const float* __restrict__ z,
                                                              const float* __restrict__ zbias, const float* __restrict__ img,
                                                              const float* __restrict__ canvas, const float* __restrict__ dout,
                                                              float* __restrict__ dz, float* __restrict__ dcanvas,
                                                              float* __restrict__ part_p, float* __restrict__ part_b, Geo g) {
  __shared__ float th[kMaxM * kTheta];
  __shared__ float zb[kMaxZ];
  __shared__ float red[kPix];
  __shared__ float wred[4 * kMaxM * kTheta];      // per wave: the 6 sums of every mask
  extern __shared__ float big[];                  // g_j, then dz_j, of pixel p at big[j * kPix + p]
  const int b = blockIdx.z, ty = blockIdx.y, tx = blockIdx.x, y0 = ty * kTile, x0 = tx * kTile;
  const int nz = g.M + 1 + kCanvas, n = g.M * kTheta, tid = threadIdx.x;
  if (tid < nz) zb[tid] = zbias ? zbias[tid] : 0.f;
  stage_theta(params, b, g.M, th);
  __syncthreads();
  const int ly = tid / kTile, lx = tid % kTile;
  const bool inside = y0 + ly < g.H && x0 + lx < g.W;
  // (a thread outside the image works on the last pixel of its row / column and contributes zeros)
  const int y = min(y0 + ly, g.H - 1), x = min(x0 + lx, g.W - 1);
  const long long pix = ((long long)b * g.H + y) * g.W + x;
  const float* src = img + (long long)b * g.H * g.W * g.pitch;
  const float* zp = z + pix * nz;
  float d[kMaxC];
#pragma unroll
  for (int i = 0; i < kMaxC; ++i) d[i] = (inside && i < g.C) ? dout[pix * g.C + i] : 0.f;
  float zmax, inv;
  softmax_stats(zp, zb, nz, &zmax, &inv);
  const float* centre = src + ((long long)y * g.W + x) * g.pitch;
  float g0 = 0.f;
#pragma unroll
  for (int i = 0; i < kMaxC; ++i)
    if (i < g.C) g0 += d[i] * centre[i];
  big[tid] = g0;
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
  const float u = 2.f * (float)x / (float)(g.W - 1) - 1.f, v = 2.f * (float)y / (float)(g.H - 1) - 1.f;
  const float half_w = 0.5f * (float)(g.W - 1), half_h = 0.5f * (float)(g.H - 1);
  const int lane = tid & 63, wave = tid >> 6;
  for (int m = 0; m < g.M; ++m) {
    float px, py, T[kMaxC], Tx[kMaxC], Ty[kMaxC];
    affine_map(th + m * kTheta, (float)x, (float)y, g.H, g.W, &px, &py);
    sample<true>(src, g, px, py, T, Tx, Ty);
    float gj = 0.f, a = 0.f, bb = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxC; ++i) {                // (d is zero outside the image and beyond C)
      gj += d[i] * T[i];
      a += d[i] * Tx[i];
      bb += d[i] * Ty[i];
    }
    big[(m + 1) * kPix + tid] = gj;
    const float s = weight(zp, zb, m + 1, zmax, inv);
    a *= s * half_w;
    bb *= s * half_h;
    const float vals[kTheta] = {a * u, a * v, a, bb * u, bb * v, bb};
#pragma unroll
    for (int i = 0; i < kTheta; ++i) {
      const float r = acg::wave_sum(vals[i]);
      if (lane == 0) wred[wave * (kMaxM * kTheta) + m * kTheta + i] = r;
    }
  }
  float gbar = 0.f;
  for (int j = 0; j < nz; ++j) gbar += weight(zp, zb, j, zmax, inv) * big[j * kPix + tid];
  float* dzp = dz + pix * nz;
  for (int j = 0; j < nz; ++j) {
    const float w = inside ? weight(zp, zb, j, zmax, inv) * (big[j * kPix + tid] - gbar) : 0.f;
    big[j * kPix + tid] = w;
    if (inside) dzp[j] = w;
  }
  __syncthreads();
  const long long tile = ((long long)b * g.tiles_y + ty) * g.tiles_x + tx;
  tile_bias_partial(big, red, part_b + tile * nz, nz);
  // the 4 waves in order
  constexpr int ws = kMaxM * kTheta;
  if (tid < n) part_p[tile * n + tid] = wred[tid] + wred[ws + tid] + wred[2 * ws + tid] + wred[3 * ws + tid];
}

// blocks 0..B-1: the sample's tile partials of dparams summed in tile order.  Block B (when dbias is wanted): dbias over all
// the partials.
__global__ __launch_bounds__(256) void affine_comp_bwd_final_k(const float* __restrict__ part_p, const float* __restrict__ part_b,
                                                               float* __restrict__ dparams, float* __restrict__ dbias,
                                                               float dbias_acc, Geo g, int nz) {
  __shared__ double scratch[16];
  const int b = blockIdx.x, ntile = g.tiles_x * g.tiles_y, n = g.M * kTheta;
  if (b == g.B) {
    final_bias_sum(part_b, dbias, dbias_acc, g.B * ntile, nz, scratch);
    return;
  }
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    double s = 0.0;
    for (int t = 0; t < ntile; ++t) s += part_p[((long long)b * ntile + t) * n + i];
    dparams[(long long)b * n + i] = (float)s;
  }
}

// (a canvas takes one of the kMaxZ mask channels: M <= kMaxM - 1)
template <bool kCanvas>
int affine_geo(const char* who, int B, int H, int W, int C, int M, int pitch, Geo* g) {
  if (int rc = make_geo(who, B, H, W, C, M, 1, pitch, false, g)) return rc;          // (K = 1: no halo)
  ACG_REQUIRE(H >= 2 && W >= 2, ACG_ERR_UNSUPPORTED, "%s: needs H, W >= 2 (got %d x %d)", who, H, W);
  ACG_REQUIRE(!kCanvas || M + 2 <= kMaxZ, ACG_ERR_UNSUPPORTED, "%s: supports masks <= %d beside a canvas", who, kMaxZ - 2);
  return ACG_OK;
}

size_t dparam_partials(const Geo& g) { return (size_t)g.B * g.tiles_x * g.tiles_y * g.M * kTheta; }

// ---- the entries, with and without a canvas -------------------------------------------------------------------------
template <bool kCanvas>
size_t comp_workspace(const char* who, int B, int H, int W, int C, int M) {
  Geo g;
  if (affine_geo<kCanvas>(who, B, H, W, C, M, 0, &g) != ACG_OK) return 0;
  return (dparam_partials(g) + (size_t)B * g.tiles_x * g.tiles_y * (M + 1 + kCanvas)) * sizeof(float);
}

template <bool kCanvas>
int comp_fwd(const char* who, const float* params, const float* z, const float* zbias, const float* image, int pitch,
             const float* canvas, float* out, int B, int H, int W, int C, int M, acg_stream_t stream) {
  Geo g;
  if (int rc = affine_geo<kCanvas>(who, B, H, W, C, M, pitch, &g)) return rc;
  ACG_REQUIRE(params && z && image && out && (!kCanvas || canvas), ACG_ERR_INVALID_ARG, "%s: null pointer", who);
  ACG_LAUNCH(affine_comp_fwd_k<kCanvas>, dim3(g.tiles_x, g.tiles_y, B), dim3(256), 0, acg::to_stream(stream), params, z, zbias, image,
             canvas, out, g);
  return acg::check_launch(who);
}

template <bool kCanvas>
int comp_bwd(const char* who, const float* params, const float* z, const float* zbias, const float* image, int pitch,
             const float* canvas, const float* dout, float* dparams, float* dz, float* dbias, float dbias_acc, float* dcanvas, int B,
             int H, int W, int C, int M, void* ws, size_t wsb, acg_stream_t stream) {
  Geo g;
  if (int rc = affine_geo<kCanvas>(who, B, H, W, C, M, pitch, &g)) return rc;
  ACG_REQUIRE(params && z && image && dout && dparams && dz && (!kCanvas || (canvas && dcanvas)), ACG_ERR_INVALID_ARG,
              "%s: null pointer", who);
  ACG_REQUIRE(ws && wsb >= comp_workspace<kCanvas>(who, B, H, W, C, M), ACG_ERR_WORKSPACE, "%s: workspace too small", who);
  hipStream_t st = acg::to_stream(stream);
  float* part_p = (float*)ws;
  float* part_b = part_p + dparam_partials(g);
  ACG_LAUNCH(affine_comp_bwd_tile_k<kCanvas>, dim3(g.tiles_x, g.tiles_y, B), dim3(256), (size_t)(M + 1 + kCanvas) * kPix * sizeof(float),
             st, params, z, zbias, image, canvas, dout, dz, dcanvas, part_p, part_b, g);
  if (int rc = acg::check_launch((std::string(who) + " tile").c_str())) return rc;
  ACG_LAUNCH(affine_comp_bwd_final_k, dim3(B + (dbias ? 1 : 0)), dim3(256), 0, st, (const float*)part_p, (const float*)part_b,
             dparams, dbias, dbias_acc, g, M + 1 + kCanvas);
  return acg::check_launch((std::string(who) + " final").c_str());
}

}  // namespace

extern "C" {

size_t acg_affine_composite_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t M) {
  return comp_workspace<false>("affine_composite_workspace_bytes", B, H, W, C, M);
}

int32_t acg_affine_composite_fwd(const float* params, const float* mask_logits, const float* mask_bias, const float* image,
                                 int32_t image_pitch, float* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t M,
                                 acg_stream_t stream) {
  return comp_fwd<false>("affine_composite_fwd", params, mask_logits, mask_bias, image, image_pitch, nullptr, out, B, H, W, C, M, stream);
}

int32_t acg_affine_composite_bwd(const float* params, const float* mask_logits, const float* mask_bias, const float* image,
                                 int32_t image_pitch, const float* dout, float* dparams, float* dmask_logits, float* dmask_bias,
                                 float dmask_bias_accumulate, int32_t B, int32_t H, int32_t W, int32_t C, int32_t M, void* ws,
                                 size_t wsb, acg_stream_t stream) {
  return comp_bwd<false>("affine_composite_bwd", params, mask_logits, mask_bias, image, image_pitch, nullptr, dout, dparams, dmask_logits,
                         dmask_bias, dmask_bias_accumulate, nullptr, B, H, W, C, M, ws, wsb, stream);
}

size_t acg_affine_composite_canvas_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t M) {
  return comp_workspace<true>("affine_composite_canvas_workspace_bytes", B, H, W, C, M);
}

int32_t acg_affine_composite_canvas_fwd(const float* params, const float* mask_logits, const float* mask_bias, const float* image,
                                        int32_t image_pitch, const float* canvas, float* out, int32_t B, int32_t H, int32_t W,
                                        int32_t C, int32_t M, acg_stream_t stream) {
  return comp_fwd<true>("affine_composite_canvas_fwd", params, mask_logits, mask_bias, image, image_pitch, canvas, out, B, H, W, C, M,
                        stream);
}

int32_t acg_affine_composite_canvas_bwd(const float* params, const float* mask_logits, const float* mask_bias, const float* image,
                                        int32_t image_pitch, const float* canvas, const float* dout, float* dparams,
                                        float* dmask_logits, float* dmask_bias, float dmask_bias_accumulate, float* dcanvas, int32_t B,
                                        int32_t H, int32_t W, int32_t C, int32_t M, void* ws, size_t wsb, acg_stream_t stream) {
  return comp_bwd<true>("affine_composite_canvas_bwd", params, mask_logits, mask_bias, image, image_pitch, canvas, dout, dparams,
                        dmask_logits, dmask_bias, dmask_bias_accumulate, dcanvas, B, H, W, C, M, ws, wsb, stream);
}

}  // extern "C"
