// Gradients of the K-step rollout trainer (include/acgan_rollout.h): the DNA tail's image gradient and the gradient of a
// tiled action vector.  Neither uses atomics; every output element has one writer that sums in a fixed order.
//
// Image gradient.  dimage[y,x] gathers, over the k*k taps (i, j), the softmax weight of tap (i, j) at the SOURCE pixel
// (y+p-i, x+p-j) times that pixel's output gradient.  A block owns a 32 x 32 tile of one image.  Phase A stages, for the
// tile and its (k-1)-pixel halo, each source pixel's softmax maximum and 1/denominator and its output gradient (dout plus
// the frame's channels of d(discriminator input)) in LDS: (32+k-1)^2 * (2 + 4) floats, 31 KB at k = 5 and 42 KB at
// k = 11, so the whole softmax row of a pixel never has to sit in LDS.  Phase B walks the taps of the block's pixels; each
// logit is read exactly once there (a source pixel's tap (i, j) belongs to one output pixel).  Logits are read twice in
// all: the stats pass (tile plus halo: 1.27x the tile at k = 5, 1.72x at k = 11) and the gather.
#include <hip/hip_runtime.h>
#include "../../include/acgan_rollout.h"
#include "common.h"

namespace {

constexpr int RT = 32;    // output tile: RT x RT pixels
constexpr int NTH = 256;  // 8 rows of 32 threads; each thread covers RT / 8 = 4 rows of the tile

struct Grad2 {            // the frame's channels of d(discriminator input), added to dout (ptr == nullptr: none)
  const void* ptr;
  int pitch, off, half;
};

__device__ __forceinline__ float grad2_load(const Grad2& g2, long long pix, int c) {
  return g2.half ? (float)reinterpret_cast<const __bf16*>(g2.ptr)[pix * g2.pitch + g2.off + c]
                 : reinterpret_cast<const float*>(g2.ptr)[pix * g2.pitch + g2.off + c];
}

// CC: compile-time channel count (3 = RGB) or 0 = runtime C
template <int K, int CC>
__global__ __launch_bounds__(NTH) void dna_dimage_kernel(const float* __restrict__ logits, const float* __restrict__ bias,
                                                         const float* __restrict__ dout, const Grad2 g2, float* __restrict__ dimage,
                                                         float acc, int H, int W, int Crt) {
  constexpr int KK = K * K, P = (K - 1) / 2, RS = RT + K - 1, NR = RS * RS;
  __shared__ float smax[NR], sinv[NR];
  __shared__ __attribute__((aligned(16))) float sg[NR * 4];
  __shared__ float bs[KK];
  const int C = CC ? CC : Crt;
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * RT, y0 = blockIdx.y * RT, b = blockIdx.z;
  const int ry0 = y0 + P - (K - 1), rx0 = x0 + P - (K - 1);     // the source region: tile rows y - p .. y + k - 1 - p
  for (int t = tid; t < KK; t += NTH) bs[t] = bias ? bias[t] : 0.f;
  __syncthreads();

  // phase A: softmax statistics and output gradient of every source pixel of the region (zero outside the image)
  for (int idx = tid; idx < NR; idx += NTH) {
    const int ly = idx / RS, lx = idx - ly * RS;
    const int gy = ry0 + ly, gx = rx0 + lx;
    float mx = 0.f, inv = 0.f, g[4] = {0.f, 0.f, 0.f, 0.f};
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const long long pix = ((long long)b * H + gy) * W + gx;
      const float* lp = logits + pix * KK;
      mx = -3.0e38f;
#pragma unroll 11
      for (int t = 0; t < KK; ++t) mx = fmaxf(mx, lp[t] + bs[t]);
      float den = 0.f;
#pragma unroll 11
      for (int t = 0; t < KK; ++t) den += __expf(lp[t] + bs[t] - mx);
      inv = 1.f / den;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) g[c] = dout[pix * C + c] + (g2.ptr ? grad2_load(g2, pix, c) : 0.f);
    }
    smax[idx] = mx;
    sinv[idx] = inv;
#pragma unroll
    for (int c = 0; c < 4; ++c) sg[idx * 4 + c] = g[c];
  }
  __syncthreads();

  // phase B: the gather, one output pixel per thread and row step
  const int tx = tid & (RT - 1), ty = tid / RT;
  const int x = x0 + tx;
  if (x >= W) return;
#pragma unroll
  for (int r = 0; r < RT / (NTH / RT); ++r) {
    const int yl = ty + r * (NTH / RT), y = y0 + yl;
    if (y >= H) break;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < K; ++i) {
      const int ly = yl + K - 1 - i, gy = ry0 + ly;              // source row y + p - i
      if (gy < 0 || gy >= H) continue;
      const float* lrow = logits + ((long long)b * H + gy) * W * KK;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const int lx = tx + K - 1 - j, gx = rx0 + lx;            // source column x + p - j
        if (gx < 0 || gx >= W) continue;
        const int idx = ly * RS + lx, t = i * K + j;
        const float wt = __expf(lrow[(long long)gx * KK + t] + bs[t] - smax[idx]) * sinv[idx];
        const float* gp = sg + idx * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < C) a[c] += wt * gp[c];
      }
    }
    float* o = dimage + (((long long)b * H + y) * W + x) * C;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) o[c] = (acc != 0.f ? acc * o[c] : 0.f) + a[c];
  }
}

template <int K>
int launch_k(const float* logits, const float* bias, const float* dout, const Grad2& g2, float* dimage, float acc, int B, int H,
             int W, int C, hipStream_t st) {
  const dim3 grid((W + RT - 1) / RT, (H + RT - 1) / RT, B);
  if (C == 3) ACG_LAUNCH((dna_dimage_kernel<K, 3>), grid, dim3(NTH), 0, st, logits, bias, dout, g2, dimage, acc, H, W, C);
  else ACG_LAUNCH((dna_dimage_kernel<K, 0>), grid, dim3(NTH), 0, st, logits, bias, dout, g2, dimage, acc, H, W, C);
  return acg::check_launch("dna_bwd_image");
}

// dact[q, a] over the rows r with (r / div) % mod == q.  The k-th such row is r = (q + (k / div) * mod) * div + k % div;
// lane l of a channel sums k = l, l + L, ... and lane sums are added in lane order: a fixed order, no atomics.
__global__ __launch_bounds__(256) void action_grad_kernel(const float* __restrict__ dcat, long long rows, int pitch, int c_off, int n,
                                                          int div, int mod, float* __restrict__ dact, float acc) {
  __shared__ double sh[256];
  const int q = blockIdx.x, tid = threadIdx.x;
  const long long nblk = (rows + div - 1) / div;                      // row blocks of div rows; block m belongs to m % mod
  const long long mine = nblk > q ? (nblk - q + mod - 1) / mod : 0;
  const long long cnt = mine * div;
  for (int a0 = 0; a0 < n; a0 += 256) {
    const int na = min(256, n - a0), L = 256 / na;
    const int a = a0 + tid % na, lane = tid / na;
    double s = 0.0;
    if (lane < L) {
      for (long long k = lane; k < cnt; k += L) {
        const long long r = (q + (k / div) * (long long)mod) * div + k % div;
        if (r < rows) s += dcat[r * pitch + c_off + a];
      }
    }
    sh[tid] = s;
    __syncthreads();
    if (tid < na) {
      double tot = 0.0;
      for (int l = 0; l < L; ++l) tot += sh[l * na + tid];
      float* o = dact + (long long)q * n + a0 + tid;
      *o = (acc != 0.f ? acc * *o : 0.f) + (float)tot;
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" {

int32_t acg_dna_bwd_image(const void* logits, const float* bias, const float* dout, const void* dout2, int32_t dout2_pitch,
                          int32_t dout2_offset, int32_t dout2_dtype, float* dimage, float acc, int32_t B, int32_t H, int32_t W,
                          int32_t C, int32_t k, int32_t dtype, acg_stream_t stream) {
  ACG_REQUIRE(dtype == ACG_F32, ACG_ERR_UNSUPPORTED, "dna_bwd_image: logits dtype %d (float32 only)", dtype);
  ACG_REQUIRE(B > 0 && H > 0 && W > 0, ACG_ERR_INVALID_ARG, "dna_bwd_image: non-positive size");
  ACG_REQUIRE(C >= 1 && C <= 4, ACG_ERR_INVALID_ARG, "dna_bwd_image: channels %d outside 1..4", C);
  ACG_REQUIRE(k >= 1 && k <= 11, ACG_ERR_UNSUPPORTED, "dna_bwd_image: ksize %d outside 1..11", k);
  ACG_REQUIRE(B <= 65535, ACG_ERR_UNSUPPORTED, "dna_bwd_image: grid too large");
  ACG_REQUIRE(logits && dout && dimage, ACG_ERR_INVALID_ARG, "dna_bwd_image: null pointer");
  Grad2 g2{dout2, dout2_pitch, dout2_offset, dout2_dtype == ACG_BF16};
  if (dout2) {
    ACG_REQUIRE(dout2_dtype == ACG_F32 || dout2_dtype == ACG_BF16, ACG_ERR_UNSUPPORTED, "dna_bwd_image: dout2 dtype %d", dout2_dtype);
    ACG_REQUIRE(dout2_offset >= 0 && dout2_pitch >= dout2_offset + C, ACG_ERR_INVALID_ARG,
                "dna_bwd_image: dout2: %d channels at offset %d do not fit pitch %d", C, dout2_offset, dout2_pitch);
  }
  hipStream_t st = acg::to_stream(stream);
  const float* lg = (const float*)logits;
  switch (k) {
#define ACG_DIMAGE_CASE(KV) case KV: return launch_k<KV>(lg, bias, dout, g2, dimage, acc, B, H, W, C, st);
    ACG_DIMAGE_CASE(1) ACG_DIMAGE_CASE(2) ACG_DIMAGE_CASE(3) ACG_DIMAGE_CASE(4) ACG_DIMAGE_CASE(5) ACG_DIMAGE_CASE(6)
    ACG_DIMAGE_CASE(7) ACG_DIMAGE_CASE(8) ACG_DIMAGE_CASE(9) ACG_DIMAGE_CASE(10) ACG_DIMAGE_CASE(11)
#undef ACG_DIMAGE_CASE
    default: return acg::fail(ACG_ERR_UNSUPPORTED, "dna_bwd_image: ksize %d", k);
  }
}

int32_t acg_action_grad(const float* dcat, int64_t rows, int32_t pitch, int32_t c_off, int32_t n, int32_t div, int32_t mod, float* dact,
                        float acc, acg_stream_t stream) {
  ACG_REQUIRE(dcat && dact, ACG_ERR_INVALID_ARG, "action_grad: null pointer");
  ACG_REQUIRE(rows > 0 && n > 0 && div > 0 && mod > 0, ACG_ERR_INVALID_ARG, "action_grad: non-positive size");
  ACG_REQUIRE(c_off >= 0 && pitch >= c_off + n, ACG_ERR_INVALID_ARG, "action_grad: %d channels at offset %d do not fit pitch %d", n, c_off,
              pitch);
  ACG_LAUNCH(action_grad_kernel, dim3(mod), dim3(256), 0, acg::to_stream(stream), dcat, (long long)rows, pitch, c_off, n, div, mod, dact,
             acc);
  return acg::check_launch("action_grad");
}

}  // extern "C"
