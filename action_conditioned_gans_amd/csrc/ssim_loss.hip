// SSIM as a training loss (include/acgan_ssim_loss.h): sum_n (1 - SSIM_n) and its gradient with respect to the prediction.
//
// Two launches for the gradient, a third small one when the value is asked for:
//
// 1. ssim_maps_k - the windowed-moments pass of ssim_window.h (one block = one frame x one strip of <= 64 map columns x one band
//    of map rows, one wave per channel, lane = map column).  A finished position is turned into its SSIM value S and into the
//    three maps of the gradient
//        M0 = U - 2 a' Pq - m' Pr,   M1 = 2 Pq,   M2 = Pr        (a', m': the means of the SHIFTED x and y)
//    which go to the workspace, planar [n][c][3][h - 10][w - 10] (lanes write consecutive floats).
// 2. ssim_adjoint_k - G^T, the zero-padded correlation of a map back to the frame, is the same VALID 11 x 11 filter run on the
//    map with a border of 10 zeros, so the pass has the same structure: one block = one frame x one strip of <= 64 PIXEL columns
//    x one band of pixel rows, one wave per channel (lane = pixel column), the three maps' rows (zeros outside the map) through
//    LDS in chunks of 11, horizontal pass, ring of vertical accumulators - no column reads from LDS at all.  The pixel whose
//    last map row this was gets gw * (F0 + x' F1 + y' F2), staged in LDS and written out by the whole block in row order
//    (16-byte stores where the rows allow them).  Every pixel belongs to exactly one block.
// 3. ssim_loss_finalize_k - one block sums the per-block float64 partials of launch 1 frame by frame in a fixed order.
//
// The shift.  x' = x - pred[n, 0, 0, c] and y' = y - truth[n, 0, 0, c]: ONE constant per (frame, channel), read by both
// passes, so the maps and the pixels they are combined with are in the same coordinates.  U and S take the true means.
//
// `#pragma clang fp contract(off)`: every fused operation below is an explicit fmaf.  The kernel is instantiated with and
// without the map writes and the value sum, and the three kinds of call must agree to the bit.
#include <hip/hip_runtime.h>

#include <math.h>

#include "../../include/acgan_ssim_loss.h"
#include "common.h"

#pragma clang fp contract(off)   // before ssim_window.h: the shared pass takes this file's mode (see there)

#include "ssim_window.h"

namespace {

using namespace acg::ssim;

// Blocking of the map (launch 1) and of the frame (launch 2).  A training batch is tens of frames, not the hundreds the metric
// pass sees: the launch is latency bound until the grid fills the device, so the bands go down to the size of the halo.
Plan loss_plan(int n, int rows, int cols) { return plan_for(n, rows, cols, 512, kTaps); }

// What ssim_maps_k does with a finished position: S and the three gradient maps.
template <bool MAPS, bool VALUE>
struct LossEpilogue {
  float sx, sy, c1, c2;
  float* mp;        // the (frame, channel)'s three planes, at (p0, q0 + lane)
  size_t plane;
  int out_w;
  double ssim_sum;

  __device__ __forceinline__ void row(int, const float*, const float*) {}
  __device__ __forceinline__ void position(int p, const float (&mo)[5]) {
    const float A = mo[0], B = mo[1], dm = A - B;
    const float vx = mo[2] - A * A, vy = mo[3] - B * B, vd = mo[4] - dm * dm;
    const float a = sx + A, m = sy + B;
    const float A1 = 2.f * (a * m) + c1, B1 = (a * a + m * m) + c1;
    const float vv = vx + vy, A2 = (vv - vd) + c2, B2 = vv + c2;
    const float i1 = 1.f / B1, i2 = 1.f / B2, i12 = i1 * i2;
    const float S = (A1 * A2) * i12;
    if constexpr (VALUE) ssim_sum += (double)S;
    if constexpr (MAPS) {
      const float Pq = -(S * i2), Pr = 2.f * (A1 * i12);
      const float U = 2.f * ((m * A2) * i12) - 2.f * ((a * S) * i1);
      const size_t o = (size_t)p * out_w;
      mp[o] = (U - 2.f * (A * Pq)) - B * Pr;
      mp[plane + o] = 2.f * Pq;
      mp[2 * plane + o] = Pr;
    }
  }
};

// blockDim.x = 64 * C.  MAPS: maps[((n C + c) 3 + k) plane + p out_w + q].  VALUE: part[block] = sum of S over the block's
// positions and channels.
template <bool VEC, bool MAPS, bool VALUE>
__global__ __launch_bounds__(256) void ssim_maps_k(const float* __restrict__ pred, const float* __restrict__ truth,
                                                   float* __restrict__ maps, double* __restrict__ part, int H, int W, int C, Plan pl,
                                                   Window win, float c1, float c2) {
  __shared__ float xs[kMaxC][kTaps][kLdsCols];
  __shared__ float ys[kMaxC][kTaps][kLdsCols];
  __shared__ double scratch[16];

  const Tile tl = tile_of(pl);
  const size_t frame = (size_t)tl.n * H * W * C;
  const bool live = tl.c < C;
  LossEpilogue<MAPS, VALUE> ep;
  ep.sx = live ? pred[frame + tl.c] : 0.f;
  ep.sy = live ? truth[frame + tl.c] : 0.f;
  ep.c1 = c1;
  ep.c2 = c2;
  ep.plane = (size_t)pl.rows * pl.cols;
  ep.out_w = pl.cols;
  ep.mp = MAPS ? maps + ((size_t)tl.n * C + (live ? tl.c : 0)) * 3 * ep.plane + (size_t)tl.p0 * pl.cols + (tl.q0 + tl.lane) : nullptr;
  ep.ssim_sum = 0.0;
  ep = moments_pass<VEC>(pred, truth, xs, ys, tl, pl, H, W, C, C, win, ep.sx, ep.sy, ep);

  if constexpr (VALUE) {
    const double s1 = acg::block_sum(ep.ssim_sum, scratch);
    if (threadIdx.x == 0) part[blockIdx.x] = s1;
  }
}

// blockDim.x = 64 * C; pl blocks the H x W frame.  gw = grad_weight * -1 / (positions * C).
template <bool VEC>
__global__ __launch_bounds__(256) void ssim_adjoint_k(const float* __restrict__ pred, const float* __restrict__ truth,
                                                      const float* __restrict__ maps, float* __restrict__ dpred, int H, int W, int C,
                                                      Plan pl, int out_h, int out_w, Window win, float gw) {
  __shared__ float ms[3][kMaxC][kTaps][kLdsCols];
  __shared__ __align__(16) float os[kTaps][kStrip * kMaxC];

  const Tile tl = tile_of(pl);
  const long long n = tl.n;
  const int j0 = tl.q0, i0 = tl.p0, c = tl.c, lane = tl.lane;
  const int rows_in = tl.rows_in;             // rows of the zero-bordered map: local row rl is map row i0 - 10 + rl
  const int cols = tl.cols_in - kHalo;        // pixel columns of this strip
  const size_t frame = (size_t)n * H * W * C;
  const size_t row_elems = (size_t)W * C;
  const bool live = c < C;
  const float sx = live ? pred[frame + c] : 0.f, sy = live ? truth[frame + c] : 0.f;
  const size_t plane = (size_t)out_h * out_w;
  const float* const mf = maps + (size_t)n * C * 3 * plane;

  float acc0[kTaps], acc1[kTaps], acc2[kTaps];  // (three arrays: as one [11][3] array the ring stays in scratch memory)
#pragma unroll
  for (int s = 0; s < kTaps; ++s) acc0[s] = acc1[s] = acc2[s] = 0.f;

  const int seg = cols * C;  // elements of one output row this block writes
  for (int r0 = 0; r0 < rows_in; r0 += kTaps) {
    const int nr = min(kTaps, rows_in - r0);
    __syncthreads();  // the previous chunk has been read and its outputs written
    // local column lc is map column j0 - 10 + lc; everything outside the map is the zero border
    for (int e = threadIdx.x; e < 3 * C * nr * kCols; e += blockDim.x) {
      const int lc = e % kCols, t = e / kCols, i = t % nr, ck = t / nr, ch = ck / 3, k = ck - 3 * ch;
      const int p = i0 - kHalo + r0 + i, q = j0 - kHalo + lc;
      float v = 0.f;
      if (p >= 0 && p < out_h && q >= 0 && q < out_w) v = mf[(size_t)ck * plane + (size_t)p * out_w + q];
      ms[k][ch][i][lc] = v;
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (int i = 0; i < kTaps; ++i) {
        if (i < nr) {
          const int o = r0 + i - kHalo;       // the pixel row (of this band) whose last map row this is
          const bool own = o >= 0 && lane < cols;
          float x = 0.f, y = 0.f;
          if (own) {
            const size_t pix = frame + (size_t)(i0 + o) * row_elems + (size_t)(j0 + lane) * C + c;
            x = pred[pix] - sx;
            y = truth[pix] - sy;
          }
          float h[3] = {0.f, 0.f, 0.f};
#pragma unroll
          for (int t = 0; t < kTaps; ++t) {
            const float g = win.g[t];
#pragma unroll
            for (int k = 0; k < 3; ++k) h[k] = fmaf(g, ms[k][c][i][lane + t], h[k]);
          }
#pragma unroll
          for (int k = 0; k < kTaps; ++k) {
            const int s = (i - k + kTaps) % kTaps;
            acc0[s] = fmaf(win.g[k], h[0], acc0[s]);
            acc1[s] = fmaf(win.g[k], h[1], acc1[s]);
            acc2[s] = fmaf(win.g[k], h[2], acc2[s]);
          }
          const int s = (i + 1) % kTaps;
          if (own) os[i][lane * C + c] = gw * fmaf(y, acc2[s], fmaf(x, acc1[s], acc0[s]));
          acc0[s] = acc1[s] = acc2[s] = 0.f;
        }
      }
    }
    __syncthreads();
    // the chunk's finished pixel rows, in row order by the whole block
    if constexpr (VEC) {
      const int seg4 = seg >> 2;  // W * C and j0 * C are multiples of 4: so is seg
      for (int e = threadIdx.x; e < nr * seg4; e += blockDim.x) {
        const int i = e / seg4, e4 = (e - i * seg4) << 2, o = r0 + i - kHalo;
        if (o >= 0)
          *reinterpret_cast<float4*>(dpred + frame + (size_t)(i0 + o) * row_elems + (size_t)j0 * C + e4) =
              *reinterpret_cast<const float4*>(&os[i][e4]);
      }
    } else {
      for (int e = threadIdx.x; e < nr * seg; e += blockDim.x) {
        const int i = e / seg, el = e - i * seg, o = r0 + i - kHalo;
        if (o >= 0) dpred[frame + (size_t)(i0 + o) * row_elems + (size_t)j0 * C + el] = os[i][el];
      }
    }
  }
}

// one block: thread t takes frames t, t + 256, ... (each frame's blocks in block order), then the block's fixed tree
__global__ __launch_bounds__(256) void ssim_loss_finalize_k(const double* __restrict__ part, float* __restrict__ value, int n, int bpf,
                                                            double positions) {
  __shared__ double scratch[16];
  double acc = 0.0;
  for (int f = threadIdx.x; f < n; f += 256) {
    double s = 0.0;
    for (int b = 0; b < bpf; ++b) s += part[(size_t)f * bpf + b];
    acc += 1.0 - s / positions;
  }
  const double total = acg::block_sum(acc, scratch);
  if (threadIdx.x == 0) value[0] = (float)total;
}

bool supported(int n, int h, int w, int c) { return n >= 1 && h >= kTaps && w >= kTaps && c >= 1 && c <= kMaxC; }

// the maps first (float32, rounded up to a multiple of 8 bytes), the float64 partials behind them
size_t maps_bytes(int n, int h, int w, int c) {
  const size_t b = (size_t)n * c * 3 * (size_t)(h - kHalo) * (size_t)(w - kHalo) * sizeof(float);
  return (b + 7) & ~(size_t)7;
}

}  // namespace

extern "C" {

size_t acg_ssim_loss_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c) {
  if (!supported(n, h, w, c)) return 0;
  const Plan pm = loss_plan(n, h - kHalo, w - kHalo);
  return maps_bytes(n, h, w, c) + (size_t)n * pm.blocks_per_frame() * sizeof(double);
}

int32_t acg_ssim_loss(const float* pred, const float* truth, float* value, float* dpred, float grad_weight, int32_t n, int32_t h,
                      int32_t w, int32_t c, float data_range, float k1, float k2, void* workspace, size_t ws_bytes, acg_stream_t stream) {
  ACG_REQUIRE(n >= 1, ACG_ERR_INVALID_ARG, "ssim_loss: n = %d (must be >= 1)", (int)n);
  ACG_REQUIRE(h >= kTaps && w >= kTaps, ACG_ERR_INVALID_ARG, "ssim_loss: %d x %d frame is smaller than the 11 x 11 SSIM window", (int)h, (int)w);
  ACG_REQUIRE(c >= 1 && c <= kMaxC, ACG_ERR_INVALID_ARG, "ssim_loss: %d channels (1..4)", (int)c);
  ACG_REQUIRE(pred && truth, ACG_ERR_INVALID_ARG, "ssim_loss: null input");
  ACG_REQUIRE(value || dpred, ACG_ERR_INVALID_ARG, "ssim_loss: neither the value nor the gradient is asked for");
  ACG_REQUIRE(data_range > 0.f, ACG_ERR_INVALID_ARG, "ssim_loss: data_range must be positive");
  const int out_h = h - kHalo, out_w = w - kHalo;
  const Plan pm = loss_plan(n, out_h, out_w), pa = loss_plan(n, h, w);
  const long long nblk_m = (long long)n * pm.blocks_per_frame(), nblk_a = (long long)n * pa.blocks_per_frame();
  ACG_REQUIRE(nblk_m < (1LL << 31) && nblk_a < (1LL << 31), ACG_ERR_INVALID_ARG, "ssim_loss: %lld blocks", nblk_a);
  ACG_REQUIRE(workspace && aligned(workspace, 8) && ws_bytes >= acg_ssim_loss_workspace_bytes(n, h, w, c), ACG_ERR_WORKSPACE,
              "ssim_loss: workspace too small or not 8-byte aligned");
  const float c1 = (k1 * data_range) * (k1 * data_range), c2 = (k2 * data_range) * (k2 * data_range);
  const Window win = gaussian_window();
  hipStream_t st = acg::to_stream(stream);
  float* maps = static_cast<float*>(workspace);
  double* part = reinterpret_cast<double*>(static_cast<char*>(workspace) + maps_bytes(n, h, w, c));
  const bool vec_rows = ((size_t)w * c) % 4 == 0;   // q0 * c = 64 k c is a multiple of 4 already
  const bool vec_in = vec_rows && aligned(pred, 16) && aligned(truth, 16);
#define ACG_SSIM_MAPS(V, M, S) \
  ACG_LAUNCH((ssim_maps_k<V, M, S>), dim3((unsigned)nblk_m), dim3(64 * c), 0, st, pred, truth, maps, part, (int)h, (int)w, (int)c, pm, win, c1, c2)
  if (vec_in) {
    if (!dpred) ACG_SSIM_MAPS(true, false, true);
    else if (!value) ACG_SSIM_MAPS(true, true, false);
    else ACG_SSIM_MAPS(true, true, true);
  } else {
    if (!dpred) ACG_SSIM_MAPS(false, false, true);
    else if (!value) ACG_SSIM_MAPS(false, true, false);
    else ACG_SSIM_MAPS(false, true, true);
  }
#undef ACG_SSIM_MAPS
  if (int rc = acg::check_launch("ssim_loss maps")) return rc;
  if (dpred) {
    const float gw = grad_weight * (float)(-1.0 / ((double)out_h * out_w * c));
    if (vec_rows && aligned(dpred, 16))
      ACG_LAUNCH((ssim_adjoint_k<true>), dim3((unsigned)nblk_a), dim3(64 * c), 0, st, pred, truth, (const float*)maps, dpred, (int)h,
                 (int)w, (int)c, pa, out_h, out_w, win, gw);
    else
      ACG_LAUNCH((ssim_adjoint_k<false>), dim3((unsigned)nblk_a), dim3(64 * c), 0, st, pred, truth, (const float*)maps, dpred, (int)h,
                 (int)w, (int)c, pa, out_h, out_w, win, gw);
    if (int rc = acg::check_launch("ssim_loss adjoint")) return rc;
  }
  if (value) {
    ACG_LAUNCH(ssim_loss_finalize_k, dim3(1), dim3(256), 0, st, (const double*)part, value, (int)n, (int)pm.blocks_per_frame(),
               (double)out_h * out_w * c);
    return acg::check_launch("ssim_loss finalize");
  }
  return ACG_OK;
}

}  // extern "C"
