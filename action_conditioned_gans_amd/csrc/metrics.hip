// Per-frame SSIM and squared error (include/acgan_metrics.h): the quality curves of the reference's report.
//
// SSIM is tf.image.ssim's definition (= skimage's with gaussian_weights=True, use_sample_covariance=False): 11x11 Gaussian
// window, sigma 1.5, normalised to sum 1; VALID filtering ((H-10) x (W-10) positions); population moments; C1 = (k1 L)^2,
// C2 = (k2 L)^2; the frame's value is the mean of the map over the positions and then over the channels.
//
// The windowed moments come from the pass of ssim_window.h (one block = one frame x one strip of <= 64 output columns x one band
// of output rows); this file adds what is done with a finished position and the squared-error side sum.
//
// Cancellation.  sigma^2 = E[x^2] - E[x]^2 loses digits where the window is flat (constant frames: all of it).  Two measures
// keep fp32 within 1e-5 of float64: every block moves x and y by a constant of its own (the first value of its channel, so a
// constant frame moves to exactly 0), and the covariance is taken through d = x - y:
//     2 sigma_xy = sigma_x^2 + sigma_y^2 - Var(d)
// which is exact in the limit pred -> truth (SSIM near 1) instead of a difference of two nearly equal numbers.
//
// Deterministic: per-block partial sums (fp64) go to the workspace, a second launch sums each frame's blocks in a fixed order.
#include <hip/hip_runtime.h>

#include <math.h>

#include "../../include/acgan_metrics.h"
#include "common.h"
#include "ssim_window.h"

namespace {

using namespace acg::ssim;

// What ssim_partial_k does with the pass's rows and positions: the SSIM value of a position, and (x - y)^2 over the input
// elements this block owns - rows [p0, p0 + band) (the last band: to H), columns [q0, q0 + 64) (the last strip: to W).
struct MetricEpilogue {
  float sx, sy, c1, c2;
  int lane, own_rows;
  bool own_a, own_b;
  double ssim_sum, sq_sum;

  __device__ __forceinline__ void row(int r, const float* x, const float* y) {
    if (r < own_rows) {
      if (own_a) { const double d = (double)x[lane] - (double)y[lane]; sq_sum += d * d; }
      if (own_b) { const double d = (double)x[kStrip + lane] - (double)y[kStrip + lane]; sq_sum += d * d; }
    }
  }
  __device__ __forceinline__ void position(int, const float (&m)[5]) {
    const float A = m[0], B = m[1];
    const float vx = m[2] - A * A, vy = m[3] - B * B, vd = m[4] - (A - B) * (A - B);
    const float mx = sx + A, my = sy + B;
    const float lum = (2.f * mx * my + c1) / (mx * mx + my * my + c1);
    const float cs = (vx + vy - vd + c2) / (vx + vy + c2);
    ssim_sum += (double)(lum * cs);
  }
};

// blockDim.x = 64 * C.  part[2 * block] = (sum of the SSIM map over this block's outputs and channels, sum of (x - y)^2 over the
// input elements this block owns); every input element is owned by exactly one block of its frame.
template <typename TA, typename TB, bool VEC>
__global__ __launch_bounds__(256) void ssim_partial_k(const TA* __restrict__ pred, const TB* __restrict__ truth,
                                                      double* __restrict__ part, int H, int W, int C, int P, Plan pl,
                                                      Window win, float c1, float c2) {
  __shared__ float xs[kMaxC][kTaps][kLdsCols];
  __shared__ float ys[kMaxC][kTaps][kLdsCols];
  __shared__ float shift[2][kMaxC];
  __shared__ double scratch[16];

  const Tile tl = tile_of(pl);
  // every block moves x and y by a constant of its own: the first value of its channel
  if (threadIdx.x < C) {
    const size_t o = (((size_t)tl.n * H + tl.p0) * W + tl.q0) * P + threadIdx.x;
    shift[0][threadIdx.x] = (float)pred[o];
    shift[1][threadIdx.x] = (float)truth[o];
  }
  __syncthreads();

  MetricEpilogue ep;
  ep.sx = shift[0][tl.c];
  ep.sy = shift[1][tl.c];
  ep.c1 = c1;
  ep.c2 = c2;
  ep.lane = tl.lane;
  ep.own_rows = tl.band == pl.bands - 1 ? tl.rows_in : tl.rows_out;
  ep.own_a = tl.q0 + tl.lane < W && tl.lane < kStrip;
  ep.own_b = tl.strip == pl.strips - 1 && tl.lane < kHalo && tl.q0 + kStrip + tl.lane < W;
  ep.ssim_sum = ep.sq_sum = 0.0;
  ep = moments_pass<VEC>(pred, truth, xs, ys, tl, pl, H, W, C, P, win, ep.sx, ep.sy, ep);

  const double s1 = acg::block_sum(ep.ssim_sum, scratch);
  const double s2 = acg::block_sum(ep.sq_sum, scratch);
  if (threadIdx.x == 0) { part[2 * (size_t)blockIdx.x] = s1; part[2 * (size_t)blockIdx.x + 1] = s2; }
}

// one thread per frame: its blocks' partials in block order
__global__ __launch_bounds__(256) void ssim_finalize_k(const double* __restrict__ part, float* __restrict__ ssim, float* __restrict__ sqerr,
                                                       int n, int bpf, double positions) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n) return;
  double s1 = 0.0, s2 = 0.0;
  for (int b = 0; b < bpf; ++b) {
    s1 += part[2 * ((size_t)f * bpf + b)];
    s2 += part[2 * ((size_t)f * bpf + b) + 1];
  }
  ssim[f] = (float)(s1 / positions);
  sqerr[f] = (float)s2;
}

// bands are halved while the grid is small (a 64x64 frame is 54 output rows: 224 frames are 224 blocks, two bands 448) and the
// halo stays under ~1/3 of the band
Plan metric_plan(int n, int h, int w) { return plan_for(n, h - kHalo, w - kHalo, 1024, 32); }

}  // namespace

extern "C" {

size_t acg_frame_metrics_workspace_bytes(int32_t n, int32_t h, int32_t w) {
  if (n < 1 || h < kTaps || w < kTaps) return 0;
  const Plan pl = metric_plan(n, h, w);
  return (size_t)n * pl.blocks_per_frame() * 2 * sizeof(double);
}

int32_t acg_frame_metrics(const void* pred, const void* truth, float* ssim, float* sqerr, int32_t n, int32_t h, int32_t w, int32_t c,
                          int32_t pitch, int32_t dtype, float data_range, float k1, float k2, void* workspace, size_t ws_bytes,
                          acg_stream_t stream) {
  ACG_REQUIRE(n >= 1, ACG_ERR_INVALID_ARG, "frame_metrics: n = %d (must be >= 1)", (int)n);
  ACG_REQUIRE(h >= kTaps && w >= kTaps, ACG_ERR_INVALID_ARG, "frame_metrics: %d x %d frame is smaller than the 11 x 11 SSIM window", (int)h, (int)w);
  ACG_REQUIRE(c >= 1 && c <= kMaxC, ACG_ERR_INVALID_ARG, "frame_metrics: %d channels (1..4)", (int)c);
  const int P = pitch ? pitch : c;
  ACG_REQUIRE(P >= c && P <= 64, ACG_ERR_INVALID_ARG, "frame_metrics: channel pitch %d for %d channels", P, (int)c);
  ACG_REQUIRE(pred && truth && ssim && sqerr, ACG_ERR_INVALID_ARG, "frame_metrics: null pointer");
  ACG_REQUIRE(data_range > 0.f, ACG_ERR_INVALID_ARG, "frame_metrics: data_range must be positive");
  const Plan pl = metric_plan(n, h, w);
  const long long nblk = (long long)n * pl.blocks_per_frame();
  ACG_REQUIRE(nblk < (1LL << 31), ACG_ERR_INVALID_ARG, "frame_metrics: %lld blocks", nblk);
  ACG_REQUIRE(workspace && ws_bytes >= acg_frame_metrics_workspace_bytes(n, h, w), ACG_ERR_WORKSPACE, "frame_metrics: workspace too small");
  const float c1 = (k1 * data_range) * (k1 * data_range), c2 = (k2 * data_range) * (k2 * data_range);
  const Window win = gaussian_window();
  hipStream_t st = acg::to_stream(stream);
  const bool vec_rows = ((size_t)w * P) % 4 == 0;   // q0 * P = 64 k P is a multiple of 4 already
  ACG_WITH_TYPES_ANY(dtype, "frame_metrics", {
    const TA* a = static_cast<const TA*>(pred);
    const TB* t = static_cast<const TB*>(truth);
    if (vec_rows && aligned(a, 4 * sizeof(TA)) && aligned(t, 4 * sizeof(TB)))
      ACG_LAUNCH((ssim_partial_k<TA, TB, true>), dim3((unsigned)nblk), dim3(64 * c), 0, st, a, t, (double*)workspace, (int)h, (int)w,
                 (int)c, P, pl, win, c1, c2);
    else
      ACG_LAUNCH((ssim_partial_k<TA, TB, false>), dim3((unsigned)nblk), dim3(64 * c), 0, st, a, t, (double*)workspace, (int)h, (int)w,
                 (int)c, P, pl, win, c1, c2);
  });
  if (int rc = acg::check_launch("frame_metrics")) return rc;
  ACG_LAUNCH(ssim_finalize_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double*)workspace, ssim, sqerr, (int)n,
             (int)pl.blocks_per_frame(), (double)pl.rows * pl.cols * c);
  return acg::check_launch("frame_metrics finalize");
}

}  // extern "C"
