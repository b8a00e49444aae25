// Per-frame SSIM and squared error (include/acgan_metrics.h): the quality curves of the reference's report.
//
// SSIM is tf.image.ssim's definition (= skimage's with gaussian_weights=True, use_sample_covariance=False): 11x11 Gaussian
// window, sigma 1.5, normalised to sum 1; VALID filtering ((H-10) x (W-10) positions); population moments; C1 = (k1 L)^2,
// C2 = (k2 L)^2; the frame's value is the mean of the map over the positions and then over the channels.
//
// One block = one frame x one strip of <= 64 output columns x one band of output rows, one wave per channel (lane = output
// column).  The band's input rows go through LDS in chunks of 11 (coalesced, 16-byte loads where the rows allow them); each
// lane runs the horizontal 11-tap pass of its column on five quantities and adds the result into a ring of 11 vertical
// accumulators (row r feeds the outputs r-10..r), so the vertical pass needs no second LDS round trip; the output whose
// window ended at this row is turned into its SSIM value and the ring slot is reused.
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

namespace {

constexpr int kTaps = 11, kHalo = kTaps - 1;
constexpr int kStrip = 64;                  // output columns per block (one per lane)
constexpr int kCols = kStrip + kHalo;       // input columns a strip reads
constexpr int kLdsCols = kCols + 2;         // (row pitch in LDS)
constexpr int kMaxC = 4;

struct Window {
  float g[kTaps];
};

// Output geometry shared by the workspace query and the launch: strips of 64 columns, bands of rows halved while the grid is
// small (a 64x64 frame is 54 output rows: 224 frames are 224 blocks, two bands 448) and the halo stays under ~1/3 of the band.
struct Plan {
  int out_h, out_w, strips, band, bands;
  __host__ __device__ long long blocks_per_frame() const { return (long long)strips * bands; }
};

Plan plan_for(int n, int h, int w) {
  Plan p;
  p.out_h = h - kHalo;
  p.out_w = w - kHalo;
  p.strips = (p.out_w + kStrip - 1) / kStrip;
  p.band = p.out_h;
  while ((long long)n * p.strips * ((p.out_h + p.band - 1) / p.band) < 1024 && p.band > 32) p.band = (p.band + 1) / 2;
  p.bands = (p.out_h + p.band - 1) / p.band;
  return p;
}

// 4 consecutive elements (16 bytes of fp32, 8 of bf16)
template <typename T>
__device__ __forceinline__ void ld4(const T* p, float (&v)[4]) {
  if constexpr (sizeof(T) == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    const acg::bf16x4 t = *reinterpret_cast<const acg::bf16x4*>(p);
    v[0] = (float)t[0]; v[1] = (float)t[1]; v[2] = (float)t[2]; v[3] = (float)t[3];
  }
}

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

  const long long bpf = pl.blocks_per_frame();
  const long long n = blockIdx.x / bpf;
  const int b = (int)(blockIdx.x - n * bpf);
  const int strip = b % pl.strips, band = b / pl.strips;
  const int q0 = strip * kStrip, p0 = band * pl.band;
  const int rows_out = min(pl.band, pl.out_h - p0);
  const int rows_in = rows_out + kHalo;
  const int cols_in = min(kCols, W - q0);
  const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t frame = (size_t)n * H * W * P;
  const size_t row_elems = (size_t)W * P;

  if (threadIdx.x < C) {
    const size_t o = frame + (size_t)p0 * row_elems + (size_t)q0 * P + threadIdx.x;
    shift[0][threadIdx.x] = (float)pred[o];
    shift[1][threadIdx.x] = (float)truth[o];
  }
  __syncthreads();
  const float sx = shift[0][c], sy = shift[1][c];

  // element ownership for the squared error: rows [p0, p0 + band) (the last band: to H), columns [q0, q0 + 64) (the last strip: to W)
  const int own_rows = band == pl.bands - 1 ? rows_in : rows_out;
  const bool own_a = q0 + lane < W && lane < kStrip;
  const bool own_b = strip == pl.strips - 1 && lane < kHalo && q0 + kStrip + lane < W;
  const bool col_ok = q0 + lane < pl.out_w;

  float acc[kTaps][5];
#pragma unroll
  for (int s = 0; s < kTaps; ++s)
#pragma unroll
    for (int k = 0; k < 5; ++k) acc[s][k] = 0.f;
  double ssim_sum = 0.0, sq_sum = 0.0;

  const int seg = cols_in * P;  // elements of one input row this block reads
  for (int r0 = 0; r0 < rows_in; r0 += kTaps) {
    const int nr = min(kTaps, rows_in - r0);
    __syncthreads();  // the previous chunk has been read
    if constexpr (VEC) {
      const int seg4 = (seg + 3) >> 2;  // rows and q0 * P are multiples of 4 elements: a vector never crosses the row end
      for (int e = threadIdx.x; e < nr * seg4; e += blockDim.x) {
        const int i = e / seg4, e4 = (e - i * seg4) << 2;
        const size_t o = frame + (size_t)(p0 + r0 + i) * row_elems + (size_t)q0 * P + e4;
        float vx[4], vy[4];
        ld4(pred + o, vx);
        ld4(truth + o, vy);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int el = e4 + j, col = el / P, ch = el - col * P;
          if (col < cols_in && ch < C) { xs[ch][i][col] = vx[j]; ys[ch][i][col] = vy[j]; }
        }
      }
    } else {
      for (int e = threadIdx.x; e < nr * seg; e += blockDim.x) {
        const int i = e / seg, el = e - i * seg, col = el / P, ch = el - col * P;
        if (ch < C) {
          const size_t o = frame + (size_t)(p0 + r0 + i) * row_elems + (size_t)q0 * P + el;
          xs[ch][i][col] = (float)pred[o];
          ys[ch][i][col] = (float)truth[o];
        }
      }
    }
    __syncthreads();
    if (c < C) {
#pragma unroll
      for (int i = 0; i < kTaps; ++i) {
        if (i < nr) {
          const int r = r0 + i;
          if (r < own_rows) {
            if (own_a) { const double d = (double)xs[c][i][lane] - (double)ys[c][i][lane]; sq_sum += d * d; }
            if (own_b) { const double d = (double)xs[c][i][kStrip + lane] - (double)ys[c][i][kStrip + lane]; sq_sum += d * d; }
          }
          // horizontal pass (columns past the frame's edge hold stale values: they only reach outputs with col_ok false)
          float h[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int t = 0; t < kTaps; ++t) {
            const float x = xs[c][i][lane + t] - sx, y = ys[c][i][lane + t] - sy, d = x - y, g = win.g[t];
            const float gx = g * x, gy = g * y;
            h[0] += gx;
            h[1] += gy;
            h[2] = fmaf(gx, x, h[2]);
            h[3] = fmaf(gy, y, h[3]);
            h[4] = fmaf(g * d, d, h[4]);
          }
          // vertical pass: input row r feeds output row r - k with weight g[k]; the slot of output p is p mod 11 = (r - k) mod 11
          // and r = r0 + i with r0 a multiple of 11, so every slot index is a compile-time constant.  Outputs p < 0 land in
          // slots that are cleared below before their own first row.
#pragma unroll
          for (int k = 0; k < kTaps; ++k) {
            const int s = (i - k + kTaps) % kTaps;
#pragma unroll
            for (int q = 0; q < 5; ++q) acc[s][q] = fmaf(win.g[k], h[q], acc[s][q]);
          }
          // output p = r - 10 is complete (slot (i + 1) mod 11)
          const int s = (i + 1) % kTaps;
          const int p = r - kHalo;
          if (p >= 0 && col_ok) {
            const float A = acc[s][0], B = acc[s][1];
            const float vx = acc[s][2] - A * A, vy = acc[s][3] - B * B, vd = acc[s][4] - (A - B) * (A - B);
            const float mx = sx + A, my = sy + B;
            const float lum = (2.f * mx * my + c1) / (mx * mx + my * my + c1);
            const float cs = (vx + vy - vd + c2) / (vx + vy + c2);
            ssim_sum += (double)(lum * cs);
          }
#pragma unroll
          for (int q = 0; q < 5; ++q) acc[s][q] = 0.f;
        }
      }
    }
  }
  const double s1 = acg::block_sum(ssim_sum, scratch);
  const double s2 = acg::block_sum(sq_sum, scratch);
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

Window gaussian_window() {
  double g[kTaps], s = 0.0;
  for (int t = 0; t < kTaps; ++t) { const double u = t - kHalo / 2; g[t] = exp(-u * u / (2.0 * 1.5 * 1.5)); s += g[t]; }
  Window w;
  for (int t = 0; t < kTaps; ++t) w.g[t] = (float)(g[t] / s);
  return w;
}

bool aligned(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) % bytes) == 0; }

}  // namespace

extern "C" {

size_t acg_frame_metrics_workspace_bytes(int32_t n, int32_t h, int32_t w) {
  if (n < 1 || h < kTaps || w < kTaps) return 0;
  const Plan pl = plan_for(n, h, w);
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
  const Plan pl = plan_for(n, h, w);
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
             (int)pl.blocks_per_frame(), (double)pl.out_h * pl.out_w * c);
  return acg::check_launch("frame_metrics finalize");
}

}  // extern "C"
