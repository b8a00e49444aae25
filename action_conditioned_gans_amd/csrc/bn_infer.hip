// BatchNorm with stored statistics (include/acgan_bn_infer.h): the apply pass on its own, and the calibration pass that
// pools the moments of the batches it is shown into (count, mean, variance).
//
// Apply.  y = act((x - mean) * rstd + beta) on a [rows, C] view: one read, one write, no reduction, no exchange, no
// workspace.  The tensors are those of a generator forward pass - 4 MB at the top, a few KB at the bottom - so the kernel
// is bound by one memory round trip plus its per-channel prologue (three small loads, a square root and a division), not
// by bytes (DESIGN section 3 on bn_apply_fwd: a prologue paid in front of the loads left the memory system idle).  So a
// thread issues the loads of its kU rows FIRST, then the prologue's, and both round trips overlap; a lane moves 16 bytes
// (float4, or eight bf16); 256 threads = CL channel lanes x 256 / CL row lanes with CL the power of two that covers a row
// (at most 64), so consecutive lanes read consecutive addresses and a thread keeps ONE channel vector for all its rows -
// no division or modulo per element.  A block takes kU * 256 / CL rows per batch: a 4 x 4 x 256 map is one block, the
// 64 x 64 x 32 map of 32 samples 1024; beyond 2048 blocks a block walks several batches.
//
// Collect.  Pass 1: a block owns a run of rows and CL channel vectors; it shifts by its own first row, sums d and d^2
// (d = x - shift, of the size of the spread, not of the mean), adds the row lanes' sums in lane order through LDS and
// leaves (shift, mean - shift, M2) per channel.  Pass 2: 32 channels per block, 8 lanes each merging every 8th block
// Chan-style in float64 in block order, lane results merged in lane order, then the merge into the running state.  Pass 3
// adds the rows to the count (a launch of its own: every block of pass 2 reads the count).  No atomics anywhere.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/acgan_bn_infer.h"
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int kU = 4;               // rows whose loads a thread keeps in flight together
constexpr int kMaxApplyBlocks = 2048;
constexpr int kMaxCollectBlocks = 128;
constexpr int kMaxChannels = 1 << 20;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// V consecutive elements as floats: V = 8 is one 16-byte access of bf16 (two of float32), V = 4 / 1 as acg::ldv / stv
template <int V, typename T>
__device__ __forceinline__ void ldn(const T* p, float (&v)[V]) {
  if constexpr (V == 8 && sizeof(T) == 2) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
  } else if constexpr (V == 8) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
    acg::ldv<V>(p, v);
  }
}
template <int V, typename T>
__device__ __forceinline__ void stn(T* p, const float (&v)[V]) {
  if constexpr (V == 8 && sizeof(T) == 2) {
    bf16x8 t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = (__bf16)v[j];
    *reinterpret_cast<bf16x8*>(p) = t;
  } else if constexpr (V == 8) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
  } else {
    acg::stv<V>(p, v);
  }
}

// 256 threads = CL = 1 << clog channel lanes (V elements each) x RL = 256 >> clog row lanes; grid.y channel chunks
struct Lanes { int V, Cv, clog, gy; };
Lanes lanes(int C, int V) {
  Lanes l;
  l.V = V;
  l.Cv = C / V;
  l.clog = 0;
  while ((1 << l.clog) < l.Cv && l.clog < 6) ++l.clog;
  l.gy = (l.Cv + (1 << l.clog) - 1) >> l.clog;
  return l;
}

template <int V, typename TX, typename TY>
__global__ __launch_bounds__(NT) void bn_infer_apply(const TX* __restrict__ x, const float* __restrict__ beta,
                                                     const float* __restrict__ mean, const float* __restrict__ variance,
                                                     TY* __restrict__ y, long long R, int Cv, int clog, int XP, int YP, float eps,
                                                     int act, float leak) {
  const int cq = threadIdx.x & ((1 << clog) - 1), rl = threadIdx.x >> clog, RL = NT >> clog;
  const int cv = (blockIdx.y << clog) + cq;
  if (cv >= Cv) return;
  const int c = cv * V;
  const long long bstep = (long long)gridDim.x * RL * kU;
  long long r0 = (long long)blockIdx.x * RL * kU + rl;       // this thread's rows of a batch: r0 + u * RL
  if (r0 >= R) return;
  float v[kU][V];
  // (rows beyond the end re-read the last row and are not stored: every load is unconditional and issued up front)
#define ACG_BNI_LOAD(rr) _Pragma("unroll") for (int u = 0; u < kU; ++u) ldn<V>(x + min((rr) + (long long)u * RL, R - 1) * XP + c, v[u])
  ACG_BNI_LOAD(r0);
  float mn[V], rs[V], bt[V];
  ldn<V>(mean + c, mn);
  ldn<V>(variance + c, rs);
  ldn<V>(beta + c, bt);
#pragma unroll
  for (int j = 0; j < V; ++j) rs[j] = 1.0f / sqrtf(rs[j] + eps);
  for (;;) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const long long r = r0 + (long long)u * RL;
      if (r < R) {
#pragma unroll
        for (int j = 0; j < V; ++j) v[u][j] = acg::act_apply(act, (v[u][j] - mn[j]) * rs[j] + bt[j], leak);
        stn<V>(y + r * YP + c, v[u]);
      }
    }
    r0 += bstep;
    if (r0 >= R) break;
    ACG_BNI_LOAD(r0);
  }
#undef ACG_BNI_LOAD
}

// part[(b * 3 + k) * C + c]: k = 0 the block's shift (its first row), 1 its mean minus the shift, 2 its sum of squared deviations
template <int V, typename TX>
__global__ __launch_bounds__(NT) void bn_collect_partial(const TX* __restrict__ x, float* __restrict__ part, long long R, int C,
                                                         int Cv, int clog, int XP, long long rpb) {
  __shared__ float sh[2][V][NT];
  const int CL = 1 << clog, cq = threadIdx.x & (CL - 1), rl = threadIdx.x >> clog, RL = NT >> clog;
  const int cv = (blockIdx.y << clog) + cq, c = cv * V, b = blockIdx.x;
  const bool valid = cv < Cv;
  const long long rb = (long long)b * rpb, re = min(R, rb + rpb);      // rb < R: the grid has ceil(R / rpb) blocks
  float pv[V], s1[V], s2[V];
#pragma unroll
  for (int j = 0; j < V; ++j) { pv[j] = 0.f; s1[j] = 0.f; s2[j] = 0.f; }
  if (valid) {
    ldn<V>(x + rb * XP + c, pv);
    for (long long r = rb + rl; r < re; r += (long long)kU * RL) {
      float v[kU][V];
#pragma unroll
      for (int u = 0; u < kU; ++u) ldn<V>(x + min(r + (long long)u * RL, re - 1) * XP + c, v[u]);
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const float w = r + (long long)u * RL < re ? 1.f : 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) { const float d = (v[u][j] - pv[j]) * w; s1[j] += d; s2[j] += d * d; }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) { sh[0][j][threadIdx.x] = s1[j]; sh[1][j][threadIdx.x] = s2[j]; }
  __syncthreads();
  if (valid && rl == 0) {
    const float n = (float)(re - rb);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float a = 0.f, q = 0.f;
      for (int k = 0; k < RL; ++k) { a += sh[0][j][k * CL + cq]; q += sh[1][j][k * CL + cq]; }
      const float m = a / n, m2 = q - a * m;
      part[((long long)b * 3 + 0) * C + c + j] = pv[j];
      part[((long long)b * 3 + 1) * C + c + j] = m;
      part[((long long)b * 3 + 2) * C + c + j] = m2 > 0.f ? m2 : 0.f;
    }
  }
}

struct Moments { double n, mean, m2; };
__device__ __forceinline__ void chan_merge(Moments& a, const Moments& b) {      // a <- a ++ b
  if (b.n == 0.0) return;
  if (a.n == 0.0) { a = b; return; }
  const double n = a.n + b.n, d = b.mean - a.mean;
  a.m2 += b.m2 + d * d * (a.n * b.n / n);
  a.mean += d * (b.n / n);
  a.n = n;
}

__global__ __launch_bounds__(NT) void bn_collect_merge(const float* __restrict__ part, const long long* __restrict__ count,
                                                       float* __restrict__ mean, float* __restrict__ variance, long long R, int C,
                                                       long long rpb, int nblk) {
  __shared__ double sh[3][NT];
  const int cl = threadIdx.x & 31, lane = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
  Moments acc{0.0, 0.0, 0.0};
  if (c < C) {
    for (int b = lane; b < nblk; b += 8) {
      const float* o = part + (long long)b * 3 * C + c;
      const long long rb = (long long)b * rpb;
      const Moments m{(double)(min(R, rb + rpb) - rb), (double)o[0] + (double)o[C], (double)o[2 * (long long)C]};
      chan_merge(acc, m);
    }
  }
  sh[0][threadIdx.x] = acc.n; sh[1][threadIdx.x] = acc.mean; sh[2][threadIdx.x] = acc.m2;
  __syncthreads();
  if (lane != 0 || c >= C) return;
  for (int k = 1; k < 8; ++k) chan_merge(acc, Moments{sh[0][k * 32 + cl], sh[1][k * 32 + cl], sh[2][k * 32 + cl]});
  const long long seen = *count;
  Moments run{0.0, 0.0, 0.0};
  if (seen > 0) run = Moments{(double)seen, (double)mean[c], (double)variance[c] * (double)seen};
  chan_merge(run, acc);
  mean[c] = (float)run.mean;
  variance[c] = (float)(run.m2 / run.n);
}

__global__ void bn_collect_count(long long* count, long long rows) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *count += rows;
}

bool aligned(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) % bytes) == 0; }

// widest vector both tensors take: 8 for bf16 x (16 bytes), 4 for float32 x, 1 when a pitch, the channel count or an address is ragged
template <typename TX, typename TY>
int pick_vector(const void* x, const void* y, int C, int XP, int YP) {
  for (int V = sizeof(TX) == 2 ? 8 : 4; V >= 4; V >>= 1) {      // 8, 4 - the widths the kernels are instantiated for
    if (C % V || XP % V || YP % V) continue;
    if (!aligned(x, V * sizeof(TX)) || (y && !aligned(y, std::min<size_t>(16, V * sizeof(TY))))) continue;
    return V;
  }
  return 1;
}

template <typename TX, typename TY>
int infer_typed(const void* x, const float* beta, const float* mean, const float* variance, void* y, long long R, int C, int XP,
                int YP, float eps, int act, float leak, hipStream_t st) {
  int V = pick_vector<TX, TY>(x, y, C, XP, YP);
  if (V > 1 && !(aligned(beta, 16) && aligned(mean, 16) && aligned(variance, 16))) V = 1;
  const Lanes l = lanes(C, V);
  const int RL = NT >> l.clog;
  long long gx = acg::ceil_div(R, (long long)RL * kU);
  gx = std::min<long long>(gx, std::max(1, kMaxApplyBlocks / l.gy));
  const dim3 grid((unsigned)gx, (unsigned)l.gy);
#define ACG_BNI(VV) ACG_LAUNCH((bn_infer_apply<VV, TX, TY>), grid, dim3(NT), 0, st, (const TX*)x, beta, mean, variance, (TY*)y, R, l.Cv, l.clog, XP, YP, eps, act, leak)
  if (V == 8) ACG_BNI(8); else if (V == 4) ACG_BNI(4); else ACG_BNI(1);
#undef ACG_BNI
  return acg::check_launch("bn_infer_apply");
}

template <typename TX>
int collect_typed(const void* x, long long* count, float* mean, float* variance, long long R, int C, int XP, float* part,
                  hipStream_t st) {
  const int V = pick_vector<TX, TX>(x, nullptr, C, XP, XP);
  const Lanes l = lanes(C, V);
  const int RL = NT >> l.clog;
  // two batches of loads per block until the block count reaches its cap
  long long rpb = std::max<long long>((long long)RL * kU * 2, acg::ceil_div(R, (long long)kMaxCollectBlocks));
  const int nblk = (int)acg::ceil_div(R, rpb);
  const dim3 grid((unsigned)nblk, (unsigned)l.gy);
#define ACG_BNC(VV) ACG_LAUNCH((bn_collect_partial<VV, TX>), grid, dim3(NT), 0, st, (const TX*)x, part, R, C, l.Cv, l.clog, XP, rpb)
  if (V == 8) ACG_BNC(8); else if (V == 4) ACG_BNC(4); else ACG_BNC(1);
#undef ACG_BNC
  if (int rc = acg::check_launch("bn_collect_partial")) return rc;
  ACG_LAUNCH(bn_collect_merge, dim3((C + 31) / 32), dim3(NT), 0, st, (const float*)part, (const long long*)count, mean, variance, R, C, rpb, nblk);
  if (int rc = acg::check_launch("bn_collect_merge")) return rc;
  ACG_LAUNCH(bn_collect_count, dim3(1), dim3(64), 0, st, count, R);
  return acg::check_launch("bn_collect_count");
}

}  // namespace

extern "C" {

int32_t acg_bn_act_infer(const void* x, const float* beta, const float* mean, const float* variance, void* y, int64_t rows, int32_t C,
                         int32_t x_pitch, int32_t y_pitch, float eps, int32_t act, float leak, int32_t dtype, acg_stream_t stream) {
  ACG_REQUIRE(rows > 0 && C > 0, ACG_ERR_INVALID_ARG, "bn_act_infer: non-positive size");
  ACG_REQUIRE(C <= kMaxChannels, ACG_ERR_UNSUPPORTED, "bn_act_infer: more than %d channels", kMaxChannels);
  const int XP = x_pitch > 0 ? x_pitch : C, YP = y_pitch > 0 ? y_pitch : C;
  ACG_REQUIRE(XP >= C && YP >= C, ACG_ERR_INVALID_ARG, "bn_act_infer: pitch smaller than the row");
  ACG_REQUIRE(x && beta && mean && variance && y, ACG_ERR_INVALID_ARG, "bn_act_infer: null pointer");
  ACG_REQUIRE(act == ACG_ACT_NONE || act == ACG_ACT_RELU || act == ACG_ACT_LRELU, ACG_ERR_UNSUPPORTED, "bn_act_infer: activation %d", act);
  ACG_REQUIRE(eps >= 0.f, ACG_ERR_INVALID_ARG, "bn_act_infer: negative eps");
  hipStream_t st = acg::to_stream(stream);
  ACG_WITH_TYPES(dtype, "bn_act_infer", return (infer_typed<TA, TB>(x, beta, mean, variance, y, rows, C, XP, YP, eps, act, leak, st)));
}

size_t acg_bn_collect_workspace_bytes(int64_t rows, int32_t channels) {
  if (rows <= 0 || channels <= 0) return 0;
  return (size_t)kMaxCollectBlocks * 3 * (size_t)channels * sizeof(float);
}

int32_t acg_bn_collect(const void* x, int64_t* count, float* mean, float* variance, int64_t rows, int32_t C, int32_t x_pitch,
                       int32_t dtype, void* ws, size_t wsb, acg_stream_t stream) {
  ACG_REQUIRE(rows > 0 && C > 0, ACG_ERR_INVALID_ARG, "bn_collect: non-positive size");
  ACG_REQUIRE(C <= kMaxChannels, ACG_ERR_UNSUPPORTED, "bn_collect: more than %d channels", kMaxChannels);
  const int XP = x_pitch > 0 ? x_pitch : C;
  ACG_REQUIRE(XP >= C, ACG_ERR_INVALID_ARG, "bn_collect: pitch smaller than the row");
  ACG_REQUIRE(x && count && mean && variance, ACG_ERR_INVALID_ARG, "bn_collect: null pointer");
  ACG_REQUIRE(aligned(count, 8), ACG_ERR_INVALID_ARG, "bn_collect: count is not 8-byte aligned");
  ACG_REQUIRE(ws && wsb >= acg_bn_collect_workspace_bytes(rows, C), ACG_ERR_WORKSPACE, "bn_collect: workspace too small");
  // the storage type of x; a two-type code names x first
  const int tx = acg::dt_valid(dtype) ? acg::dt_first(dtype) : -1;
  hipStream_t st = acg::to_stream(stream);
  static_assert(sizeof(long long) == sizeof(int64_t), "count is one 64-bit integer");
  if (tx == ACG_BF16) return collect_typed<__bf16>(x, (long long*)count, mean, variance, rows, C, XP, (float*)ws, st);
  if (tx == ACG_F32) return collect_typed<float>(x, (long long*)count, mean, variance, rows, C, XP, (float*)ws, st);
  return acg::fail(ACG_ERR_UNSUPPORTED, "bn_collect: dtype %d", (int)dtype);
}

}  // extern "C"
