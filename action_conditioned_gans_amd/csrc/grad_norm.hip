// Clip a flat gradient buffer by its global norm (include/acgan_rollout.h: acg_grad_clip_norm).  Three launches on one stream:
//   grad_norm_partials_k  one block per (segment, 8192-element chunk of it): the chunk's sum of squares in double -> workspace;
//   grad_norm_finalize_k  one block: every segment's partials summed in a fixed order, the norms and the scale -> stats;
//   grad_norm_apply_k     the first launch's grid again: a block reads stats[1] and returns when it is 1, else scales its chunk.
// A launch boundary is the only hand-off between them: nothing spins, nothing is read across blocks inside one launch, and there
// are no atomics - the same (n, segs) gives the same summation order and so the same bits.  The host skips the third launch
// for max_norm = +inf (measure only).  Elements between segments are never touched.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/acgan_rollout.h"
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kFinalThreads = 1024;                        // the one finalizing block: 16 waves, one segment each per trip
constexpr int kBatch = 8;                                  // float4 loads per thread, all issued before the first multiply
constexpr long long kChunk = (long long)kThreads * kBatch * 4;     // = ACG_NORM_CHUNK elements per block
static_assert(kChunk == ACG_NORM_CHUNK, "acgan_rollout.h documents the chunk");

// The segments and the block -> (segment, chunk) map, by value in the kernel arguments (as acg_prep_list travels): no host
// pointer survives the call, so a captured graph replays it.
struct Plan {
  int count;
  int first[ACG_NORM_SEGMENTS_MAX + 1];       // first[i] = index of segment i's first block / partial; first[count] = their number
  long long offset[ACG_NORM_SEGMENTS_MAX];
  long long length[ACG_NORM_SEGMENTS_MAX];
};

struct Chunk {
  long long base;     // element index of the chunk's first element (a multiple of 4)
  int m;              // elements in it, 1..kChunk
};

// Every segment owns a non-empty run of consecutive blocks: the segment of a block is the last s with first[s] <= block, found
// by bisection - at most 6 scalar loads of kernel arguments, uniform over the block, no LDS and no barrier in front of the
// block's first gradient load.  (A walk along the table cost a dependent load per segment; one thread per table entry
// answering through LDS cost two vector loads and a barrier: profiles/clip_norm/lookup_ab.txt.)
__device__ __forceinline__ int segment_of(const Plan& pl, int block) {
  int lo = 0, hi = pl.count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pl.first[mid] <= block) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ Chunk chunk_of(const Plan& pl, int block) {
  const int s = segment_of(pl, block);
  const long long c = block - pl.first[s];
  const long long left = pl.length[s] - c * kChunk;
  return Chunk{pl.offset[s] + c * kChunk, (int)(left < kChunk ? left : kChunk)};
}

__global__ __launch_bounds__(kThreads) void grad_norm_partials_k(const float* __restrict__ grad, Plan pl, double* __restrict__ partials) {
  __shared__ double s_red[16];
  const Chunk ch = chunk_of(pl, blockIdx.x);
  const float4* g4 = reinterpret_cast<const float4*>(grad + ch.base);
  const int m4 = ch.m >> 2, t = threadIdx.x;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 v[kBatch];
  float tail = 0.f;
  // Every load is UNCONDITIONAL inside its (block-uniform) branch: behind a per-lane condition the compiler sinks the
  // conversions to double into the load's arm and waits for each load before it issues the next - eight round trips.
  if (ch.m == kChunk) {                                             // a whole chunk: nearly every block of a large variable
#pragma unroll
    for (int j = 0; j < kBatch; ++j) v[j] = g4[t + j * kThreads];
  } else {
    if (m4 > 0) {                                                   // a lane past the end re-reads the segment's last float4 ...
#pragma unroll
      for (int j = 0; j < kBatch; ++j) v[j] = g4[min(t + j * kThreads, m4 - 1)];
    }
    const int it = (m4 << 2) + t;                                   // the scalar tail: up to 3 elements
    if (it < ch.m) tail = grad[ch.base + it];
#pragma unroll
    for (int j = 0; j < kBatch; ++j)                                // ... and drops it once all loads are on their way
      if (m4 == 0 || t + j * kThreads >= m4) v[j] = zero;
  }
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < kBatch; ++j) {
    const double x = v[j].x, y = v[j].y, z = v[j].z, w = v[j].w;
    acc += x * x; acc += y * y; acc += z * z; acc += w * w;
  }
  acc += (double)tail * (double)tail;
  const double sum = acg::block_sum(acc, s_red);
  if (t == 0) partials[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kFinalThreads) void grad_norm_finalize_k(const double* __restrict__ partials, Plan pl, float pre_scale, float max_norm,
                                                                 float* __restrict__ stats) {
  __shared__ double s_ss[ACG_NORM_SEGMENTS_MAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // wave w of 16 sums segments w, w + 16, ...: each lane its strided share in index order, then the shuffle tree - a fixed order;
  // up to 16 segments in one trip, their loads in flight together
  // (every wave makes the same number of trips: the host build of this file runs a block's shuffles in step)
  for (int s0 = 0; s0 < pl.count; s0 += kFinalThreads / 64) {
    const int s = s0 + wave;
    double a = 0.0;
    if (s < pl.count)
      for (int i = pl.first[s] + lane; i < pl.first[s + 1]; i += 64) a += partials[i];
    a = acg::wave_sum(a);
    if (lane == 0 && s < pl.count) s_ss[s] = a;
  }
  __syncthreads();
  const double ps = fabs((double)pre_scale);
  if (threadIdx.x < pl.count) stats[2 + threadIdx.x] = (float)(ps * sqrt(s_ss[threadIdx.x]));
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int s = 0; s < pl.count; ++s) total += s_ss[s];             // in segment order
    const double norm = ps * sqrt(total);
    float scale = 1.f;
    if (isfinite(norm) && norm > (double)max_norm) scale = (float)((double)max_norm / norm);
    stats[0] = (float)norm;
    stats[1] = scale;
  }
}

__global__ __launch_bounds__(kThreads) void grad_norm_apply_k(float* __restrict__ grad, Plan pl, const float* __restrict__ stats) {
  const float scale = stats[1];
  if (scale == 1.f) return;                                         // the gradient fits, or is not finite: nothing is written
  const Chunk ch = chunk_of(pl, blockIdx.x);
  float4* g4 = reinterpret_cast<float4*>(grad + ch.base);
  const int m4 = ch.m >> 2, t = threadIdx.x;
  float4 v[kBatch];
#pragma unroll
  for (int j = 0; j < kBatch; ++j) {
    const int i = t + j * kThreads;
    if (i < m4) v[j] = g4[i];
  }
#pragma unroll
  for (int j = 0; j < kBatch; ++j) {
    const int i = t + j * kThreads;
    if (i < m4) g4[i] = make_float4(v[j].x * scale, v[j].y * scale, v[j].z * scale, v[j].w * scale);
  }
  const int it = (m4 << 2) + t;
  if (it < ch.m) grad[ch.base + it] *= scale;
}

// Validates (n, segs) and fills the plan; ACG_OK or the error with its message.
int make_plan(int64_t n, const acg_norm_segments* segs, Plan* pl) {
  ACG_REQUIRE(segs != nullptr, ACG_ERR_INVALID_ARG, "grad_clip_norm: no segment list");
  ACG_REQUIRE(n > 0, ACG_ERR_INVALID_ARG, "grad_clip_norm: n = %lld", (long long)n);
  ACG_REQUIRE(segs->count >= 1 && segs->count <= ACG_NORM_SEGMENTS_MAX, ACG_ERR_INVALID_ARG,
              "grad_clip_norm: %d segments (1..%d)", (int)segs->count, ACG_NORM_SEGMENTS_MAX);
  long long blocks = 0;
  for (int i = 0; i < segs->count; ++i) {
    const int64_t off = segs->offset[i], len = segs->length[i];
    ACG_REQUIRE(off >= 0 && len >= 1 && off <= n && len <= n - off, ACG_ERR_INVALID_ARG,
                "grad_clip_norm: segment %d [%lld, +%lld) is outside the %lld elements", i, (long long)off, (long long)len, (long long)n);
    ACG_REQUIRE((off & 3) == 0, ACG_ERR_INVALID_ARG, "grad_clip_norm: segment %d starts at element %lld, not a multiple of 4 (16 bytes)", i,
                (long long)off);
    for (int j = 0; j < i; ++j)
      ACG_REQUIRE(off + len <= segs->offset[j] || segs->offset[j] + segs->length[j] <= off, ACG_ERR_INVALID_ARG,
                  "grad_clip_norm: segments %d and %d overlap", j, i);
    pl->offset[i] = off;
    pl->length[i] = len;
    pl->first[i] = (int)blocks;
    blocks += acg::ceil_div(len, kChunk);
    ACG_REQUIRE(blocks <= 0x7fffffffLL, ACG_ERR_UNSUPPORTED, "grad_clip_norm: more than 2^31 - 1 chunks");
  }
  pl->count = segs->count;
  pl->first[segs->count] = (int)blocks;
  return ACG_OK;
}

}  // namespace

extern "C" {

size_t acg_grad_clip_norm_workspace_bytes(int64_t n, const acg_norm_segments* segs) {
  Plan pl;
  if (make_plan(n, segs, &pl) != ACG_OK) return 0;
  return (size_t)pl.first[pl.count] * sizeof(double);
}

int32_t acg_grad_clip_norm(float* grad, int64_t n, const acg_norm_segments* segs, float pre_scale, float max_norm, float* stats,
                           void* workspace, size_t workspace_bytes, acg_stream_t stream) {
  Plan pl;
  const int rc = make_plan(n, segs, &pl);
  if (rc != ACG_OK) return rc;
  ACG_REQUIRE(grad && stats && workspace, ACG_ERR_INVALID_ARG, "grad_clip_norm: null pointer");
  ACG_REQUIRE((reinterpret_cast<uintptr_t>(grad) & 15) == 0, ACG_ERR_INVALID_ARG, "grad_clip_norm: the gradient buffer is not 16-byte aligned");
  ACG_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(stats) & 3) == 0, ACG_ERR_INVALID_ARG,
              "grad_clip_norm: the workspace must be 8-byte and stats 4-byte aligned");
  ACG_REQUIRE(max_norm > 0.f, ACG_ERR_INVALID_ARG, "grad_clip_norm: max_norm %g is not > 0 (+inf measures only)", (double)max_norm);
  ACG_REQUIRE(isfinite(pre_scale), ACG_ERR_INVALID_ARG, "grad_clip_norm: pre_scale %g is not finite", (double)pre_scale);
  const int blocks = pl.first[pl.count];
  ACG_REQUIRE(workspace_bytes >= (size_t)blocks * sizeof(double), ACG_ERR_WORKSPACE, "grad_clip_norm: workspace of %zu bytes, %zu needed",
              workspace_bytes, (size_t)blocks * sizeof(double));
  hipStream_t s = acg::to_stream(stream);
  double* partials = static_cast<double*>(workspace);
  ACG_LAUNCH(grad_norm_partials_k, dim3(blocks), dim3(kThreads), 0, s, grad, pl, partials);
  if (int e = acg::check_launch("grad_clip_norm (partials)")) return e;
  ACG_LAUNCH(grad_norm_finalize_k, dim3(1), dim3(kFinalThreads), 0, s, partials, pl, pre_scale, max_norm, stats);
  if (int e = acg::check_launch("grad_clip_norm (finalize)")) return e;
  if (isinf(max_norm)) return ACG_OK;                                // measure only: the scale is 1 whatever the norm
  ACG_LAUNCH(grad_norm_apply_k, dim3(blocks), dim3(kThreads), 0, s, grad, pl, stats);
  return acg::check_launch("grad_clip_norm (apply)");
}

}  // extern "C"
