// Differentiable augmentation of the discriminator's inputs (include/acgan_rollout.h: acg_d_augment_draw / _fwd / _bwd).
//
// Draw.  One block, as the noise draw (noise.hip): a row's eight parameters come out of two Philox blocks, 1024 rows at most, so
// the block that draws also advances the counter behind a barrier.  Integer arithmetic and exact float32 conversions only.
//
// Forward and adjoint.  The frame mean couples every pixel of a (row, frame): a reduction, then a streaming pass.  Both passes
// are multi-block - one block per (row, frame) would leave half the CUs of the chip idle at config 2's 64 rows - so the
// reduction is a launch of its own that leaves double partials in the workspace ([rows, 2, chunks], at most 64 chunks of at
// least 1024 pixels a row), and every block of the streaming launch adds its row's partials in the same fixed order before it
// moves its 256 pixels.  The second read of the tensor (8.4 MB at config 2) comes out of the L2 / Infinity Cache.  The adjoint
// is the same pair of launches with the roles of the pixel and its source exchanged: its reduction sums dout over the pixels the
// forward pass wrote from a source ("live"), its streaming pass gathers dout[q + t].
//
// One thread per pixel moves both frames and the pad channels: 16-byte vectors where pitch * 4 is a multiple of 16 and the
// bases are aligned, elements otherwise - the same arithmetic on the same values, so the same bits.  The channel loops run to
// the constant 8 under predicates, never over a runtime-indexed register array: no scratch.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/acgan_rollout.h"
#include "common.h"
#include "philox.h"

namespace {

constexpr int NTH = 256;
constexpr int MAXC = 8;               // frames * cf at most
constexpr int CHUNKS_MAX = 64;        // partials per (row, frame) at most: every block of the streaming launch adds them
constexpr int CHUNK_PIXELS = 1024;    // pixels per partial at least (longer frames: longer chunks)
constexpr int SIDE_MAX = 1024;
constexpr float FIELD_LIM = 4096.f;   // |shift and cut fields| at most, checked in float before the conversion

int chunks_for(int h, int w) {
  const int n = (h * w + CHUNK_PIXELS - 1) / CHUNK_PIXELS;
  return n < CHUNKS_MAX ? n : CHUNKS_MAX;
}

__global__ __launch_bounds__(NTH) void d_augment_draw_kernel(unsigned long long* __restrict__ state, float* __restrict__ params,
                                                             int rows, int h, int w, int policy, uint32_t stream_word) {
  const acg::DrawState draw = acg::load_draw_state(state);
  const unsigned ry = (unsigned)(h + 4) / 8, rx = (unsigned)(w + 4) / 8;
  const int n = ((h < w ? h : w) + 1) / 2;
  for (int r = threadIdx.x; r < rows; r += NTH) {
    uint32_t lo[4], hi[4];
    acg::draw_block(draw, 2u * (uint32_t)r, stream_word, lo);
    acg::draw_block(draw, 2u * (uint32_t)r + 1u, stream_word, hi);
    const uint32_t m0 = lo[0] >> 9, m1 = lo[1] >> 9, m2 = lo[2] >> 9, m3 = lo[3] >> 9, m4 = hi[0] >> 9, m5 = hi[1] >> 9, m6 = hi[2] >> 9;
    float* __restrict__ p = params + (long long)r * 8;
    const bool colour = policy & ACG_DA_COLOR, shift = policy & ACG_DA_TRANSLATION, cut = policy & ACG_DA_CUTOUT;
    // every product and sum below is exact in float32: 23-bit integers times a power of two
    p[0] = colour ? (float)((int)m0 - (1 << 22)) * 1.1920928955078125e-07f : 0.f;
    p[1] = colour ? (float)m1 * 2.384185791015625e-07f : 1.f;
    p[2] = colour ? 0.5f + (float)m2 * 1.1920928955078125e-07f : 1.f;
    p[3] = shift ? (float)((int)(((unsigned long long)m3 * (2u * ry + 1u)) >> 23) - (int)ry) : 0.f;
    p[4] = shift ? (float)((int)(((unsigned long long)m4 * (2u * rx + 1u)) >> 23) - (int)rx) : 0.f;
    p[5] = cut ? (float)((int)(((unsigned long long)m5 * (unsigned)(h + 1)) >> 23) - n / 2) : 0.f;
    p[6] = cut ? (float)((int)(((unsigned long long)m6 * (unsigned)(w + 1)) >> 23) - n / 2) : 0.f;
    p[7] = cut ? (float)n : 0.f;
  }
  acg::advance_draw_state(state, draw);
}

// a row's parameters as the kernels use them; ok: every shift and cut field passed its range check
struct Row {
  float k1, k2, k3, b;
  int ty, tx, cy0, cx0, cy1, cx1;
  bool ok;
};

__device__ __forceinline__ bool field_ok(float v) { return v >= -FIELD_LIM && v <= FIELD_LIM; }      // false for NaN

__device__ __forceinline__ Row load_row(const float* __restrict__ p) {
#pragma clang fp contract(off)
  Row r;
  const float b = p[0], s = p[1], c = p[2], ty = p[3], tx = p[4], cy0 = p[5], cx0 = p[6], n = p[7];
  r.k1 = c * s;
  r.k2 = c * (1.f - s);
  r.k3 = 1.f - c;
  r.b = b;
  r.ok = field_ok(ty) && field_ok(tx) && field_ok(cy0) && field_ok(cx0) && field_ok(n);
  r.ty = r.ok ? (int)ty : 0;          // (converted only behind the check)
  r.tx = r.ok ? (int)tx : 0;
  r.cy0 = r.ok ? (int)cy0 : 0;
  r.cx0 = r.ok ? (int)cx0 : 0;
  r.cy1 = r.cy0 + (r.ok ? (int)n : 0);
  r.cx1 = r.cx0 + (r.ok ? (int)n : 0);
  return r;
}

// the forward pass writes output pixel (y, x) from a source pixel: it is inside, its source (y - ty, x - tx) is inside, and it
// is not in the cut rectangle
__device__ __forceinline__ bool live_out(const Row& r, int y, int x, int h, int w) {
  return r.ok && (unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w && (unsigned)(y - r.ty) < (unsigned)h &&
         (unsigned)(x - r.tx) < (unsigned)w && !(y >= r.cy0 && y < r.cy1 && x >= r.cx0 && x < r.cx1);
}

__device__ __forceinline__ float as_float(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ uint32_t as_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// v[ch] = the valid channels of the pixel at px, 0 behind them
template <bool VEC>
__device__ __forceinline__ void load_valid(const uint32_t* __restrict__ px, int nvalid, float (&v)[MAXC]) {
  if (VEC) {
    const uint4 a = *reinterpret_cast<const uint4*>(px);
    uint4 b = make_uint4(0u, 0u, 0u, 0u);
    if (nvalid > 4) b = *reinterpret_cast<const uint4*>(px + 4);          // (pitch >= nvalid > 4 and pitch % 4 == 0: pitch >= 8)
    const uint32_t u[MAXC] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int ch = 0; ch < MAXC; ++ch) v[ch] = ch < nvalid ? as_float(u[ch]) : 0.f;
  } else {
#pragma unroll
    for (int ch = 0; ch < MAXC; ++ch) v[ch] = ch < nvalid ? as_float(px[ch]) : 0.f;
  }
}

// partials[(r * 2 + f) * nchunks + k] = the sum of frame f of row r over the pixels of chunk k, in double.  BWD: over the live
// pixels only (x is dout).
template <bool BWD, bool VEC>
__global__ __launch_bounds__(NTH) void d_augment_sum_kernel(const uint32_t* __restrict__ x, const float* __restrict__ params,
                                                            double* __restrict__ partials, int h, int w, int pitch, int frames, int cf,
                                                            int nchunks) {
  __shared__ double scratch[16];
  const int r = blockIdx.x / nchunks, k = blockIdx.x % nchunks;
  const int hw = h * w, nvalid = frames * cf;
  const int per = (hw + nchunks - 1) / nchunks;
  const int p0 = k * per, p1 = p0 + per < hw ? p0 + per : hw;
  Row row = {};
  if (BWD) row = load_row(params + (long long)r * 8);
  double s0 = 0.0, s1 = 0.0;
  for (int p = p0 + (int)threadIdx.x; p < p1; p += NTH) {
    if (BWD) {
      const int y = p / w;
      if (!live_out(row, y, p - y * w, h, w)) continue;
    }
    float v[MAXC];
    load_valid<VEC>(x + ((long long)r * hw + p) * pitch, nvalid, v);
#pragma unroll
    for (int ch = 0; ch < MAXC; ++ch) {
      if (ch < cf) s0 += (double)v[ch];
      else s1 += (double)v[ch];        // (0 behind the valid channels)
    }
  }
  s0 = acg::block_sum(s0, scratch);
  s1 = acg::block_sum(s1, scratch);
  if (threadIdx.x == 0) {
    partials[((long long)r * 2 + 0) * nchunks + k] = s0;
    partials[((long long)r * 2 + 1) * nchunks + k] = s1;
  }
}

// One thread per pixel.  Forward: dst pixel p <- colour map of src pixel p - t, 0 where p is not live; the pad channels are the
// bits of src at p.  BWD (src = dout, dst = din): dst pixel q <- colour adjoint of g' = dout[q + t] where q + t is live, 0
// elsewhere; the pad channels are +0.
template <bool BWD, bool VEC>
__global__ __launch_bounds__(NTH) void d_augment_apply_kernel(const uint32_t* __restrict__ src, const float* __restrict__ params,
                                                              uint32_t* __restrict__ dst, const double* __restrict__ partials, int h, int w,
                                                              int pitch, int frames, int cf, int nchunks, int blocks_per_row) {
  __shared__ double scratch[16];
  __shared__ float means[2];
  const int r = blockIdx.x / blocks_per_row, p = (blockIdx.x % blocks_per_row) * NTH + (int)threadIdx.x;
  const int hw = h * w, nvalid = frames * cf;
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    double t = (int)threadIdx.x < nchunks ? partials[((long long)r * 2 + f) * nchunks + threadIdx.x] : 0.0;
    t = acg::block_sum(t, scratch);
    if (threadIdx.x == 0) means[f] = (float)(t / ((double)hw * (double)cf));
  }
  __syncthreads();
  const Row row = load_row(params + (long long)r * 8);
  const float add0 = fmaf(row.k3, means[0], BWD ? 0.f : row.b), add1 = fmaf(row.k3, means[1], BWD ? 0.f : row.b);
  if (p >= hw) return;                // (behind every barrier)
  const int y = p / w, xx = p - y * w;
  const int oy = BWD ? y + row.ty : y, ox = BWD ? xx + row.tx : xx;        // the output pixel of the forward pass this thread is about
  const bool live = live_out(row, oy, ox, h, w);
  const int sp = BWD ? oy * w + ox : (y - row.ty) * w + (xx - row.tx);       // read only when live: then inside [0, hw)
  const long long rbase = (long long)r * hw;
  float v[MAXC] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) load_valid<VEC>(src + (rbase + sp) * pitch, nvalid, v);
  float a0 = 0.f, a1 = 0.f;
#pragma unroll
  for (int ch = 0; ch < MAXC; ++ch) {
    if (ch < cf) a0 += v[ch];
    else a1 += v[ch];
  }
  const float fcf = (float)cf;
  const float pm0 = a0 / fcf, pm1 = a1 / fcf;
  uint32_t o[MAXC];
#pragma unroll
  for (int ch = 0; ch < MAXC; ++ch) {
    const float val = ch < cf ? fmaf(row.k1, v[ch], fmaf(row.k2, pm0, add0)) : fmaf(row.k1, v[ch], fmaf(row.k2, pm1, add1));
    o[ch] = as_bits((BWD || live) ? val : 0.f);
  }
  const uint32_t* __restrict__ own = src + (rbase + p) * pitch;             // this pixel's own pad channels (forward)
  uint32_t* __restrict__ q = dst + (rbase + p) * pitch;
  if (VEC) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j * 4 < pitch) {
        uint4 pad = make_uint4(0u, 0u, 0u, 0u);
        if (!BWD && j * 4 + 4 > nvalid) pad = *reinterpret_cast<const uint4*>(own + j * 4);
        const int c0 = j * 4;
        *reinterpret_cast<uint4*>(q + c0) = make_uint4(c0 + 0 < nvalid ? o[c0 + 0] : pad.x, c0 + 1 < nvalid ? o[c0 + 1] : pad.y,
                                                      c0 + 2 < nvalid ? o[c0 + 2] : pad.z, c0 + 3 < nvalid ? o[c0 + 3] : pad.w);
      }
    }
    for (int c0 = 8; c0 < pitch; c0 += 4)
      *reinterpret_cast<uint4*>(q + c0) = BWD ? make_uint4(0u, 0u, 0u, 0u) : *reinterpret_cast<const uint4*>(own + c0);
  } else {
#pragma unroll
    for (int ch = 0; ch < MAXC; ++ch)
      if (ch < nvalid) q[ch] = o[ch];
    for (int ch = nvalid; ch < pitch; ++ch) q[ch] = BWD ? 0u : own[ch];
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the argument rules the three tensor entries share; 0 or the refusal's code
int check_shape(const char* who, int rows, int h, int w, int frames, int cf) {
  ACG_REQUIRE(rows >= 1 && h >= 1 && w >= 1 && frames >= 1 && cf >= 1, ACG_ERR_INVALID_ARG, "%s: rows %d, %d x %d, %d frames of %d channels",
              who, rows, h, w, frames, cf);
  ACG_REQUIRE(rows <= ACG_DA_ROWS_MAX, ACG_ERR_UNSUPPORTED, "%s: %d rows (at most %d)", who, rows, ACG_DA_ROWS_MAX);
  ACG_REQUIRE(h <= SIDE_MAX && w <= SIDE_MAX, ACG_ERR_UNSUPPORTED, "%s: %d x %d pixels (at most %d a side)", who, h, w, SIDE_MAX);
  ACG_REQUIRE(frames <= 2 && cf <= 4, ACG_ERR_UNSUPPORTED, "%s: %d frames of %d channels (at most 2 of 4)", who, frames, cf);
  return 0;
}

template <bool BWD>
int launch(const char* who, const float* src, const float* params, float* dst, int rows, int h, int w, int pitch, int frames, int cf,
           void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  ACG_REQUIRE(src && params && dst, ACG_ERR_INVALID_ARG, "%s: null pointer", who);
  ACG_REQUIRE(src != dst, ACG_ERR_INVALID_ARG, "%s: in and out are the same buffer (the transform is not in place)", who);
  if (const int rc = check_shape(who, rows, h, w, frames, cf)) return rc;
  ACG_REQUIRE(pitch >= frames * cf, ACG_ERR_INVALID_ARG, "%s: %d frames of %d channels at a pitch of %d", who, frames, cf, pitch);
  const int nchunks = chunks_for(h, w);
  const int64_t need = (int64_t)rows * 2 * nchunks * (int64_t)sizeof(double);
  ACG_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, ACG_ERR_INVALID_ARG,
              "%s: the workspace must be 8-byte aligned and hold %lld bytes (got %lld)", who, (long long)need, (long long)workspace_bytes);
  const bool vec = pitch % 4 == 0 && aligned16(src) && aligned16(dst);
  const int bpr = (h * w + NTH - 1) / NTH;
  const dim3 sum_grid((unsigned)(rows * nchunks)), apply_grid((unsigned)((int64_t)rows * bpr));
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
  uint32_t* d = reinterpret_cast<uint32_t*>(dst);
  double* partials = static_cast<double*>(workspace);
  if (vec) {
    ACG_LAUNCH((d_augment_sum_kernel<BWD, true>), sum_grid, dim3(NTH), 0, stream, s, params, partials, h, w, pitch, frames, cf, nchunks);
    ACG_LAUNCH((d_augment_apply_kernel<BWD, true>), apply_grid, dim3(NTH), 0, stream, s, params, d, (const double*)partials, h, w, pitch,
               frames, cf, nchunks, bpr);
  } else {
    ACG_LAUNCH((d_augment_sum_kernel<BWD, false>), sum_grid, dim3(NTH), 0, stream, s, params, partials, h, w, pitch, frames, cf, nchunks);
    ACG_LAUNCH((d_augment_apply_kernel<BWD, false>), apply_grid, dim3(NTH), 0, stream, s, params, d, (const double*)partials, h, w, pitch,
               frames, cf, nchunks, bpr);
  }
  return acg::check_launch(who);
}

}  // namespace

extern "C" {

int32_t acg_d_augment_draw(uint64_t* state, float* params, int32_t rows, int32_t h, int32_t w, int32_t policy, int32_t stream_id,
                           acg_stream_t stream) {
  ACG_REQUIRE(state && params, ACG_ERR_INVALID_ARG, "d_augment_draw: null pointer");
  ACG_REQUIRE(rows >= 1 && h >= 1 && w >= 1 && policy >= 0, ACG_ERR_INVALID_ARG, "d_augment_draw: rows %d, %d x %d, policy %d", rows, h, w,
              policy);
  ACG_REQUIRE(rows <= ACG_DA_ROWS_MAX, ACG_ERR_UNSUPPORTED, "d_augment_draw: %d rows (at most %d)", rows, ACG_DA_ROWS_MAX);
  ACG_REQUIRE(h <= SIDE_MAX && w <= SIDE_MAX, ACG_ERR_UNSUPPORTED, "d_augment_draw: %d x %d pixels (at most %d a side)", h, w, SIDE_MAX);
  ACG_REQUIRE(policy <= (ACG_DA_COLOR | ACG_DA_TRANSLATION | ACG_DA_CUTOUT), ACG_ERR_UNSUPPORTED, "d_augment_draw: policy %d has unknown bits",
              policy);
  ACG_LAUNCH(d_augment_draw_kernel, dim3(1), dim3(NTH), 0, acg::to_stream(stream), (unsigned long long*)state, params, (int)rows, (int)h,
             (int)w, (int)policy, (uint32_t)stream_id ^ ACG_DA_STREAM_TAG);
  return acg::check_launch("d_augment_draw");
}

int64_t acg_d_augment_workspace_bytes(int32_t rows, int32_t h, int32_t w, int32_t frames, int32_t cf) {
  if (rows < 1 || rows > ACG_DA_ROWS_MAX || h < 1 || w < 1 || h > SIDE_MAX || w > SIDE_MAX || frames < 1 || frames > 2 || cf < 1 || cf > 4)
    return 0;
  return (int64_t)rows * 2 * chunks_for(h, w) * (int64_t)sizeof(double);
}

int32_t acg_d_augment_fwd(const float* in, const float* params, float* out, int32_t rows, int32_t h, int32_t w, int32_t pitch,
                          int32_t frames, int32_t cf, void* workspace, int64_t workspace_bytes, acg_stream_t stream) {
  return launch<false>("d_augment_fwd", in, params, out, rows, h, w, pitch, frames, cf, workspace, workspace_bytes, acg::to_stream(stream));
}

int32_t acg_d_augment_bwd(const float* dout, const float* params, float* din, int32_t rows, int32_t h, int32_t w, int32_t pitch,
                          int32_t frames, int32_t cf, void* workspace, int64_t workspace_bytes, acg_stream_t stream) {
  return launch<true>("d_augment_bwd", dout, params, din, rows, h, w, pitch, frames, cf, workspace, workspace_bytes, acg::to_stream(stream));
}

}  // extern "C"
