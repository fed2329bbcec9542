// Weight gradient of a linear layer (proqa_linear_wgrad_f16 / proqa_linear_wgrad_plan in proqa_hip.h):
//   dw[N, K] fp32 = (accumulate ? dw : 0) + sum_t dy[t, n] * x[t, k],   dy [T, N], x [T, K] fp16 row-major.
// fp16 operands, one fp32 sum over the whole token axis on v_mfma_f32_32x32x16_f16, fp32 output: the product never
// passes through fp16 (the library's GEMM rounds it there: inf above 65504 at the reference's loss scale and batch).
//
// Orientation.  A = dy^T (rows n), B = x (columns k): lane l of the 32x32x16 MFMA wants A[n = l & 31][t = 8 (l >> 5) + j]
// and B[t = 8 (l >> 5) + j][k = l & 31], j = 0..7 -- for BOTH operands 8 consecutive t of one column of a row-major
// tile whose row index is t.  The tiles are staged [t][column] exactly as they come from memory (16-byte chunks,
// coalesced) and read back with ds_read_b64_tr_b16, the transposed LDS read of gfx950: two reads (4 t each) make one
// fragment.  Chosen over the DPP transposition of attention_bwd_dkv because that one transposes while STAGING (a second,
// transposed image written with 2-byte stores); here both operands need only the transposed view, so the hardware read
// leaves no extra image, no extra stores and no lane shuffles.  The image is the 256-byte-row form with the 16-byte
// chunk index XORed by ((t & 3) << 2) | ((t >> 2) & 3), which keeps the transposed reads of the 32x32x16 operand free of
// bank conflicts.  Requirements of the instruction, all met by construction: EXEC is all ones at every read (the reads sit in
// workgroup-uniform control flow of 256-thread workgroups; edges are padded with zeros, never masked), every lane's
// address is 8-byte aligned, the LDS array is 16-byte aligned.
//
// Tiling.  A workgroup of 4 waves owns a 128 (n) x 128 (k) tile of dw and one slice of the token axis; a wave owns 64 x 64
// (2 x 2 accumulators of 32 x 32).  The contraction step is kStep = 32 tokens: global -> registers for step s + 1 is
// issued before the MFMAs of step s, registers -> LDS after them (two LDS stages, one barrier per step).  Rows at or
// past T and columns at or past N / K are written to LDS as zeros and never read from memory; edge tiles predicate
// their stores.
//
// Split and reduction order (determinism).  proqa_linear_wgrad_plan cuts the token axis into `splits` slices whose
// boundaries are multiples of kStep, as a pure function of (T, N, K, n_cus); no slice is empty.  splits == 1: the
// workgroup writes (or adds to) dw itself.  Otherwise it writes its partial tile to ws[slice][N][K] (every element of
// every slice, so nothing of the workspace's previous contents is read) and wgrad_reduce adds the slices in ascending
// order, the existing dw last.  No atomics, one fixed association: the result is bit-identical from run to run.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): wgrad_tile_kernel<0 / 2> 76 VGPRs + 64 AGPRs
// (<1>: 103 + 64), 50-52 SGPRs, 32768 bytes of LDS, no scratch, no spills, occupancy 3 waves / SIMD; wgrad_reduce 12 VGPRs,
// occupancy 8.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "common.h"

namespace proqa {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 128;            // output tile edge (n and k)
constexpr int kStep = 32;             // tokens per contraction step (two MFMA k-steps of 16)
constexpr int kMinStepsPerSlice = 4;  // a slice is at least 128 tokens (the last one may be shorter)
constexpr int kRowBytes = kTile * 2;  // one LDS row: 128 fp16
constexpr int kStageBytes = 2 * kStep * kRowBytes;   // dy tile + x tile of one step

// byte offset of 16-byte chunk ch (0..15) of row t (0..31) in a [32][128 x fp16] image
__device__ __forceinline__ int image_off(int t, int ch) {
  return kRowBytes * t + 16 * (ch ^ (((t & 3) << 2) | ((t >> 2) & 3)));
}

__device__ __forceinline__ f16x4 read_tr(const char* lds, int byte_off) {
  typedef __fp16 fp16x4 __attribute__((ext_vector_type(4)));
  typedef fp16x4 __attribute__((address_space(3))) * lds_ptr;
  const fp16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_ptr)(lds + byte_off));
  return __builtin_bit_cast(f16x4, v);
}

// One (tile, slice) workgroup.  MODE 0: dw = sum; 1: dw += sum; 2: ws[slice] = sum.
template <int MODE>
__global__ __launch_bounds__(256) void wgrad_tile_kernel(const _Float16* __restrict__ dy, const _Float16* __restrict__ x,
                                                         long long T, int N, int K, int tiles_k, int n_tiles,
                                                         long long steps_per_slice, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kStageBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x % n_tiles, slice = blockIdx.x / n_tiles;
  const int n0 = (tile / tiles_k) * kTile, k0 = (tile % tiles_k) * kTile;
  const long long t_begin = (long long)slice * steps_per_slice * kStep;
  const long long t_end = std::min<long long>(T, t_begin + steps_per_slice * kStep);
  const int n_steps = (int)((t_end - t_begin + kStep - 1) / kStep);      // >= 1 by the plan

  // staging: chunk ids tid and tid + 256 of the 512 chunks of a [32][16 chunks] tile, for dy and for x
  const int st_row = tid >> 4, st_ch = tid & 15;                          // rows st_row and st_row + 16
  const bool dy_col_ok = n0 + st_ch * 8 < N, x_col_ok = k0 + st_ch * 8 < K;
  const _Float16* dy_src = dy + n0 + st_ch * 8;
  const _Float16* x_src = x + k0 + st_ch * 8;
  const int st_off0 = image_off(st_row, st_ch), st_off1 = image_off(st_row + 16, st_ch);
  const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  f16x8 rdy[2], rx[2];
  auto load_step = [&](int s) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long long t = t_begin + (long long)s * kStep + st_row + 16 * i;
      rdy[i] = rx[i] = zero8;
      if (t < t_end) {
        if (dy_col_ok) rdy[i] = *(const f16x8*)(dy_src + t * N);
        if (x_col_ok) rx[i] = *(const f16x8*)(x_src + t * K);
      }
    }
  };
  auto store_step = [&](int stage) {
    char* base = smem + stage * kStageBytes;
    *(f16x8*)(base + st_off0) = rdy[0];
    *(f16x8*)(base + st_off1) = rdy[1];
    *(f16x8*)(base + kStep * kRowBytes + st_off0) = rx[0];
    *(f16x8*)(base + kStep * kRowBytes + st_off1) = rx[1];
  };

  // transposed reads: lane 4q + p of 16-lane group g supplies row q, columns 4p .. 4p + 3 of a 4-row x 16-column block and
  // receives column (lane & 15) of its 4 rows.  Groups 0 / 1 are columns 0..15 / 16..31 of the 32-wide operand at
  // t = 0..7 of the k-step, groups 2 / 3 the same columns at t = 8..15; read u (0, 1) takes t + 4u.
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int wn = (wave >> 1) * 64, wk = (wave & 1) * 64;                  // the wave's 64 x 64 corner in the tile
  int a_off[2][2], b_off[2][2];                                           // [32-wide sub-tile][u], k-step 0 of stage 0
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = 8 * (g >> 1) + 4 * u + q;
      a_off[m][u] = image_off(t, (wn + 32 * m) / 8 + 2 * (g & 1) + (p >> 1)) + 8 * (p & 1);
      b_off[m][u] = kStep * kRowBytes + image_off(t, (wk + 32 * m) / 8 + 2 * (g & 1) + (p >> 1)) + 8 * (p & 1);
    }

  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  load_step(0);
  store_step(0);
  __syncthreads();
  for (int s = 0; s < n_steps; ++s) {
    const bool more = s + 1 < n_steps;                                    // workgroup-uniform
    if (more) load_step(s + 1);
    const char* stage = smem + (s & 1) * kStageBytes;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      // image_off's XOR term does not depend on bit 4 of t: k-step 1 is the same addresses 16 rows further
      f16x8 a[2], b[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const f16x4 a_lo = read_tr(stage, a_off[m][0] + ks * 16 * kRowBytes), a_hi = read_tr(stage, a_off[m][1] + ks * 16 * kRowBytes);
        const f16x4 b_lo = read_tr(stage, b_off[m][0] + ks * 16 * kRowBytes), b_hi = read_tr(stage, b_off[m][1] + ks * 16 * kRowBytes);
        a[m] = __builtin_shufflevector(a_lo, a_hi, 0, 1, 2, 3, 4, 5, 6, 7);
        b[m] = __builtin_shufflevector(b_lo, b_hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[m], b[n], acc[m][n], 0, 0, 0);
    }
    if (more) store_step((s + 1) & 1);
    __syncthreads();
  }

  // C/D map of the 32x32 MFMA: column (k) = lane & 31, row (n) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float* dst = MODE == 2 ? out + (size_t)slice * (size_t)N * (size_t)K : out;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int kk = k0 + wk + 32 * n + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int nn = n0 + wn + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (nn < N && kk < K) {
          float* ptr = dst + (size_t)nn * K + kk;
          *ptr = MODE == 1 ? *ptr + acc[m][n][r] : acc[m][n][r];
        }
      }
    }
}

// dw = ws[0] + ws[1] + ... + ws[splits - 1] (+ dw, last); four elements per thread
__global__ __launch_bounds__(256) void wgrad_reduce(const float* __restrict__ ws, int splits, long long n_vec4, float* dw,
                                                    int accumulate) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_vec4) return;
  const f32x4* src = (const f32x4*)ws;
  f32x4 s = src[i];
  for (int b = 1; b < splits; ++b) s += src[(long long)b * n_vec4 + i];
  f32x4* out = (f32x4*)dw;
  out[i] = accumulate ? s + out[i] : s;
}

}  // namespace
}  // namespace proqa

using namespace proqa;

extern "C" {

int proqa_linear_wgrad_plan(int64_t T, int N, int K, int n_cus, int* splits, size_t* ws_bytes) {
  if (!splits || !ws_bytes) return fail(PROQA_EINVAL, "linear_wgrad_plan: NULL argument");
  if (T < 0 || N <= 0 || K <= 0 || N % 8 || K % 8)
    return fail(PROQA_EINVAL, "linear_wgrad_plan: T=%lld must be >= 0, N=%d and K=%d positive multiples of 8", (long long)T, N, K);
  if (n_cus <= 0) return fail(PROQA_EINVAL, "linear_wgrad_plan: n_cus=%d must be positive", n_cus);
  const int64_t tiles = (int64_t)ceil_div(N, kTile) * ceil_div(K, kTile);
  const int64_t steps = ceil_div<int64_t>(T, kStep);
  // two workgroups per compute unit when the token axis allows it, no slice shorter than kMinStepsPerSlice steps
  int64_t want = std::min<int64_t>(ceil_div<int64_t>(2 * (int64_t)n_cus, tiles), std::max<int64_t>(1, steps / kMinStepsPerSlice));
  want = std::max<int64_t>(1, std::min<int64_t>(want, 4096));
  const int64_t per = std::max<int64_t>(1, ceil_div<int64_t>(steps, want));
  const int64_t n = std::max<int64_t>(1, ceil_div<int64_t>(steps, per));     // no empty slice
  *splits = (int)n;
  *ws_bytes = n > 1 ? (size_t)n * (size_t)N * (size_t)K * sizeof(float) : 0;
  return PROQA_OK;
}

int proqa_linear_wgrad_f16(const void* dy, const void* x, int64_t T, int N, int K, float* dw, int accumulate, void* ws,
                           size_t ws_bytes, void* stream) {
  if (!dw) return fail(PROQA_EINVAL, "linear_wgrad: NULL dw");
  if (T < 0 || N <= 0 || K <= 0 || N % 8 || K % 8)
    return fail(PROQA_EINVAL, "linear_wgrad: T=%lld must be >= 0, N=%d and K=%d positive multiples of 8", (long long)T, N, K);
  if (T > 0 && (!dy || !x)) return fail(PROQA_EINVAL, "linear_wgrad: NULL operand");
  if (((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dw | (uintptr_t)ws) & 15)
    return fail(PROQA_EINVAL, "linear_wgrad: dy, x, dw and ws must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  if (T == 0) {
    if (!accumulate) PROQA_HIP(hipMemsetAsync(dw, 0, (size_t)N * (size_t)K * sizeof(float), st));
    return PROQA_OK;
  }
  int splits;
  size_t need;
  if (int rc = proqa_linear_wgrad_plan(T, N, K, device_cu_count(), &splits, &need)) return rc;
  if (need && (!ws || ws_bytes < need))
    return fail(PROQA_EINVAL, "linear_wgrad: workspace of %zu bytes, %zu needed (proqa_linear_wgrad_plan)", ws_bytes, need);
  const int tiles_k = ceil_div(K, kTile), n_tiles = ceil_div(N, kTile) * tiles_k;
  const long long steps = ceil_div<long long>(T, kStep), per = ceil_div<long long>(steps, splits);
  if ((long long)n_tiles * splits > 0x7fffffffll) return fail(PROQA_EINVAL, "linear_wgrad: N=%d x K=%d is too large", N, K);
  const dim3 grid((unsigned)(n_tiles * splits)), block(256);
  const _Float16* a = (const _Float16*)dy;
  const _Float16* b = (const _Float16*)x;
  if (splits == 1) {
    if (accumulate)
      hipLaunchKernelGGL(wgrad_tile_kernel<1>, grid, block, 0, st, a, b, (long long)T, N, K, tiles_k, n_tiles, per, dw);
    else
      hipLaunchKernelGGL(wgrad_tile_kernel<0>, grid, block, 0, st, a, b, (long long)T, N, K, tiles_k, n_tiles, per, dw);
    PROQA_LAUNCH_CHECK();
    return PROQA_OK;
  }
  hipLaunchKernelGGL(wgrad_tile_kernel<2>, grid, block, 0, st, a, b, (long long)T, N, K, tiles_k, n_tiles, per, (float*)ws);
  PROQA_LAUNCH_CHECK();
  const long long n_vec4 = (long long)N * K / 4;
  hipLaunchKernelGGL(wgrad_reduce, dim3((unsigned)ceil_div<long long>(n_vec4, 256)), block, 0, st, (const float*)ws, splits,
                     n_vec4, dw, accumulate);
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

}  // extern "C"
