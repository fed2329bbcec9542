// The body of inbatch_loss_grad and inbatch_loss_blocks_grad (train_kernels.hip), included between the braces of both kernels
// (no include guard): ONE text, so both compile the same instruction sequence on their rectangle.  It reads BY_ROW, xs, nx,
// ys, ny, target, lse, grad_in, nq and dx from the enclosing scope; blockIdx.x is the X tile.
  __shared__ __attribute__((aligned(16))) _Float16 y_lds[32 * kEmbStride];     // [32 y][136]
  __shared__ __attribute__((aligned(16))) _Float16 yt_lds[kEmb * kEmbTStride];  // [128 d][36]
  __shared__ float lse_lds[32];
  __shared__ int tgt_lds[32];
  const int lane = threadIdx.x, li = lane & 31, half = lane >> 5;
  const int x0 = blockIdx.x * 32, x = x0 + li;
  const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  f16x8 xf[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) xf[j] = x < nx ? *(const f16x8*)(xs + (long long)x * kEmb + (2 * j + half) * 8) : zero8;
  // BY_ROW: the statistics of the lane's own question
  const float lse_x = BY_ROW && x < nx ? lse[x] : 0.f;
  const int tgt_x = BY_ROW && x < nx ? (target ? target[x] : x) : -1;
  f32x16 acc[4] = {{0}, {0}, {0}, {0}};
  for (int y0 = 0; y0 < ny; y0 += 32) {
    // stage 32 rows of Y: 32 x 16 pieces of 16 bytes, 8 per lane; (r, c) = (i >> 3, i & 7) of a 64-column half so that rows
    // r and r ^ 1 sit 8 lanes apart (stage_transposed)
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int i = lane + 64 * (it & 3), r = i >> 3, c = i & 7, hc = it >> 2;   // hc: columns 0-63 / 64-127
      const int y = y0 + r;
      const f16x8 v = y < ny ? *(const f16x8*)(ys + (long long)y * kEmb + hc * 64 + c * 8) : zero8;
      *(f16x8*)(y_lds + r * kEmbStride + hc * 64 + c * 8) = v;
      stage_transposed(v, r, c, yt_lds + hc * 64 * kEmbTStride, kEmbTStride);
    }
    if (!BY_ROW && lane < 32) {
      const int y = y0 + lane;       // Y = the questions
      lse_lds[lane] = y < ny ? lse[y] : __builtin_inff();
      tgt_lds[lane] = y < ny ? (target ? target[y] : y) : -1;
    }
    __syncthreads();                 // (one wave: orders the LDS writes before the reads for the compiler)
    f32x16 g = {0};
    const _Float16* yrow = y_lds + li * kEmbStride + half * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) g = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const f16x8*)(yrow + j * 16), xf[j], g, 0, 0, 0);
    // the coefficients as fp16 hi + lo: p - 1 of a gold pair carries the whole gradient of a well-trained row
    f16x8 cf[2], cl[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int yi = (r & 3) + 8 * (r >> 2) + 4 * half, y = y0 + yi;
      float p, hot;
      if (BY_ROW) {
        p = __expf(g[r] - lse_x);
        hot = y == tgt_x ? 1.f : 0.f;
      } else {
        p = __expf(g[r] - lse_lds[yi]);
        hot = tgt_lds[yi] == x ? 1.f : 0.f;
      }
      const float coef = y < ny ? p - hot : 0.f;
      const _Float16 hi = (_Float16)coef;
      cf[r >> 3][r & 7] = hi;
      cl[r >> 3][r & 7] = (_Float16)(coef - (float)hi);
    }
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int k0 = 16 * jj + 4 * half;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f16x8 yt = transposed_fragment(yt_lds, kEmbTStride, 32 * t + li, k0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(yt, cf[jj], acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(yt, cl[jj], acc[t], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // lane = x, registers of acc[t] = columns 32 t + (r & 3) + 8 (r >> 2) + 4 half: 8-byte pieces straight to the row
  if (x >= nx) return;
  const float scale = grad_in[0] / (float)nq;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      f16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (_Float16)(acc[t][gq * 4 + e] * scale);
      *(f16x4*)(dx + (long long)x * kEmb + 32 * t + gq * 8 + 4 * half) = o;
    }
