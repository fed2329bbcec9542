// The body of inbatch_eval and inbatch_eval_blocks, included between the braces of both kernels (no include guard): ONE text,
// so both compile the same instruction sequence on their rectangle.  It reads q, c, target, nq, nc, tiles_per_split, the five
// outputs and partial from the enclosing scope; blockIdx.x is the query tile, blockIdx.y the column split.
  __shared__ RowState red[kWaves][kTile];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 31, half = lane >> 5;
  const int row = blockIdx.x * kTile + li;            // this lane's query row; rows >= nq compute on row nq - 1, unwritten
  const int lrow = row < nq ? row : nq - 1;
  f16x8 qf[8];
  load_frags(qf, q + (size_t)lrow * kRowBytes, half);

  // gold: A row li = passage target[query li]; the diagonal element (li, li) sits in the lane half (li >> 2) & 1 at
  // register (li & 3) + 4 * (li >> 3)
  const int t = target ? target[lrow] : lrow;
  const int target_ok = t >= 0 && t < nc;
  float gold;
  {
    f16x8 af[8];
    load_frags(af, c + (size_t)(target_ok ? t : 0) * kRowBytes, half);
    f32x16 acc = {0};
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[j], qf[j], acc, 0, 0, 0);
    const int dreg = (li & 3) + 4 * (li >> 3);
    float d = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) d = r == dreg ? acc[r] : d;
    const float other = __shfl_xor(d, 32, 64);
    gold = ((li >> 2) & 1) == half ? d : other;
    if (!target_ok) gold = NAN;   // a target outside [0, nc): gold NaN, rank -1
  }
  const bool gold_nan = gold != gold;

  RowState st = {-INFINITY, INT_MAX, 0, 0.f, INT_MAX};
  const int n_tiles = (nc + kTile - 1) / kTile;
  const int tile_lo = blockIdx.y * tiles_per_split;
  const int tile_hi = min(n_tiles, tile_lo + tiles_per_split);
  // the next tile's fragments are requested before the current tile's arithmetic
  f16x8 af[8], nf[8];
  int tile = tile_lo + wave;
  if (tile < tile_hi) load_frags(af, c + (size_t)min(tile * kTile + li, nc - 1) * kRowBytes, half);
  for (; tile < tile_hi; tile += kWaves) {
    const int next = tile + kWaves;
    if (next < tile_hi) load_frags(nf, c + (size_t)min(next * kTile + li, nc - 1) * kRowBytes, half);
    f32x16 acc = {0};
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[j], qf[j], acc, 0, 0, 0);
    // register r of lane (li, half): query li, passage (r & 3) + 8 (r >> 2) + 4 half of the tile -- increasing in r, and
    // a wave's tiles increase, so a strict > keeps the lowest column of equal scores
    const int col0 = tile * kTile + 4 * half;
    float tm = st.m;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int col = col0 + (r & 3) + 8 * (r >> 2);
      const float s = acc[r];
      if (col < nc) {
        const bool s_nan = s != s;
        if (s_nan) {
          st.nan = min(st.nan, col);
        } else if (s > tm || (s == tm && col < st.arg)) {   // (the second clause: the row's first -inf)
          tm = s;
          st.arg = col;
        }
        const bool gt = s_nan ? !gold_nan : s > gold;
        const bool eq = s_nan ? gold_nan : s == gold;
        st.cnt += (col != t && (gt || (eq && col < t))) ? 1 : 0;
      }
    }
    float sum = rescale(st.sum, st.m, tm);
    const float sh = shift_of(tm);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int col = col0 + (r & 3) + 8 * (r >> 2);
      const float s = acc[r];
      if (col < nc && s == s) sum += expf(s - sh);
    }
    st.sum = sum;
    st.m = tm;
    if (next < tile_hi) {
#pragma unroll
      for (int j = 0; j < 8; ++j) af[j] = nf[j];
    }
  }

  // the other lane half holds the other 16 passages of every tile
  {
    RowState o;
    o.m = __shfl_xor(st.m, 32, 64);
    o.arg = __shfl_xor(st.arg, 32, 64);
    o.cnt = __shfl_xor(st.cnt, 32, 64);
    o.sum = __shfl_xor(st.sum, 32, 64);
    o.nan = __shfl_xor(st.nan, 32, 64);
    merge(st, o);
  }
  if (half == 0) red[wave][li] = st;
  __syncthreads();
  if (threadIdx.x < kTile) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) merge(st, red[w][li]);
    if (row < nq) {
      if (partial) {
        Partial p = {st.m, st.sum, st.arg, st.cnt, st.nan};
        partial[(size_t)blockIdx.y * nq + row] = p;
        if (blockIdx.y == 0 && gold_out) gold_out[row] = gold;
      } else {
        finalize(st, gold, target_ok, row, argmax_out, rank_out, max_out, gold_out, lse_out);
      }
    }
  }
