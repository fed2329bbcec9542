// The dropout masks of retriever training: a counter-based generator, so that a mask is a pure function of
// (seed, site, call, coordinates) and every kernel that needs it -- the forward, and the backward kernels that recompute
// what the forward saw -- regenerates the same bits.  No mask tensor ever reaches memory.
//
// Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), key = (seed & 0xffffffff,
// seed >> 32).  One call gives four 32-bit words = eight 16-bit decisions: decision (w, h) is bits 16h .. 16h+15 of word w.
// An element is KEPT iff its 16 bits >= thr, thr = min(65535, floor(p * 65536 + 0.5)); the effective rate is thr / 65536
// and the survivors are scaled by 1 / (1 - thr / 65536), computed in fp32.
//
// Coordinates.  site (8 bits): 0 the embeddings, 1 + 3 layer + {0 attention probabilities, 1 attention output, 2 FFN
// output}.  call (24 bits, wraps): the host's count of tower passes in training mode.
//   hidden element (row, col) of a packed [T, H] matrix:  counter (col >> 3, row, 0, site | call << 8),
//                                                         w = (col & 7) >> 1, h = col & 1
//   probability (b, head, query i, key j):                counter (j >> 2, i >> 1, b * n_heads + head, site | call << 8),
//                                                         w = j & 3, h = i & 1
// (four consecutive keys of a query are one call: the forward's and attention_bwd_dq's accumulator layout; four consecutive
// queries of a key are two calls: attention_bwd_dkv's.)  tests/dropout_oracle.py restates all of this in numpy.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PROQA_HD __host__ __device__ __forceinline__
#else
#define PROQA_HD inline
#endif

namespace proqa {

struct Philox4 {
  uint32_t w[4];
};

PROQA_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// what a kernel is handed: the key, the last counter word, the threshold and the survivors' factor
struct DropoutParams {
  uint32_t key0, key1, c3, thr;
  float factor;
};

inline uint32_t dropout_threshold(double p) {
  const double t = p * 65536.0 + 0.5;
  return t >= 65535.0 ? 65535u : (t <= 0.0 ? 0u : (uint32_t)t);   // (truncation of a positive value = floor)
}

// p in [0, 1), site in [0, 255]; call wraps at 24 bits
inline bool make_dropout_params(double p, uint64_t seed, int site, uint32_t call, DropoutParams* out) {
  if (!(p >= 0.0) || !(p < 1.0) || site < 0 || site > 255) return false;
  out->key0 = (uint32_t)(seed & 0xffffffffu);
  out->key1 = (uint32_t)(seed >> 32);
  out->c3 = (uint32_t)site | (call << 8);
  out->thr = dropout_threshold(p);
  out->factor = 1.0f / (1.0f - (float)out->thr / 65536.0f);
  return true;
}

PROQA_HD uint32_t dropout_bits(const Philox4& r, int w, int h) { return (r.w[w] >> (16 * h)) & 0xffffu; }

// the eight decisions of columns 8 chunk .. 8 chunk + 7 of a hidden row
PROQA_HD Philox4 dropout_hidden_call(const DropoutParams& d, uint32_t row, uint32_t chunk) {
  return philox4x32_10(chunk, row, 0u, d.c3, d.key0, d.key1);
}
PROQA_HD bool dropout_hidden_keep(const DropoutParams& d, const Philox4& r, int i) {   // i = col & 7
  return dropout_bits(r, i >> 1, i & 1) >= d.thr;
}

// the eight decisions of keys 4 kgroup .. 4 kgroup + 3 of queries 2 qpair, 2 qpair + 1 of (sequence, head) `pair`
PROQA_HD Philox4 dropout_prob_call(const DropoutParams& d, uint32_t pair, uint32_t qpair, uint32_t kgroup) {
  return philox4x32_10(kgroup, qpair, pair, d.c3, d.key0, d.key1);
}
PROQA_HD bool dropout_prob_keep(const DropoutParams& d, const Philox4& r, int query, int key) {
  return dropout_bits(r, key & 3, query & 1) >= d.thr;
}

}  // namespace proqa
