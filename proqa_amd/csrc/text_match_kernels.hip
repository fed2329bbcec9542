// Answer pre-filter of the matched-paragraph file (qa/prepro_dense.py:process_ground_paras of the reference): which of a
// question's retrieved passages can contain one of its answer aliases at all.  The reference tokenises every (question,
// passage) pair; eval_retrieval._may_match rejects most pairs first with substring tests on the folded text.  This file is
// that test on the device: the folded texts of the corpus live in HBM (proqa_textstore), the candidate rows are the ids a
// search left on the device, and one bit per (question, slot) comes back.
//
// Store layout: every distinct text starts at a multiple of 16 bytes and is followed by zeros up to the next multiple, so a
// 16-byte load that starts inside a text never leaves the allocation.  A row is (offset / 16, length); matching never looks
// past `length`, so neither the padding nor a neighbouring text can complete a needle.
//
// text_prefilter: a workgroup of four waves takes one question and four mask words; the question's needle record (alias
// masks, token offsets, token bytes; built on the host) goes into LDS once.  A wave owns ONE mask word: it walks the word's
// 32 slots, passage after passage, and stores the word with a plain store.  Per passage and 1 KiB step every lane loads
// 16 bytes (one coalesced 1 KiB wave load; the first step of the NEXT passage is in flight while this one is matched) into
// the wave's LDS window, which also holds the 272 bytes that follow, so a needle of up to 255 bytes may straddle the step.
// Per distinct token the lane screens its 16 start positions by the token's first two bytes on the four dwords it already
// holds (a zero-byte test that may over-accept, never miss) and compares the token from the window only where that hit.  A token found anywhere in the wave (ballot) sets its bit in a
// wave-uniform 128-bit mask; lane a holds alias a's mask of required tokens, so "some alias complete" is one ballot, and the
// passage is left as soon as it holds.  No atomics, no order dependence: the bits are a function of the inputs alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <new>
#include <unordered_map>
#include <vector>

#include "common.h"

struct proqa_textstore {
  int device = 0;
  int64_t rows = 0;
  int64_t text_bytes = 0;   // bytes of the device blob (distinct texts, padded)
  void* blob = nullptr;     // device
  void* spans = nullptr;    // device: rows x {uint32 offset / 16, uint32 length}
};

struct proqa_text_needles {
  int device = 0;
  int64_t nq = 0;
  void* recs = nullptr;     // device: the questions' needle records, each a multiple of 16 bytes
  void* qrec = nullptr;     // device: nq x {uint32 offset / 16, uint32 sixteenths}
};

namespace proqa {
namespace {

constexpr int kWaves = 4;                 // waves of a workgroup = mask words of a workgroup
constexpr int kStep = 1024;               // text bytes a wave loads per step (16 per lane)
constexpr int kOverlap = 272;             // bytes kept behind a step: 255 of the longest token, rounded up to 17 lanes' loads
constexpr int kWindow = kStep + kOverlap;
constexpr int kMaxTokenBytes = 255;
constexpr int kMaxTokens = 128;           // distinct tokens of a question (two 64-bit words of found bits)
constexpr int kMaxAliases = 64;           // one lane per alias
constexpr int kMaxNeedleBytes = 4096;
constexpr int kMaxK = 16384;
// needle record of a question: header {n_tokens, n_aliases, 0, 0}, kMaxAliases-at-most alias masks (2 x uint64), token
// offsets (n_tokens + 1) x uint16, token bytes; every part starts at a multiple of 16
constexpr int kRecHeader = 16;
constexpr int kRecMax = kRecHeader + kMaxAliases * 16 + 272 /* 129 offsets, rounded */ + kMaxNeedleBytes;

struct Span {
  uint32_t off16;
  uint32_t len;
};

__device__ __forceinline__ void wave_lds_sync() {
  // the window is written and read by the lanes of ONE wave: order its LDS traffic, no workgroup barrier (the waves of a
  // workgroup walk passages of different lengths)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// bit 7 of every zero byte of x is set -- and, through the borrow, possibly that of bytes above a zero byte: a screen that
// never misses, for positions that are compared in full afterwards (the other bits are garbage: mask with 0x80808080)
__device__ __forceinline__ unsigned zero_bytes_screen(unsigned x) { return (x - 0x01010101u) & ~x; }

__device__ __forceinline__ uint4 load_piece(const uint8_t* __restrict__ text, unsigned pos, unsigned len) {
  // a piece that starts inside the text lies inside the store's allocation (texts are padded to 16 bytes)
  return pos < len ? *reinterpret_cast<const uint4*>(text + pos) : make_uint4(0, 0, 0, 0);
}

// grid: nq * blocks_per_q workgroups; workgroup b serves question b / blocks_per_q, words (b % blocks_per_q) * kWaves ...
__global__ __launch_bounds__(kWaves * 64) void text_prefilter(const uint8_t* __restrict__ blob, const Span* __restrict__ spans,
                                                              long long rows, const long long* __restrict__ ids, int k,
                                                              int n_words, int blocks_per_q, const uint8_t* __restrict__ recs,
                                                              const Span* __restrict__ qrec, uint32_t* __restrict__ mask_out) {
  __shared__ __attribute__((aligned(16))) uint8_t rec[kRecMax];
  __shared__ __attribute__((aligned(16))) uint8_t window[kWaves][kWindow];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long q = blockIdx.x / blocks_per_q;
  const int word = (int)(blockIdx.x % blocks_per_q) * kWaves + wave;
  {
    const Span r = qrec[q];
    const uint4* src = reinterpret_cast<const uint4*>(recs + (size_t)r.off16 * 16);
    const unsigned n16 = min(r.len, (unsigned)(kRecMax / 16));
    for (unsigned i = threadIdx.x; i < n16; i += kWaves * 64) reinterpret_cast<uint4*>(rec)[i] = src[i];
  }
  __syncthreads();
  if (word >= n_words) return;   // wave-uniform; no workgroup barrier below

  const int n_tokens = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(rec)[0]);
  const int n_aliases = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(rec)[1]);
  const unsigned long long* alias_mask = reinterpret_cast<const unsigned long long*>(rec + kRecHeader);
  const uint16_t* tok_off = reinterpret_cast<const uint16_t*>(rec + kRecHeader + n_aliases * 16);
  const uint8_t* tok_bytes = rec + kRecHeader + n_aliases * 16 + ((n_tokens + 1) * 2 + 15) / 16 * 16;
  const bool has_alias = lane < n_aliases;
  const unsigned long long need0 = has_alias ? alias_mask[2 * lane] : 0ull;
  const unsigned long long need1 = has_alias ? alias_mask[2 * lane + 1] : 0ull;
  const bool empty_alias = __ballot(has_alias && (need0 | need1) == 0ull) != 0ull;   // matches every row of the store

  // lane i < 32 looks after slot i of the word: its id and its row's span
  const int slot = word * 32 + (lane & 31);
  long long id = -1;
  if (lane < 32 && slot < k) id = ids[q * k + slot];
  const bool valid = id >= 0 && id < rows;
  Span mine = {0u, 0u};
  if (valid) mine = spans[id];
  unsigned todo = (unsigned)__ballot(valid);   // (lanes 32.. are never valid)
  unsigned bits = 0;
  if (empty_alias) {
    bits = todo;
    todo = 0;
  } else if (n_aliases == 0 || n_tokens == 0) {
    todo = 0;
  }

  uint8_t* win = window[wave];
  uint4 piece = make_uint4(0, 0, 0, 0);
  if (todo) {
    const int i = __builtin_ctz(todo);
    piece = load_piece(blob + (size_t)(unsigned)__shfl((int)mine.off16, i, 64) * 16, lane * 16, (unsigned)__shfl((int)mine.len, i, 64));
  }
  while (todo) {
    const int i = __builtin_ctz(todo);
    todo &= todo - 1;
    const uint8_t* text = blob + (size_t)(unsigned)__shfl((int)mine.off16, i, 64) * 16;
    const unsigned len = (unsigned)__shfl((int)mine.len, i, 64);
    uint4 cur = piece;
    if (todo) {   // the next passage's first step, in flight while this one is matched
      const int i2 = __builtin_ctz(todo);
      piece = load_piece(blob + (size_t)(unsigned)__shfl((int)mine.off16, i2, 64) * 16, lane * 16, (unsigned)__shfl((int)mine.len, i2, 64));
    }
    unsigned long long found0 = 0ull, found1 = 0ull;
    bool hit_row = false;
    for (unsigned base = 0; base < len && !hit_row; base += kStep) {
      if (base) cur = load_piece(text, base + lane * 16, len);
      wave_lds_sync();   // every lane is done with the previous window
      *reinterpret_cast<uint4*>(win + lane * 16) = cur;
      if (base + kStep < len && lane < kOverlap / 16)   // (a text that ends in this step: no start position reads behind it)
        *reinterpret_cast<uint4*>(win + kStep + lane * 16) = load_piece(text, base + kStep + lane * 16, len);
      wave_lds_sync();
      const unsigned at = base + lane * 16;   // text position of this lane's first byte
      // w: the lane's 16 bytes; s: the 16 bytes one position on (the last one is the next lane's first byte; behind the text
      // it is stale, and every start position that would read it is refused by its length)
      const unsigned next = *reinterpret_cast<const unsigned*>(win + lane * 16 + 16);
      const unsigned w[4] = {cur.x, cur.y, cur.z, cur.w};
      const unsigned s[4] = {(w[0] >> 8) | (w[1] << 24), (w[1] >> 8) | (w[2] << 24), (w[2] >> 8) | (w[3] << 24),
                             (w[3] >> 8) | (next << 24)};
      for (int t = 0; t < n_tokens; ++t) {
        if ((t < 64 ? found0 >> t : found1 >> (t - 64)) & 1ull) continue;
        const unsigned t0 = tok_off[t];
        const unsigned tl = tok_off[t + 1] - t0;
        if (tl > len) continue;
        const uint8_t* tb = tok_bytes + t0;
        // screen the 16 start positions by the token's first two bytes, in registers
        const unsigned b0 = tb[0] * 0x01010101u;
        unsigned m[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) m[d] = zero_bytes_screen(w[d] ^ b0);
        if (tl > 1) {
          const unsigned b1 = tb[1] * 0x01010101u;
#pragma unroll
          for (int d = 0; d < 4; ++d) m[d] &= zero_bytes_screen(s[d] ^ b1);
        }
        // one word of candidates: byte j of dword d sits at bit 8 * j + 7 - d
        unsigned cand = (m[0] & 0x80808080u) | (m[1] & 0x80808080u) >> 1 | (m[2] & 0x80808080u) >> 2 | (m[3] & 0x80808080u) >> 3;
        bool hit = false;
        while (cand && !hit) {
          const unsigned b = __builtin_ctz(cand);
          cand &= cand - 1;
          const unsigned j = (7 - (b & 7)) * 4 + (b >> 3);
          if (at + j + tl > len) continue;   // would end behind the text
          const uint8_t* p = win + lane * 16 + j;
          unsigned n = 0;
          while (n < tl && p[n] == tb[n]) ++n;
          hit = n == tl;
        }
        if (__ballot(hit) != 0ull) {
          if (t < 64) found0 |= 1ull << t; else found1 |= 1ull << (t - 64);
          hit_row = __ballot(has_alias && (need0 & found0) == need0 && (need1 & found1) == need1) != 0ull;
          if (hit_row) break;
        }
      }
    }
    if (hit_row) bits |= 1u << i;
  }
  if (lane == 0) mask_out[q * n_words + word] = bits;
}

// one wave per question: the popcount of its mask words
__global__ __launch_bounds__(256) void text_prefilter_count(const uint32_t* __restrict__ mask, long long nq, int n_words,
                                                            int* __restrict__ count_out) {
  const int lane = threadIdx.x & 63;
  const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  int n = 0;
  for (int w = lane; w < n_words; w += 64) n += __popc(mask[q * n_words + w]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
  if (lane == 0) count_out[q] = n;
}

struct SpanKey {
  int64_t lo, hi;
  bool operator==(const SpanKey& o) const { return lo == o.lo && hi == o.hi; }
};
struct SpanKeyHash {
  size_t operator()(const SpanKey& s) const {
    return (size_t)((uint64_t)s.lo * 0x9E3779B97F4A7C15ull ^ (uint64_t)s.hi * 0xC2B2AE3D27D4EB4Full);
  }
};

}  // namespace
}  // namespace proqa

extern "C" {

int proqa_textstore_create(const void* blob_host, int64_t blob_bytes, const int64_t* spans_host, int64_t rows,
                           proqa_textstore** out) {
  using namespace proqa;
  if (!out) return fail(PROQA_EINVAL, "textstore_create: NULL argument");
  *out = nullptr;
  if (blob_bytes < 0 || rows < 0 || rows >= (1ll << 31) || (!blob_host && blob_bytes > 0) || (!spans_host && rows > 0))
    return fail(PROQA_EINVAL, "textstore_create: bad argument (rows %lld, blob bytes %lld)", (long long)rows,
                (long long)blob_bytes);
  // the device layout, on the host first: every distinct (first, end) span once, in order of first use
  std::vector<Span> spans((size_t)rows);
  std::vector<SpanKey> order;
  uint64_t total = 0;
  try {
    std::unordered_map<SpanKey, uint32_t, SpanKeyHash> seen;
    seen.reserve((size_t)rows);
    for (int64_t r = 0; r < rows; ++r) {
      const SpanKey key = {spans_host[2 * r], spans_host[2 * r + 1]};
      if (key.lo < 0 || key.hi < key.lo || key.hi > blob_bytes || key.hi - key.lo >= (1ll << 31))
        return fail(PROQA_EINVAL, "textstore_create: row %lld has the span [%lld, %lld) outside the blob of %lld bytes",
                    (long long)r, (long long)key.lo, (long long)key.hi, (long long)blob_bytes);
      auto it = seen.find(key);
      if (it == seen.end()) {
        if (total / 16 >= 0xFFFFFFFFull) return fail(PROQA_EINVAL, "textstore_create: more than 64 GiB of text");
        it = seen.emplace(key, (uint32_t)(total / 16)).first;
        order.push_back(key);
        total += round_up<uint64_t>((uint64_t)(key.hi - key.lo), 16);
      }
      spans[(size_t)r] = {it->second, (uint32_t)(key.hi - key.lo)};
    }
  } catch (const std::bad_alloc&) {
    return fail(PROQA_ENOMEM, "textstore_create: out of host memory");
  }
  proqa_textstore* s = new (std::nothrow) proqa_textstore;
  if (!s) return fail(PROQA_ENOMEM, "textstore_create: out of host memory");
  s->rows = rows;
  s->text_bytes = (int64_t)total;
  int rc = PROQA_OK;
  const size_t kStage = 32u << 20;
  void* stage = nullptr;
  do {
    if (const hipError_t e = hipGetDevice(&s->device)) {
      rc = hip_fail(e, "hipGetDevice", __FILE__, __LINE__);
      break;
    }
    if (try_malloc(&s->blob, (size_t)total + 16) != hipSuccess || try_malloc(&s->spans, (size_t)rows * sizeof(Span) + 16) != hipSuccess) {
      rc = fail(PROQA_ENOMEM, "textstore_create: cannot allocate %llu bytes of device memory", (unsigned long long)total);
      break;
    }
    if (hipHostMalloc(&stage, kStage, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      stage = nullptr;
      rc = fail(PROQA_ENOMEM, "textstore_create: cannot allocate the staging buffer");
      break;
    }
    // texts -> staging buffer (padded) -> device, a buffer at a time; a text longer than the buffer goes in slices
    uint64_t dev_pos = 0;   // where the staged bytes start on the device
    size_t fill = 0;
    hipError_t e = hipSuccess;
    auto flush = [&]() {
      if (fill && e == hipSuccess) e = hipMemcpy((char*)s->blob + dev_pos, stage, fill, hipMemcpyHostToDevice);
      dev_pos += fill;
      fill = 0;
    };
    for (const SpanKey& key : order) {
      const char* src = (const char*)blob_host + key.lo;
      uint64_t left = (uint64_t)(key.hi - key.lo);
      const size_t pad = (size_t)(round_up<uint64_t>(left, 16) - left);
      while (left) {
        if (fill == kStage) flush();
        const size_t n = (size_t)(left < kStage - fill ? left : kStage - fill);
        memcpy((char*)stage + fill, src, n);
        fill += n;
        src += n;
        left -= n;
      }
      if (fill + pad > kStage) flush();
      memset((char*)stage + fill, 0, pad);
      fill += pad;
    }
    flush();
    if (e == hipSuccess) e = hipMemset((char*)s->blob + total, 0, 16);
    if (e == hipSuccess && rows) e = hipMemcpy(s->spans, spans.data(), (size_t)rows * sizeof(Span), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = hip_fail(e, "textstore upload", __FILE__, __LINE__);
  } while (0);
  if (stage) (void)hipHostFree(stage);
  if (rc != PROQA_OK) {
    if (s->blob) (void)hipFree(s->blob);
    if (s->spans) (void)hipFree(s->spans);
    delete s;
    return rc;
  }
  *out = s;
  return PROQA_OK;
}

int proqa_textstore_destroy(proqa_textstore* s) {
  if (!s) return PROQA_OK;
  PROQA_ON_DEVICE(s->device);
  const hipError_t e1 = hipFree(s->blob), e2 = hipFree(s->spans);
  delete s;
  PROQA_HIP(e1);
  PROQA_HIP(e2);
  return PROQA_OK;
}

int proqa_textstore_info(const proqa_textstore* s, int64_t* rows, int64_t* device_text_bytes) {
  if (!s) return proqa::fail(PROQA_EINVAL, "textstore_info: NULL store");
  if (rows) *rows = s->rows;
  if (device_text_bytes) *device_text_bytes = s->text_bytes;
  return PROQA_OK;
}

int proqa_text_needles_create(const void* token_bytes, const int64_t* token_off, const int64_t* question_token_off,
                              const int32_t* alias_tokens, const int64_t* alias_off, const int64_t* question_alias_off,
                              int64_t nq, proqa_text_needles** out) {
  using namespace proqa;
  if (!out) return fail(PROQA_EINVAL, "text_needles_create: NULL argument");
  *out = nullptr;
  if (nq < 0 || nq >= (1ll << 24)) return fail(PROQA_EINVAL, "text_needles_create: nq %lld out of range", (long long)nq);
  if (nq > 0 && (!token_off || !question_token_off || !alias_off || !question_alias_off))
    return fail(PROQA_EINVAL, "text_needles_create: NULL argument");
  // every limit is checked, and the records are built, before the device is touched
  std::vector<uint8_t> recs;
  std::vector<Span> qrec((size_t)nq);
  try {
    for (int64_t q = 0; q < nq; ++q) {
      const int64_t t0 = question_token_off[q], t1 = question_token_off[q + 1];
      const int64_t a0 = question_alias_off[q], a1 = question_alias_off[q + 1];
      if (t0 < 0 || t1 < t0 || a0 < 0 || a1 < a0)
        return fail(PROQA_EINVAL, "text_needles_create: question %lld: descending offsets", (long long)q);
      const int64_t nt = t1 - t0, na = a1 - a0;
      if (nt > kMaxTokens)
        return fail(PROQA_EINVAL, "text_needles_create: question %lld has %lld distinct tokens (limit %d)", (long long)q,
                    (long long)nt, kMaxTokens);
      if (na > kMaxAliases)
        return fail(PROQA_EINVAL, "text_needles_create: question %lld has %lld aliases (limit %d)", (long long)q, (long long)na,
                    kMaxAliases);
      if ((nt > 0 && !token_bytes) || (na > 0 && alias_off[a1] > alias_off[a0] && !alias_tokens))
        return fail(PROQA_EINVAL, "text_needles_create: NULL argument");
      const int64_t b0 = token_off[t0], b1 = token_off[t1];
      if (b0 < 0 || b1 < b0) return fail(PROQA_EINVAL, "text_needles_create: question %lld: descending offsets", (long long)q);
      for (int64_t t = t0; t < t1; ++t) {
        const int64_t tl = token_off[t + 1] - token_off[t];
        if (tl < 1 || tl > kMaxTokenBytes)
          return fail(PROQA_EINVAL, "text_needles_create: question %lld: a token of %lld bytes (1..%d allowed)", (long long)q,
                      (long long)tl, kMaxTokenBytes);
      }
      if (b1 - b0 > kMaxNeedleBytes)
        return fail(PROQA_EINVAL, "text_needles_create: question %lld has %lld needle bytes (limit %d)", (long long)q,
                    (long long)(b1 - b0), kMaxNeedleBytes);
      const size_t off_bytes = (size_t)round_up<int64_t>((nt + 1) * 2, 16);
      const size_t rec_bytes = kRecHeader + (size_t)na * 16 + off_bytes + (size_t)round_up<int64_t>(b1 - b0, 16);
      const size_t start = recs.size();
      recs.resize(start + rec_bytes, 0);
      uint8_t* rec = recs.data() + start;
      const int32_t head[4] = {(int32_t)nt, (int32_t)na, 0, 0};
      memcpy(rec, head, 16);
      uint64_t* masks = reinterpret_cast<uint64_t*>(rec + kRecHeader);
      for (int64_t a = a0; a < a1; ++a) {
        if (alias_off[a] < 0 || alias_off[a + 1] < alias_off[a])
          return fail(PROQA_EINVAL, "text_needles_create: question %lld: descending offsets", (long long)q);
        uint64_t m[2] = {0, 0};
        for (int64_t e = alias_off[a]; e < alias_off[a + 1]; ++e) {
          const int32_t t = alias_tokens[e];
          if (t < 0 || t >= nt)
            return fail(PROQA_EINVAL, "text_needles_create: question %lld: alias token index %d outside its %lld tokens",
                        (long long)q, t, (long long)nt);
          m[t >> 6] |= 1ull << (t & 63);
        }
        memcpy(&masks[2 * (a - a0)], m, 16);
      }
      uint16_t* offs = reinterpret_cast<uint16_t*>(rec + kRecHeader + na * 16);
      for (int64_t t = t0; t <= t1; ++t) offs[t - t0] = (uint16_t)(token_off[t] - b0);
      if (b1 > b0) memcpy(rec + kRecHeader + na * 16 + off_bytes, (const uint8_t*)token_bytes + b0, (size_t)(b1 - b0));
      if (start / 16 > 0xFFFFFFFFull) return fail(PROQA_EINVAL, "text_needles_create: needle table too large");
      qrec[(size_t)q] = {(uint32_t)(start / 16), (uint32_t)(rec_bytes / 16)};
    }
  } catch (const std::bad_alloc&) {
    return fail(PROQA_ENOMEM, "text_needles_create: out of host memory");
  }
  proqa_text_needles* n = new (std::nothrow) proqa_text_needles;
  if (!n) return fail(PROQA_ENOMEM, "text_needles_create: out of host memory");
  n->nq = nq;
  int rc = PROQA_OK;
  do {
    hipError_t e = hipGetDevice(&n->device);
    if (e == hipSuccess) e = try_malloc(&n->recs, recs.size() + 16);
    if (e == hipSuccess) e = try_malloc(&n->qrec, qrec.size() * sizeof(Span) + 16);
    if (e == hipSuccess && !recs.empty()) e = hipMemcpy(n->recs, recs.data(), recs.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && nq) e = hipMemcpy(n->qrec, qrec.data(), qrec.size() * sizeof(Span), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = hip_fail(e, "needle table upload", __FILE__, __LINE__);
  } while (0);
  if (rc != PROQA_OK) {
    if (n->recs) (void)hipFree(n->recs);
    if (n->qrec) (void)hipFree(n->qrec);
    delete n;
    return rc;
  }
  *out = n;
  return PROQA_OK;
}

int proqa_text_needles_destroy(proqa_text_needles* n) {
  if (!n) return PROQA_OK;
  PROQA_ON_DEVICE(n->device);
  const hipError_t e1 = hipFree(n->recs), e2 = hipFree(n->qrec);
  delete n;
  PROQA_HIP(e1);
  PROQA_HIP(e2);
  return PROQA_OK;
}

int proqa_text_prefilter(const proqa_textstore* store, const proqa_text_needles* needles, const int64_t* ids_dev, int64_t nq,
                         int k, uint32_t* mask_out, int32_t* count_out, void* stream) {
  using namespace proqa;
  if (k < 1 || k > kMaxK) return fail(PROQA_EINVAL, "text_prefilter: k %d outside 1..%d", k, kMaxK);
  if (nq < 0) return fail(PROQA_EINVAL, "text_prefilter: negative nq %lld", (long long)nq);
  if (!store) return fail(PROQA_EINVAL, "text_prefilter: NULL store");
  if (!needles) return fail(PROQA_EINVAL, "text_prefilter: NULL needle table");
  if (nq != needles->nq)
    return fail(PROQA_EINVAL, "text_prefilter: nq %lld, the needle table holds %lld questions", (long long)nq,
                (long long)needles->nq);
  if (nq == 0) return PROQA_OK;
  if (!ids_dev || !mask_out) return fail(PROQA_EINVAL, "text_prefilter: NULL argument");
  if (store->device != needles->device) return fail(PROQA_EINVAL, "text_prefilter: store and needle table on different devices");
  PROQA_ON_DEVICE(store->device);
  const int n_words = ceil_div(k, 32);
  const int blocks_per_q = ceil_div(n_words, kWaves);   // nq < 2^24, blocks_per_q <= 128: the grid stays below 2^31
  text_prefilter<<<dim3((unsigned)(nq * blocks_per_q)), dim3(kWaves * 64), 0, as_stream(stream)>>>(
      (const uint8_t*)store->blob, (const Span*)store->spans, (long long)store->rows, (const long long*)ids_dev, k, n_words,
      blocks_per_q, (const uint8_t*)needles->recs, (const Span*)needles->qrec, mask_out);
  PROQA_LAUNCH_CHECK();
  if (count_out) {
    text_prefilter_count<<<dim3((unsigned)ceil_div<int64_t>(nq, 4)), dim3(256), 0, as_stream(stream)>>>(mask_out, (long long)nq,
                                                                                                       n_words, count_out);
    PROQA_LAUNCH_CHECK();
  }
  return PROQA_OK;
}

}  // extern "C"
