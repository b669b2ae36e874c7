// values.hip — the value read-out of plain sets: RoaringBitmap.toArray, contains, rankLong and select
// (RoaringBitmap.java:3224, 1693, 2574, 2820) for a batch, decoded on the device from the containers where they lie.
//
// Everything rests on one derived item kept with the set: cpre[c] = the members held by the set's containers
// before container c (u64[nc + 1], the exclusive prefix of `card`).  A bitmap's members start at cpre[begin[b]], so
// the decode needs no pass of its own to place a container's values, rank adds the containers below the key in one
// load, and select finds its container with one search.
//
//   k_set_values    one wave per container (the store-bound hot path): every store instruction of a wave writes 64
//                   consecutive values, whatever the container type (Bitmap and Run go through an LDS stage)
//   k_set_contains  one query per lane: independent gathers (a key search, then container_has)
//   k_set_rank /    one wave per query: the search is wave-uniform, the part inside the container takes the 64
//   k_set_select    lanes (popcounts of a Bitmap's words, the lengths of a Run's runs)
#include <algorithm>
#include <cstring>

#include "internal.hpp"
#include "kernels.hpp"
#include "lookup.hpp"
#include "wave.hpp"

namespace rbg {

// ---------------------------------------------------------------- the prefix of the cardinalities
__global__ __launch_bounds__(256) void k_set_card64(const uint32_t *__restrict__ card, uint64_t n,
                                                    uint64_t *__restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) out[i] = card[i];
}
// offs[i] = members of the bitmaps [first, first + i), i in [0, count]
__global__ __launch_bounds__(256) void k_set_value_offsets(const uint64_t *__restrict__ begin,
                                                           const uint64_t *__restrict__ cpre, uint32_t first,
                                                           uint32_t count, uint64_t *__restrict__ offs) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i <= count) offs[i] = cpre[begin[first + i]] - cpre[begin[first]];
}

// ---------------------------------------------------------------- toArray
constexpr int kValWin = 4096; // values of one 64-word step of a Bitmap, at most (low halves, u16)
// The decode: one wave per container of [c0, c1), four per block, grid-stride.  Container c's values go to
// dst[cpre[c] - cpre[c0] ...), ascending.
//   Array   the u16 values widened, lane <-> value
//   Bitmap  64 words per step, lane <-> word: popcount, wave scan, each lane scatters its bit positions to their
//           ranks in the wave's LDS window, and the window leaves with lane <-> rank, four ranks per lane in flight
//   Run     64 runs per step, lane <-> run, lengths scanned.  Long runs (32 values a run or more on average) stream
//           out one run at a time, lane <-> value, with no LDS; short ones stage the scanned lengths in LDS and each
//           output slot finds its run there (a search over 64 entries, four slots per lane in flight), lane <-> slot
// Nothing is written when the call's total offs[count] exceeds cap, and no store goes past the container's own
// range or the total.
__global__ __launch_bounds__(256, 2) void k_set_values(SetView s, const uint64_t *__restrict__ cpre, uint64_t c0,
                                                       uint64_t c1, const uint64_t *__restrict__ offs, uint32_t count,
                                                       uint64_t cap, uint32_t *__restrict__ dst, uint64_t *stats) {
  __shared__ __attribute__((aligned(16))) uint16_t win[4][kValWin];
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t total = offs[count];
  if (total > cap) return;
  const uint64_t p0 = cpre[c0];
  uint64_t inb = 0, nout = 0; // this wave's share of the call's counters
  for (uint64_t c = c0 + (uint64_t)blockIdx.x * 4 + wv; c < c1; c += (uint64_t)gridDim.x * 4) {
    const int type = s.type[c];
    const uint32_t card = s.card[c], nr = s.nruns[c], hi = (uint32_t)s.key[c] << 16;
    const uint8_t *p = s.payload + s.off[c];
    const uint64_t pos = cpre[c] - p0, lim = min(pos + card, total);
    inb += payload_bytes(type, card, nr) + 16;
    nout += lim - pos;
    if (type == kArray) {
      const uint16_t *a = reinterpret_cast<const uint16_t *>(p);
      for (uint32_t i0 = 0; i0 < card; i0 += 256) { // four loads in flight per lane
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t i = i0 + 64 * k + lane;
          v[k] = i < card ? a[i] : 0u;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t i = i0 + 64 * k + lane;
          if (i < card && pos + i < lim) dst[pos + i] = hi | v[k];
        }
      }
    } else if (type == kBitmap) {
      const uint64_t *w = reinterpret_cast<const uint64_t *>(p);
      uint16_t *sw = win[wv];
      uint64_t g0 = pos;
      uint64_t nx = w[lane];
      for (int step = 0; step < 16; ++step) {
        uint64_t x = nx;
        if (step < 15) nx = w[(step + 1) * 64 + lane]; // the next step's word is in flight during this one
        const uint32_t n = (uint32_t)__popcll(x);
        const uint32_t incl = wave_scan_u32(n, lane), T = readlane(incl, 63);
        if (!T) continue;
        // The kernel is bound by instruction issue in these two loops, not by its stores or the LDS (the scattered
        // ranks of neighbouring lanes lie a popcount apart and do conflict, with LDS time to spare): the word goes
        // as two 32-bit halves, whose find-first-bit and clear-lowest-bit are one instruction each.
        uint16_t *o = sw + (incl - n);
        const uint32_t base = (uint32_t)(step * 64 + lane) * 64;
        for (uint32_t h = (uint32_t)x; h; h &= h - 1) *o++ = (uint16_t)(base + (uint32_t)__builtin_ctz(h));
        for (uint32_t h = (uint32_t)(x >> 32); h; h &= h - 1) *o++ = (uint16_t)(base + 32 + (uint32_t)__builtin_ctz(h));
        wave_lds_sync();
        const uint32_t nw = (uint32_t)min((uint64_t)T, lim > g0 ? lim - g0 : 0ull); // T when card matches the payload
        for (uint32_t i0 = 0; i0 < nw; i0 += 256) {
          uint32_t v[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = sw[(i0 + 64 * k + lane) & (kValWin - 1)];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const uint32_t i = i0 + 64 * k + lane;
            if (i < nw) dst[g0 + i] = hi | v[k];
          }
        }
        wave_lds_sync();
        g0 += T;
      }
    } else {
      const uint32_t *rl = reinterpret_cast<const uint32_t *>(p);
      uint32_t *sr = reinterpret_cast<uint32_t *>(win[wv]); // [0, 64) slots up to each run's end, [64, 128) start - slot
      uint64_t g0 = pos;
      for (uint32_t r0 = 0; r0 < nr; r0 += 64) {
        const bool live = r0 + lane < nr;
        const uint32_t q = live ? rl[r0 + lane] : 0u, len = live ? (q >> 16) + 1 : 0u;
        const uint32_t incl = wave_scan_u32(len, lane), T = readlane(incl, 63);
        const uint32_t nrc = min(nr - r0, 64u);
        const uint32_t nw = (uint32_t)min((uint64_t)T, lim > g0 ? lim - g0 : 0ull); // T when card matches the payload
        if (T >= 32 * nrc) {
          for (uint32_t k = 0; k < nrc; ++k) { // run k of the step: its start, length and first slot, wave-uniform
            const uint32_t st = readlane(q & 0xFFFF, (int)k), ln = readlane(len, (int)k);
            const uint32_t ex = readlane(incl - len, (int)k);
            for (uint32_t i = (uint32_t)lane; i < ln; i += 64)
              if (ex + i < nw) dst[g0 + ex + i] = hi | ((st + i) & 0xFFFF);
          }
        } else {
          sr[lane] = incl;
          sr[64 + lane] = (q & 0xFFFF) - (incl - len);
          wave_lds_sync();
          for (uint32_t i0 = 0; i0 < nw; i0 += 256) {
            uint32_t k[4] = {0, 0, 0, 0}; // per slot: the first run whose slots end after it (a slot past T: run 63)
#pragma unroll
            for (uint32_t h = 32; h; h >>= 1) {
#pragma unroll
              for (int u = 0; u < 4; ++u)
                if (sr[k[u] + h - 1] <= i0 + 64 * u + lane) k[u] += h;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const uint32_t i = i0 + 64 * u + lane;
              if (i < nw) dst[g0 + i] = hi | ((i + sr[64 + k[u]]) & 0xFFFF);
            }
          }
          wave_lds_sync();
        }
        g0 += T;
      }
    }
  }
  if (lane == 0 && inb) {
    const uint32_t stripe = (blockIdx.x * 4 + wv) & (kStripes - 1);
    atomicAdd((unsigned long long *)&stats[0 * kStripes + stripe], (unsigned long long)inb);
    atomicAdd((unsigned long long *)&stats[1 * kStripes + stripe], (unsigned long long)(4 * nout));
    atomicAdd((unsigned long long *)&stats[7 * kStripes + stripe], (unsigned long long)nout);
  }
}

// ---------------------------------------------------------------- contains / rank / select
// first container c of [lo, hi) with key[c] >= hb (hi: none)
__device__ __forceinline__ uint64_t key_lower_bound(const uint16_t *key, uint64_t lo, uint64_t hi, uint32_t hb) {
  uint64_t n = hi - lo;
  while (n) {
    const uint64_t h = n >> 1;
    if (key[lo + h] < hb) {
      lo += h + 1;
      n -= h + 1;
    } else {
      n = h;
    }
  }
  return lo;
}

__global__ __launch_bounds__(256, 2) void k_set_contains(SetView s, const uint32_t *__restrict__ bitmap,
                                                         const uint32_t *__restrict__ values, uint64_t n,
                                                         uint8_t *__restrict__ out) {
  for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (uint64_t)gridDim.x * 256) {
    const uint32_t b = bitmap ? bitmap[q] : 0u, v = values[q], hb = v >> 16;
    const uint64_t hi = s.begin[b + 1], c = key_lower_bound(s.key, s.begin[b], hi, hb);
    bool has = false;
    if (c < hi && s.key[c] == hb) has = container_has(s.type[c], s.payload + s.off[c], s.card[c], s.nruns[c], v & 0xFFFF);
    out[q] = has ? 1 : 0;
  }
}

// rankLong: the members of the containers below x's key from the prefix, plus the members <= x of the container at
// the key.  Array: a search; Bitmap: the lanes popcount the words up to x's (the last one masked); Run: the lanes
// stride over the runs, each giving x + 1 - start clamped to [0, length].
__global__ __launch_bounds__(256, 2) void k_set_rank(SetView s, const uint64_t *__restrict__ cpre,
                                                     const uint32_t *__restrict__ bitmap,
                                                     const uint32_t *__restrict__ values, uint64_t n,
                                                     uint64_t *__restrict__ out) {
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint64_t q = (uint64_t)blockIdx.x * 4 + wv; q < n; q += (uint64_t)gridDim.x * 4) {
    const uint32_t b = bitmap ? bitmap[q] : 0u, v = values[q], hb = v >> 16, x = v & 0xFFFF;
    const uint64_t lo = s.begin[b], hi = s.begin[b + 1], c = key_lower_bound(s.key, lo, hi, hb);
    uint64_t rank = cpre[c] - cpre[lo];
    if (c < hi && s.key[c] == hb) { // wave-uniform
      const int type = s.type[c];
      const uint8_t *p = s.payload + s.off[c];
      if (type == kArray) {
        rank += lower_bound_u16(reinterpret_cast<const uint16_t *>(p), s.card[c], x + 1);
      } else if (type == kBitmap) {
        const uint64_t *w = reinterpret_cast<const uint64_t *>(p);
        const uint32_t last = x >> 6;
        const uint64_t mask = ~0ull >> (63 - (x & 63));
        uint32_t cnt = 0;
        for (uint32_t j = (uint32_t)lane; j <= last; j += 64) cnt += (uint32_t)__popcll(j == last ? w[j] & mask : w[j]);
        rank += wave_sum_u32(cnt);
      } else {
        const uint32_t *rl = reinterpret_cast<const uint32_t *>(p);
        const uint32_t nr = s.nruns[c];
        uint32_t cnt = 0;
        for (uint32_t j = (uint32_t)lane; j < nr; j += 64) {
          const uint32_t r = rl[j], st = r & 0xFFFF;
          cnt += min((r >> 16) + 1, max(x + 1, st) - st); // the run's members <= x: x + 1 - start clamped to [0, length]
        }
        rank += wave_sum_u32(cnt);
      }
    }
    if (lane == 0) out[q] = rank;
  }
}

// select: the container comes from a search of the prefix within the bitmap's containers, then the r-th member
// of it.  Array: one load; Bitmap: each lane owns 16 contiguous words, their popcounts are scanned and the owning
// lane walks its words to the bit; Run: the lengths are scanned 64 runs at a time.
__global__ __launch_bounds__(256, 2) void k_set_select(SetView s, const uint64_t *__restrict__ cpre,
                                                       const uint32_t *__restrict__ bitmap,
                                                       const uint64_t *__restrict__ js, uint64_t n,
                                                       uint32_t *__restrict__ out, uint8_t *__restrict__ found) {
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint64_t q = (uint64_t)blockIdx.x * 4 + wv; q < n; q += (uint64_t)gridDim.x * 4) {
    const uint32_t b = bitmap ? bitmap[q] : 0u;
    const uint64_t j = js[q], lo = s.begin[b], hi = s.begin[b + 1], base = cpre[lo];
    bool done = false; // wave-uniform: some lane has written the answer
    if (j < cpre[hi] - base) {
      const uint64_t target = base + j;
      uint64_t c = lo, m = hi - lo; // the last container of [lo, hi) with cpre[c] <= target
      while (m > 1) {
        const uint64_t h = m >> 1;
        if (cpre[c + h] <= target) {
          c += h;
          m -= h;
        } else {
          m = h;
        }
      }
      const uint32_t r = (uint32_t)(target - cpre[c]), hb = (uint32_t)s.key[c] << 16;
      const int type = s.type[c];
      const uint8_t *p = s.payload + s.off[c];
      if (type == kArray) {
        if (lane == 0 && r < s.card[c]) {
          out[q] = hb | reinterpret_cast<const uint16_t *>(p)[r];
          found[q] = 1;
        }
        done = r < s.card[c];
      } else if (type == kBitmap) {
        const uint64_t *w = reinterpret_cast<const uint64_t *>(p) + lane * 16;
        uint32_t cnt = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const uint4 u = reinterpret_cast<const uint4 *>(w)[k];
          cnt += (uint32_t)(__popc(u.x) + __popc(u.y) + __popc(u.z) + __popc(u.w));
        }
        const uint32_t incl = wave_scan_u32(cnt, lane);
        const uint64_t own = __ballot(incl > r);
        if (own) {
          if (lane == __builtin_ctzll(own)) {
            uint32_t rr = r - (incl - cnt), val = 0;
            for (int k = 0; k < 16; ++k) {
              uint64_t x = w[k];
              const uint32_t pc = (uint32_t)__popcll(x);
              if (rr < pc) {
                for (; rr; --rr) x &= x - 1;
                val = (uint32_t)(lane * 16 + k) * 64 + (uint32_t)__builtin_ctzll(x);
                break;
              }
              rr -= pc;
            }
            out[q] = hb | val;
            found[q] = 1;
          }
          done = true;
        }
      } else {
        const uint32_t *rl = reinterpret_cast<const uint32_t *>(p);
        const uint32_t nr = s.nruns[c];
        uint32_t rr = r;
        for (uint32_t r0 = 0; r0 < nr && !done; r0 += 64) {
          const bool live = r0 + lane < nr;
          const uint32_t rn = live ? rl[r0 + lane] : 0u, len = live ? (rn >> 16) + 1 : 0u;
          const uint32_t incl = wave_scan_u32(len, lane), T = readlane(incl, 63);
          if (rr < T) {
            const uint64_t own = __ballot(incl > rr);
            if (lane == __builtin_ctzll(own)) {
              out[q] = hb | (((rn & 0xFFFF) + rr - (incl - len)) & 0xFFFF);
              found[q] = 1;
            }
            done = true;
          } else {
            rr -= T;
          }
        }
      }
    }
    if (!done && lane == 0) { // j at or past the cardinality
      out[q] = 0;
      found[q] = 0;
    }
  }
}

// ---------------------------------------------------------------- host side
static unsigned nblk(uint64_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }
constexpr uint64_t kMaxBlocks = 2048; // 256 CUs x 8 blocks; the rest is grid-stride

// the set's prefix of cardinalities, built once on the set's stream (the set is immutable) and timed like the
// other derived items; 4 B read and 8 B written per container
static int ensure_card_prefix(const rbgpu_set *cs) {
  rbgpu_set *s = const_cast<rbgpu_set *>(cs);
  if (s->cpre) return RB_OK;
  Scratch w(s->ctx->pool);
  hipStream_t st = s->ctx->stream;
  uint64_t *pre = nullptr, *c64 = nullptr, *tmp = nullptr;
  if (!w.get(pre, s->nc + 1) || !w.get(c64, s->nc) || !w.get(tmp, scan_tmp_words(s->nc) + 1))
    return fail(RB_ENOMEM, "cardinality prefix of %llu containers", (unsigned long long)s->nc);
  {
    DeriveTimer t(s, -1);
    if (s->nc) k_set_card64<<<(unsigned)std::min<uint64_t>(nblk(s->nc, 256), kMaxBlocks), 256, 0, st>>>(s->card, s->nc, c64);
    scan_exclusive(c64, pre, s->nc, tmp, st);
  } // the timer's end waits for the stream: the scratch is free again
  if (hipGetLastError() != hipSuccess) return fail(RB_EDEVICE, "cardinality-prefix kernels failed");
  s->cpre = w.keep(pre);
  s->derive_bytes += 12ull * s->nc;
  return RB_OK;
}

int set_values(const rbgpu_set *s, uint32_t first, uint32_t count, uint32_t *dst, uint64_t cap, uint64_t *offsets,
               bool host_dst) {
  rbgpu_ctx *ctx = s->ctx;
  hipStream_t st = ctx->stream;
  int rc = ensure_h_begin(s);
  if (rc) return rc;
  const uint64_t c0 = s->h_begin[first], c1 = s->h_begin[(size_t)first + count], ncont = c1 - c0;
  if (!ncont) { // no bitmap, or none with a container: no launch
    for (uint32_t i = 0; i <= count; ++i) offsets[i] = 0;
    stats_begin(ctx);
    return stats_end(ctx, 0, 0, nullptr, 0);
  }
  rc = ensure_card_prefix(s);
  if (rc) return rc;
  stats_begin(ctx);
  Scratch w(ctx->pool);
  uint64_t *d_offs = nullptr;
  uint32_t *d_dst = host_dst ? nullptr : dst;
  if (!w.get(d_offs, count + 1ull)) return fail(RB_ENOMEM, "value offsets of %u bitmaps", count);
  auto decode = [&]() { // between the call's kernel events
    hipError_t e = hipEventRecord(ctx->ev[1], st);
    if (e == hipSuccess) {
      k_set_values<<<(unsigned)std::min<uint64_t>(nblk(ncont, 4), kMaxBlocks), 256, 0, st>>>(
          s->view(), s->cpre, c0, c1, d_offs, count, cap, d_dst, ctx->d_stats);
      e = hipEventRecord(ctx->ev[2], st);
    }
    return e;
  };
  k_set_value_offsets<<<nblk(count + 1ull, 256), 256, 0, st>>>(s->begin, s->cpre, first, count, d_offs);
  // device output: the decode follows in stream order with no host wait (it writes nothing when the total exceeds cap)
  bool decoded = false;
  hipError_t e = hipSuccess;
  if (dst && !host_dst) {
    e = decode();
    decoded = true;
  }
  if (e == hipSuccess) e = hipMemcpyAsync(offsets, d_offs, (count + 1ull) * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return fail(RB_EDEVICE, "set values failed: %s", hipGetErrorString(e));
  const uint64_t total = offsets[count];
  if (dst && total > cap)
    return fail(RB_EINVAL, "set values: %llu values exceed the capacity %llu", (unsigned long long)total,
                (unsigned long long)cap);
  if (dst && host_dst && total) { // host output: the staging buffer takes the size the read-back gave
    if (!w.get(d_dst, total)) return fail(RB_ENOMEM, "set values: %llu values", (unsigned long long)total);
    e = decode();
    decoded = true;
    if (e == hipSuccess) e = hipMemcpyAsync(dst, d_dst, total * 4, hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return fail(RB_EDEVICE, "set values failed: %s", hipGetErrorString(e));
  }
  const KernelSpan spans[1] = {{"k_set_values", 0, 1, ncont}};
  return decoded ? stats_end(ctx, ncont, 0, spans, 1) : stats_end(ctx, 0, 0, spans, 0);
}

int set_lookup(const rbgpu_set *s, int kind, const uint32_t *bitmap, const void *queries, uint64_t n, void *out,
               uint8_t *found) {
  static const char *const kName[3] = {"k_set_contains", "k_set_rank", "k_set_select"};
  rbgpu_ctx *ctx = s->ctx;
  hipStream_t st = ctx->stream;
  if (!n) { // no launch
    stats_begin(ctx);
    return stats_end(ctx, 0, 0, nullptr, 0);
  }
  if (kind != kLookupContains) {
    const int rc = ensure_card_prefix(s);
    if (rc) return rc;
  }
  stats_begin(ctx);
  const size_t qsz = kind == kLookupSelect ? 8 : 4, osz = kind == kLookupContains ? 1 : kind == kLookupRank ? 8 : 4;
  Scratch w(ctx->pool);
  uint32_t *d_b = nullptr;
  uint8_t *d_q = nullptr, *d_o = nullptr, *d_f = nullptr;
  if ((bitmap && !w.get(d_b, n)) || !w.get(d_q, n * qsz) || !w.get(d_o, n * osz) ||
      (kind == kLookupSelect && !w.get(d_f, n)))
    return fail(RB_ENOMEM, "set lookups of %llu queries", (unsigned long long)n);
  hipError_t e = hipMemcpyAsync(d_q, queries, n * qsz, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && bitmap) e = hipMemcpyAsync(d_b, bitmap, n * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipEventRecord(ctx->ev[1], st);
  if (e == hipSuccess) {
    const SetView v = s->view();
    const unsigned waves = (unsigned)std::min<uint64_t>(nblk(n, 4), 2 * kMaxBlocks);
    if (kind == kLookupContains)
      k_set_contains<<<(unsigned)std::min<uint64_t>(nblk(n, 256), kMaxBlocks), 256, 0, st>>>(
          v, d_b, reinterpret_cast<const uint32_t *>(d_q), n, d_o);
    else if (kind == kLookupRank)
      k_set_rank<<<waves, 256, 0, st>>>(v, s->cpre, d_b, reinterpret_cast<const uint32_t *>(d_q), n,
                                        reinterpret_cast<uint64_t *>(d_o));
    else
      k_set_select<<<waves, 256, 0, st>>>(v, s->cpre, d_b, reinterpret_cast<const uint64_t *>(d_q), n,
                                          reinterpret_cast<uint32_t *>(d_o), d_f);
    e = hipEventRecord(ctx->ev[2], st);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_o, n * osz, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && kind == kLookupSelect) e = hipMemcpyAsync(found, d_f, n, hipMemcpyDeviceToHost, st);
  if (e != hipSuccess) return fail(RB_EDEVICE, "set lookups failed: %s", hipGetErrorString(e));
  const KernelSpan spans[1] = {{kName[kind], -1, -1, n}};
  return stats_end(ctx, n, 0, spans, 1);
}

// this file's code object, loaded at context creation (rbgpu_open, context.hip)
__global__ void k_warm_values() {}
void warm_values(hipStream_t st) { k_warm_values<<<1, 64, 0, st>>>(); }

} // namespace rbg
