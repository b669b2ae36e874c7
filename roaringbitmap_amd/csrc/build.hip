// build.hip — sets and bit-sliced indexes built from member values on the device: RoaringBitmap.bitmapOf / add(int...)
// (RoaringBitmap.java:483-566), optionally followed by runOptimize (:2764-2775), for a batch of bitmaps, and
// Roaring64BitmapSliceIndex.setValues on a fresh index (longlong/Roaring64BitmapSliceIndex.java:291-348).  The inverse
// of values.hip and of the BSI value read-back.
//
// The pipeline, on one stream:
//   order check       plain sets: does a high key ever descend inside a bitmap?  Asked by discovery's counting pass
//                     over the caller's values where they lie, with one bit per element that starts a bitmap
//                     (k_build_mark_starts).  If not — the common case, and every output of the read-out calls —
//                     nothing is copied or sorted.  BSI: k_bsi_order — do the columns strictly ascend?
//   sort              only when the check says so (build_sort.hip).  Plain sets: key[j] = bitmap << 32 | value
//                     (k_build_keys), sorted on key bits 16 and up: the image below does not care about the order of
//                     the low halves (the reference's partialRadixSort makes the same observation).  BSI sorts the
//                     pairs stably by column; k_bsi_reduce then clears the value of every pair but the last of its
//                     column and reduces min / max over the pairs kept.
//   discovery         a head is an element whose (bitmap, high key) differs from its predecessor's: heads counted
//                     per tile of RB_BUILD_TILE elements (k_build_count_heads), the counts scanned, and each
//                     container's first element and key written at its rank (k_build_write_heads).  64-bit indices.
//   k_set_build       one wave per container, twice: the wave ORs the low halves of its span into an 8 KiB LDS image
//                     with single-bit LDS atomics (duplicates and order cost nothing, a span may be any length),
//                     reads the image into the register bitmap and takes its cardinality and run count (wave.hpp
//                     metrics).  The measuring pass writes type and size; after a scan of the sizes has laid out the
//                     (tight) arena, the emitting pass stages again and writes metadata and payload (emit_container).
// A BSI goes through the same kernels: its candidates are (slice, high key) pairs over the sorted columns, the
// element source becomes a predicate (bit `slice` of the pair's value; none for ebM), and candidates that turn out
// empty are dropped by the scan.  A key's pairs are re-read once per slice.
#include <algorithm>
#include <cstring>
#include <vector>

#include "internal.hpp"
#include "kernels.hpp"
#include "wave.hpp"

namespace rbg {

// build_sort.hip
hipError_t build_sort_keys(void *tmp, size_t *tmp_bytes, const uint64_t *in, uint64_t *out, uint64_t n,
                           unsigned begin_bit, unsigned end_bit, hipStream_t st);
hipError_t build_sort_pairs(void *tmp, size_t *tmp_bytes, const uint32_t *kin, uint32_t *kout, const uint64_t *vin,
                            uint64_t *vout, uint64_t n, hipStream_t st);

constexpr int kTile = RB_BUILD_TILE; // elements per discovery block: 256 threads x 4
static_assert(kTile == 1024, "k_build_count_heads / k_build_write_heads take four elements per thread");
constexpr uint64_t kMaxBlocks = 2048; // 256 CUs x 8 blocks; the rest is grid-stride

// The grouped element stream, in one of three forms:
//   plain sets whose high keys never descend inside a bitmap: the caller's values where they lie (v32) and a bit per
//     element that starts a bitmap (starts) — nothing is copied or sorted;
//   plain sets that had to be sorted: keys[j] = bitmap << 32 | value (v32 null);
//   BSI: the columns, strictly ascending or sorted (v32), and their values (vals); starts null.
struct BuildSrc {
  const uint64_t *keys;
  const uint32_t *v32;
  const uint32_t *starts;
  const uint64_t *vals;
  uint64_t n;
};
__device__ __forceinline__ uint32_t value_of(const BuildSrc &s, uint64_t j) {
  return s.keys ? (uint32_t)s.keys[j] : s.v32[j];
}
__device__ __forceinline__ bool starts_bitmap(const BuildSrc &s, uint64_t j) {
  return s.starts && ((s.starts[j >> 5] >> (j & 31)) & 1u);
}

// ---------------------------------------------------------------- keys and the order checks
// offs[nb + 1] ascending with offs[0] = 0 and offs[nb] = n: element j belongs to the last bitmap b with offs[b] <= j
__global__ __launch_bounds__(256) void k_build_keys(const uint32_t *__restrict__ values,
                                                    const uint64_t *__restrict__ offs, uint32_t nb, uint64_t n,
                                                    uint64_t *__restrict__ keys) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256) {
    uint32_t lo = 0, len = nb; // offs[lo] <= j < offs[lo + len]
    while (len > 1) {
      const uint32_t h = len >> 1;
      if (offs[lo + h] <= j) {
        lo += h;
        len -= h;
      } else {
        len = h;
      }
    }
    keys[j] = ((uint64_t)lo << 32) | values[j];
  }
}
__global__ __launch_bounds__(256) void k_bsi_order(const uint32_t *__restrict__ cols, uint64_t n, uint32_t *unsorted) {
  bool bad = false;
  for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x + 1; j < n; j += (uint64_t)gridDim.x * 256)
    bad |= cols[j] <= cols[j - 1];
  if (__ballot(bad) && lane_id() == 0) atomicOr(unsorted, 1u);
}
// A pair is kept when it is the last of its column (the pairs are sorted stably by column).  mm[0] / mm[1] = min /
// max over the values kept; out (may be null): the values with those of the pairs not kept cleared — their column
// still goes into ebM, where a duplicate costs nothing.
__global__ __launch_bounds__(256) void k_bsi_reduce(const uint32_t *__restrict__ cols, const uint64_t *vals, uint64_t n,
                                                    uint64_t *out /* null, or vals itself */, uint64_t *mm) {
  uint64_t lo = ~0ull, hi = 0;
  for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256) {
    const bool kept = j + 1 == n || cols[j + 1] != cols[j];
    const uint64_t v = vals[j];
    if (out) out[j] = kept ? v : 0ull;
    if (kept) {
      lo = min(lo, v);
      hi = max(hi, v);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, (uint64_t)__shfl_xor((unsigned long long)lo, o));
    hi = max(hi, (uint64_t)__shfl_xor((unsigned long long)hi, o));
  }
  if (lane_id() == 0) {
    atomicMin((unsigned long long *)&mm[0], (unsigned long long)lo);
    atomicMax((unsigned long long *)&mm[1], (unsigned long long)hi);
  }
}

// ---------------------------------------------------------------- container discovery
// `descends` (may be null): set when element j continues its predecessor's bitmap with a smaller high key
__device__ __forceinline__ bool is_head(const BuildSrc &s, uint64_t j, bool *descends = nullptr) {
  if (j >= s.n) return false;
  if (j == 0) return true;
  if (s.keys) return (s.keys[j] >> 16) != (s.keys[j - 1] >> 16);
  const uint32_t hi = s.v32[j] >> 16, before = s.v32[j - 1] >> 16;
  const bool first = starts_bitmap(s, j);
  if (descends && !first && hi < before) *descends = true;
  return first || hi != before;
}
// unsorted (may be null): the order check of plain sets, made in the same pass
__global__ __launch_bounds__(256) void k_build_count_heads(BuildSrc s, uint64_t *__restrict__ tile_heads,
                                                           uint32_t *unsorted) {
  __shared__ uint32_t wt[4];
  const uint64_t base = (uint64_t)blockIdx.x * kTile;
  uint32_t c = 0;
  bool bad = false;
#pragma unroll
  for (int i = 0; i < 4; ++i) c += (uint32_t)__popcll(__ballot(is_head(s, base + 256 * i + threadIdx.x, &bad)));
  // in an unordered input nearly every wave finds a descent: only the waves that still read 0 write the flag (a
  // million atomics on one word take milliseconds)
  if (unsorted && __ballot(bad) && lane_id() == 0 &&
      __hip_atomic_load(unsorted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
    atomicOr(unsorted, 1u);
  if (lane_id() == 0) wt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_heads[blockIdx.x] = wt[0] + wt[1] + wt[2] + wt[3];
}
// bit offs[b] of `starts` for every bitmap b that holds an element
__global__ __launch_bounds__(256) void k_build_mark_starts(const uint64_t *__restrict__ offs, uint32_t nb,
                                                           uint32_t *starts) {
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b < nb && offs[b + 1] > offs[b]) atomicOr(&starts[offs[b] >> 5], 1u << (offs[b] & 31));
}
// tile_pre: the exclusive scan of the tile counts ([tiles] = G).  Container r starts at element cstart[r] and has
// the high key ckey[r]; cstart[G] = n.
__global__ __launch_bounds__(256) void k_build_write_heads(BuildSrc s, const uint64_t *__restrict__ tile_pre,
                                                           uint64_t *__restrict__ cstart, uint16_t *__restrict__ ckey) {
  __shared__ uint32_t wt[4];
  const uint64_t base = (uint64_t)blockIdx.x * kTile;
  const int wv = threadIdx.x >> 6;
  uint64_t r = tile_pre[blockIdx.x];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint64_t j = base + 256 * i + threadIdx.x;
    const bool h = is_head(s, j);
    const uint64_t m = __ballot(h);
    if (lane_id() == 0) wt[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int k = 0; k < 4; ++k) {
      before += k < wv ? wt[k] : 0u;
      total += wt[k];
    }
    if (h) {
      const uint64_t at = r + before + mbcnt64(m);
      cstart[at] = j;
      ckey[at] = (uint16_t)(value_of(s, j) >> 16);
    }
    r += total;
    __syncthreads();
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) cstart[tile_pre[gridDim.x]] = s.n;
}
// plain sets: begin[b] = the containers that start before bitmap b's first element, b in [0, nb]
__global__ __launch_bounds__(256) void k_build_begin(const uint64_t *__restrict__ cstart, uint64_t G,
                                                     const uint64_t *__restrict__ offs, uint32_t nb,
                                                     uint64_t *__restrict__ begin) {
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b > nb) return;
  const uint64_t x = offs[b];
  uint64_t lo = 0, n = G;
  while (n) {
    const uint64_t h = n >> 1;
    if (cstart[lo + h] < x) {
      lo += h + 1;
      n -= h + 1;
    } else {
      n = h;
    }
  }
  begin[b] = lo;
}
// BSI: bitmap `slice` holds the kept candidates of [slice * G, (slice + 1) * G)
__global__ void k_bsi_begin(const uint64_t *__restrict__ tpos, uint64_t G, uint32_t nsl, uint64_t *__restrict__ begin) {
  const uint32_t b = threadIdx.x;
  if (b <= nsl) begin[b] = tpos[(uint64_t)b * G];
}

// ---------------------------------------------------------------- measure and emit
struct BuildArgs {
  BuildSrc src;
  const uint64_t *cstart; // [G + 1]
  const uint16_t *ckey;   // [G]
  uint64_t G;
  uint32_t nsl;           // candidates per group: 1 (plain sets), or the slices and ebM (BSI: nbits + 1)
  int runopt;             // RB_BUILD_RUN_OPTIMIZE
  int emit;               // 0: the measuring pass, 1: the emitting pass
  // per candidate t = slice * G + group, written by the measuring pass: the type (kEmpty: dropped), 1 / 0, and the
  // payload bytes rounded up to 16
  uint8_t *ttype;
  uint64_t *tkeep, *tbytes;
  // their exclusive scans, read by the emitting pass: the candidate's container index and payload offset
  const uint64_t *tpos, *toff;
  OutView out;
  uint8_t *payload;
  uint64_t in_bytes; // the call's input bytes (accounting)
  uint64_t *stats;
};

__global__ __launch_bounds__(256, 2) void k_set_build(BuildArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[4][2048];
  typedef __attribute__((address_space(3))) uint32_t lds_u32;
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t *s = lds[wv];
  lds_u32 *ls = (lds_u32 *)s;
  const uint64_t T = a.G * a.nsl;
  uint64_t outb = 0, members = 0; // this wave's share of the call's counters
  for (uint64_t t = (uint64_t)blockIdx.x * 4 + wv; t < T; t += (uint64_t)gridDim.x * 4) {
    if (a.emit && a.ttype[t] == kEmpty) continue;
    const uint64_t g = t % a.G;
    const uint32_t slice = (uint32_t)(t / a.G);
    const bool pred = a.src.vals && slice + 1 < a.nsl; // a BSI slice (the last bitmap of a BSI is ebM)
    const uint64_t e0 = a.cstart[g], e1 = a.cstart[g + 1];
    lds_zero(s, lane);
    wave_lds_sync();
    // Eight consecutive elements per lane.  LDS atomics of one instruction that hit the same word take turns, and in
    // an ascending span neighbouring elements share words: a lane folds the bits of neighbours with the same word
    // into one atomic first (whatever the order, the image is the same: OR commutes), and a slot left with nothing
    // to add issues none.  A word index is below 2048 whatever the element holds (16 bits >> 5).
    for (uint64_t j0 = e0; j0 < e1; j0 += 512) {
      uint32_t wd[8], bit[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint64_t j = j0 + 8 * lane + k;
        const bool live = j < e1;
        const uint32_t x = live ? value_of(a.src, j) & 0xFFFFu : 0u;
        wd[k] = x >> 5;
        bit[k] = live && (!pred || ((a.src.vals[j] >> slice) & 1ull)) ? 1u << (x & 31) : 0u;
      }
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const bool same = wd[k + 1] == wd[k];
        bit[k + 1] |= same ? bit[k] : 0u;
        bit[k] = same ? 0u : bit[k];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (bit[k]) __hip_atomic_fetch_or(ls + wd[k], bit[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    wave_lds_sync();
    uint64_t w[kW];
    lds_read_words(s, w, lane);
    wave_lds_sync();
    int c, r;
    metrics(w, lane, true, c, r);
    const int ty = c == 0 ? (int)kEmpty : a.runopt ? type_runopt(c, r) : type_ab(c);
    if (!a.emit) {
      if (lane == 0) {
        a.ttype[t] = (uint8_t)ty;
        a.tkeep[t] = c != 0;
        a.tbytes[t] = c ? round16(payload_bytes(ty, (uint32_t)c, (uint32_t)r)) : 0ull;
      }
      continue;
    }
    const uint64_t at = a.tpos[t], off = a.toff[t];
    if (lane == 0) {
      a.out.key[at] = a.ckey[g];
      a.out.type[at] = (uint8_t)ty;
      a.out.card[at] = (uint32_t)c;
      a.out.nruns[at] = (uint16_t)(ty == kRun ? r : 0);
      a.out.off[at] = off;
    }
    outb += emit_container(ty, w, c, r, a.payload + off, s, lane) + 16;
    members += (uint64_t)c;
    wave_lds_sync();
  }
  if (a.emit && lane == 0) {
    const uint32_t stripe = (blockIdx.x * 4 + wv) & (kStripes - 1);
    if (blockIdx.x == 0 && wv == 0) atomicAdd((unsigned long long *)&a.stats[0 * kStripes], (unsigned long long)a.in_bytes);
    if (outb) {
      atomicAdd((unsigned long long *)&a.stats[1 * kStripes + stripe], (unsigned long long)outb);
      atomicAdd((unsigned long long *)&a.stats[7 * kStripes + stripe], (unsigned long long)members);
    }
  }
}

// ---------------------------------------------------------------- host side
namespace {
unsigned nblk(uint64_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }
unsigned grid_for(uint64_t n, unsigned per) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>(nblk(n, per), 1), kMaxBlocks); }

// a set of nb bitmaps without containers
int empty_set(rbgpu_ctx *ctx, uint32_t nb, rbgpu_set **out) {
  SetPtr s;
  int rc = make_set(ctx, nb, 0, 0, s);
  if (rc) return rc;
  stats_begin(ctx);
  if (hipMemsetAsync(s->begin, 0, (nb + 1ull) * 8, ctx->stream) != hipSuccess)
    return fail(RB_EDEVICE, "value build: memset failed");
  s->h_begin.assign((size_t)nb + 1, 0);
  if ((rc = stats_end(ctx, 0, 0, nullptr, 0))) return rc;
  *out = s.release();
  return RB_OK;
}

// Discovery's first half: the heads of every tile counted and scanned; *G = the containers of the stream.  d_flag
// (may be null): plain sets' order check, made in the same pass and read back with G into *unsorted — when it is
// set the counts are void and the caller sorts and comes again.
struct Discovery {
  uint64_t tiles = 0, G = 0;
  uint64_t *tile_pre = nullptr;
};
int discover(rbgpu_ctx *ctx, Scratch &tmp, const BuildSrc &src, uint32_t *d_flag, uint32_t *unsorted, Discovery &d) {
  hipStream_t st = ctx->stream;
  d.tiles = (src.n + kTile - 1) / kTile;
  if (d.tiles >= (1ull << 31)) return fail(RB_EINVAL, "value build: %llu elements in one call", (unsigned long long)src.n);
  uint64_t *tile_heads, *scan_tmp;
  if (!tmp.get(tile_heads, d.tiles) || !tmp.get(d.tile_pre, d.tiles + 1) ||
      !tmp.get(scan_tmp, scan_tmp_words(d.tiles) + 1))
    return fail(RB_ENOMEM, "value build: discovery of %llu elements", (unsigned long long)src.n);
  k_build_count_heads<<<(unsigned)d.tiles, 256, 0, st>>>(src, tile_heads, d_flag);
  scan_exclusive(tile_heads, d.tile_pre, d.tiles, scan_tmp, st);
  HIPCHK(hipMemcpyAsync(&d.G, d.tile_pre + d.tiles, 8, hipMemcpyDeviceToHost, st));
  if (d_flag) HIPCHK(hipMemcpyAsync(unsorted, d_flag, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  LAUNCHCHK();
  return RB_OK;
}

// From the discovered stream to the set: the containers' starts and keys, the measuring pass, the layout, the
// emitting pass.  d_offs: plain sets' element offsets on the device ([nb + 1]); null: a BSI of nb = nsl bitmaps.
// stats_begin has been called.
int build_grouped(rbgpu_ctx *ctx, Scratch &tmp, const BuildSrc &src, const Discovery &d, const uint64_t *d_offs,
                  uint32_t nb, uint32_t nsl, uint32_t flags, uint64_t in_bytes, rbgpu_set **out) {
  hipStream_t st = ctx->stream;
  const uint64_t tiles = d.tiles, G = d.G;
  const uint64_t *tile_pre = d.tile_pre;
  const uint64_t T = G * nsl;
  uint64_t *cstart, *tkeep, *tbytes, *tpos, *toff, *scan_tmp2;
  uint16_t *ckey;
  uint8_t *ttype;
  if (!tmp.get(cstart, G + 1) || !tmp.get(ckey, G) || !tmp.get(ttype, T) || !tmp.get(tkeep, T) ||
      !tmp.get(tbytes, T) || !tmp.get(tpos, T + 1) || !tmp.get(toff, T + 1) ||
      !tmp.get(scan_tmp2, scan_tmp_words(T) + 1))
    return fail(RB_ENOMEM, "value build: workspace of %llu containers", (unsigned long long)T);
  k_build_write_heads<<<(unsigned)tiles, 256, 0, st>>>(src, tile_pre, cstart, ckey);
  BuildArgs a{};
  a.src = src;
  a.cstart = cstart;
  a.ckey = ckey;
  a.G = G;
  a.nsl = nsl;
  a.runopt = (flags & RB_BUILD_RUN_OPTIMIZE) != 0;
  a.ttype = ttype;
  a.tkeep = tkeep;
  a.tbytes = tbytes;
  a.tpos = tpos;
  a.toff = toff;
  a.in_bytes = in_bytes;
  a.stats = ctx->d_stats;
  const unsigned grid = grid_for(T, 4);
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  k_set_build<<<grid, 256, 0, st>>>(a);
  HIPCHK(hipEventRecord(ctx->ev[2], st));
  scan_exclusive(tkeep, tpos, T, scan_tmp2, st);
  scan_exclusive(tbytes, toff, T, scan_tmp2, st);
  uint64_t tot[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(&tot[0], tpos + T, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&tot[1], toff + T, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  LAUNCHCHK();
  const uint64_t nc = tot[0], total = tot[1];
  SetPtr s;
  int rc = make_set(ctx, nb, nc, total, s);
  if (rc) return rc;
  auto drop = [&](int r) { // the set goes back to the pool behind its kernels
    (void)hipStreamSynchronize(st);
    return r;
  };
  if (d_offs) k_build_begin<<<nblk(nb + 1ull, 256), 256, 0, st>>>(cstart, G, d_offs, nb, s->begin);
  else k_bsi_begin<<<1, 128, 0, st>>>(tpos, G, nsl, s->begin);
  a.emit = 1;
  a.out = OutView{s->key, s->type, s->card, s->nruns, s->off};
  a.payload = s->payload;
  if (hipEventRecord(ctx->ev[3], st) != hipSuccess) return drop(fail(RB_EDEVICE, "value build: event"));
  k_set_build<<<grid, 256, 0, st>>>(a);
  if (hipEventRecord(ctx->ev[4], st) != hipSuccess) return drop(fail(RB_EDEVICE, "value build: event"));
  const KernelSpan spans[2] = {{"k_set_build", 0, -1, T}, {"k_set_build", 0, 1, nc, ctx->ev[3], ctx->ev[4]}};
  rc = stats_end(ctx, nc, nc, spans, 2);
  if (rc) return drop(rc);
  *out = s.release();
  return RB_OK;
}
} // namespace

// d_values: device memory, bitmap i at [offsets[i], offsets[i + 1]) (host offsets, checked by the caller)
int build_set_values(rbgpu_ctx *ctx, const uint32_t *d_values, const uint64_t *offsets, uint32_t nb, uint32_t flags,
                     rbgpu_set **out) {
  const uint64_t base = nb ? offsets[0] : 0, n = nb ? offsets[nb] - base : 0;
  if (!n) return empty_set(ctx, nb, out);
  hipStream_t st = ctx->stream;
  Scratch tmp(ctx->pool); // back to the pool when the call leaves (every path has waited for the stream, or failed)
  std::vector<uint64_t> rel((size_t)nb + 1);
  for (uint32_t i = 0; i <= nb; ++i) rel[i] = offsets[i] - base;
  uint64_t *d_offs;
  uint32_t *flag, *starts;
  const uint64_t start_words = n / 32 + 1;
  if (!tmp.get(d_offs, nb + 1ull) || !tmp.get(starts, start_words) || !tmp.get(flag, 1))
    return fail(RB_ENOMEM, "value build: %llu values", (unsigned long long)n);
  stats_begin(ctx);
  HIPCHK(hipMemcpyAsync(d_offs, rel.data(), (nb + 1ull) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(flag, 0, 4, st));
  HIPCHK(hipMemsetAsync(starts, 0, start_words * 4, st));
  k_build_mark_starts<<<nblk(nb, 256), 256, 0, st>>>(d_offs, nb, starts);
  // the values where they lie: right when no high key descends inside a bitmap, which the same pass finds out
  BuildSrc src{nullptr, d_values + base, starts, nullptr, n};
  Discovery d;
  uint32_t unsorted = 0;
  int rc = discover(ctx, tmp, src, flag, &unsorted, d); // its wait also covers the copy from `rel`
  if (rc) return rc;
  if (unsorted) {
    unsigned end_bit = 32; // the value's high half, then as many bits as the bitmap indices take
    while (end_bit < 64 && ((uint64_t)(nb - 1) >> (end_bit - 32))) ++end_bit;
    size_t bytes = 0;
    uint64_t *keys, *sorted;
    uint8_t *stmp;
    HIPCHK(build_sort_keys(nullptr, &bytes, nullptr, nullptr, n, 16, end_bit, st));
    if (!tmp.get(keys, n) || !tmp.get(sorted, n) || !tmp.get(stmp, bytes))
      return fail(RB_ENOMEM, "value build: sort of %llu values", (unsigned long long)n);
    k_build_keys<<<grid_for(n, 256), 256, 0, st>>>(d_values + base, d_offs, nb, n, keys);
    HIPCHK(build_sort_keys(stmp, &bytes, keys, sorted, n, 16, end_bit, st));
    src = BuildSrc{sorted, nullptr, nullptr, nullptr, n};
    rc = discover(ctx, tmp, src, nullptr, nullptr, d);
    if (rc) return rc;
  }
  return build_grouped(ctx, tmp, src, d, d_offs, nb, 1, flags, 4 * n, out);
}

int build_bsi_pairs(rbgpu_ctx *ctx, const uint32_t *d_cols, const uint64_t *d_vals, uint64_t n, uint32_t flags,
                    rbgpu_set **out, uint64_t *min_value, uint64_t *max_value) {
  if (min_value) *min_value = 0;
  if (max_value) *max_value = 0;
  if (!n) return empty_set(ctx, 1, out);
  hipStream_t st = ctx->stream;
  Scratch tmp(ctx->pool); // back to the pool when the call leaves (every path has waited for the stream, or failed)
  uint32_t *flag;
  uint64_t *mm;
  if (!tmp.get(flag, 1) || !tmp.get(mm, 2)) return fail(RB_ENOMEM, "BSI build");
  stats_begin(ctx);
  const uint64_t mm0[2] = {~0ull, 0ull};
  HIPCHK(hipMemsetAsync(flag, 0, 4, st));
  HIPCHK(hipMemcpyAsync(mm, mm0, 16, hipMemcpyHostToDevice, st));
  k_bsi_order<<<grid_for(n, 256), 256, 0, st>>>(d_cols, n, flag);
  uint32_t unsorted = 0;
  HIPCHK(hipMemcpyAsync(&unsorted, flag, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  LAUNCHCHK();
  const uint32_t *cols = d_cols;
  const uint64_t *vals = d_vals;
  uint64_t *kept = nullptr;
  if (unsorted) {
    size_t bytes = 0;
    uint32_t *scol;
    uint64_t *sval;
    uint8_t *stmp;
    HIPCHK(build_sort_pairs(nullptr, &bytes, d_cols, nullptr, d_vals, nullptr, n, st));
    if (!tmp.get(scol, n) || !tmp.get(sval, n) || !tmp.get(stmp, bytes))
      return fail(RB_ENOMEM, "BSI build: sort of %llu pairs", (unsigned long long)n);
    HIPCHK(build_sort_pairs(stmp, &bytes, d_cols, scol, d_vals, sval, n, st));
    cols = scol;
    vals = kept = sval; // cleared in place
  }
  k_bsi_reduce<<<grid_for(n, 256), 256, 0, st>>>(cols, vals, n, kept, mm);
  uint64_t h_mm[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(h_mm, mm, 16, hipMemcpyDeviceToHost, st));
  const BuildSrc src{nullptr, cols, nullptr, vals, n};
  Discovery d;
  int rc = discover(ctx, tmp, src, nullptr, nullptr, d); // its wait brings min / max too: the set is sized after it
  if (rc) return rc;
  uint32_t nbits = 1;
  while (nbits < 64 && (h_mm[1] >> nbits)) ++nbits;
  rc = build_grouped(ctx, tmp, src, d, nullptr, nbits + 1, nbits + 1, flags, 12 * n, out);
  if (rc) return rc;
  if (min_value) *min_value = h_mm[0];
  if (max_value) *max_value = h_mm[1];
  return RB_OK;
}

// this file's code object, loaded at context creation (rbgpu_open, context.hip)
__global__ void k_warm_build() {}
void warm_build(hipStream_t st) { k_warm_build<<<1, 64, 0, st>>>(); }

} // namespace rbg
