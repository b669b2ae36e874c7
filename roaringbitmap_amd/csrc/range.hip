// range.hip — range mutations on the device: RoaringBitmap.add / remove / flip over [start, end) for a batch of
// bitmaps, static (RoaringBitmap.java:298-344, 995-1037, 626-664) and in place (:1181-1208, 2656-2711, 1893-1925),
// and with them bitmapOfRange (:588-615: ADD on an empty bitmap).  One range per output bitmap.
//
// The container rules (each result is the reference's type, hence its bytes):
//   key absent      add / flip: Container.rangeOfOnes (Container.java:29-37): a span of 1 or 2 is an Array, else one Run;
//                   remove: nothing
//   Array           add: Array up to 4096 values, else a Bitmap that stays a Bitmap even when full (ArrayContainer.java:
//                   103-135, 464-); remove: Array (:1039-, 759-); not: Array up to 4096, else Bitmap (:876-929, 652-)
//   Bitmap          add: Bitmap, full included (BitmapContainer.java:131-144, 517-); remove and not: Array up to 4096
//                   values, else Bitmap (:1175-1190, 797-811, 688-696, 1003-1006)
//   Run             add / remove: a Run whatever its size, runs maximal (RunContainer.java:242-245, 1068-, 2032-2035,
//                   1553-); not: toEfficientContainer (:1900-1918, 1267-1364, 2326-2335)
//   a result without members is dropped (remove, flip).
// The two forms agree except in one place: the static add replaces every key strictly inside the span by
// rangeOfOnes(0, 65536), a full Run, whatever was there (RoaringBitmap.java:332-335), while x.add(range) calls iadd on
// the containers it finds (:1199-1202), so a middle Array or Bitmap becomes a full Bitmap and only absent keys get the
// Run.  `inplace` selects that.
//
// The pipeline, on one stream:
//   k_range_plan      a thread per output bitmap: the range split into hbStart / hbLast, two binary searches over the
//                     member's keys, and the number of CANDIDATE result containers: the copies before and after the
//                     span, and inside it one per key (add, flip) or one per container present (remove).
//   scan              candidates per bitmap -> the candidate space [0, T).
//   k_range_cands     a thread per candidate: its bitmap (a search over the scan), its kind and source container, the
//                     range inside its key — 12 B per candidate, read by the passes below.  Copies, fresh ranges of
//                     ones and whole-container removals are measured here, from metadata alone; a candidate that
//                     touches an existing container joins a list.
//   k_range_touch     measure: a wave per touched container: load_container into the register image, the range set /
//                     cleared / xor-ed on the lane's words, metrics, the type rule above -> (type or dropped, bytes).
//   scans             kept candidates -> container indices and begin[]; payload bytes -> offsets in a tight arena.
//   k_range_plain     emit: a wave per 64 candidates writes the metadata of the copies and of the fresh ranges of ones
//                     (with their one run or two values) and moves the copies' payloads.
//   k_range_touch     emit: the same work as its measuring pass again, then metadata and payload (emit_container).
//                     The image is not held across the scan (the list is unbounded, registers are not): a touched
//                     container is read twice.
#include <algorithm>
#include <vector>

#include "internal.hpp"
#include "kernels.hpp"
#include "wave.hpp"

namespace rbg {

namespace {
constexpr uint64_t kMaxBlocks = 4096;
enum { kCopy = 0, kTouch = 1, kFresh = 2, kGone = 3, kNone = 4 };

struct RangeArgs {
  int op, inplace;
  SetView in;
  const uint32_t *members; // null: identity
  const uint64_t *start, *end;
  uint32_t n;
  const uint64_t *lo, *hi;  // [n] first container with key >= hbStart / > hbLast (both the member's end: empty range)
  const uint64_t *cbase;    // [n + 1] first candidate of each output bitmap
  uint64_t T;
};

struct Cand {
  int kind;
  uint64_t src;    // source container (kCopy, kTouch)
  uint32_t key;
  uint32_t cb, ce; // the range inside the container, [cb, ce) within [0, 65536]
};

__device__ __forceinline__ uint64_t lower_key(const uint16_t *key, uint64_t l, uint64_t h, uint32_t k) {
  while (l < h) {
    const uint64_t mid = (l + h) >> 1;
    if (key[mid] < k) l = mid + 1;
    else h = mid;
  }
  return l;
}

__device__ __forceinline__ Cand decode(const RangeArgs &a, uint64_t t) {
  Cand c{kNone, 0, 0, 0, 0};
  if (t >= a.T) return c;
  uint32_t i = 0, len = a.n; // the last bitmap with cbase[i] <= t (bitmaps without candidates share a value)
  while (len > 1) {
    const uint32_t h = len >> 1;
    if (a.cbase[i + h] <= t) {
      i += h;
      len -= h;
    } else {
      len = h;
    }
  }
  const uint64_t j = t - a.cbase[i];
  const uint32_t m = a.members ? a.members[i] : i;
  const uint64_t b0 = a.in.begin[m], lo = a.lo[i], hi = a.hi[i];
  const uint64_t before = lo - b0;
  if (j < before) {
    c.kind = kCopy;
    c.src = b0 + j;
    return c;
  }
  const uint64_t s = a.start[i], e = a.end[i];
  uint64_t span = 0;
  uint32_t hbS = 0, hbL = 0;
  if (s < e) {
    hbS = (uint32_t)(s >> 16);
    hbL = (uint32_t)((e - 1) >> 16);
    span = a.op == RB_RANGE_REMOVE ? hi - lo : (uint64_t)(hbL - hbS) + 1;
  }
  if (j >= before + span) {
    c.kind = kCopy;
    c.src = hi + (j - before - span);
    return c;
  }
  const uint64_t q = j - before;
  bool present = true;
  if (a.op == RB_RANGE_REMOVE) {
    c.src = lo + q;
    c.key = a.in.key[c.src];
  } else {
    c.key = hbS + (uint32_t)q;
    c.src = lower_key(a.in.key, lo, hi, c.key);
    present = c.src < hi && a.in.key[c.src] == c.key;
  }
  c.cb = c.key == hbS ? (uint32_t)(s & 0xFFFF) : 0u;
  c.ce = c.key == hbL ? (uint32_t)((e - 1) & 0xFFFF) + 1u : (uint32_t)kSpan;
  const bool whole = c.cb == 0 && c.ce == (uint32_t)kSpan;
  if (!present) c.kind = kFresh;
  else if (a.op == RB_RANGE_ADD && !a.inplace && c.key != hbS && c.key != hbL) c.kind = kFresh; // :332-335
  else if (a.op == RB_RANGE_REMOVE && whole) c.kind = kGone;
  else c.kind = kTouch;
  return c;
}

// A candidate as the plan leaves it for the two passes over the candidate space: source container (40 bits), key (16),
// kind (3) in one word, and the range inside the container as cb | (ce - 1) << 16 (ce >= 1 wherever it is read).
__device__ __forceinline__ uint64_t pack_cand(const Cand &c) {
  return c.src | ((uint64_t)c.key << 40) | ((uint64_t)c.kind << 56);
}
__device__ __forceinline__ Cand unpack_cand(uint64_t r, uint32_t g) {
  Cand c;
  c.src = r & ((1ull << 40) - 1);
  c.key = (uint32_t)(r >> 40) & 0xFFFFu;
  c.kind = (int)(r >> 56);
  c.cb = g & 0xFFFFu;
  c.ce = (g >> 16) + 1u;
  return c;
}

struct ApplyArgs {
  int op;
  SetView in;
  uint64_t T;
  uint64_t *crec;   // [T] pack_cand
  uint32_t *crng;   // [T]
  uint64_t *tlist;  // [ntouch[0]] the touched candidates, in any order
  uint64_t *ntouch; // [2]: their number, and how many of them end as a Run of 2045 runs or more (big_run)
  // per candidate, written by the measuring pass: the type (kEmpty: dropped), 1 / 0, the payload bytes rounded to 16
  uint8_t *ttype;
  uint64_t *tkeep, *tbytes;
  // their exclusive scans, read by the emitting pass
  const uint64_t *tpos, *toff;
  OutView out;
  uint8_t *payload;
  uint64_t *stats;
};

// the op over bits [cb, ce) of the register image: word j = 2k + h of lane L is container word 128 k + 2 L + h
__device__ __forceinline__ void apply_range(int op, uint64_t (&w)[kW], uint32_t cb, uint32_t ce, int lane) {
#pragma unroll
  for (int j = 0; j < kW; ++j) {
    const int base = (128 * (j >> 1) + 2 * lane + (j & 1)) << 6;
    const int lo = max((int)cb - base, 0), hi = min((int)ce - base, 64); // a word is touched iff lo < hi; then
    uint64_t m = 0;                                                      // 0 <= lo <= 63 and 1 <= hi <= 64
    if (lo < hi) m = (~0ull << (lo & 63)) & (~0ull >> ((64 - hi) & 63)); // hi == 64 (and e == 65536): no shift
    w[j] = op == RB_RANGE_ADD ? w[j] | m : op == RB_RANGE_REMOVE ? w[j] & ~m : w[j] ^ m;
  }
}

// the result type of (source type, op) for a result of c values in r maximal runs
__device__ __forceinline__ int range_type(int src, int op, int c, int r) {
  if (c == 0) return kEmpty;
  if (src == kRun) return op == RB_RANGE_FLIP ? type_eff(c, r) : (int)kRun;
  if (op == RB_RANGE_ADD) return src == kBitmap ? (int)kBitmap : type_ab(c);
  if (op == RB_RANGE_REMOVE) return src == kArray ? (int)kArray : type_ab(c);
  return type_ab(c);
}

// emit_container's Run form for any run count: add and remove keep a Run whatever its size (up to 32768 runs, 128 KiB)
// and emit_container's LDS stage holds 2048 starts and ends.  A rare shape (a canonical input Run of that size is
// larger than the Bitmap of the same set), so this one is plain: starts and ends go straight to the slot by rank,
// 2 B at a time, and a second sweep turns each end into the run's length - 1.
__device__ __forceinline__ uint32_t emit_runs_any(const uint64_t (&w)[kW], int runs, uint8_t *out, int lane) {
  const Neigh nb = neighbours(w, lane);
  uint32_t ns[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) ns[k] = __popcll(run_starts(w, nb, 2 * k)) + __popcll(run_starts(w, nb, 2 * k + 1));
  // a row holds 8192 bits, at most 4096 run starts: the packed 16-bit fields cannot carry
  const uint64_t P0 = (uint64_t)ns[0] | ((uint64_t)ns[1] << 16) | ((uint64_t)ns[2] << 32) | ((uint64_t)ns[3] << 48);
  const uint64_t P1 = (uint64_t)ns[4] | ((uint64_t)ns[5] << 16) | ((uint64_t)ns[6] << 32) | ((uint64_t)ns[7] << 48);
  const uint64_t S0 = wave_scan_u64(P0, lane), S1 = wave_scan_u64(P1, lane);
  const uint64_t E0 = S0 - P0, E1 = S1 - P1;
  const uint64_t T0 = pack2(readlane((uint32_t)S0, 63), readlane((uint32_t)(S0 >> 32), 63));
  const uint64_t T1 = pack2(readlane((uint32_t)S1, 63), readlane((uint32_t)(S1 >> 32), 63));
  // (start, end) of run i at out16[2 i], out16[2 i + 1] first: the i-th end closes the i-th run
  uint16_t *o16 = reinterpret_cast<uint16_t *>(out);
  uint32_t rowoff = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint64_t Ex = k < 4 ? E0 : E1, T = k < 4 ? T0 : T1;
    const int sh = 16 * (k & 3);
    uint32_t sp = rowoff + (uint32_t)((Ex >> sh) & 0xFFFF);
    rowoff += (uint32_t)((T >> sh) & 0xFFFF);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = 2 * k + h;
      const uint32_t open = (uint32_t)(h ? (w[j - 1] >> 63) : ((nb.prev_top_h0 >> k) & 1)) & (uint32_t)(w[j] & 1);
      uint32_t ep = sp - open;
      const uint32_t base = (uint32_t)(128 * k + 2 * lane + h) << 6;
      uint64_t x = run_starts(w, nb, j), y = run_ends(w, nb, j);
      while (x | y) {
        if (x) {
          o16[2 * sp++] = (uint16_t)(base + __builtin_ctzll(x));
          x &= x - 1;
        }
        if (y) {
          o16[2 * ep++ + 1] = (uint16_t)(base + __builtin_ctzll(y));
          y &= y - 1;
        }
      }
    }
  }
  // the halves of one word come from different lanes: every store lands before any lane reads the words back
  __threadfence();
  __builtin_amdgcn_wave_barrier();
  uint32_t *o32 = reinterpret_cast<uint32_t *>(out);
  const int padded = (runs + 3) & ~3; // the slot is 16-B padded; the pad is zeroed
  for (int i = lane; i < padded; i += 64) {
    const uint32_t v = i < runs ? __hip_atomic_load(o32 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    o32[i] = i < runs ? (v & 0xFFFFu) | (((v >> 16) - (v & 0xFFFFu)) << 16) : 0u;
  }
  return 4u * (uint32_t)runs;
}

__device__ __forceinline__ uint64_t bcast64(uint64_t x, int l) {
  return pack2(readlane((uint32_t)x, l), readlane((uint32_t)(x >> 32), l));
}
} // namespace

// lo / hi / candidate count of every output bitmap
__global__ __launch_bounds__(256) void k_range_plan(RangeArgs a, uint64_t *__restrict__ lo, uint64_t *__restrict__ hi,
                                                    uint64_t *__restrict__ ncand) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t m = a.members ? a.members[i] : i;
  const uint64_t b0 = a.in.begin[m], b1 = a.in.begin[m + 1];
  const uint64_t s = a.start[i], e = a.end[i];
  if (s >= e) { // the bitmap as it is
    lo[i] = hi[i] = b1;
    ncand[i] = b1 - b0;
    return;
  }
  const uint32_t hbS = (uint32_t)(s >> 16), hbL = (uint32_t)((e - 1) >> 16);
  const uint64_t l = lower_key(a.in.key, b0, b1, hbS), h = lower_key(a.in.key, l, b1, hbL + 1);
  lo[i] = l;
  hi[i] = h;
  ncand[i] = (l - b0) + (a.op == RB_RANGE_REMOVE ? h - l : (uint64_t)(hbL - hbS) + 1) + (b1 - h);
}

__global__ __launch_bounds__(256) void k_range_begin(const uint64_t *__restrict__ cbase, const uint64_t *__restrict__ tpos,
                                                     uint32_t n, uint64_t *__restrict__ begin) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i <= n) begin[i] = tpos[cbase[i]];
}

// Every candidate decoded once.  What metadata alone settles is measured here: a copy keeps its type and size, a fresh
// range of ones takes one 16-B slot, a container removed whole is dropped.  A touched candidate joins the list the
// register-image kernel walks (in any order: every result is written at its candidate's own place).
__global__ __launch_bounds__(256) void k_range_cands(RangeArgs a, ApplyArgs o) {
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < a.T; t += (uint64_t)gridDim.x * 256) {
    const Cand c = decode(a, t);
    o.crec[t] = pack_cand(c);
    o.crng[t] = c.kind == kCopy ? 0u : c.cb | ((c.ce - 1u) << 16);
    if (c.kind == kTouch) {
      o.tlist[atomicAdd((unsigned long long *)o.ntouch, 1ull)] = t;
      continue;
    }
    int ty = kEmpty;
    uint64_t bytes = 0;
    if (c.kind == kCopy) {
      ty = a.in.type[c.src];
      bytes = round16(payload_bytes(ty, a.in.card[c.src], a.in.nruns[c.src]));
    } else if (c.kind == kFresh) { // Container.rangeOfOnes
      ty = c.ce - c.cb <= 2 ? kArray : kRun;
      bytes = 16;
    }
    o.ttype[t] = (uint8_t)ty;
    o.tkeep[t] = c.kind != kGone;
    o.tbytes[t] = bytes;
  }
}

// The touched containers, a wave each: load_container into the register image, the range set / cleared / xor-ed on
// the lane's words, metrics, the type rule.  kTouchMeasure measures (type or dropped, payload bytes); the emitting
// modes do the same work again and write metadata and payload where the scans put them: kTouchEmit every result but
// the Runs of 2045 runs and more, kTouchEmitBig those (big_run: a padded payload, round16(4 r), of 8 KiB and up — a
// Run that add or remove left with a list at or past emit_container's LDS stage of 2048 starts and ends; launched
// only when the measuring pass counted one — with both emitters in one kernel it spilled scalars).
enum { kTouchMeasure = 0, kTouchEmit = 1, kTouchEmitBig = 2 };
__device__ __forceinline__ bool big_run(int ty, uint64_t bytes) { return ty == kRun && bytes >= (uint64_t)kBitmapBytes; }
template <int MODE> __global__ __launch_bounds__(256, 2) void k_range_touch(ApplyArgs a) {
  constexpr bool EMIT = MODE != kTouchMeasure;
  __shared__ __attribute__((aligned(16))) uint32_t lds[4][2048];
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t *s = lds[wv];
  const uint64_t nt = a.ntouch[0];
  uint64_t inb = 0, outb = 0, members = 0; // this wave's share of the call's counters
  for (uint64_t i = (uint64_t)blockIdx.x * 4 + wv; i < nt; i += (uint64_t)gridDim.x * 4) {
    const uint64_t t = a.tlist[i];
    if (EMIT && (a.ttype[t] == kEmpty || big_run(a.ttype[t], a.tbytes[t]) != (MODE == kTouchEmitBig))) continue;
    const Cand c = unpack_cand(a.crec[t], a.crng[t]);
    const int st = a.in.type[c.src];
    const uint32_t scard = a.in.card[c.src], snr = a.in.nruns[c.src];
    uint64_t w[kW];
    load_container(st, a.in.payload + a.in.off[c.src], scard, snr, s, w, lane);
    apply_range(a.op, w, c.cb, c.ce, lane);
    int cd, r;
    metrics(w, lane, true, cd, r);
    const int ty = range_type(st, a.op, cd, r);
    inb += payload_bytes(st, scard, snr) + 16;
    if (!EMIT) {
      if (lane == 0) {
        a.ttype[t] = (uint8_t)ty;
        a.tkeep[t] = cd != 0;
        const uint64_t bytes = cd ? round16(payload_bytes(ty, (uint32_t)cd, (uint32_t)r)) : 0ull;
        a.tbytes[t] = bytes;
        if (big_run(ty, bytes)) atomicAdd((unsigned long long *)&a.ntouch[1], 1ull);
      }
      continue;
    }
    // the measuring pass kept this candidate, and the same image gives the same type and size
    const uint64_t at = a.tpos[t], off = a.toff[t];
    if (lane == 0) {
      a.out.key[at] = (uint16_t)c.key;
      a.out.type[at] = (uint8_t)ty;
      a.out.card[at] = (uint32_t)cd;
      a.out.nruns[at] = (uint16_t)(ty == kRun ? r : 0);
      a.out.off[at] = off;
    }
    if (MODE == kTouchEmitBig) outb += emit_runs_any(w, r, a.payload + off, lane) + 16;
    else outb += emit_container(ty, w, cd, r, a.payload + off, s, lane) + 16;
    members += (uint64_t)cd;
    wave_lds_sync();
  }
  if (lane == 0 && inb) {
    const uint32_t stripe = (blockIdx.x * 4 + wv) & (kStripes - 1);
    if (!EMIT) { // word 2: what the measuring pass read
      atomicAdd((unsigned long long *)&a.stats[2 * kStripes + stripe], (unsigned long long)inb);
    } else {
      atomicAdd((unsigned long long *)&a.stats[0 * kStripes + stripe], (unsigned long long)inb);
      atomicAdd((unsigned long long *)&a.stats[1 * kStripes + stripe], (unsigned long long)outb);
      atomicAdd((unsigned long long *)&a.stats[7 * kStripes + stripe], (unsigned long long)members);
    }
  }
}

// The emitting pass of everything else, a wave per 64 candidates: every lane writes its own candidate's metadata (and
// the one or two values, or the one run, of a fresh range of ones); the copies' payloads then go through the whole
// wave one at a time.
__global__ __launch_bounds__(256) void k_range_plain(ApplyArgs a) {
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t chunks = (a.T + 63) >> 6;
  uint64_t inb = 0, outb = 0, members = 0;
  for (uint64_t ch = (uint64_t)blockIdx.x * 4 + wv; ch < chunks; ch += (uint64_t)gridDim.x * 4) {
    const uint64_t t = (ch << 6) + lane;
    Cand c{kNone, 0, 0, 0, 0};
    if (t < a.T) c = unpack_cand(a.crec[t], a.crng[t]);
    uint64_t off = 0, cp_src = 0, cp_bytes = 0;
    if (c.kind == kCopy) {
      const uint64_t at = a.tpos[t];
      off = a.toff[t];
      const int ty = a.in.type[c.src];
      const uint32_t card = a.in.card[c.src], nr = a.in.nruns[c.src];
      const uint64_t bytes = payload_bytes(ty, card, nr);
      a.out.key[at] = a.in.key[c.src];
      a.out.type[at] = (uint8_t)ty;
      a.out.card[at] = card;
      a.out.nruns[at] = (uint16_t)nr;
      a.out.off[at] = off;
      cp_src = a.in.off[c.src];
      cp_bytes = bytes; // the exact size: the buffer bound zeroes the slot's pad
      inb += bytes + 16;
      outb += bytes + 16;
      members += card;
    } else if (c.kind == kFresh) {
      const uint64_t at = a.tpos[t];
      off = a.toff[t];
      const uint32_t span = c.ce - c.cb;
      const int ty = span <= 2 ? kArray : kRun;
      a.out.key[at] = (uint16_t)c.key;
      a.out.type[at] = (uint8_t)ty;
      a.out.card[at] = span;
      a.out.nruns[at] = (uint16_t)(ty == kRun ? 1 : 0);
      a.out.off[at] = off;
      const uint32_t w0 = ty == kRun ? c.cb | ((span - 1) << 16) : span == 2 ? c.cb | ((c.cb + 1) << 16) : c.cb;
      *reinterpret_cast<uint4 *>(a.payload + off) = make_uint4(w0, 0, 0, 0);
      outb += (ty == kRun ? 4 : 2 * span) + 16;
      members += span;
    }
    uint64_t cm = __ballot(cp_bytes != 0);
    while (cm) {
      const int l = __builtin_ctzll(cm);
      cm &= cm - 1;
      copy_payload(a.in.payload + bcast64(cp_src, l), a.payload + bcast64(off, l), bcast64(cp_bytes, l), lane);
    }
  }
  inb = wave_sum_u64(inb);
  outb = wave_sum_u64(outb);
  members = wave_sum_u64(members);
  if (lane == 0 && outb) {
    const uint32_t stripe = (blockIdx.x * 4 + wv) & (kStripes - 1);
    atomicAdd((unsigned long long *)&a.stats[0 * kStripes + stripe], (unsigned long long)inb);
    atomicAdd((unsigned long long *)&a.stats[1 * kStripes + stripe], (unsigned long long)outb);
    atomicAdd((unsigned long long *)&a.stats[7 * kStripes + stripe], (unsigned long long)members);
  }
}

// ---------------------------------------------------------------- host side
namespace {
int empty_result(rbgpu_ctx *ctx, uint32_t nb, rbgpu_set **out) {
  SetPtr s;
  int rc = make_set(ctx, nb, 0, 0, s);
  if (rc) return rc;
  if (hipMemsetAsync(s->begin, 0, (nb + 1ull) * 8, ctx->stream) != hipSuccess)
    return fail(RB_EDEVICE, "range op: memset failed");
  s->h_begin.assign((size_t)nb + 1, 0);
  if ((rc = stats_end(ctx, 0, 0, nullptr, 0))) return rc;
  *out = s.release();
  return RB_OK;
}
} // namespace

// the arguments are checked (entry.hip): ranges sane, members inside the set
int range_op(rbgpu_ctx *ctx, int op, bool inplace, const rbgpu_set *in, const uint32_t *members, const uint64_t *start,
             const uint64_t *end, uint32_t n, rbgpu_set **out) {
  hipStream_t st = ctx->stream;
  Scratch tmp(ctx->pool); // back to the pool when the call leaves (every path has waited for the stream, or failed)
  stats_begin(ctx);
  if (!n) return empty_result(ctx, 0, out);
  uint32_t *d_members = nullptr;
  uint64_t *d_start, *d_end, *lo, *hi, *ncand, *cbase, *scan_tmp;
  if ((members && !tmp.get(d_members, n)) || !tmp.get(d_start, n) || !tmp.get(d_end, n) || !tmp.get(lo, n) ||
      !tmp.get(hi, n) || !tmp.get(ncand, n) || !tmp.get(cbase, n + 1ull) || !tmp.get(scan_tmp, scan_tmp_words(n) + 1))
    return fail(RB_ENOMEM, "range op: plan of %u bitmaps", n);
  if (members) HIPCHK(hipMemcpyAsync(d_members, members, 4ull * n, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_start, start, 8ull * n, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_end, end, 8ull * n, hipMemcpyHostToDevice, st));
  RangeArgs p{};
  p.op = op;
  p.inplace = inplace;
  p.in = in->view();
  p.members = d_members;
  p.start = d_start;
  p.end = d_end;
  p.n = n;
  k_range_plan<<<(n + 255) / 256, 256, 0, st>>>(p, lo, hi, ncand);
  scan_exclusive(ncand, cbase, n, scan_tmp, st);
  uint64_t T = 0;
  HIPCHK(hipMemcpyAsync(&T, cbase + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  LAUNCHCHK();
  if (!T) return empty_result(ctx, n, out);
  if (in->nc >= (1ull << 40)) return fail(RB_EINVAL, "range op: %llu source containers", (unsigned long long)in->nc);
  ApplyArgs a{};
  uint64_t *tpos, *toff, *scan_tmp2;
  if (!tmp.get(a.crec, T) || !tmp.get(a.crng, T) || !tmp.get(a.tlist, T) || !tmp.get(a.ntouch, 2) ||
      !tmp.get(a.ttype, T) || !tmp.get(a.tkeep, T) || !tmp.get(a.tbytes, T) || !tmp.get(tpos, T + 1) ||
      !tmp.get(toff, T + 1) || !tmp.get(scan_tmp2, scan_tmp_words(T) + 1))
    return fail(RB_ENOMEM, "range op: workspace of %llu candidate containers", (unsigned long long)T);
  p.lo = lo;
  p.hi = hi;
  p.cbase = cbase;
  p.T = T;
  a.op = op;
  a.in = in->view();
  a.T = T;
  a.tpos = tpos;
  a.toff = toff;
  a.stats = ctx->d_stats;
  const unsigned grid_t = (unsigned)std::min<uint64_t>((T + 255) / 256, kMaxBlocks);   // a thread per candidate
  const unsigned grid_c = (unsigned)std::min<uint64_t>((T + 255) / 256, kMaxBlocks);   // a wave per 64 candidates
  auto grid_for_touched = [](uint64_t k) { return (unsigned)std::min<uint64_t>((k + 3) / 4, kMaxBlocks); }; // a wave each
  HIPCHK(hipMemsetAsync(a.ntouch, 0, 16, st));
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  k_range_cands<<<grid_t, 256, 0, st>>>(p, a);
  k_range_touch<kTouchMeasure><<<grid_for_touched(T), 256, 0, st>>>(a); // the list's length is on the device
  HIPCHK(hipEventRecord(ctx->ev[2], st));
  scan_exclusive(a.tkeep, tpos, T, scan_tmp2, st);
  scan_exclusive(a.tbytes, toff, T, scan_tmp2, st);
  uint64_t tot[2] = {0, 0}, nt[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(nt, a.ntouch, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&tot[0], tpos + T, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&tot[1], toff + T, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  LAUNCHCHK();
  const uint64_t nc = tot[0], total = tot[1];
  // the result is exact-sized: when it cannot be allocated the call ends here, before anything is written
  SetPtr s;
  int rc = make_set(ctx, n, nc, total, s);
  if (rc) return rc;
  auto drop = [&](int r) { // the set goes back to the pool behind its kernels
    (void)hipStreamSynchronize(st);
    return r;
  };
  k_range_begin<<<(n + 256) / 256, 256, 0, st>>>(cbase, tpos, n, s->begin);
  a.out = OutView{s->key, s->type, s->card, s->nruns, s->off};
  a.payload = s->payload;
  if (hipEventRecord(ctx->ev[3], st) != hipSuccess) return drop(fail(RB_EDEVICE, "range op: event"));
  k_range_plain<<<grid_c, 256, 0, st>>>(a);
  if (nt[0]) k_range_touch<kTouchEmit><<<grid_for_touched(nt[0]), 256, 0, st>>>(a);
  if (nt[1]) k_range_touch<kTouchEmitBig><<<grid_for_touched(nt[0]), 256, 0, st>>>(a);
  if (hipEventRecord(ctx->ev[4], st) != hipSuccess) return drop(fail(RB_EDEVICE, "range op: event"));
  const KernelSpan spans[2] = {{"k_range_measure", 2, -1, T}, {"k_range_emit", 0, 1, nc, ctx->ev[3], ctx->ev[4]}};
  rc = stats_end(ctx, nc, nc, spans, 2);
  if (rc) return drop(rc);
  *out = s.release();
  return RB_OK;
}

// this file's code object, loaded at context creation (rbgpu_open, context.hip)
__global__ void k_warm_range() {}
void warm_range(hipStream_t st) { k_warm_range<<<1, 64, 0, st>>>(); }

} // namespace rbg

