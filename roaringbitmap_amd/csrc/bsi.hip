// bsi.hip — bit-sliced index compare (bsi module: Roaring64BitmapSliceIndex.compare /
// RoaringBitmapSliceIndex.compare, the O'Neil chains of oNeilCompare) as ONE fused pass per high key.
//
// The reference evaluates a query as ~2 static RoaringBitmap ops per slice over whole bitmaps
// (RoaringBitmapSliceIndex.java:432-472), materialising EQ / GT / LT after every slice.  Every high
// key is independent, so here ONE WAVE PER KEY walks the slices once: EQ lives in registers as a
// 65536-bit register bitmap, the GT or LT accumulator in an 8 KiB LDS image, the current slice is
// staged in a second LDS image while the next slice's payload is already in flight (registers).
// Each intermediate carries the container type the reference's static op would have produced
// (pairwise contract, SURVEY §8a: AND R&R->EFF else AB, ANDNOT R\R, R\A(|A|<32)->EFF else AB, OR any
// Bitmap->LR, A|A->AB, else EFF; absent keys: and -> absent, andNot(x, absent) -> clone x,
// or(x, absent) -> clone x; empty results dropped), so the result is byte-identical.
#include <algorithm>
#include <cstring>

#include "internal.hpp"
#include "kernels.hpp"
#include "lookup.hpp"
#include "wave.hpp"

namespace rbg {

struct Meta {
  int present, type, card, runs;
};

// table[row * 65536 + key] = container index of bitmap (first + row) at key, else -1
__global__ __launch_bounds__(256) void k_bsi_index(SetView s, uint32_t first, int32_t *table) {
  const uint32_t row = blockIdx.y;
  const uint64_t lo = s.begin[first + row], hi = s.begin[first + row + 1];
  for (uint64_t c = lo + (uint64_t)blockIdx.x * 256 + threadIdx.x; c < hi; c += (uint64_t)gridDim.x * 256)
    table[(uint64_t)row * 65536 + s.key[c]] = (int32_t)c;
}
// keys of F (ebM or foundSet) inside the shard's [key_lo, key_hi), in a per-block layout: k_bsi_active
// leaves each 256-key block's count in bt, the counts are scanned (bts, bts[256] = nk) and k_bsi_list
// places the keys
__global__ __launch_bounds__(256) void k_bsi_active(const int32_t *frow, uint32_t key_lo, uint32_t key_hi,
                                                    uint64_t *bt) {
  __shared__ uint32_t wt[4];
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  const uint32_t n = block_flag_count(frow[k] >= 0 && k >= key_lo && k < key_hi, wt);
  if (threadIdx.x == 0) bt[blockIdx.x] = n;
}
__global__ __launch_bounds__(256) void k_bsi_list(const int32_t *frow, uint32_t key_lo, uint32_t key_hi,
                                                  const uint64_t *bts, uint32_t *klist) {
  __shared__ uint32_t wt[4];
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  const bool f = frow[k] >= 0 && k >= key_lo && k < key_hi;
  const uint32_t r = block_flag_rank(f, wt);
  if (f) klist[bts[blockIdx.x] + r] = k;
}

// ---- per-key value algebra with the reference's type rules --------------------------------
__device__ __forceinline__ uint64_t lds_word(const uint32_t *s, int j, int lane) {
  const uint2 v = reinterpret_cast<const uint2 *>(s)[(j >> 1) * 128 + 2 * lane + (j & 1)];
  return pack2(v.x, v.y);
}
__device__ __forceinline__ void lds_put_word(uint32_t *s, int j, int lane, uint64_t w) {
  reinterpret_cast<uint2 *>(s)[(j >> 1) * 128 + 2 * lane + (j & 1)] = make_uint2((uint32_t)w, (uint32_t)(w >> 32));
}
// metadata of a fresh result in w under rule `eff` (EFF) / `or_bitmap` (LR) / otherwise AB
__device__ __forceinline__ Meta classify(const uint64_t (&w)[kW], int lane, bool eff, bool lr, bool never_empty) {
  Meta m;
  int c, r;
  metrics(w, lane, eff, c, r);
  m.card = c;
  m.runs = 0;
  m.present = c > 0 || never_empty;
  if (!m.present) return m;
  if (eff) {
    m.type = type_eff(c, r);
    m.runs = m.type == kRun ? r : 0;
  } else if (lr) {
    m.type = type_lr(c);
    m.runs = m.type == kRun ? 1 : 0;
  } else {
    m.type = type_ab(c);
  }
  return m;
}
__device__ __forceinline__ bool eff_and(const Meta &a, const Meta &b) { return a.type == kRun && b.type == kRun; }
__device__ __forceinline__ bool eff_andnot(const Meta &a, const Meta &b) {
  return a.type == kRun && (b.type == kRun || (b.type == kArray && b.card < kRunArrayThreshold));
}
__device__ __forceinline__ bool lr_or(const Meta &a, const Meta &b) { return a.type == kBitmap || b.type == kBitmap; }
__device__ __forceinline__ bool eff_or(const Meta &a, const Meta &b) {
  return !lr_or(a, b) && !(a.type == kArray && b.type == kArray);
}

// Any container (global payload) -> LDS image s.
__device__ __forceinline__ Meta stage_global(const SetView &v, int32_t c, uint32_t *s, int lane) {
  Meta m{0, 0, 0, 0};
  if (c < 0) return m;
  m.present = 1;
  m.type = v.type[c];
  m.card = (int)v.card[c];
  m.runs = v.nruns[c];
  stage_container(m.type, v.payload + v.off[c], (uint32_t)m.card, (uint32_t)m.runs, s, lane);
  return m;
}

enum { kBsiEQ = 0, kBsiNEQ = 1, kBsiLE = 2, kBsiLT = 3, kBsiGE = 4, kBsiGT = 5 };

template <int FINAL>
__global__ __launch_bounds__(256, 2) void k_bsi_chain(SetView bsi, SetView fnd, int has_found,
                                                      const int32_t *__restrict__ table, uint32_t nbits, uint64_t pred,
                                                      const uint32_t *__restrict__ klist, uint32_t nk,
                                                      uint8_t *__restrict__ out, WideOut wo, uint64_t *stats) {
  constexpr int TRACK = (FINAL == kBsiGE || FINAL == kBsiGT) ? 1 : (FINAL == kBsiLE || FINAL == kBsiLT) ? 2 : 0;
  __shared__ __attribute__((aligned(16))) uint32_t lds[4][2][2048];
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t q = xcd_swizzle(blockIdx.x, gridDim.x) * 4 + wv;
  if (q >= nk) return;
  uint32_t *sS = lds[wv][0], *sX = lds[wv][1];
  const uint32_t key = klist[q];
  uint64_t inb = 0;

  // EQ = ebM's container (RoaringBitmapSliceIndex.java:438: EQ = this.ebM, no copy)
  uint64_t e[kW];
  Meta eq = stage_global(bsi, table[(uint64_t)nbits * 65536 + key], sS, lane);
  if (eq.present) {
    lds_read_words(sS, e, lane);
    inb += payload_bytes(eq.type, eq.card, eq.runs) + 16;
  } else {
#pragma unroll
    for (int j = 0; j < kW; ++j) e[j] = 0;
  }
  wave_lds_sync();
  Meta x{0, 0, 0, 0};

  // slice descriptors, lane i <-> slice i (nbits <= 64)
  const int32_t sc = lane < (int)nbits ? table[(uint64_t)lane * 65536 + key] : -1;
  int st = 0;
  uint32_t scard = 0, sruns = 0;
  uint64_t soff = 0;
  if (sc >= 0) {
    st = bsi.type[sc];
    scard = bsi.card[sc];
    sruns = bsi.nruns[sc];
    soff = bsi.off[sc];
  }
  auto sbytes = [&](int i) -> uint32_t {
    const int t = (int)readlane((uint32_t)st, i);
    return (uint32_t)payload_bytes(t, readlane(scard, i), readlane(sruns, i));
  };
  auto sptr = [&](int i) -> const uint8_t * {
    return bsi.payload + pack2(readlane((uint32_t)soff, i), readlane((uint32_t)(soff >> 32), i));
  };
  uint4 pq[8];
  if (nbits) {
    const int i0 = (int)nbits - 1;
    const bool ok = (int)readlane((uint32_t)sc, i0) >= 0 && sbytes(i0) <= (uint32_t)kBitmapBytes;
    load_chunks(pq, ok ? sptr(i0) : bsi.payload, ok ? sbytes(i0) : 16u, lane);
  }
  for (int i = (int)nbits - 1; i >= 0; --i) {
    const bool spresent = (int)readlane((uint32_t)sc, i) >= 0;
    Meta sm{0, 0, 0, 0};
    if (spresent) {
      sm.present = 1;
      sm.type = (int)readlane((uint32_t)st, i);
      sm.card = (int)readlane(scard, i);
      sm.runs = (int)readlane(sruns, i);
      inb += payload_bytes(sm.type, sm.card, sm.runs) + 16;
      if (payload_bytes(sm.type, sm.card, sm.runs) > (uint64_t)kBitmapBytes) {
        // > 2047 runs: straight from global
        lds_zero(sS, lane);
        wave_lds_sync();
        const uint32_t *r32 = reinterpret_cast<const uint32_t *>(sptr(i));
        for (int k = lane; k < sm.runs; k += 64) toggle_run(sS, r32[k]);
        wave_lds_sync();
        toggles_to_words_lds(sS, lane);
        wave_lds_sync();
      } else {
        stage_from_chunks(sm.type, pq, (uint32_t)sm.card, (uint32_t)sm.runs, sS, lane);
      }
    }
    // ---- next slice in flight during this step's algebra
    __builtin_amdgcn_sched_barrier(0);
    if (i > 0) {
      const bool ok = (int)readlane((uint32_t)sc, i - 1) >= 0 && sbytes(i - 1) <= (uint32_t)kBitmapBytes;
      load_chunks(pq, ok ? sptr(i - 1) : bsi.payload, ok ? sbytes(i - 1) : 16u, lane);
    }
    if (!eq.present) continue; // and/andNot of an absent EQ stay absent; GT/LT unchanged
    const int bit = (int)((pred >> i) & 1);
    const bool feeds = (TRACK == 2 && bit) || (TRACK == 1 && !bit);
    // t = bit ? andNot(EQ, S) : and(EQ, S);  EQ = bit ? and(EQ, S) : andNot(EQ, S)
    uint64_t t[kW];
#pragma unroll
    for (int j = 0; j < kW; ++j) {
      const uint64_t sw = spresent ? lds_word(sS, j, lane) : 0ull;
      t[j] = bit ? (e[j] & ~sw) : (e[j] & sw);
      e[j] = bit ? (e[j] & sw) : (e[j] & ~sw);
    }
    wave_lds_sync();
    Meta tm{0, 0, 0, 0};
    if (!spresent) {
      if (bit) {
        tm = eq;          // andNot(EQ, absent) = clone of EQ
        eq.present = 0;   // and(EQ, absent) = absent
      } // else: t absent, EQ = clone of EQ (unchanged)
    } else {
      const Meta e0 = eq;
      if (feeds) tm = classify(t, lane, bit ? eff_andnot(e0, sm) : eff_and(e0, sm), false, false);
      eq = classify(e, lane, bit ? eff_and(e0, sm) : eff_andnot(e0, sm), false, false);
    }
    if (feeds && tm.present) {
      if (!x.present) {
        lds_write_words(sX, t, lane); // or(absent, t) = clone of t
        x = tm;
      } else {
        const Meta x0 = x;
#pragma unroll
        for (int j = 0; j < kW; ++j) t[j] |= lds_word(sX, j, lane);
        x = classify(t, lane, eff_or(x0, tm), lr_or(x0, tm), true);
        lds_write_words(sX, t, lane);
      }
      wave_lds_sync();
    }
  }

  // ---- the final ops with the found set F (foundSet, or ebM when null)
  const int32_t fc = has_found ? table[(uint64_t)(nbits + 1) * 65536 + key] : table[(uint64_t)nbits * 65536 + key];
  const Meta fm = stage_global(has_found ? fnd : bsi, fc, sS, lane); // present: keys come from F
  if (has_found) inb += payload_bytes(fm.type, fm.card, fm.runs) + 16;
  // EQ = and(fixedFoundSet, EQ)
  if (eq.present) {
    const Meta e0 = eq;
#pragma unroll
    for (int j = 0; j < kW; ++j) e[j] &= lds_word(sS, j, lane);
    eq = classify(e, lane, eff_and(fm, e0), false, false);
  }
  Meta rm{0, 0, 0, 0};
  uint64_t t[kW]; // the result (EQ copies e in)
  if (FINAL == kBsiEQ) {
    rm = eq;
#pragma unroll
    for (int j = 0; j < kW; ++j) t[j] = e[j];
  } else if (FINAL == kBsiNEQ) { // andNot(fixedFoundSet, EQ)
    if (!eq.present) {
#pragma unroll
      for (int j = 0; j < kW; ++j) t[j] = lds_word(sS, j, lane);
      rm = fm;
    } else {
#pragma unroll
      for (int j = 0; j < kW; ++j) t[j] = lds_word(sS, j, lane) & ~e[j];
      rm = classify(t, lane, eff_andnot(fm, eq), false, false);
    }
  } else {
    // Y = GT / LT, or or(LT|GT, EQ) for LE / GE
    Meta ym = x;
#pragma unroll
    for (int j = 0; j < kW; ++j) t[j] = x.present ? lds_word(sX, j, lane) : 0ull;
    if (FINAL == kBsiLE || FINAL == kBsiGE) {
      if (!x.present) {
#pragma unroll
        for (int j = 0; j < kW; ++j) t[j] = e[j];
        ym = eq;
      } else if (eq.present) {
#pragma unroll
        for (int j = 0; j < kW; ++j) t[j] |= e[j];
        ym = classify(t, lane, eff_or(x, eq), lr_or(x, eq), true);
      }
    }
    // and(Y, fixedFoundSet)
    if (ym.present) {
#pragma unroll
      for (int j = 0; j < kW; ++j) t[j] &= lds_word(sS, j, lane);
      rm = classify(t, lane, eff_and(ym, fm), false, false);
    }
  }
  wave_lds_sync();
  const int ty = rm.present ? rm.type : kEmpty;
  if (rm.present) emit_container(ty, t, rm.card, rm.runs, out + (uint64_t)q * kBitmapBytes, sS, lane);
  if (lane == 0) {
    wo.type[q] = (uint8_t)ty;
    wo.card[q] = (uint32_t)(rm.present ? rm.card : 0);
    wo.nruns[q] = (uint16_t)(ty == kRun ? rm.runs : 0);
    if (inb) atomicAdd((unsigned long long *)&stats[0 * kStripes + (q & (kStripes - 1))], (unsigned long long)inb);
    if (rm.present)
      atomicAdd((unsigned long long *)&stats[1 * kStripes + (q & (kStripes - 1))],
                (unsigned long long)(payload_bytes(ty, rm.card, rm.runs) + (ty == kRun ? 2 : 0) + 16));
  }
}

// ---- RANGE fused: both O'Neil chains (GE(start) and LE(end)) walk the slices in ONE pass, so every
// slice container is staged once for the two comparators; the keyed static AND of the two results
// (RoaringBitmapSliceIndex.java:492-497; AND rule R&R -> EFF else AB, empty / one-sided dropped)
// closes the kernel.  Each chain keeps its own EQ (registers) and GT / LT accumulator (LDS image)
// with the same per-step type rules as k_bsi_chain.
// One chain step (k_bsi_chain's loop body after the slice is staged): TRACK 1 = GT (GE), 2 = LT (LE).
// ior: the accumulator takes the in-place or (Container.ior), whose types are the static or's except
// BitmapContainer.ior(ArrayContainer), which keeps a Bitmap even when the result is full (BitmapContainer.java:749-766)
__device__ __forceinline__ void bsi_step(uint64_t (&e)[kW], Meta &eq, Meta &x, uint32_t *sX, int bit, int track,
                                         bool spresent, const Meta &sm, const uint32_t *sS, int lane,
                                         bool ior = false) {
  if (!eq.present) return; // and/andNot of an absent EQ stay absent; GT/LT unchanged
  const bool feeds = (track == 2 && bit) || (track == 1 && !bit);
  uint64_t t[kW];
#pragma unroll
  for (int j = 0; j < kW; ++j) {
    const uint64_t sw = spresent ? lds_word(sS, j, lane) : 0ull;
    t[j] = bit ? (e[j] & ~sw) : (e[j] & sw);
    e[j] = bit ? (e[j] & sw) : (e[j] & ~sw);
  }
  wave_lds_sync();
  Meta tm{0, 0, 0, 0};
  if (!spresent) {
    if (bit) {
      tm = eq;        // andNot(EQ, absent) = clone of EQ
      eq.present = 0; // and(EQ, absent) = absent
    }
  } else {
    const Meta e0 = eq;
    if (feeds) tm = classify(t, lane, bit ? eff_andnot(e0, sm) : eff_and(e0, sm), false, false);
    eq = classify(e, lane, bit ? eff_and(e0, sm) : eff_andnot(e0, sm), false, false);
  }
  if (feeds && tm.present) {
    if (!x.present) {
      lds_write_words(sX, t, lane); // or(absent, t) = clone of t
      x = tm;
    } else {
      const Meta x0 = x;
#pragma unroll
      for (int j = 0; j < kW; ++j) t[j] |= lds_word(sX, j, lane);
      x = classify(t, lane, eff_or(x0, tm), lr_or(x0, tm), true);
      if (ior && x0.type == kBitmap && tm.type == kArray) {
        x.type = kBitmap;
        x.runs = 0;
      }
      lds_write_words(sX, t, lane);
    }
    wave_lds_sync();
  }
}
// GE / LE result of one chain: Y = or(GT|LT, EQ), then and(Y, fixedFoundSet) (F staged in sS)
__device__ __forceinline__ Meta bsi_final_ge_le(uint64_t (&t)[kW], const uint64_t (&e)[kW], const Meta &eq,
                                                const Meta &x, const uint32_t *sX, const Meta &fm,
                                                const uint32_t *sS, int lane) {
  Meta ym = x;
#pragma unroll
  for (int j = 0; j < kW; ++j) t[j] = x.present ? lds_word(sX, j, lane) : 0ull;
  if (!x.present) {
#pragma unroll
    for (int j = 0; j < kW; ++j) t[j] = e[j];
    ym = eq;
  } else if (eq.present) {
#pragma unroll
    for (int j = 0; j < kW; ++j) t[j] |= e[j];
    ym = classify(t, lane, eff_or(x, eq), lr_or(x, eq), true);
  }
  Meta rm{0, 0, 0, 0};
  if (ym.present) {
#pragma unroll
    for (int j = 0; j < kW; ++j) t[j] &= lds_word(sS, j, lane);
    rm = classify(t, lane, eff_and(ym, fm), false, false);
  }
  return rm;
}
// RANGE's one launch: per key both chains and the final AND (bsi_range_key), then the call's tail in the
// last block to finish (the hand-off of wave.hpp's st_sc1 / ld_sc1): the keyed results compacted into the
// result SoA and CSR, the counters and the result count written to host-visible words, the call's sequence
// number last (the host returns on it: wait_call_seq).
struct BsiTail {
  uint64_t *kmeta;  // [nk] per key: card (bits 0-16), type (19-20; 3 = none), key (24-39), run count (40-55)
  uint64_t *ctr;    // [0] finished blocks, [8] / [16] / [24] input bytes / output bytes / cardinality
  OutView ov;
  uint64_t *rbegin; // [2]
  uint64_t *hout;   // host-visible: [0] result containers, [1..3] the counters, [5] = seq
  uint64_t seq;
  uint32_t nblocks;
};
__device__ __forceinline__ uint64_t bsi_meta(uint32_t key, int ty, uint32_t card, uint32_t nr) {
  return (card & 0x1FFFFu) | ((uint64_t)(ty == (int)kEmpty ? 3u : (uint32_t)ty) << 19) | ((uint64_t)key << 24) |
         ((uint64_t)nr << 40);
}
__global__ __launch_bounds__(128, 2) void k_bsi_range(SetView bsi, SetView fnd, int has_found,
                                                      const int32_t *__restrict__ table, uint32_t nbits,
                                                      uint64_t start, uint64_t end, const uint32_t *__restrict__ klist,
                                                      uint32_t nk, uint8_t *__restrict__ out, BsiTail tl) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[2][3][2048];
  __shared__ uint64_t red[2][3];
  __shared__ uint32_t s_last, wt[4];
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t q = xcd_swizzle(blockIdx.x, gridDim.x) * 2 + wv;
  uint64_t inb = 0, outb = 0, csum = 0;
  if (q < nk) { // wave-uniform
  uint32_t *sS = lds[wv][0], *sG = lds[wv][1], *sL = lds[wv][2];
  const uint32_t key = klist[q];
  uint64_t eg[kW], el[kW];
  Meta eqg = stage_global(bsi, table[(uint64_t)nbits * 65536 + key], sS, lane);
  if (eqg.present) {
    lds_read_words(sS, eg, lane);
    inb += payload_bytes(eqg.type, eqg.card, eqg.runs) + 16; // ebM, read once for both comparators
  } else {
#pragma unroll
    for (int j = 0; j < kW; ++j) eg[j] = 0;
  }
#pragma unroll
  for (int j = 0; j < kW; ++j) el[j] = eg[j];
  Meta eql = eqg;
  wave_lds_sync();
  Meta xg{0, 0, 0, 0}, xl{0, 0, 0, 0};
  const int32_t sc = lane < (int)nbits ? table[(uint64_t)lane * 65536 + key] : -1;
  int st = 0;
  uint32_t scard = 0, sruns = 0;
  uint64_t soff = 0;
  if (sc >= 0) {
    st = bsi.type[sc];
    scard = bsi.card[sc];
    sruns = bsi.nruns[sc];
    soff = bsi.off[sc];
  }
  auto sbytes = [&](int i) -> uint32_t {
    const int t = (int)readlane((uint32_t)st, i);
    return (uint32_t)payload_bytes(t, readlane(scard, i), readlane(sruns, i));
  };
  auto sptr = [&](int i) -> const uint8_t * {
    return bsi.payload + pack2(readlane((uint32_t)soff, i), readlane((uint32_t)(soff >> 32), i));
  };
  uint4 pq[8];
  if (nbits) {
    const int i0 = (int)nbits - 1;
    const bool ok = (int)readlane((uint32_t)sc, i0) >= 0 && sbytes(i0) <= (uint32_t)kBitmapBytes;
    load_chunks(pq, ok ? sptr(i0) : bsi.payload, ok ? sbytes(i0) : 16u, lane);
  }
  for (int i = (int)nbits - 1; i >= 0; --i) {
    const bool spresent = (int)readlane((uint32_t)sc, i) >= 0;
    Meta sm{0, 0, 0, 0};
    if (spresent) {
      sm.present = 1;
      sm.type = (int)readlane((uint32_t)st, i);
      sm.card = (int)readlane(scard, i);
      sm.runs = (int)readlane(sruns, i);
      inb += payload_bytes(sm.type, sm.card, sm.runs) + 16; // one read serves both comparators
      if (payload_bytes(sm.type, sm.card, sm.runs) > (uint64_t)kBitmapBytes) {
        lds_zero(sS, lane);
        wave_lds_sync();
        const uint32_t *r32 = reinterpret_cast<const uint32_t *>(sptr(i));
        for (int k = lane; k < sm.runs; k += 64) toggle_run(sS, r32[k]);
        wave_lds_sync();
        toggles_to_words_lds(sS, lane);
        wave_lds_sync();
      } else {
        stage_from_chunks(sm.type, pq, (uint32_t)sm.card, (uint32_t)sm.runs, sS, lane);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (i > 0) {
      const bool ok = (int)readlane((uint32_t)sc, i - 1) >= 0 && sbytes(i - 1) <= (uint32_t)kBitmapBytes;
      load_chunks(pq, ok ? sptr(i - 1) : bsi.payload, ok ? sbytes(i - 1) : 16u, lane);
    }
    bsi_step(eg, eqg, xg, sG, (int)((start >> i) & 1), 1, spresent, sm, sS, lane);
    bsi_step(el, eql, xl, sL, (int)((end >> i) & 1), 2, spresent, sm, sS, lane);
  }
  // ---- the final ops with the found set F (foundSet, or ebM when null), per chain
  const int32_t fc = has_found ? table[(uint64_t)(nbits + 1) * 65536 + key] : table[(uint64_t)nbits * 65536 + key];
  const Meta fm = stage_global(has_found ? fnd : bsi, fc, sS, lane);
  if (has_found) inb += payload_bytes(fm.type, fm.card, fm.runs) + 16;
  // EQ = and(fixedFoundSet, EQ), both chains
  if (eqg.present) {
    const Meta e0 = eqg;
#pragma unroll
    for (int j = 0; j < kW; ++j) eg[j] &= lds_word(sS, j, lane);
    eqg = classify(eg, lane, eff_and(fm, e0), false, false);
  }
  if (eql.present) {
    const Meta e0 = eql;
#pragma unroll
    for (int j = 0; j < kW; ++j) el[j] &= lds_word(sS, j, lane);
    eql = classify(el, lane, eff_and(fm, e0), false, false);
  }
  uint64_t t[kW];
  const Meta rg = bsi_final_ge_le(t, eg, eqg, xg, sG, fm, sS, lane);
  wave_lds_sync();
  lds_write_words(sG, t, lane); // GE result parked in its (now free) accumulator image
  wave_lds_sync();
  const Meta rl = bsi_final_ge_le(t, el, eql, xl, sL, fm, sS, lane);
  Meta rm{0, 0, 0, 0};
  if (rg.present && rl.present) {
#pragma unroll
    for (int j = 0; j < kW; ++j) t[j] &= lds_word(sG, j, lane);
    rm = classify(t, lane, eff_and(rg, rl), false, false);
  }
  wave_lds_sync();
  const int ty = rm.present ? rm.type : kEmpty;
  if (rm.present) emit_container(ty, t, rm.card, rm.runs, out + (uint64_t)q * kBitmapBytes, sS, lane);
  if (lane == 0)
    st_sc1(tl.kmeta + q, bsi_meta(key, ty, rm.present ? (uint32_t)rm.card : 0u, ty == kRun ? (uint32_t)rm.runs : 0u));
  if (rm.present) {
    outb = payload_bytes(ty, rm.card, rm.runs) + (ty == kRun ? 2 : 0) + 16;
    csum = (uint64_t)rm.card;
  }
  } // q < nk
  // ---- the block's counters (one agent atomic per counter), then the finished-block add
  if (lane == 0) {
    red[wv][0] = inb;
    red[wv][1] = outb;
    red[wv][2] = csum;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const uint64_t x = red[0][threadIdx.x] + red[1][threadIdx.x];
    if (x) __hip_atomic_fetch_add(tl.ctr + 8 + 8 * threadIdx.x, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0)
    s_last = __hip_atomic_fetch_add(tl.ctr, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == tl.nblocks - 1ull;
  __syncthreads();
  if (!s_last) return;
  // ---- the last block: the keyed results compacted in key order (dropped keys leave no container)
  const uint64_t v = threadIdx.x < 3 ? ld_sc1(tl.ctr + 8 + 8 * threadIdx.x) : 0;
  constexpr int kPer = 16;
  uint32_t base = 0;
  for (uint32_t t0 = 0; t0 < nk; t0 += kPer * blockDim.x) {
    const uint32_t lo = t0 + kPer * threadIdx.x;
    uint64_t m[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) m[k] = lo + k < nk ? ld_sc1(tl.kmeta + lo + k) : (3ull << 19);
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) cnt += ((m[k] >> 19) & 3u) != 3u;
    uint32_t tot;
    uint32_t r = base + block_xscan(cnt, wt, tot);
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      if (((m[k] >> 19) & 3u) == 3u) continue;
      tl.ov.key[r] = (uint16_t)(m[k] >> 24);
      tl.ov.type[r] = (uint8_t)((m[k] >> 19) & 3u);
      tl.ov.card[r] = (uint32_t)(m[k] & 0x1FFFFu);
      tl.ov.nruns[r] = (uint16_t)(m[k] >> 40);
      tl.ov.off[r] = (uint64_t)(lo + k) * kBitmapBytes;
      ++r;
    }
    base += tot;
  }
  if (threadIdx.x < 3) {
    red[0][threadIdx.x] = v;
    __hip_atomic_store(tl.ctr + 8 + 8 * threadIdx.x, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_store(tl.ctr, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // ready for the next call
    tl.rbegin[0] = 0;
    tl.rbegin[1] = base;
    for (int k = 0; k < 3; ++k) tl.hout[1 + k] = red[0][k];
    tl.hout[0] = base;
    __hip_atomic_store(tl.hout + 5, tl.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---------------------------------------------------------------- host side
static unsigned nblk(uint64_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

// Keyed slots of one reduction: an 8 KiB payload slot per active key plus its type / card / runs (the call's
// scratch).
struct KeyedSlots {
  uint8_t *payload = nullptr;
  WideOut wo{nullptr, nullptr, nullptr};
  int alloc(Scratch &w, uint32_t nk, bool with_payload) {
    if ((with_payload && !w.get(payload, (uint64_t)std::max<uint32_t>(nk, 1) * kBitmapBytes)) || !w.get(wo.type, nk) ||
        !w.get(wo.card, nk) || !w.get(wo.nruns, nk))
      return fail(RB_ENOMEM, "bsi slots for %u keys", nk);
    return RB_OK;
  }
};

// One O'Neil chain (oNeilCompare with `final_op`) over the keys of F into keyed slots.
static void bsi_chain(rbgpu_ctx *ctx, const rbgpu_set *bsi, uint32_t nbits, int final_op, uint64_t pred,
                      const rbgpu_set *found, const int32_t *d_table, const uint32_t *d_klist, uint32_t nk,
                      uint8_t *o, const WideOut &wo) {
  if (!nk) return;
  hipStream_t st = ctx->stream;
  const SetView bv = bsi->view();
  const SetView fv = found ? found->view() : bv;
  const int hf = found != nullptr;
  const unsigned g = nblk(nk, 4);
  switch (final_op) {
  case kBsiEQ: k_bsi_chain<kBsiEQ><<<g, 256, 0, st>>>(bv, fv, hf, d_table, nbits, pred, d_klist, nk, o, wo, ctx->d_stats); break;
  case kBsiNEQ: k_bsi_chain<kBsiNEQ><<<g, 256, 0, st>>>(bv, fv, hf, d_table, nbits, pred, d_klist, nk, o, wo, ctx->d_stats); break;
  case kBsiLE: k_bsi_chain<kBsiLE><<<g, 256, 0, st>>>(bv, fv, hf, d_table, nbits, pred, d_klist, nk, o, wo, ctx->d_stats); break;
  case kBsiLT: k_bsi_chain<kBsiLT><<<g, 256, 0, st>>>(bv, fv, hf, d_table, nbits, pred, d_klist, nk, o, wo, ctx->d_stats); break;
  case kBsiGE: k_bsi_chain<kBsiGE><<<g, 256, 0, st>>>(bv, fv, hf, d_table, nbits, pred, d_klist, nk, o, wo, ctx->d_stats); break;
  default: k_bsi_chain<kBsiGT><<<g, 256, 0, st>>>(bv, fv, hf, d_table, nbits, pred, d_klist, nk, o, wo, ctx->d_stats); break;
  }
}

// compareUsingMinMax (RoaringBitmapSliceIndex.java:505-577), values unsigned: 1 = all, 0 = empty,
// -1 = evaluate
static int min_max_shortcut(int op, uint64_t a, uint64_t b, uint64_t mn, uint64_t mx) {
  switch (op) {
  case kBsiLT: return a > mx ? 1 : a <= mn ? 0 : -1;
  case kBsiLE: return a >= mx ? 1 : a < mn ? 0 : -1;
  case kBsiGT: return a < mn ? 1 : a >= mx ? 0 : -1;
  case kBsiGE: return a <= mn ? 1 : a > mx ? 0 : -1;
  case kBsiEQ: return (mn == mx && mn == a) ? 1 : (a < mn || a > mx) ? 0 : -1;
  case kBsiNEQ: return mn == mx ? (mn == a ? 0 : 1) : -1;
  default: return (a <= mn && b >= mx) ? 1 : (a > mx || b < mn) ? 0 : -1; // RANGE
  }
}

// The set's key -> container tables (rows 0..nbits: its slices and ebM; row nbits + 1: a call's foundSet)
// and ebM's key list, built on the set's first compare and kept with it (sets are immutable): the device
// time and bytes are the set's setup part 3 (rbgpu_set_setup_parts).
int ensure_bsi_tables(rbgpu_ctx *ctx, const rbgpu_set *cs, uint32_t nbits) {
  rbgpu_set *s = const_cast<rbgpu_set *>(cs);
  if (s->bsi_table) return RB_OK;
  int rc = ensure_h_begin(s);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  Scratch w(ctx->pool);
  int32_t *t = nullptr;
  uint32_t *kl = nullptr;
  uint64_t *bt = nullptr, *bts = nullptr;
  if (!w.get(t, (nbits + 2ull) * 65536) || !w.get(kl, 65536) || !w.get(bt, 65537) || !w.get(bts, 65537))
    return fail(RB_ENOMEM, "bsi tables");
  {
    DeriveTimer tm(s, 3);
    if (hipMemsetAsync(t, 0xFF, (nbits + 1ull) * 65536 * 4, st) != hipSuccess)
      return fail(RB_EDEVICE, "bsi table memset failed");
    k_bsi_index<<<dim3(64, nbits + 1), 256, 0, st>>>(s->view(), 0, t);
    const int32_t *frow = t + (uint64_t)nbits * 65536;
    k_bsi_active<<<256, 256, 0, st>>>(frow, 0, 65536, bt);
    const uint64_t *in1[1] = {bt};
    uint64_t *out1[1] = {bts};
    scan_blocks_multi(in1, out1, 1, 256, nullptr, st);
    k_bsi_list<<<256, 256, 0, st>>>(frow, 0, 65536, bts, kl);
  }
  w.give_back(bt); // stream-ordered: the pool hands them only to later work on this stream
  w.give_back(bts);
  if (hipGetLastError() != hipSuccess) return fail(RB_EDEVICE, "bsi table kernels failed");
  s->bsi_nk = (uint32_t)(s->h_begin[nbits + 1] - s->h_begin[nbits]);
  if (s->bsi_nk) { // ebM's first and last key: a key-range shard that holds them all takes the cached list
    uint32_t *h = reinterpret_cast<uint32_t *>(ctx->h_pinned);
    if (hipMemcpyAsync(h, kl, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(h + 1, kl + s->bsi_nk - 1, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return fail(RB_EDEVICE, "bsi key list read-back failed");
    s->bsi_kmin = h[0];
    s->bsi_kmax = h[1];
  }
  s->bsi_table = w.keep(t);
  s->bsi_klist = w.keep(kl);
  // keys read, table entries written (4 B per container), ebM's key list written
  const uint64_t b = 6ull * (s->h_begin[nbits + 1] - s->h_begin[0]) + 4ull * s->bsi_nk;
  s->derive_bytes += b;
  s->part_bytes[3] += b;
  return RB_OK;
}

// The tables of a call (ensure_bsi_tables, plus the foundSet's row) and F's keys inside [key_lo, key_hi), F = the
// foundSet or ebM: ebM's over the whole key range are the set's cached list; a foundSet's or a shard's are
// listed per call (in the call's scratch), and their count comes from F's host CSR over the whole range, else by
// a read-back.
struct BsiKeys {
  const uint32_t *d_klist = nullptr;
  uint32_t nk = 0;
};
static int bsi_keys(rbgpu_ctx *ctx, Scratch &w, const rbgpu_set *bsi, uint32_t nbits, const rbgpu_set *found,
                    uint32_t key_lo, uint32_t key_hi, BsiKeys &ks) {
  hipStream_t st = ctx->stream;
  // key -> container tables: rows 0..nbits-1 slices, nbits ebM (the set's, cached), nbits+1 foundSet
  int rc = ensure_bsi_tables(ctx, bsi, nbits);
  if (rc) return rc;
  int32_t *d_table = bsi->bsi_table;
  if (found) {
    int32_t *frow = d_table + (uint64_t)(nbits + 1) * 65536;
    HIPCHK(hipMemsetAsync(frow, 0xFF, 65536 * 4, st));
    k_bsi_index<<<dim3(64, 1), 256, 0, st>>>(found->view(), 0, frow);
  }
  const bool full = key_lo == 0 && key_hi >= 65536;
  if (!found && (full || !bsi->bsi_nk || (key_lo <= bsi->bsi_kmin && bsi->bsi_kmax < key_hi))) {
    // every key of ebM lies in the range (the whole range, or a shard holding the index's own keys)
    ks.d_klist = bsi->bsi_klist;
    ks.nk = bsi->bsi_nk;
    return RB_OK;
  }
  uint64_t *d_active = nullptr, *d_pos = nullptr;
  uint32_t *d_kl = nullptr;
  if (!w.get(d_active, 65537) || !w.get(d_pos, 65537) || !w.get(d_kl, 65536)) return fail(RB_ENOMEM, "bsi key list");
  const int32_t *frow = d_table + (uint64_t)(found ? nbits + 1 : nbits) * 65536;
  k_bsi_active<<<256, 256, 0, st>>>(frow, key_lo, key_hi, d_active);
  const uint64_t *in1[1] = {d_active};
  uint64_t *out1[1] = {d_pos};
  scan_blocks_multi(in1, out1, 1, 256, nullptr, st);
  k_bsi_list<<<256, 256, 0, st>>>(frow, key_lo, key_hi, d_pos, d_kl);
  ks.d_klist = d_kl;
  const rbgpu_set *fs = found ? found : bsi;
  const uint32_t fb = found ? 0u : nbits;
  hipError_t e = hipSuccess;
  if (full && !ensure_h_begin(fs)) {
    ks.nk = (uint32_t)(fs->h_begin[fb + 1] - fs->h_begin[fb]);
    e = hipGetLastError();
  } else {
    e = hipMemcpyAsync(ctx->h_pinned, d_pos + 256, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipGetLastError();
    ks.nk = (uint32_t)ctx->h_pinned[0];
  }
  if (e != hipSuccess) return fail(RB_EDEVICE, "bsi key list failed: %s", hipGetErrorString(e));
  return RB_OK;
}

// RANGE over nk >= 1 keys of F: k_bsi_range writes the result set (CSR, SoA, payload slots) and the call's
// counters itself; the host returns on the call's sequence number (wait_call_seq).
static int bsi_range_one_launch(rbgpu_ctx *ctx, const rbgpu_set *bsi, const rbgpu_set *found, const int32_t *d_table,
                                uint32_t nbits, uint64_t start, uint64_t end, const uint32_t *d_klist, uint32_t nk,
                                rbgpu_set *res) {
  hipStream_t st = ctx->stream;
  int rc = ensure_call_words(ctx);
  if (!rc) rc = seq_begin(ctx);
  if (rc) return rc;
  Scratch scratch(ctx->pool);
  uint64_t *kmeta = nullptr;
  if (!scratch.get(kmeta, nk)) return fail(RB_ENOMEM, "bsi key results");
  const uint32_t nblocks = nblk(nk, 2);
  BsiTail tl{kmeta, ctx->d_small_ctr, OutView{res->key, res->type, res->card, res->nruns, res->off}, res->begin,
             reinterpret_cast<uint64_t *>(ctx->d_small), ++ctx->small_seq, nblocks};
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  k_bsi_range<<<nblocks, 128, 0, st>>>(bsi->view(), found ? found->view() : bsi->view(), found != nullptr, d_table,
                                       nbits, start, end, d_klist, nk, res->payload, tl);
  HIPCHK(hipEventRecord(ctx->ev[2], st));
  HIPCHK(hipEventRecord(ctx->ev[5], st));
  scratch.give_back(kmeta); // stream-ordered: handed out again only to later work on this stream
  bool seen = false;
  rc = seq_end(ctx, tl.seq, true, "bsi range", &seen);
  if (rc) return rc;
  const uint64_t *hout = reinterpret_cast<const uint64_t *>(ctx->h_small);
  uint64_t *w = ctx->words;
  for (int i = 0; i < kStatWords; ++i) w[i] = 0;
  w[0] = hout[1]; // input bytes
  w[1] = hout[2]; // output bytes
  w[7] = hout[3]; // result cardinality
  w[8] = hout[0]; // result containers
  const uint64_t nres = hout[0];
  const KernelSpan spans[1] = {{"k_bsi_range", 0, 1, 2ull * nk}};
  rc = stats_fill(ctx, nk, nres, spans, 1, !seen);
  ctx->stats_pending = seen;
  ctx->stats_pending_k = seen;
  if (rc) return rc;
  ctx->last.result_containers = nres;
  res->nc = nres;
  res->h_begin = {0, nres};
  res->end_seq = seen ? tl.seq : 0;
  return RB_OK;
}

// An empty one-bitmap result (new RoaringBitmap()); rb_stats describes it: no kernel ran, nothing counted.
static int empty_result(rbgpu_ctx *ctx, rbgpu_set **out) {
  SetPtr e;
  const int rc = make_set(ctx, 1, 0, 16, e);
  if (rc) return rc;
  const uint64_t hb[2] = {0, 0};
  if (hipMemcpyAsync(e->begin, hb, 16, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess || hipGetLastError() != hipSuccess)
    return fail(RB_EDEVICE, "empty result");
  e->h_begin = {0, 0};
  for (int i = 0; i < kStatWords; ++i) ctx->words[i] = 0;
  *out = e.release();
  return stats_fill(ctx, 0, 0, nullptr, 0, false);
}

int bsi_compare(rbgpu_ctx *ctx, const rbgpu_set *bsi, int op, uint64_t start, uint64_t end, uint64_t vmin,
                uint64_t vmax, const rbgpu_set *found, uint32_t key_lo, uint32_t key_hi, rbgpu_set **out) {
  const uint32_t nbits = bsi->nb - 1;
  hipStream_t st = ctx->stream;
  stats_begin(ctx);
  const int sc = min_max_shortcut(op, start, end, vmin, vmax);
  if (sc >= 0 && (key_lo > 0 || key_hi < 65536)) {
    // a key-range shard of the shortcut's answer: the whole-range answer, restricted
    rbgpu_set *whole = nullptr;
    const int rc = bsi_compare(ctx, bsi, op, start, end, vmin, vmax, found, 0, 65536, &whole);
    if (rc) return rc;
    const SetPtr owner(whole);
    return set_key_subset(whole, key_lo, key_hi, out);
  }
  if (sc >= 0) {
    // all = foundSet == null ? ebM.clone() : and(ebM, foundSet); empty = new bitmap.  rb_stats describes this
    // call's answer (no compare kernel ran: no kernel times), not the previous call's
    auto shortcut_stats = [&](rbgpu_set *r, uint64_t card) {
      for (int i = 0; i < kStatWords; ++i) ctx->words[i] = 0;
      ctx->words[7] = card;
      return stats_fill(ctx, 0, r->nc, nullptr, 0, false);
    };
    if (sc == 0) return empty_result(ctx, out);
    if (!found) {
      int rc = rbgpu_set_extract(bsi, nbits, 1, out);
      uint64_t card = 0;
      if (!rc) rc = rbgpu_set_cardinalities(*out, &card);
      if (!rc) rc = shortcut_stats(*out, card);
      if (rc && *out) {
        rbgpu_set_free(*out);
        *out = nullptr;
      }
      return rc;
    }
    const uint32_t ai = nbits, bi = 0;
    return rbgpu_pairwise(ctx, RB_AND, bsi, found, &ai, &bi, 1, out); // its own stats: the AND's answer
  }
  // key -> container tables and F's keys in the range
  Scratch w(ctx->pool);
  BsiKeys ks;
  int rc = bsi_keys(ctx, w, bsi, nbits, found, key_lo, key_hi, ks);
  if (rc) return rc;
  const int32_t *d_table = bsi->bsi_table;
  const uint32_t *d_klist = ks.d_klist;
  const uint32_t nk = ks.nk;
  // result set: one 8 KiB slot per key of F, compacted at the end
  SetPtr res;
  if ((rc = make_set(ctx, 1, nk, (uint64_t)std::max<uint32_t>(nk, 1) * kBitmapBytes, res))) return rc;
  if (op == 6 && nk) { // RANGE: one launch (k_bsi_range's tail compacts and hands the results to the host)
    if ((rc = bsi_range_one_launch(ctx, bsi, found, d_table, nbits, start, end, d_klist, nk, res.get()))) return rc;
    *out = res.release();
    return RB_OK;
  }
  KeyedSlots fin;
  if ((rc = fin.alloc(w, nk, false))) return rc;
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  if (op != 6) {
    bsi_chain(ctx, bsi, nbits, op, start, found, d_table, d_klist, nk, res->payload, fin.wo);
  }
  HIPCHK(hipEventRecord(ctx->ev[2], st));
  if ((rc = compact_keyed(ctx, d_klist, nk, fin.wo, res.get()))) return rc;
  const KernelSpan spans[1] = {{op == 6 ? "k_bsi_range" : "k_bsi_chain", 0, 1, op == 6 ? 2ull * nk : nk}};
  if ((rc = stats_end(ctx, nk, 0, spans, 1))) return rc;
  keyed_result_count(ctx, res.get());
  *out = res.release();
  return RB_OK;
}

// ---------------------------------------------------------------- aggregates: sum and topK
// Roaring64BitmapSliceIndex.sum / topK (bsi/.../longlong/Roaring64BitmapSliceIndex.java:559-594).  Both walk
// the slices of one high key with the found set's container held as a register bitmap, as k_bsi_chain holds EQ.

// The slices' containers at one key, lane i <-> slice i (nbits <= 64), and the staged walk over them
// (k_bsi_chain's loop head: payloads of at most 8 KiB arrive through registers, a Run of more than 2047 runs is
// toggled straight from global).
struct SliceDesc {
  int32_t sc;
  int st;
  uint32_t scard, sruns;
  uint64_t soff;
  __device__ __forceinline__ void load(const SetView &bsi, const int32_t *table, uint32_t nbits, uint32_t key, int lane) {
    sc = lane < (int)nbits ? table[(uint64_t)lane * 65536 + key] : -1;
    st = 0;
    scard = sruns = 0;
    soff = 0;
    if (sc >= 0) {
      st = bsi.type[sc];
      scard = bsi.card[sc];
      sruns = bsi.nruns[sc];
      soff = bsi.off[sc];
    }
  }
  __device__ __forceinline__ bool present(int i) const { return (int)readlane((uint32_t)sc, i) >= 0; }
  __device__ __forceinline__ Meta meta(int i) const {
    return Meta{1, (int)readlane((uint32_t)st, i), (int)readlane(scard, i), (int)readlane(sruns, i)};
  }
  __device__ __forceinline__ uint32_t bytes(int i) const {
    return (uint32_t)payload_bytes((int)readlane((uint32_t)st, i), readlane(scard, i), readlane(sruns, i));
  }
  __device__ __forceinline__ const uint8_t *ptr(const SetView &bsi, int i) const {
    return bsi.payload + pack2(readlane((uint32_t)soff, i), readlane((uint32_t)(soff >> 32), i));
  }
  // slice i's payload into pq (i < 0, an absent slice or a payload past 8 KiB: one dummy chunk)
  __device__ __forceinline__ void prefetch(uint4 (&pq)[8], const SetView &bsi, int i, int lane) const {
    const bool ok = i >= 0 && present(i) && bytes(i) <= (uint32_t)kBitmapBytes;
    load_chunks(pq, ok ? ptr(bsi, i) : bsi.payload, ok ? bytes(i) : 16u, lane);
  }
  // present slice i (metadata sm, payload prefetched in pq) -> membership image sS
  __device__ __forceinline__ void stage(const uint4 (&pq)[8], const SetView &bsi, int i, const Meta &sm, uint32_t *sS,
                                        int lane) const {
    if (payload_bytes(sm.type, sm.card, sm.runs) > (uint64_t)kBitmapBytes) {
      lds_zero(sS, lane);
      wave_lds_sync();
      const uint32_t *r32 = reinterpret_cast<const uint32_t *>(ptr(bsi, i));
      for (int k = lane; k < sm.runs; k += 64) toggle_run(sS, r32[k]);
      wave_lds_sync();
      toggles_to_words_lds(sS, lane);
      wave_lds_sync();
    } else {
      stage_from_chunks(sm.type, pq, (uint32_t)sm.card, (uint32_t)sm.runs, sS, lane);
    }
  }
};

// sum's slice counts: one wave per key of F.  F's container is a register bitmap, every slice that has a container
// at the key is staged once (the next one's payload in flight) and popcount(F & S) is reduced over the wave so that
// lane i keeps slice i's count; an absent slice costs nothing.  The block's four waves add up in LDS and leave as
// one 64-lane u64 add into the block's stripe of acc[kStripes][kAccRow] (word 64: |F|); k_bsi_sum_fold sums the
// stripes.  Integer adds commute: the counts are exact whatever the order.
constexpr int kAccRow = 65;
__global__ __launch_bounds__(256, 2) void k_bsi_sum(SetView bsi, SetView fnd, int has_found,
                                                    const int32_t *__restrict__ table, uint32_t nbits,
                                                    const uint32_t *__restrict__ klist, uint32_t nk,
                                                    uint64_t *__restrict__ acc, uint64_t *stats) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[4][2048];
  __shared__ uint32_t part[4][kAccRow];
  __shared__ uint64_t red[4];
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t q = xcd_swizzle(blockIdx.x, gridDim.x) * 4 + wv;
  uint32_t mine = 0, fcard = 0;
  uint64_t inb = 0;
  if (q < nk) { // wave-uniform
    uint32_t *sS = lds[wv];
    const uint32_t key = klist[q];
    uint64_t e[kW];
    const Meta fm = stage_global(has_found ? fnd : bsi, table[(uint64_t)(has_found ? nbits + 1 : nbits) * 65536 + key],
                                 sS, lane); // present: the keys come from F
    lds_read_words(sS, e, lane);
    wave_lds_sync();
    fcard = (uint32_t)fm.card;
    inb += payload_bytes(fm.type, fm.card, fm.runs) + 16;
    SliceDesc d;
    d.load(bsi, table, nbits, key, lane);
    uint64_t todo = __ballot(d.sc >= 0);
    uint4 pq[8];
    if (todo) d.prefetch(pq, bsi, __builtin_ctzll(todo), lane);
    while (todo) {
      const int i = __builtin_ctzll(todo);
      todo &= todo - 1;
      const Meta sm = d.meta(i);
      inb += payload_bytes(sm.type, sm.card, sm.runs) + 16;
      d.stage(pq, bsi, i, sm, sS, lane);
      // ---- the next present slice in flight during this one's count
      __builtin_amdgcn_sched_barrier(0);
      if (todo) d.prefetch(pq, bsi, __builtin_ctzll(todo), lane);
      uint32_t p = 0;
#pragma unroll
      for (int j = 0; j < kW; ++j) p += (uint32_t)__popcll(e[j] & lds_word(sS, j, lane));
      wave_lds_sync();
      const uint32_t tot = wave_sum_u32(p);
      if (lane == i) mine = tot;
    }
  }
  part[wv][lane] = mine;
  if (lane == 0) {
    part[wv][64] = fcard;
    red[wv] = inb;
  }
  __syncthreads();
  if (wv != 0) return;
  const uint32_t stripe = blockIdx.x & (kStripes - 1);
  const uint64_t c = (uint64_t)part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
  if (c) atomicAdd((unsigned long long *)&acc[stripe * kAccRow + lane], (unsigned long long)c);
  if (lane == 0) {
    const uint64_t f = (uint64_t)part[0][64] + part[1][64] + part[2][64] + part[3][64];
    if (f) atomicAdd((unsigned long long *)&acc[stripe * kAccRow + 64], (unsigned long long)f);
    const uint64_t b = red[0] + red[1] + red[2] + red[3];
    if (b) atomicAdd((unsigned long long *)&stats[0 * kStripes + stripe], (unsigned long long)b);
  }
}
// out[i] = the stripes' sum of word i (slice i's count), out[nbits] = |F| (word 64 of the rows)
__global__ __launch_bounds__(128) void k_bsi_sum_fold(const uint64_t *__restrict__ acc, uint32_t nbits,
                                                      uint64_t *__restrict__ out) {
  const uint32_t t = threadIdx.x;
  if (t > nbits) return;
  const uint32_t w = t == nbits ? 64u : t;
  uint64_t s = 0;
  for (int k = 0; k < kStripes; ++k) s += acc[k * kAccRow + w];
  out[t] = s;
}

int bsi_slice_counts(rbgpu_ctx *ctx, const rbgpu_set *bsi, const rbgpu_set *found, uint32_t key_lo, uint32_t key_hi,
                     uint64_t *counts) {
  const uint32_t nbits = bsi->nb - 1;
  hipStream_t st = ctx->stream;
  stats_begin(ctx);
  Scratch w(ctx->pool);
  BsiKeys ks;
  int rc = bsi_keys(ctx, w, bsi, nbits, found, key_lo, key_hi, ks);
  if (rc) return rc;
  uint64_t *acc = nullptr; // [kStripes][kAccRow], then the folded nbits + 1 words
  if (!w.get(acc, (kStripes + 1ull) * kAccRow)) return fail(RB_ENOMEM, "bsi slice counts");
  uint64_t *folded = acc + kStripes * kAccRow;
  hipError_t e = hipMemsetAsync(acc, 0, (kStripes + 1ull) * kAccRow * 8, st);
  if (e == hipSuccess) e = hipEventRecord(ctx->ev[1], st);
  if (e == hipSuccess && ks.nk) {
    k_bsi_sum<<<nblk(ks.nk, 4), 256, 0, st>>>(bsi->view(), found ? found->view() : bsi->view(), found != nullptr,
                                              bsi->bsi_table, nbits, ks.d_klist, ks.nk, acc, ctx->d_stats);
    k_bsi_sum_fold<<<1, 128, 0, st>>>(acc, nbits, folded);
  }
  if (e == hipSuccess) e = hipEventRecord(ctx->ev[2], st);
  // the call's one read-back (stats_end waits for the stream)
  if (e == hipSuccess) e = hipMemcpyAsync(counts, folded, (nbits + 1ull) * 8, hipMemcpyDeviceToHost, st);
  w.give_back(acc); // stream-ordered: handed out again only to later work on this stream
  const uint32_t nk = ks.nk;
  if (e != hipSuccess) return fail(RB_EDEVICE, "bsi slice counts failed: %s", hipGetErrorString(e));
  const KernelSpan spans[1] = {{"k_bsi_sum", 0, -1, nk}};
  return stats_end(ctx, nk, 0, spans, 1);
}

// ---- topK.  The decision at slice x (keep the rows with the bit, or emit them and go on with the rest) needs the
// global count |cand AND bA[x]|, so the keys are not independent: phase A carries the dependence in stream order,
// one launch per slice, and leaves the counts; phase B, with every decision known, is key-local again.
//
// Phase A, the launch of slice x, one wave per key of found.  The candidates of a key are a dense 8 KiB image in
// global memory.  A wave first replays the chain of decisions of the slices above x from counts[] (final: their
// launches ended before this one began) and from k and |found|, which every wave does alike, so no wave waits for
// another; once the chain is over (k used up, or no candidate left) the launch returns at once.  It then applies
// slice x+1's decision to its image (and / andNot with bA[x+1]) and adds |cand AND bA[x]| to counts[x].  A slice
// container is read twice over the phase: counted in its own launch, applied in the next.
__global__ __launch_bounds__(256, 2) void k_bsi_topk_count(SetView bsi, SetView fnd, const int32_t *__restrict__ table,
                                                           uint32_t nbits, int x, uint64_t k0, uint64_t card0,
                                                           const uint32_t *__restrict__ klist, uint32_t nk,
                                                           uint8_t *__restrict__ img, uint64_t *counts) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[4][2048];
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t q = xcd_swizzle(blockIdx.x, gridDim.x) * 4 + wv;
  if (q >= nk) return;
  const uint64_t cv = lane < (int)nbits && lane > x ? counts[lane] : 0ull;
  uint64_t k = k0, cand = card0;
  int keep = 0; // slice x+1's decision: 1 = cand.and(bA[x+1]), 0 = re.or(...), cand.andNot(bA[x+1])
  for (int y = (int)nbits - 1; y > x; --y) {
    if (!cand || !k) return;
    const uint64_t c = pack2(readlane((uint32_t)cv, y), readlane((uint32_t)(cv >> 32), y));
    keep = c > k;
    if (keep) {
      cand = c;
    } else {
      cand -= c;
      k -= c;
    }
  }
  if (!cand || !k) return;
  uint32_t *sS = lds[wv];
  const uint32_t key = klist[q];
  uint8_t *im = img + (uint64_t)q * kBitmapBytes;
  uint64_t e[kW];
  if (x == (int)nbits - 1) { // candidates = foundSet.clone()
    stage_global(fnd, table[(uint64_t)(nbits + 1) * 65536 + key], sS, lane);
    lds_read_words(sS, e, lane);
    wave_lds_sync();
  } else {
    load_bitmap(im, e, lane);
    const Meta sm = stage_global(bsi, table[(uint64_t)(x + 1) * 65536 + key], sS, lane);
#pragma unroll
    for (int j = 0; j < kW; ++j) {
      const uint64_t sw = sm.present ? lds_word(sS, j, lane) : 0ull;
      e[j] = keep ? (e[j] & sw) : (e[j] & ~sw);
    }
    wave_lds_sync();
  }
  {
    uint4 *o = reinterpret_cast<uint4 *>(im);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j * 64 + lane] = make_uint4((uint32_t)e[2 * j], (uint32_t)(e[2 * j] >> 32), (uint32_t)e[2 * j + 1],
                                    (uint32_t)(e[2 * j + 1] >> 32));
  }
  const Meta sm = stage_global(bsi, table[(uint64_t)x * 65536 + key], sS, lane);
  if (!sm.present) return;
  uint32_t p = 0;
#pragma unroll
  for (int j = 0; j < kW; ++j) p += (uint32_t)__popcll(e[j] & lds_word(sS, j, lane));
  const uint32_t tot = wave_sum_u32(p);
  if (lane == 0 && tot) atomicAdd((unsigned long long *)&counts[x], (unsigned long long)tot);
}

// Phase B, the typed emit: k_bsi_chain's GT-tracking loop (bsi_step, track 1) with EQ = found's container, the
// decisions as the predicate (bit x set: cand.and(bA[x]); clear: re.or(and(cand, bA[x])), cand.andNot(bA[x])), the
// loop ending at the descent's last slice `stop`, the accumulator taking Roaring64Bitmap's in-place or, and no
// final AND: the result is the accumulator.
__global__ __launch_bounds__(256, 2) void k_bsi_topk_emit(SetView bsi, SetView fnd, const int32_t *__restrict__ table,
                                                          uint32_t nbits, uint64_t pred, int stop,
                                                          const uint32_t *__restrict__ klist, uint32_t nk,
                                                          uint8_t *__restrict__ out, WideOut wo, uint64_t *stats) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[4][2][2048];
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t q = xcd_swizzle(blockIdx.x, gridDim.x) * 4 + wv;
  if (q >= nk) return;
  uint32_t *sS = lds[wv][0], *sX = lds[wv][1];
  const uint32_t key = klist[q];
  uint64_t e[kW];
  Meta eq = stage_global(fnd, table[(uint64_t)(nbits + 1) * 65536 + key], sS, lane); // present: found's own key
  lds_read_words(sS, e, lane);
  wave_lds_sync();
  uint64_t inb = payload_bytes(eq.type, eq.card, eq.runs) + 16;
  Meta x{0, 0, 0, 0};
  SliceDesc d;
  d.load(bsi, table, nbits, key, lane);
  uint4 pq[8];
  d.prefetch(pq, bsi, (int)nbits - 1, lane);
  for (int i = (int)nbits - 1; i >= stop; --i) {
    const bool spresent = d.present(i);
    Meta sm{0, 0, 0, 0};
    if (spresent) {
      sm = d.meta(i);
      inb += payload_bytes(sm.type, sm.card, sm.runs) + 16;
      d.stage(pq, bsi, i, sm, sS, lane);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (i > stop) d.prefetch(pq, bsi, i - 1, lane);
    bsi_step(e, eq, x, sX, (int)((pred >> i) & 1), 1, spresent, sm, sS, lane, true);
  }
  uint64_t t[kW];
#pragma unroll
  for (int j = 0; j < kW; ++j) t[j] = x.present ? lds_word(sX, j, lane) : 0ull;
  wave_lds_sync();
  const int ty = x.present ? x.type : kEmpty;
  if (x.present) emit_container(ty, t, x.card, x.runs, out + (uint64_t)q * kBitmapBytes, sS, lane);
  if (lane == 0) {
    wo.type[q] = (uint8_t)ty;
    wo.card[q] = (uint32_t)(x.present ? x.card : 0);
    wo.nruns[q] = (uint16_t)(ty == kRun ? x.runs : 0);
    atomicAdd((unsigned long long *)&stats[0 * kStripes + (q & (kStripes - 1))], (unsigned long long)inb);
    if (x.present)
      atomicAdd((unsigned long long *)&stats[1 * kStripes + (q & (kStripes - 1))],
                (unsigned long long)(payload_bytes(ty, x.card, x.runs) + (ty == kRun ? 2 : 0) + 16));
  }
}

int bsi_topk(rbgpu_ctx *ctx, const rbgpu_set *bsi, const rbgpu_set *found, uint64_t k, rbgpu_set **out) {
  const uint32_t nbits = bsi->nb - 1;
  hipStream_t st = ctx->stream;
  uint64_t fcard = 0;
  if (found) {
    const int rc = rbgpu_set_cardinalities(found, &fcard);
    if (rc) return rc;
  }
  stats_begin(ctx);
  if (!fcard) return empty_result(ctx, out);                       // null or empty foundSet: new Roaring64Bitmap()
  if (k >= fcard) return rbgpu_set_extract(found, 0, 1, out);      // foundSet itself: here a clone, the same bytes
  if (!k || !nbits) return empty_result(ctx, out);                 // the loop does not run: re stays empty
  Scratch w(ctx->pool);
  BsiKeys ks;
  int rc = bsi_keys(ctx, w, bsi, nbits, found, 0, 65536, ks);
  if (rc) return rc;
  const uint32_t nk = ks.nk; // >= 1: found is not empty
  const SetView bv = bsi->view(), fv = found->view();
  uint8_t *img = nullptr;
  uint64_t *counts = nullptr;
  KeyedSlots fin;
  if (!w.get(img, (uint64_t)nk * kBitmapBytes) || !w.get(counts, 64))
    return fail(RB_ENOMEM, "bsi topK candidates of %u keys", nk);
  // ---- phase A: one launch per slice, no host wait in between; one read-back of the counts
  hipError_t e = hipMemsetAsync(counts, 0, 64 * 8, st);
  if (e == hipSuccess) e = hipEventRecord(ctx->ev[1], st);
  if (e == hipSuccess)
    for (int x = (int)nbits - 1; x >= 0; --x)
      k_bsi_topk_count<<<nblk(nk, 4), 256, 0, st>>>(bv, fv, bsi->bsi_table, nbits, x, k, fcard, ks.d_klist, nk, img, counts);
  if (e == hipSuccess) e = hipEventRecord(ctx->ev[2], st);
  uint64_t hc[64];
  if (e == hipSuccess) e = hipMemcpyAsync(hc, counts, 64 * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return fail(RB_EDEVICE, "bsi topK descent failed: %s", hipGetErrorString(e));
  // the decisions, as the kernels replayed them (Roaring64BitmapSliceIndex.java:582-592)
  uint64_t pred = 0, kk = k, cand = fcard;
  int stop = (int)nbits;
  for (int x = (int)nbits - 1; x >= 0 && cand && kk; --x) {
    stop = x;
    if (hc[x] > kk) {
      pred |= 1ull << x;
      cand = hc[x];
    } else {
      cand -= hc[x];
      kk -= hc[x];
    }
  }
  // ---- phase B: every key on its own again
  SetPtr res;
  if ((rc = make_set(ctx, 1, nk, (uint64_t)nk * kBitmapBytes, res)) || (rc = fin.alloc(w, nk, false))) return rc;
  if (hipEventRecord(ctx->ev[3], st) != hipSuccess) return fail(RB_EDEVICE, "event record failed");
  k_bsi_topk_emit<<<nblk(nk, 4), 256, 0, st>>>(bv, fv, bsi->bsi_table, nbits, pred, stop, ks.d_klist, nk, res->payload,
                                               fin.wo, ctx->d_stats);
  if (hipEventRecord(ctx->ev[4], st) != hipSuccess) return fail(RB_EDEVICE, "event record failed");
  rc = compact_keyed(ctx, ks.d_klist, nk, fin.wo, res.get());
  const KernelSpan spans[2] = {{"k_bsi_topk_count", -1, -1, (uint64_t)nk * nbits},
                               {"k_bsi_topk_emit", 0, 1, nk, ctx->ev[3], ctx->ev[4]}};
  if (!rc) rc = stats_end(ctx, nk, 0, spans, 2);
  if (rc) return rc;
  keyed_result_count(ctx, res.get());
  *out = res.release();
  return RB_OK;
}

// ---------------------------------------------------------------- value read-back: toPairList and getValue
// BitSliceIndexBase.toPairList(foundSet) (bsi/.../buffer/BitSliceIndexBase.java:534-549) and
// Roaring64BitmapSliceIndex.getValue / valueExist (longlong/Roaring64BitmapSliceIndex.java:127-136, 177-184, 284-286).
// The export is a 64 x 65536 bit-matrix transpose per high key restricted to the rows of F AND ebM; the lookup
// probes the 64 slices of one column with the 64 lanes of a wave.

// membership bits of the rows [base, base + 32) of an Array or Run container (base a multiple of 32): the values
// and runs clipped to the word
__device__ __forceinline__ uint32_t container_word(int type, const uint8_t *p, uint32_t card, uint32_t nruns,
                                                   uint32_t base) {
  uint32_t w = 0;
  if (type == kArray) {
    const uint16_t *a = reinterpret_cast<const uint16_t *>(p);
    for (uint32_t i = lower_bound_u16(a, card, base); i < card; ++i) {
      const uint32_t v = a[i];
      if (v >= base + 32) break;
      w |= 1u << (v - base);
    }
  } else {
    const uint32_t *r = reinterpret_cast<const uint32_t *>(p);
    for (uint32_t i = first_run_ending_from(r, nruns, base); i < nruns; ++i) {
      const uint32_t q = r[i], s = q & 0xFFFF, e = s + (q >> 16);
      if (s >= base + 32) break;
      const uint32_t lo = max(s, base) - base, hi = min(e, base + 31) - base;
      w |= (~0u >> (31 - hi)) & (~0u << lo);
    }
  }
  return w;
}

// Phase A of the export: cnt[q] = |F AND ebM| at key klist[q].  F = ebM: the container's card from the metadata,
// one thread per key, no payload read.  Else one wave per key stages ebM's container into registers, F's into LDS
// and counts the AND; a key of F that ebM lacks counts 0.
__global__ __launch_bounds__(256, 2) void k_bsi_values_count(SetView bsi, SetView fnd, int has_found,
                                                             const int32_t *__restrict__ table, uint32_t nbits,
                                                             const uint32_t *__restrict__ klist, uint32_t nk,
                                                             uint64_t *__restrict__ cnt) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[4][2048];
  if (!has_found) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q < nk) cnt[q] = bsi.card[table[(uint64_t)nbits * 65536 + klist[q]]]; // klist holds ebM's own keys
    return;
  }
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t q = blockIdx.x * 4 + wv;
  if (q >= nk) return;
  const uint32_t key = klist[q];
  const int32_t ec = table[(uint64_t)nbits * 65536 + key];
  uint32_t c = 0;
  if (ec >= 0) { // wave-uniform
    uint32_t *sS = lds[wv];
    uint64_t e[kW];
    stage_global(bsi, ec, sS, lane);
    lds_read_words(sS, e, lane);
    wave_lds_sync();
    stage_global(fnd, table[(uint64_t)(nbits + 1) * 65536 + key], sS, lane); // present: the keys come from F
    uint32_t p = 0;
#pragma unroll
    for (int j = 0; j < kW; ++j) p += (uint32_t)__popcll(e[j] & lds_word(sS, j, lane));
    c = wave_sum_u32(p);
  }
  if (lane == 0) cnt[q] = c;
}

// 32 x 32 bit transpose in registers: a[i] bit r  ->  a[r] bit i (five rounds of masked block swaps)
template <int J>
__device__ __forceinline__ void transpose32_round(uint32_t (&a)[32], uint32_t m) {
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    if (k & J) continue;
    const uint32_t t = ((a[k] >> J) ^ a[k + J]) & m;
    a[k + J] ^= t;
    a[k] ^= t << J;
  }
}
__device__ __forceinline__ void transpose32(uint32_t (&a)[32]) {
  transpose32_round<16>(a, 0x0000FFFFu);
  transpose32_round<8>(a, 0x00FF00FFu);
  transpose32_round<4>(a, 0x0F0F0F0Fu);
  transpose32_round<2>(a, 0x33333333u);
  transpose32_round<1>(a, 0x55555555u);
}

// The 32-row words of the slices S0 .. S0 + 31 for a tile (2048 rows: lane l <-> u32 word 64 * tile + l of the
// container): a[i] = slice S0 + i's word.  A Bitmap slice's word is one coalesced 256-B read of its payload; the
// words of the Array and Run slices are first built in the wave's tile buffer tbw[32][64] (container_word, only by
// lanes that hold a row of F'); a slice without a container at the key is zero and its payload is not touched
// (`dummy`: 64 readable words such a slice's lane reads instead).
template <int S0>
__device__ __forceinline__ void tile_words(uint32_t (&a)[32], const SliceDesc &d, const SetView &bsi, uint64_t pres,
                                           uint64_t bm, uint32_t tile, uint32_t f, uint32_t *tbw,
                                           const uint32_t *dummy, int lane) {
  const uint32_t ph = (uint32_t)(pres >> S0), bh = (uint32_t)(bm >> S0);
  uint32_t todo = ph & ~bh; // wave-uniform
  while (todo) {
    const int i = __builtin_ctz(todo);
    todo &= todo - 1;
    const Meta sm = d.meta(S0 + i);
    tbw[i * 64 + lane] =
        f ? container_word(sm.type, d.ptr(bsi, S0 + i), (uint32_t)sm.card, (uint32_t)sm.runs, (tile * 64 + lane) * 32) : 0u;
  }
  wave_lds_sync();
  // 32 loads back to back with no branch between them (a branch per slice made the compiler wait for each load
  // before it issued the next): a slice that is no Bitmap here reads the dummy word instead, which stays cached
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const uint32_t *p = (bh >> i) & 1u ? reinterpret_cast<const uint32_t *>(d.ptr(bsi, S0 + i)) + tile * 64 : dummy;
    a[i] = p[lane];
  }
  if (ph & ~bh) { // wave-uniform: some slice's word is in the tile buffer
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const uint32_t t = tbw[i * 64 + lane];
      a[i] = (bh >> i) & 1u ? a[i] : (ph >> i) & 1u ? t : 0u;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 32; ++i) a[i] = (bh >> i) & 1u ? a[i] : 0u;
  }
  wave_lds_sync();
}

// The gather's per-wave LDS: the tile buffer of tile_words (32 x 64 words), then the store stage: kValStage
// (value, column) slots, one pad slot per 32 (slot p at p + p / 32: the 64 lanes of a wave write ranks 32 apart, which
// would otherwise share one bank).
constexpr int kValStage = 1024, kValStagePad = kValStage + kValStage / 32, kValStageWords = 3 * kValStagePad;
static_assert(kValStageWords >= 32 * 64, "the stage also holds tile_words' buffer");
__device__ __forceinline__ uint32_t val_slot(uint32_t p) { return p + (p >> 5); }

// Phase B of the export, the gather: one block per key of F.  Prologue: ebM's container and F's are staged into
// two LDS images, F' = F AND ebM replaces the first and the 32 tiles' row counts go to LDS.  Then the four waves
// take the tiles round-robin; a tile without a row of F' is skipped before any slice is touched.  A lane transposes
// its own 32 x 32 bit blocks in registers (slices 0-31: the low dwords of its 32 rows, slices 32-63: the high
// dwords, skipped when nbits <= 32); the rows of F' then go, compacted, to offs[q] + the rows of F' before them,
// through an LDS stage so that a wave's stores are contiguous.
// Nothing is written when the call's total offs[nk] exceeds cap.  No block waits for another: offs comes from the
// launches before this one.
__global__ __launch_bounds__(256, 2) void k_bsi_values(SetView bsi, SetView fnd, int has_found,
                                                       const int32_t *__restrict__ table, uint32_t nbits,
                                                       const uint32_t *__restrict__ klist, uint32_t nk,
                                                       const uint64_t *__restrict__ offs, uint64_t cap,
                                                       uint32_t *__restrict__ cols, uint64_t *__restrict__ vals,
                                                       uint64_t *stats) {
  __shared__ __attribute__((aligned(16))) uint32_t img[2][2048];
  __shared__ __attribute__((aligned(16))) uint32_t wbuf[4][kValStageWords]; // per wave: tile words, then the stage
  __shared__ uint32_t tcnt[32];
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t q = blockIdx.x;
  if (offs[nk] > cap) return;
  const uint32_t key = klist[q];
  const uint64_t base = offs[q], lim = offs[q + 1];
  const int32_t ec = table[(uint64_t)nbits * 65536 + key];
  const int32_t fc = has_found ? table[(uint64_t)(nbits + 1) * 65536 + key] : -1;
  SliceDesc d;
  d.load(bsi, table, nbits, key, lane);
  if (wv == 0) { // the call's counters: what the two phases read at this key, what this block writes
    uint64_t inb = d.sc >= 0 && lim > base ? payload_bytes(d.st, d.scard, d.sruns) + 16 : 0;
    inb = wave_sum_u64(inb);
    if (ec >= 0) inb += payload_bytes(bsi.type[ec], bsi.card[ec], bsi.nruns[ec]) + 16;
    if (fc >= 0) inb += payload_bytes(fnd.type[fc], fnd.card[fc], fnd.nruns[fc]) + 16;
    if (lane == 0) {
      const uint32_t stripe = q & (kStripes - 1);
      atomicAdd((unsigned long long *)&stats[0 * kStripes + stripe], (unsigned long long)inb);
      if (lim > base) {
        atomicAdd((unsigned long long *)&stats[1 * kStripes + stripe], (unsigned long long)(12 * (lim - base)));
        atomicAdd((unsigned long long *)&stats[7 * kStripes + stripe], (unsigned long long)(lim - base));
      }
    }
  }
  if (lim == base) return; // no row of F in ebM at this key (ebM may lack the key altogether)
  if (wv == 0) stage_global(bsi, ec, img[0], lane);
  else if (wv == 1 && has_found) stage_global(fnd, fc, img[1], lane);
  __syncthreads();
#pragma unroll
  for (int m = 0; m < 8; ++m) { // wave wv, round m: tile 4 m + wv, lane <-> word
    const int j = 256 * m + (int)threadIdx.x;
    const uint32_t f = img[0][j] & (has_found ? img[1][j] : ~0u);
    img[0][j] = f;
    const uint32_t c = wave_sum_u32((uint32_t)__popc(f));
    if (lane == 0) tcnt[4 * m + wv] = c;
  }
  __syncthreads();
  // exclusive prefix of the tiles' row counts, lane t <-> tile t (every wave computes its own copy)
  const uint32_t tc = lane < 32 ? tcnt[lane] : 0u;
  const uint32_t tbase = wave_scan_u32(tc, lane) - tc;
  const uint64_t pres = __ballot(d.sc >= 0), bm = __ballot(d.sc >= 0 && d.st == kBitmap);
  uint32_t *tbw = wbuf[wv];
  const uint32_t *dummy = reinterpret_cast<const uint32_t *>(table); // 64 readable words for tile_words
  for (uint32_t tile = (uint32_t)wv; tile < 32; tile += 4) {
    if (!readlane(tc, (int)tile)) continue;
    const uint32_t f = img[0][tile * 64 + lane];
    const uint32_t n = (uint32_t)__popc(f);
    uint32_t lo[32], hi[32];
    tile_words<0>(lo, d, bsi, pres, bm, tile, f, tbw, dummy, lane);
    transpose32(lo);
    if (nbits > 32) {
      tile_words<32>(hi, d, bsi, pres, bm, tile, f, tbw, dummy, lane);
      transpose32(hi);
    } else {
#pragma unroll
      for (int r = 0; r < 32; ++r) hi[r] = 0;
    }
    // ---- the tile's rows leave through the wave's LDS stage, kValStage ranks at a time: a lane's rows are
    // consecutive ranks, so direct stores would put the 64 lanes of one instruction on 64 different lines
    const uint32_t col0 = (key << 16) | ((tile * 64 + lane) * 32);
    const uint32_t ntile = readlane(tc, (int)tile), rank0 = wave_scan_u32(n, lane) - n;
    const uint64_t tpos = base + readlane(tbase, (int)tile);
    uint64_t *sv = reinterpret_cast<uint64_t *>(tbw);
    uint32_t *sc = tbw + 2 * kValStagePad;
    for (uint32_t w0 = 0; w0 < ntile; w0 += kValStage) {
      uint32_t p = rank0 - w0; // this window's slots are the ranks w0 .. w0 + kValStage - 1 (unsigned compare)
#pragma unroll
      for (int r = 0; r < 32; ++r) {
        if ((f >> r) & 1u) {
          if (p < (uint32_t)kValStage) {
            sv[val_slot(p)] = pack2(lo[r], hi[r]);
            sc[val_slot(p)] = col0 + r;
          }
          ++p;
        }
      }
      wave_lds_sync();
      const uint32_t nw = min(ntile - w0, (uint32_t)kValStage);
      for (uint32_t i = (uint32_t)lane; i < nw; i += 64) {
        const uint64_t g = tpos + w0 + i;
        if (g < lim) { // holds when the metadata's card matches the payload
          vals[g] = sv[val_slot(i)];
          cols[g] = sc[val_slot(i)];
        }
      }
      wave_lds_sync();
    }
  }
}

// getValue / valueExist of a batch of columns: one wave per query, grid-stride, four queries per block.  ebM's
// container is probed first (wave-uniform); then lane i probes slice i and one ballot is the 64-bit value.
__global__ __launch_bounds__(256, 2) void k_bsi_get(SetView bsi, const int32_t *__restrict__ table, uint32_t nbits,
                                                    const uint32_t *__restrict__ columns, uint64_t n,
                                                    uint64_t *__restrict__ values, uint8_t *__restrict__ exists) {
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint64_t q = (uint64_t)blockIdx.x * 4 + wv; q < n; q += (uint64_t)gridDim.x * 4) {
    const uint32_t col = columns[q], key = col >> 16, x = col & 0xFFFF;
    const int32_t ec = table[(uint64_t)nbits * 65536 + key];
    const bool e = ec >= 0 && container_has(bsi.type[ec], bsi.payload + bsi.off[ec], bsi.card[ec], bsi.nruns[ec], x);
    bool hit = false;
    if (e && lane < (int)nbits) {
      const int32_t sc = table[(uint64_t)lane * 65536 + key];
      if (sc >= 0) hit = container_has(bsi.type[sc], bsi.payload + bsi.off[sc], bsi.card[sc], bsi.nruns[sc], x);
    }
    const uint64_t v = __ballot(hit);
    if (lane == 0) {
      if (values) values[q] = v;
      if (exists) exists[q] = e ? 1 : 0;
    }
  }
}

// the export's host side; host_dst: cols / vals are host memory (gathered into pool buffers and copied out)
int bsi_values(rbgpu_ctx *ctx, const rbgpu_set *bsi, const rbgpu_set *found, uint32_t key_lo, uint32_t key_hi,
               uint32_t *cols, uint64_t *vals, uint64_t cap, uint64_t *count, bool host_dst) {
  const uint32_t nbits = bsi->nb - 1;
  hipStream_t st = ctx->stream;
  const bool count_only = !cols && !vals;
  *count = 0;
  stats_begin(ctx);
  Scratch w(ctx->pool);
  BsiKeys ks;
  int rc = bsi_keys(ctx, w, bsi, nbits, found, key_lo, key_hi, ks);
  if (rc) return rc;
  const uint32_t nk = ks.nk;
  uint64_t *cnt = nullptr, *offs = nullptr, *tmp = nullptr;
  uint32_t *d_cols = host_dst ? nullptr : cols;
  uint64_t *d_vals = host_dst ? nullptr : vals;
  if (!w.get(cnt, nk + 1ull) || !w.get(offs, nk + 2ull) || !w.get(tmp, scan_tmp_words(nk) + 1))
    return fail(RB_ENOMEM, "bsi values: counts of %u keys", nk);
  const SetView bv = bsi->view(), fv = found ? found->view() : bv;
  const int hf = found != nullptr;
  auto gather = [&]() { // phase B, between its own events
    hipError_t e = hipEventRecord(ctx->ev[3], st);
    if (e == hipSuccess) {
      k_bsi_values<<<nk, 256, 0, st>>>(bv, fv, hf, bsi->bsi_table, nbits, ks.d_klist, nk, offs, cap, d_cols, d_vals,
                                       ctx->d_stats);
      e = hipEventRecord(ctx->ev[4], st);
    }
    return e;
  };
  // ---- phase A: the keys' row counts and their exclusive scan (offs[nk] = the call's count)
  hipError_t e = hipEventRecord(ctx->ev[1], st);
  if (e == hipSuccess && nk) {
    k_bsi_values_count<<<hf ? nblk(nk, 4) : nblk(nk, 256), 256, 0, st>>>(bv, fv, hf, bsi->bsi_table, nbits, ks.d_klist,
                                                                        nk, cnt);
    scan_exclusive(cnt, offs, nk, tmp, st);
  }
  if (e == hipSuccess) e = hipEventRecord(ctx->ev[2], st);
  // device outputs: phase B follows in stream order with no host wait (it writes nothing when the count exceeds cap)
  bool gathered = false;
  if (e == hipSuccess && nk && !count_only && !host_dst) {
    e = gather();
    gathered = true;
  }
  // the call's one read-back before any host copy
  uint64_t total = 0;
  if (e == hipSuccess && nk) {
    e = hipMemcpyAsync(ctx->h_pinned, offs + nk, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipGetLastError();
    total = ctx->h_pinned[0];
  }
  if (e != hipSuccess) return fail(RB_EDEVICE, "bsi values failed: %s", hipGetErrorString(e));
  *count = total;
  if (!count_only && total > cap)
    return fail(RB_EINVAL, "bsi values: %llu pairs exceed the capacity %llu", (unsigned long long)total,
                (unsigned long long)cap);
  if (!count_only && host_dst && total) { // host outputs: the buffers take the count the read-back gave
    if (!w.get(d_cols, total) || !w.get(d_vals, total))
      return fail(RB_ENOMEM, "bsi values: %llu pairs", (unsigned long long)total);
    e = gather();
    gathered = true;
    if (e == hipSuccess) e = hipMemcpyAsync(cols, d_cols, total * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(vals, d_vals, total * 8, hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return fail(RB_EDEVICE, "bsi values failed: %s", hipGetErrorString(e));
  }
  const KernelSpan spans[2] = {{"k_bsi_values", 0, 1, nk, ctx->ev[3], ctx->ev[4]},
                               {"k_bsi_values_count", -1, -1, nk, ctx->ev[1], ctx->ev[2]}};
  rc = gathered ? stats_end(ctx, nk, 0, spans, 2) : stats_end(ctx, nk, 0, spans + 1, 1);
  if (!rc && gathered) { // the gather is the call's main kernel, whichever phase took longer
    rb_stats &s = ctx->last;
    s.main_kernel_ms = s.kernel_ms[0];
    s.main_kernel_bytes = s.kernel_bytes[0];
    std::snprintf(s.main_kernel, sizeof s.main_kernel, "%s", s.kernel_name[0]);
  }
  return rc;
}

int bsi_get_values(rbgpu_ctx *ctx, const rbgpu_set *bsi, const uint32_t *columns, uint64_t n, uint64_t *values,
                   uint8_t *exists) {
  const uint32_t nbits = bsi->nb - 1;
  hipStream_t st = ctx->stream;
  stats_begin(ctx);
  int rc = ensure_bsi_tables(ctx, bsi, nbits);
  if (rc) return rc;
  Scratch w(ctx->pool);
  uint32_t *d_c = nullptr;
  uint64_t *d_v = nullptr;
  uint8_t *d_e = nullptr;
  if (n && (!w.get(d_c, n) || (values && !w.get(d_v, n)) || (exists && !w.get(d_e, n))))
    return fail(RB_ENOMEM, "bsi lookups of %llu columns", (unsigned long long)n);
  hipError_t e = n ? hipMemcpyAsync(d_c, columns, n * 4, hipMemcpyHostToDevice, st) : hipSuccess;
  if (e == hipSuccess) e = hipEventRecord(ctx->ev[1], st);
  if (e == hipSuccess && n)
    k_bsi_get<<<(unsigned)std::min<uint64_t>((n + 3) / 4, 4096), 256, 0, st>>>(bsi->view(), bsi->bsi_table, nbits, d_c,
                                                                              n, d_v, d_e);
  if (e == hipSuccess) e = hipEventRecord(ctx->ev[2], st);
  if (e == hipSuccess && n && values) e = hipMemcpyAsync(values, d_v, n * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && n && exists) e = hipMemcpyAsync(exists, d_e, n, hipMemcpyDeviceToHost, st);
  if (e != hipSuccess) return fail(RB_EDEVICE, "bsi lookups failed: %s", hipGetErrorString(e));
  const KernelSpan spans[1] = {{"k_bsi_get", -1, -1, n}};
  return stats_end(ctx, n, 0, spans, n ? 1 : 0);
}

// this file's code object, loaded at context creation (rbgpu_open, context.hip)
__global__ void k_warm_bsi() {}
void warm_bsi(hipStream_t st) { k_warm_bsi<<<1, 64, 0, st>>>(); }

} // namespace rbg
