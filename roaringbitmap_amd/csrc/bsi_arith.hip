// bsi_arith.hip — bit-sliced index arithmetic on the device: Roaring64BitmapSliceIndex.add (longlong/
// Roaring64BitmapSliceIndex.java:64-93; RoaringBitmapSliceIndex.java:66-95; buffer/MutableBitSliceIndex.java:121-215),
// merge (:357-383) and minValue / maxValue (:95-125).
//
// add.  The reference adds one digit of the other index at a time: carry = and(bA[i], digit), bA[i].xor(digit), and
// the carry ripples upwards as the next digit while it is not empty (addDigit) — up to O(slices^2) whole-bitmap
// operations, every intermediate carry a bitmap of its own.  Every 2^16-column high key is independent, so here ONE
// WAVE PER KEY walks the slices once, k_bsi_chain's shape: the carry lives in the wave's registers as a 65536-bit
// bitmap, a_j and b_j are staged through two 8 KiB LDS images, sum = a ^ b ^ c, c = maj(a, b, c).  With c_j the carry
// into slice j at the key (c_0 = 0), the container the reference leaves at (slice j, key) is
//   b_j absent, c_j = 0      a_j's container as it is (a Run included); absent if absent   — nothing touched it
//   a_j absent, c_j = 0      b_j's container as it is (the xor inserts a clone)
//   anything else            the bits a_j ^ b_j ^ c_j, an Array up to 4096 members, a Bitmap above, dropped when empty
// (for one column at most one of the per-digit ripples carries into position j, so the containers xored into slice
// j at the key are non-empty exactly where c_j is; every and / ixor among Array and Bitmap containers returns the
// canonical type).  The first two rows stage nothing: the candidate is a copy of the payload and the carry stays zero
// — on the inputs that matter most (slice, key) pairs are such copies.  The rule fails where a Run is touched:
// RunContainer.xor looks at its operand's type and at |x| < 32, Run ^ Run goes through toEfficientContainer, and each
// intermediate's type feeds the next step, so the result depends on the ripple history, which one pass does not have.
// The planning pass therefore asks whether some key holds slice containers of both indexes and a Run among them; if
// so the whole call takes the CHAIN, the reference's algorithm over rbgpu_pairwise(RB_AND) / rbgpu_pairwise_inplace(
// RB_XOR) — slow, and exact for every container class by construction (RB_BSI_ADD_CHAIN forces it).
// 64-bit quirk: Roaring64Bitmap.xor keeps a container that ends empty (Roaring64Bitmap.java:392-411) where
// RoaringBitmap.xor drops it (RoaringBitmap.java:3296-3348); a device set cannot hold an empty container (card is
// 1..65536), so both paths give RoaringBitmapSliceIndex.add's result: such a container is absent, and the slice
// bitmap stays in the count even when it has no container left.
//
// The fused pipeline, on one stream: key tables of both sets (bsi.hip ensure_bsi_tables, cached with the sets), the
// keys at which either index holds a slice container and the plainness decision (k_bsi_add_keys / k_bsi_add_list),
// ebM by rbgpu_pairwise_inplace(RB_OR), k_bsi_add<measure> (type and size of one candidate per (slice 0..n, key); the
// candidates of slice n are the carry out of the top slice), a scan that lays out a tight arena and drops the empty
// candidates (as build.hip), k_bsi_add<emit> (the same walk, metadata and payload), ebM's containers appended.
//
// merge needs no kernel of its own: static or per slice, runOptimize, in-place or of the ebMs, all existing calls; the
// pieces are put together by the tight concatenation below (k_cat_*), which also clones.
// minValue / maxValue: one wave per high key of ebM descends the slices once for both (k_bsi_minmax).
#include <algorithm>
#include <vector>

#include "internal.hpp"
#include "kernels.hpp"
#include "wave.hpp"

namespace rbg {

// ---------------------------------------------------------------- plan
// act[k] = some slice of a or of b holds a container at high key k; bt[block] = the block's count of such keys;
// *notplain is set when a key holds slice containers of both indexes and a Run among them
__global__ __launch_bounds__(256) void k_bsi_add_keys(SetView A, SetView B, const int32_t *__restrict__ ta,
                                                      const int32_t *__restrict__ tb, uint32_t na, uint32_t nb,
                                                      uint8_t *__restrict__ act, uint64_t *__restrict__ bt,
                                                      uint32_t *notplain) {
  __shared__ uint32_t wt[4];
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  bool ha = false, hb = false, run = false;
  for (uint32_t r = 0; r < na; ++r) {
    const int32_t c = ta[(uint64_t)r * 65536 + k];
    if (c >= 0) {
      ha = true;
      run |= A.type[c] == kRun;
    }
  }
  for (uint32_t r = 0; r < nb; ++r) {
    const int32_t c = tb[(uint64_t)r * 65536 + k];
    if (c >= 0) {
      hb = true;
      run |= B.type[c] == kRun;
    }
  }
  act[k] = ha || hb;
  if (__ballot(ha && hb && run) && lane_id() == 0) atomicOr(notplain, 1u);
  const uint32_t n = block_flag_count(ha || hb, wt);
  if (threadIdx.x == 0) bt[blockIdx.x] = n;
}
__global__ __launch_bounds__(256) void k_bsi_add_list(const uint8_t *__restrict__ act, const uint64_t *__restrict__ bts,
                                                      uint32_t *__restrict__ klist) {
  __shared__ uint32_t wt[4];
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  const bool f = act[k] != 0;
  const uint32_t r = block_flag_rank(f, wt);
  if (f) klist[bts[blockIdx.x] + r] = k;
}

// ---------------------------------------------------------------- add: measure and emit
struct AddArgs {
  SetView A, B;
  const int32_t *ta, *tb; // key -> container tables of the two sets (row = bitmap)
  uint32_t na, nb, n;     // slices of a, of b, max of the two; candidates exist for slices 0..n
  const uint32_t *klist;  // [nk] the keys walked
  uint32_t nk;
  // per candidate t = slice * nk + q, written by the measuring pass: the type (kEmpty: dropped), 1 / 0, and the
  // payload bytes rounded up to 16
  uint8_t *ttype;
  uint64_t *tkeep, *tbytes;
  // their exclusive scans, read by the emitting pass: the candidate's container index and payload offset
  const uint64_t *tpos, *toff;
  OutView out;
  uint8_t *payload;
  uint64_t *stats;
};

template <int EMIT>
__global__ __launch_bounds__(256, 2) void k_bsi_add(AddArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[4][2][2048];
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t q = xcd_swizzle(blockIdx.x, gridDim.x) * 4 + wv;
  if (q >= a.nk) return;
  uint32_t *sA = lds[wv][0], *sB = lds[wv][1];
  const uint32_t key = a.klist[q];
  // slice descriptors, lane i <-> slice i (at most 64 slices a side)
  const int32_t ca = lane < (int)a.na ? a.ta[(uint64_t)lane * 65536 + key] : -1;
  const int32_t cb = lane < (int)a.nb ? a.tb[(uint64_t)lane * 65536 + key] : -1;
  uint64_t c[kW]; // the carry into the current slice
#pragma unroll
  for (int i = 0; i < kW; ++i) c[i] = 0;
  bool cz = true; // the carry is zero (wave-uniform)
  uint64_t inb = 0, outb = 0, members = 0;
  for (uint32_t j = 0; j <= a.n; ++j) {
    const uint64_t t = (uint64_t)j * a.nk + q;
    const int32_t ia = j < a.na ? (int32_t)readlane((uint32_t)ca, (int)j) : -1;
    const int32_t ib = j < a.nb ? (int32_t)readlane((uint32_t)cb, (int)j) : -1;
    if (cz && (ia < 0 || ib < 0)) {
      // nothing touches this slice at the key: absent, or a copy of the one container there; the carry stays zero
      const bool from_a = ib < 0;
      const int32_t src = from_a ? ia : ib;
      if (src < 0) {
        if (!EMIT && lane == 0) {
          a.ttype[t] = kEmpty;
          a.tkeep[t] = 0;
          a.tbytes[t] = 0;
        }
        continue;
      }
      const int ty = from_a ? a.A.type[src] : a.B.type[src];
      const uint32_t card = from_a ? a.A.card[src] : a.B.card[src], nr = from_a ? a.A.nruns[src] : a.B.nruns[src];
      const uint64_t bytes = payload_bytes(ty, card, nr);
      inb += bytes + 16;
      if (!EMIT) {
        if (lane == 0) {
          a.ttype[t] = (uint8_t)ty;
          a.tkeep[t] = 1;
          a.tbytes[t] = round16(bytes);
        }
        continue;
      }
      const uint64_t at = a.tpos[t], off = a.toff[t];
      if (lane == 0) {
        a.out.key[at] = (uint16_t)key;
        a.out.type[at] = (uint8_t)ty;
        a.out.card[at] = card;
        a.out.nruns[at] = (uint16_t)nr;
        a.out.off[at] = off;
      }
      copy_payload(from_a ? a.A.payload + a.A.off[src] : a.B.payload + a.B.off[src], a.payload + off, bytes, lane);
      outb += bytes + 16;
      members += card;
      continue;
    }
    // sum = a_j ^ b_j ^ c, c = maj(a_j, b_j, c)
    uint64_t s[kW];
    if (ia >= 0) {
      const int ty = a.A.type[ia];
      const uint32_t card = a.A.card[ia], nr = a.A.nruns[ia];
      stage_container(ty, a.A.payload + a.A.off[ia], card, nr, sA, lane);
      lds_read_words(sA, s, lane);
      inb += payload_bytes(ty, card, nr) + 16;
    } else {
#pragma unroll
      for (int i = 0; i < kW; ++i) s[i] = 0;
    }
    uint32_t cnz = 0;
    if (ib >= 0) {
      const int ty = a.B.type[ib];
      const uint32_t card = a.B.card[ib], nr = a.B.nruns[ib];
      stage_container(ty, a.B.payload + a.B.off[ib], card, nr, sB, lane);
      inb += payload_bytes(ty, card, nr) + 16;
      const uint4 *b4 = reinterpret_cast<const uint4 *>(sB);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint4 v = b4[k * 64 + lane];
        const uint64_t y[2] = {pack2(v.x, v.y), pack2(v.z, v.w)};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint64_t x = s[2 * k + h], cc = c[2 * k + h], xy = x ^ y[h];
          s[2 * k + h] = xy ^ cc;
          c[2 * k + h] = (x & y[h]) | (cc & xy);
          cnz |= (uint32_t)(c[2 * k + h] != 0);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < kW; ++i) {
        const uint64_t x = s[i], cc = c[i];
        s[i] = x ^ cc;
        c[i] = x & cc;
        cnz |= (uint32_t)(c[i] != 0);
      }
    }
    wave_lds_sync(); // both images are free again
    cz = __ballot(cnz != 0) == 0ull;
    int card, runs;
    metrics(s, lane, false, card, runs);
    const int ty = card == 0 ? (int)kEmpty : type_ab(card);
    if (!EMIT) {
      if (lane == 0) {
        a.ttype[t] = (uint8_t)ty;
        a.tkeep[t] = card != 0;
        a.tbytes[t] = card ? round16(payload_bytes(ty, (uint32_t)card, 0)) : 0ull;
      }
      continue;
    }
    if (!card) continue;
    // the measuring pass kept this candidate, and the same walk gives the same type and size
    const uint64_t at = a.tpos[t], off = a.toff[t];
    if (lane == 0) {
      a.out.key[at] = (uint16_t)key;
      a.out.type[at] = (uint8_t)ty;
      a.out.card[at] = (uint32_t)card;
      a.out.nruns[at] = 0;
      a.out.off[at] = off;
    }
    outb += emit_container(ty, s, card, 0, a.payload + off, sA, lane) + 16;
    members += (uint64_t)card;
    wave_lds_sync();
  }
  if (lane == 0 && inb) {
    const uint32_t stripe = q & (kStripes - 1);
    if (!EMIT) { // word 2: what the measuring pass read (copies: their metadata only, counted as in the emit)
      atomicAdd((unsigned long long *)&a.stats[2 * kStripes + stripe], (unsigned long long)inb);
    } else {
      atomicAdd((unsigned long long *)&a.stats[0 * kStripes + stripe], (unsigned long long)inb);
      atomicAdd((unsigned long long *)&a.stats[1 * kStripes + stripe], (unsigned long long)outb);
      atomicAdd((unsigned long long *)&a.stats[7 * kStripes + stripe], (unsigned long long)members);
    }
  }
}
// slice bitmap b of the result holds the kept candidates of [b * nk, (b + 1) * nk)
__global__ void k_bsi_add_begin(const uint64_t *__restrict__ tpos, uint32_t nk, uint32_t nres,
                                uint64_t *__restrict__ begin) {
  const uint32_t b = threadIdx.x;
  if (b <= nres) begin[b] = tpos[(uint64_t)b * nk];
}

// ---------------------------------------------------------------- minValue / maxValue
// mm[0] / mm[1] (all ones / 0 on entry) = min / max over the keys of the per-key smallest / largest value: the
// candidate masks start as ebM's container; per slice from the top, min keeps m & ~s and max keeps m & s whenever
// that leaves a column (the reference's descent, both at once: the slice is staged once)
__global__ __launch_bounds__(256, 2) void k_bsi_minmax(SetView bsi, const int32_t *__restrict__ table, uint32_t nbits,
                                                       const uint32_t *__restrict__ klist, uint32_t nk, uint64_t *mm,
                                                       uint64_t *stats) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[4][2048];
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t q = xcd_swizzle(blockIdx.x, gridDim.x) * 4 + wv;
  if (q >= nk) return;
  uint32_t *s = lds[wv];
  const uint32_t key = klist[q];
  const int32_t ec = table[(uint64_t)nbits * 65536 + key];
  if (ec < 0) return; // the list holds ebM's keys
  uint64_t inb = 0;
  uint64_t lo[kW], hi[kW];
  {
    const int ty = bsi.type[ec];
    const uint32_t card = bsi.card[ec], nr = bsi.nruns[ec];
    stage_container(ty, bsi.payload + bsi.off[ec], card, nr, s, lane);
    lds_read_words(s, lo, lane);
    inb += payload_bytes(ty, card, nr) + 16;
  }
#pragma unroll
  for (int i = 0; i < kW; ++i) hi[i] = lo[i];
  wave_lds_sync();
  const int32_t sc = lane < (int)nbits ? table[(uint64_t)lane * 65536 + key] : -1;
  uint64_t vmin = 0, vmax = 0;
  for (int j = (int)nbits - 1; j >= 0; --j) {
    const int32_t ci = (int32_t)readlane((uint32_t)sc, j);
    if (ci < 0) continue; // an absent slice: m & ~s = m and m & s is empty, so both masks stay and both bits are 0
    const int ty = bsi.type[ci];
    const uint32_t card = bsi.card[ci], nr = bsi.nruns[ci];
    stage_container(ty, bsi.payload + bsi.off[ci], card, nr, s, lane);
    inb += payload_bytes(ty, card, nr) + 16;
    const uint4 *s4 = reinterpret_cast<const uint4 *>(s);
    uint64_t anylo = 0, anyhi = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint4 v = s4[k * 64 + lane];
      const uint64_t y0 = pack2(v.x, v.y), y1 = pack2(v.z, v.w);
      anylo |= (lo[2 * k] & ~y0) | (lo[2 * k + 1] & ~y1);
      anyhi |= (hi[2 * k] & y0) | (hi[2 * k + 1] & y1);
    }
    const bool keep_lo = __ballot(anylo != 0) != 0ull, keep_hi = __ballot(anyhi != 0) != 0ull;
    if (keep_lo || keep_hi) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint4 v = s4[k * 64 + lane];
        const uint64_t y0 = pack2(v.x, v.y), y1 = pack2(v.z, v.w);
        if (keep_lo) {
          lo[2 * k] &= ~y0;
          lo[2 * k + 1] &= ~y1;
        }
        if (keep_hi) {
          hi[2 * k] &= y0;
          hi[2 * k + 1] &= y1;
        }
      }
    }
    if (!keep_lo) vmin |= 1ull << j; // every candidate of the minimum holds the bit
    if (keep_hi) vmax |= 1ull << j;
    wave_lds_sync();
  }
  if (lane == 0) {
    atomicMin((unsigned long long *)&mm[0], (unsigned long long)vmin);
    atomicMax((unsigned long long *)&mm[1], (unsigned long long)vmax);
    if (stats) atomicAdd((unsigned long long *)&stats[0 * kStripes + (q & (kStripes - 1))], (unsigned long long)inb);
  }
}

// ---------------------------------------------------------------- tight concatenation
// bytes[i] = the 16-B padded payload size of container c0 + i
__global__ __launch_bounds__(256) void k_cat_bytes(SetView s, uint64_t c0, uint64_t n, uint64_t *__restrict__ bytes) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    bytes[i] = round16(payload_bytes(s.type[c0 + i], s.card[c0 + i], s.nruns[c0 + i]));
}
// dbegin[i] = cont_base + the containers of the part before its bitmap i, i in [0, count]
__global__ __launch_bounds__(256) void k_cat_begin(const uint64_t *__restrict__ sbegin, uint32_t count, uint64_t c0,
                                                   uint64_t cont_base, uint64_t *__restrict__ dbegin) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i <= count) dbegin[i] = cont_base + (sbegin[i] - c0);
}
// containers [c0, c0 + n) of s to containers cont_base.. of the result, payloads at pay_base + doff[i]; a wave each
__global__ __launch_bounds__(256) void k_cat_copy(SetView s, uint64_t c0, uint64_t n, const uint64_t *__restrict__ doff,
                                                  uint64_t cont_base, uint64_t pay_base, OutView out, uint8_t *payload) {
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint64_t i = (uint64_t)blockIdx.x * 4 + wv; i < n; i += (uint64_t)gridDim.x * 4) {
    const uint64_t c = c0 + i, at = cont_base + i, off = pay_base + doff[i];
    const int ty = s.type[c];
    const uint32_t card = s.card[c], nr = s.nruns[c];
    if (lane == 0) {
      out.key[at] = s.key[c];
      out.type[at] = (uint8_t)ty;
      out.card[at] = card;
      out.nruns[at] = (uint16_t)nr;
      out.off[at] = off;
    }
    copy_payload(s.payload + s.off[c], payload + off, payload_bytes(ty, card, nr), lane);
  }
}

// ---------------------------------------------------------------- host side
namespace {
constexpr uint64_t kMaxBlocks = 2048; // 256 CUs x 8 blocks; the rest is grid-stride
unsigned nblk(uint64_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }
unsigned grid_for(uint64_t n, unsigned per) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>(nblk(n, per), 1), kMaxBlocks); }

// Bitmaps [first, first + count) of a set as one part of a concatenation: measure lays out its containers' payloads
// tightly (doff, total: read back by the caller's next wait), emit writes them into a result set.
struct CatPart {
  const rbgpu_set *s = nullptr;
  uint32_t first = 0, count = 0;
  uint64_t c0 = 0, nc = 0, total = 0;
  uint64_t *doff = nullptr;
};
int cat_measure(rbgpu_ctx *ctx, Scratch &tmp, CatPart &p) {
  int rc = ensure_h_begin(p.s);
  if (rc) return rc;
  p.c0 = p.s->h_begin[p.first];
  p.nc = p.s->h_begin[p.first + p.count] - p.c0;
  p.total = 0;
  if (!p.nc) return RB_OK;
  hipStream_t st = ctx->stream;
  uint64_t *bytes, *scan_tmp;
  if (!tmp.get(bytes, p.nc) || !tmp.get(p.doff, p.nc + 1) || !tmp.get(scan_tmp, scan_tmp_words(p.nc) + 1))
    return fail(RB_ENOMEM, "bsi arithmetic: layout of %llu containers", (unsigned long long)p.nc);
  k_cat_bytes<<<grid_for(p.nc, 256), 256, 0, st>>>(p.s->view(), p.c0, p.nc, bytes);
  scan_exclusive(bytes, p.doff, p.nc, scan_tmp, st);
  HIPCHK(hipMemcpyAsync(&p.total, p.doff + p.nc, 8, hipMemcpyDeviceToHost, st));
  return RB_OK;
}
void cat_emit(rbgpu_ctx *ctx, const CatPart &p, rbgpu_set *dst, uint32_t bitmap_base, uint64_t cont_base,
              uint64_t pay_base) {
  hipStream_t st = ctx->stream;
  k_cat_begin<<<nblk(p.count + 1ull, 256), 256, 0, st>>>(p.s->begin + p.first, p.count, p.c0, cont_base,
                                                         dst->begin + bitmap_base);
  if (p.nc)
    k_cat_copy<<<grid_for(p.nc, 4), 256, 0, st>>>(p.s->view(), p.c0, p.nc, p.doff, cont_base, pay_base,
                                                  OutView{dst->key, dst->type, dst->card, dst->nruns, dst->off},
                                                  dst->payload);
}
// the parts back to back as one new set (a clone when there is one part)
int cat_sets(rbgpu_ctx *ctx, CatPart *parts, int np, rbgpu_set **out) {
  hipStream_t st = ctx->stream;
  Scratch tmp(ctx->pool);
  int rc;
  for (int i = 0; i < np; ++i)
    if ((rc = cat_measure(ctx, tmp, parts[i]))) return rc;
  HIPCHK(hipStreamSynchronize(st));
  LAUNCHCHK();
  uint64_t nb = 0, nc = 0, total = 0;
  for (int i = 0; i < np; ++i) nb += parts[i].count, nc += parts[i].nc, total += parts[i].total;
  SetPtr s;
  if ((rc = make_set(ctx, (uint32_t)nb, nc, total, s))) return rc;
  uint32_t bb = 0;
  uint64_t cb = 0, pb = 0;
  for (int i = 0; i < np; ++i) {
    cat_emit(ctx, parts[i], s.get(), bb, cb, pb);
    bb += parts[i].count, cb += parts[i].nc, pb += parts[i].total;
  }
  const hipError_t e = hipStreamSynchronize(st), e2 = hipGetLastError();
  if (e != hipSuccess || e2 != hipSuccess)
    return fail(RB_EDEVICE, "bsi arithmetic: concatenation failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
  *out = s.release();
  return RB_OK;
}

bool ebm_empty(const rbgpu_set *s) { return s->h_begin[s->nb] == s->h_begin[s->nb - 1]; }

// a.ebM after or(b.ebM) in place, a one-bitmap set
int ebm_union(rbgpu_ctx *ctx, const rbgpu_set *a, const rbgpu_set *b, SetPtr &e) {
  const uint32_t ia = a->nb - 1, ib = b->nb - 1;
  rbgpu_set *r = nullptr;
  const int rc = pairwise_call(ctx, RB_OR, a, b, &ia, &ib, 1, &r, true, false);
  e.reset(r);
  return rc;
}

// The fused path.  *ran = false (and nothing created): some key is not plain, the caller takes the chain.
int add_fused(rbgpu_ctx *ctx, const rbgpu_set *a, const rbgpu_set *b, rbgpu_set **out, bool *ran) {
  *ran = false;
  hipStream_t st = ctx->stream;
  const uint32_t na = a->nb - 1, nb = b->nb - 1, n = std::max(na, nb);
  int rc;
  if ((rc = ensure_bsi_tables(ctx, a, na)) || (rc = ensure_bsi_tables(ctx, b, nb))) return rc;
  Scratch tmp(ctx->pool); // back to the pool when the call leaves (every path has waited for the stream, or failed)
  uint8_t *act;
  uint64_t *bt, *bts;
  uint32_t *klist, *notplain;
  if (!tmp.get(act, 65536) || !tmp.get(bt, 256) || !tmp.get(bts, 257) || !tmp.get(klist, 65536) || !tmp.get(notplain, 1))
    return fail(RB_ENOMEM, "bsi add: plan");
  HIPCHK(hipMemsetAsync(notplain, 0, 4, st));
  k_bsi_add_keys<<<256, 256, 0, st>>>(a->view(), b->view(), a->bsi_table, b->bsi_table, na, nb, act, bt, notplain);
  const uint64_t *in1[1] = {bt};
  uint64_t *out1[1] = {bts};
  scan_blocks_multi(in1, out1, 1, 256, nullptr, st);
  k_bsi_add_list<<<256, 256, 0, st>>>(act, bts, klist);
  uint64_t nk64 = 0;
  uint32_t np = 0;
  HIPCHK(hipMemcpyAsync(&nk64, bts + 256, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&np, notplain, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  LAUNCHCHK();
  if (np) return RB_OK;
  const uint32_t nk = (uint32_t)nk64;
  SetPtr ebm;
  if ((rc = ebm_union(ctx, a, b, ebm))) return rc;
  CatPart ep;
  ep.s = ebm.get();
  ep.count = 1;

  stats_begin(ctx);
  const uint64_t T = (uint64_t)nk * (n + 1);
  AddArgs g{};
  uint64_t *tpos = nullptr, *toff = nullptr, *scan_tmp = nullptr;
  uint64_t tot[3] = {0, 0, 0}; // kept candidates below slice n, kept candidates, their payload bytes
  if (T) {
    if (!tmp.get(g.ttype, T) || !tmp.get(g.tkeep, T) || !tmp.get(g.tbytes, T) || !tmp.get(tpos, T + 1) ||
        !tmp.get(toff, T + 1) || !tmp.get(scan_tmp, scan_tmp_words(T) + 1))
      return fail(RB_ENOMEM, "bsi add: workspace of %llu candidate containers", (unsigned long long)T);
    g.A = a->view();
    g.B = b->view();
    g.ta = a->bsi_table;
    g.tb = b->bsi_table;
    g.na = na;
    g.nb = nb;
    g.n = n;
    g.klist = klist;
    g.nk = nk;
    g.tpos = tpos;
    g.toff = toff;
    g.stats = ctx->d_stats;
    HIPCHK(hipEventRecord(ctx->ev[1], st));
    k_bsi_add<0><<<nblk(nk, 4), 256, 0, st>>>(g);
    HIPCHK(hipEventRecord(ctx->ev[2], st));
    scan_exclusive(g.tkeep, tpos, T, scan_tmp, st);
    scan_exclusive(g.tbytes, toff, T, scan_tmp, st);
    HIPCHK(hipMemcpyAsync(&tot[0], tpos + (uint64_t)nk * n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&tot[1], tpos + T, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&tot[2], toff + T, 8, hipMemcpyDeviceToHost, st));
  }
  if ((rc = cat_measure(ctx, tmp, ep))) return rc;
  HIPCHK(hipStreamSynchronize(st));
  LAUNCHCHK();
  const bool grows = tot[1] > tot[0]; // the carry out of slice n - 1 is not empty at some key
  if (grows && n == 64)
    return fail(RB_EINVAL, "bsi add: the sum of some column needs a 65th slice (the carry out of slice 63 is not empty)");
  const uint32_t nres = n + (grows ? 1u : 0u);
  const uint64_t nc = tot[1], total = tot[2];
  // the result is exact-sized: when it cannot be allocated the call ends here, before anything is written
  SetPtr s;
  if ((rc = make_set(ctx, nres + 1, nc + ep.nc, total + ep.total, s))) return rc;
  auto drop = [&](int r) { // the sets go back to the pool behind their kernels
    (void)hipStreamSynchronize(st);
    return r;
  };
  if (T) {
    k_bsi_add_begin<<<1, 128, 0, st>>>(tpos, nk, nres, s->begin);
    g.out = OutView{s->key, s->type, s->card, s->nruns, s->off};
    g.payload = s->payload;
    if (hipEventRecord(ctx->ev[3], st) != hipSuccess) return drop(fail(RB_EDEVICE, "bsi add: event"));
    k_bsi_add<1><<<nblk(nk, 4), 256, 0, st>>>(g);
    if (hipEventRecord(ctx->ev[4], st) != hipSuccess) return drop(fail(RB_EDEVICE, "bsi add: event"));
  } else if (hipMemsetAsync(s->begin, 0, (nres + 1ull) * 8, st) != hipSuccess) {
    return drop(fail(RB_EDEVICE, "bsi add: memset failed"));
  }
  cat_emit(ctx, ep, s.get(), nres, nc, total);
  const KernelSpan spans[2] = {{"k_bsi_add<measure>", 2, -1, T}, {"k_bsi_add<emit>", 0, 1, nk, ctx->ev[3], ctx->ev[4]}};
  rc = stats_end(ctx, nk, nc, spans, T ? 2 : 0);
  if (rc) return drop(rc);
  *out = s.release();
  *ran = true;
  return RB_OK;
}

// The chain: addDigit over the library's own calls.  The state is a set whose bitmap i is slice i (first `a` itself
// through an index list, then each step's result); a digit is bitmap fi of set F.
int add_chain(rbgpu_ctx *ctx, const rbgpu_set *a, const rbgpu_set *b, rbgpu_set **out) {
  const uint32_t na = a->nb - 1, nb = b->nb - 1;
  const rbgpu_set *S = a;
  SetPtr state, carry;
  std::vector<uint32_t> sidx(std::max(na, nb), kEmptyBitmap), bidx; // grow(otherBsi.bitCount())
  for (uint32_t i = 0; i < na; ++i) sidx[i] = i;
  int rc;
  for (uint32_t d = 0; d < nb; ++d) {
    const rbgpu_set *F = b;
    uint32_t fi = d;
    for (uint32_t i = d;; ++i) {
      rbgpu_set *cr = nullptr, *nx = nullptr;
      if ((rc = pairwise_call(ctx, RB_AND, S, F, &sidx[i], &fi, 1, &cr, false, false))) return rc;
      SetPtr next_carry(cr);
      bidx.assign(sidx.size(), kEmptyBitmap);
      bidx[i] = fi;
      if ((rc = pairwise_call(ctx, RB_XOR, S, F, sidx.data(), bidx.data(), (uint32_t)sidx.size(), &nx, true, false)))
        return rc;
      state.reset(nx); // the step's inputs are released behind its kernels (stream order)
      S = nx;
      for (uint32_t k = 0; k < sidx.size(); ++k) sidx[k] = k;
      carry = std::move(next_carry);
      if (carry->nc == 0) break; // and() drops empty containers: no container, no member
      if (i + 1 >= sidx.size()) {
        if (sidx.size() >= 64)
          return fail(RB_EINVAL, "bsi add: the sum of some column needs a 65th slice (the carry out of slice 63 is not empty)");
        sidx.push_back(kEmptyBitmap); // grow(bitCount() + 1)
      }
      F = carry.get();
      fi = 0;
    }
  }
  SetPtr ebm;
  if ((rc = ebm_union(ctx, a, b, ebm))) return rc;
  CatPart parts[2]; // without a digit (nb = 0) the state is still a's own slices, bitmaps [0, na)
  parts[0].s = S;
  parts[0].count = (uint32_t)sidx.size();
  parts[1].s = ebm.get();
  parts[1].count = 1;
  return cat_sets(ctx, parts, 2, out);
}

int clone_set(rbgpu_ctx *ctx, const rbgpu_set *a, rbgpu_set **out) {
  CatPart p;
  p.s = a;
  p.count = a->nb;
  stats_begin(ctx); // rb_stats describes the copy: no kernel span, no counted bytes, the clone's containers
  int rc = cat_sets(ctx, &p, 1, out);
  if (!rc && (rc = stats_end(ctx, 0, p.nc, nullptr, 0))) {
    rbgpu_set_free(*out);
    *out = nullptr;
  }
  return rc;
}
} // namespace

int bsi_min_max(rbgpu_ctx *ctx, const rbgpu_set *bsi, uint64_t *min_value, uint64_t *max_value, bool with_stats) {
  if (min_value) *min_value = 0;
  if (max_value) *max_value = 0;
  const uint32_t nbits = bsi->nb - 1;
  int rc = ensure_h_begin(bsi);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  if (ebm_empty(bsi)) {
    if (with_stats) {
      stats_begin(ctx);
      return stats_end(ctx, 0, 0, nullptr, 0);
    }
    return RB_OK;
  }
  if ((rc = ensure_bsi_tables(ctx, bsi, nbits))) return rc;
  Scratch tmp(ctx->pool);
  uint64_t *mm;
  if (!tmp.get(mm, 2)) return fail(RB_ENOMEM, "bsi min / max");
  if (with_stats) stats_begin(ctx);
  const uint64_t mm0[2] = {~0ull, 0ull};
  uint64_t h[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(mm, mm0, 16, hipMemcpyHostToDevice, st));
  if (with_stats) HIPCHK(hipEventRecord(ctx->ev[1], st));
  k_bsi_minmax<<<nblk(bsi->bsi_nk, 4), 256, 0, st>>>(bsi->view(), bsi->bsi_table, nbits, bsi->bsi_klist, bsi->bsi_nk, mm,
                                                     with_stats ? ctx->d_stats : nullptr);
  if (with_stats) HIPCHK(hipEventRecord(ctx->ev[2], st));
  HIPCHK(hipMemcpyAsync(h, mm, 16, hipMemcpyDeviceToHost, st));
  if (with_stats) {
    const KernelSpan spans[1] = {{"k_bsi_minmax", 0, -1, bsi->bsi_nk}};
    if ((rc = stats_end(ctx, bsi->bsi_nk, 0, spans, 1))) return rc;
  } else {
    HIPCHK(hipStreamSynchronize(st));
    LAUNCHCHK();
  }
  if (min_value) *min_value = h[0];
  if (max_value) *max_value = h[1];
  return RB_OK;
}

int bsi_add(rbgpu_ctx *ctx, const rbgpu_set *a, const rbgpu_set *b, uint32_t flags, rbgpu_set **out, uint64_t *min_value,
            uint64_t *max_value) {
  int rc;
  if ((rc = ensure_h_begin(a)) || (rc = ensure_h_begin(b))) return rc;
  rbgpu_set *r = nullptr;
  if (ebm_empty(b)) { // the reference returns early: a as it is, its bitmap count kept
    rc = clone_set(ctx, a, &r);
  } else {
    bool ran = false;
    rc = (flags & RB_BSI_ADD_CHAIN) ? RB_OK : add_fused(ctx, a, b, &r, &ran);
    if (!rc && !ran) rc = add_chain(ctx, a, b, &r);
  }
  if (rc) return rc;
  SetPtr res(r);
  if ((min_value || max_value) && (rc = bsi_min_max(ctx, r, min_value, max_value, false))) return rc;
  *out = res.release();
  return RB_OK;
}

int bsi_merge(rbgpu_ctx *ctx, const rbgpu_set *a, const rbgpu_set *b, uint32_t flags, rbgpu_set **out) {
  int rc;
  if ((rc = ensure_h_begin(a)) || (rc = ensure_h_begin(b))) return rc;
  if (ebm_empty(b)) return clone_set(ctx, a, out);
  const uint32_t na = a->nb - 1, nb = b->nb - 1, n = std::max(na, nb);
  uint64_t common = 0;
  if ((rc = pairwise_impl(ctx, RB_AND, a, b, &na, &nb, 1, nullptr, &common, PairOpts{}))) return rc;
  if (common) return fail(RB_EINVAL, "merge can be used only in bsiA  bsiB  is null");
  SetPtr slices, ebm;
  if (n) {
    std::vector<uint32_t> ai(n, kEmptyBitmap), bi(n, kEmptyBitmap); // a missing slice stands in as an empty bitmap
    for (uint32_t i = 0; i < na; ++i) ai[i] = i;
    for (uint32_t i = 0; i < nb; ++i) bi[i] = i;
    rbgpu_set *r = nullptr;
    if ((rc = pairwise_call(ctx, RB_OR, a, b, ai.data(), bi.data(), n, &r, false, false))) return rc;
    slices.reset(r);
    if (flags & RB_BUILD_RUN_OPTIMIZE) {
      if ((rc = rbgpu_set_run_optimize(slices.get(), &r, nullptr))) return rc;
      slices.reset(r);
    }
  }
  if ((rc = ebm_union(ctx, a, b, ebm))) return rc;
  CatPart parts[2];
  int np = 0;
  if (n) {
    parts[np].s = slices.get();
    parts[np++].count = n;
  }
  parts[np].s = ebm.get();
  parts[np++].count = 1;
  return cat_sets(ctx, parts, np, out);
}

// this file's code object, loaded at context creation (rbgpu_open, context.hip)
__global__ void k_warm_bsi_arith() {}
void warm_bsi_arith(hipStream_t st) { k_warm_bsi_arith<<<1, 64, 0, st>>>(); }

} // namespace rbg

// ===================================================================== C ABI
using namespace rbg;

static int check_bsi_arg(rbgpu_ctx *ctx, const rbgpu_set *s, const char *name) {
  if (!s) return fail(RB_EINVAL, "null %s", name);
  if (s->ctx != ctx) return fail(RB_EINVAL, "%s belongs to another context", name);
  if (s->nb < 1 || s->nb > 65) return fail(RB_EINVAL, "%s: a bsi set holds 0..64 slices and the existence bitmap", name);
  return RB_OK;
}

extern "C" {

int rbgpu_bsi_add(rbgpu_ctx *ctx, const rbgpu_set *a, const rbgpu_set *b, uint32_t flags, rbgpu_set **out,
                  uint64_t *min_value, uint64_t *max_value) {
  if (!out) return fail(RB_EINVAL, "null out");
  *out = nullptr; // before anything can fail: no path leaves the caller's word as it was
  if (min_value) *min_value = 0;
  if (max_value) *max_value = 0;
  SETTLE(a, b);
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_bsi_arg(ctx, a, "a")) || (rc = check_bsi_arg(ctx, b, "b"))) return rc;
  if (flags & ~(uint32_t)RB_BSI_ADD_CHAIN) return fail(RB_EINVAL, "unknown bsi add flags %#x", flags);
  return bsi_add(ctx, a, b, flags, out, min_value, max_value);
}

int rbgpu_bsi_merge(rbgpu_ctx *ctx, const rbgpu_set *a, const rbgpu_set *b, uint32_t flags, rbgpu_set **out) {
  if (!out) return fail(RB_EINVAL, "null out");
  *out = nullptr;
  SETTLE(a, b);
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_bsi_arg(ctx, a, "a")) || (rc = check_bsi_arg(ctx, b, "b"))) return rc;
  if (flags & ~(uint32_t)RB_BUILD_RUN_OPTIMIZE) return fail(RB_EINVAL, "unknown bsi merge flags %#x", flags);
  return bsi_merge(ctx, a, b, flags, out);
}

int rbgpu_bsi_min_max(rbgpu_ctx *ctx, const rbgpu_set *bsi, uint64_t *min_value, uint64_t *max_value) {
  if (!min_value || !max_value) return fail(RB_EINVAL, "null out");
  *min_value = *max_value = 0;
  SETTLE(bsi);
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_bsi_arg(ctx, bsi, "bsi"))) return rc;
  return bsi_min_max(ctx, bsi, min_value, max_value, true);
}

} // extern "C"
