// aggregate.hip — the wide (many-bitmap) entry points and the priority-queue aggregations, whose order the host
// computes: each step is one pairwise call on the device.
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "format.hpp"
#include "internal.hpp"
#include "kernels.hpp"

using namespace rbg;

extern "C" {

// ---------------------------------------------------------------- wide
// FastAggregation.priorityqueue_xor (FastAggregation.java:732-752): a queue of bitmaps ordered by
// getLongSizeInBytes (java.util.PriorityQueue, Collections.addAll order); the two smallest are
// replaced by their RoaringBitmap.xor — one pairwise call on the device — until one is left.
static int empty_result(rbgpu_ctx *ctx, rbgpu_set **out) {
  SetPtr e;
  const int rc = make_set(ctx, 1, 0, 16, e);
  if (rc) return rc;
  const uint64_t hb[2] = {0, 0};
  // on the library stream (it is non-blocking: a null-stream copy would not be ordered after its kernels)
  HIPCHK(hipMemcpyAsync(e->begin, hb, 16, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  e->h_begin = {0, 0};
  *out = e.release();
  return RB_OK;
}
// The size a priority queue orders bitmaps by, per bitmap of s (one metadata read-back):
//   kSizeLong       RoaringBitmap.getLongSizeInBytes (RoaringBitmap.java:2212-2219): 8 + per container
//                   2 + getSizeInBytes (Array 2c + 4, Bitmap 8192 lazy or not, Run 4r + 4);
//   kSizeImmutable  ImmutableRoaringBitmap.getLongSizeInBytes (buffer/ImmutableRoaringBitmap.java:1508-1521):
//                   4 + per container 4 + (Run 2 + 4r; else getCardinality() > 4096 ? 8192 : 2 getCardinality()),
//                   a lazy Bitmap's getCardinality() being -1 (MappeableBitmapContainer.java:540-542);
//   kSizeSerialized ImmutableRoaringBitmap.serializedSizeInBytes (buffer/MutableRoaringArray.java:756-764).
// Intermediate results of priorityqueue_or carry the lazy marks in their card words (common.hpp).
enum { kSizeLong = 0, kSizeImmutable = 1, kSizeSerialized = 2 };
static int pq_sizes(const rbgpu_set *s, int kind, std::vector<int64_t> &out) {
  int rc = ensure_h_begin(s);
  if (rc) return rc;
  std::vector<uint8_t> type;
  std::vector<uint16_t> nruns;
  std::vector<uint32_t> card;
  if ((rc = read_meta(s, 0, s->nc, type, nruns, card))) return rc;
  out.assign(s->nb, 0);
  for (uint32_t b = 0; b < s->nb; ++b) {
    const uint64_t lo = s->h_begin[b], hi = s->h_begin[b + 1], k = hi - lo;
    int64_t v = kind == kSizeLong ? 8 : kind == kSizeImmutable ? 4 : 0;
    bool hasrun = false;
    for (uint64_t i = lo; i < hi; ++i) {
      const int64_t r = nruns[i], c = card[i] & ~kCardMarks;
      const bool lazy = type[i] == RB_BITMAP && (card[i] & kLazyCard);
      hasrun |= type[i] == RB_RUN;
      if (kind == kSizeLong)
        v += 2 + (type[i] == RB_BITMAP ? 8192 : type[i] == RB_ARRAY ? 2 * c + 4 : 4 * r + 4);
      else if (kind == kSizeImmutable)
        v += 4 + (type[i] == RB_RUN ? 2 + 4 * r : lazy ? -2 : c > kMaxArray ? 8192 : 2 * c);
      else
        v += type[i] == RB_BITMAP ? 8192 : type[i] == RB_ARRAY ? 2 * c : 2 + 4 * r;
    }
    if (kind == kSizeSerialized)
      v += (int64_t)serialized_header_bytes(hasrun, k);
    out[b] = v;
  }
  return RB_OK;
}

// buffered: BufferFastAggregation.priorityqueue_xor (buffer/BufferFastAggregation.java:933-958) — fewer
// than 2 bitmaps throw, the queue orders by ImmutableRoaringBitmap.getLongSizeInBytes.
static int pq_xor(rbgpu_ctx *ctx, const rbgpu_set *in, const std::vector<uint32_t> &mem, rbgpu_set **out,
                  bool buffered) {
  const size_t n = mem.size();
  if (buffered && n < 2) return fail(RB_EINVAL, "Expecting at least 2 bitmaps");
  if (n == 0) return empty_result(ctx, out);
  const int kind = buffered ? kSizeImmutable : kSizeLong;
  std::vector<int64_t> sz;
  int rc = pq_sizes(in, kind, sz);
  if (rc) return rc;
  struct Node {
    const rbgpu_set *s;
    uint32_t idx;
    int64_t size;
    SetPtr owned;
  };
  std::vector<Node> nodes;
  nodes.reserve(2 * n);
  for (uint32_t m : mem) nodes.push_back(Node{in, m, sz[m], nullptr});
  auto cmp = [&](uint32_t a, uint32_t b) { return (int)(nodes[a].size - nodes[b].size); };
  JavaHeap<uint32_t, decltype(cmp)> pq(cmp);
  for (uint32_t k = 0; k < n; ++k) pq.offer(k);
  while (pq.size() > 1) {
    const uint32_t x1 = pq.poll(), x2 = pq.poll();
    const uint32_t i1 = nodes[x1].idx, i2 = nodes[x2].idx;
    rbgpu_set *raw = nullptr;
    rc = rbgpu_pairwise(ctx, RB_XOR, nodes[x1].s, nodes[x2].s, &i1, &i2, 1, &raw);
    SetPtr r(raw);
    std::vector<int64_t> rs;
    if (!rc) rc = pq_sizes(raw, kind, rs);
    if (rc) return rc;
    for (uint32_t x : {x1, x2}) nodes[x].owned.reset(); // the operands are not referenced again
    nodes.push_back(Node{raw, 0, rs[0], std::move(r)});
    pq.offer((uint32_t)nodes.size() - 1);
  }
  Node &last = nodes[pq.poll()];
  if (last.owned) {
    *out = last.owned.release();
    return RB_OK;
  }
  return rbgpu_set_extract(last.s, last.idx, 1, out); // one member: the reference returns it as is
}

// FastAggregation.priorityqueue_or(RoaringBitmap...) (FastAggregation.java:675-721; oracle wide_pq_or):
// the bitmaps in a java.util.PriorityQueue by getLongSizeInBytes; the two smallest are lazily OR'd —
// RoaringBitmap.lazyor (static) when neither is a temporary, this.lazyor(other) on the temporary one,
// lazyorfromlazyinputs when both are — the result re-queued with its size; the survivor is repaired
// (repairAfterLazy).  Each step is one device pairwise call in a lazy role (pairwise.hip
// lazy_or_type); its size comes back from the result's summary.  The repair is one more call, the
// survivor with itself in the kLazyRepair role (a lazy Bitmap -> LR, an exact one kept, Run -> EFF).
// BufferFastAggregation.priorityqueue_or (buffer/BufferFastAggregation.java:810-930) runs the same merges
// ordered by serializedSizeInBytes (varargs, kind kSizeSerialized) or ImmutableRoaringBitmap.
// getLongSizeInBytes (Iterator, kSizeImmutable), and returns a lone bitmap as a copy, unrepaired.
static int pq_or(rbgpu_ctx *ctx, const rbgpu_set *in, const std::vector<uint32_t> &mem, rbgpu_set **out,
                 int kind) {
  const size_t n = mem.size();
  if (n == 0) return empty_result(ctx, out);
  if (n == 1 && kind != kSizeLong) return rbgpu_set_extract(in, mem[0], 1, out); // toMutableRoaringBitmap
  std::vector<int64_t> sz;
  int rc = pq_sizes(in, kind, sz);
  if (rc) return rc;
  struct Node {
    const rbgpu_set *s;
    uint32_t idx;
    int64_t size;
    SetPtr owned;
    bool tmp; // a temporary of the queue (istmp)
  };
  std::vector<Node> nodes;
  nodes.reserve(2 * n);
  for (uint32_t m : mem) nodes.push_back(Node{in, m, sz[m], nullptr, false});
  auto cmp = [&](uint32_t a, uint32_t b) { return (int)(nodes[a].size - nodes[b].size); };
  JavaHeap<uint32_t, decltype(cmp)> pq(cmp);
  for (uint32_t k = 0; k < n; ++k) pq.offer(k);
  while (pq.size() > 1) {
    const uint32_t x1 = pq.poll(), x2 = pq.poll();
    // target (left operand) and role, FastAggregation.java:690-716
    uint32_t t = x1, o = x2;
    int role = kLazyStatic;
    if (nodes[x1].tmp && nodes[x2].tmp) role = kLazyIorBf;
    else if (nodes[x2].tmp) t = x2, o = x1, role = kLazyIor;
    else if (nodes[x1].tmp) role = kLazyIor;
    const uint32_t it = nodes[t].idx, io = nodes[o].idx;
    rbgpu_set *raw = nullptr;
    rc = pairwise_impl(ctx, role, nodes[t].s, nodes[o].s, &it, &io, 1, &raw, nullptr, PairOpts{});
    SetPtr r(raw);
    std::vector<int64_t> rs;
    if (!rc) rc = pq_sizes(raw, kind, rs);
    if (rc) return rc;
    for (uint32_t x : {x1, x2}) nodes[x].owned.reset(); // the operands are not referenced again
    nodes.push_back(Node{raw, 0, rs[0], std::move(r), true});
    pq.offer((uint32_t)nodes.size() - 1);
  }
  const Node &last = nodes[pq.poll()];
  const uint32_t il = last.idx;
  return pairwise_impl(ctx, kLazyRepair, last.s, last.s, &il, &il, 1, out, nullptr, PairOpts{}); // repairAfterLazy
}

int rbgpu_wide(rbgpu_ctx *ctx, int sem, const rbgpu_set *in, const uint32_t *members, uint32_t n, rbgpu_set **out) {
  return rbgpu_wide_keys(ctx, sem, in, members, n, 0, 65536, out);
}

int rbgpu_wide_keys(rbgpu_ctx *ctx, int sem, const rbgpu_set *in, const uint32_t *members, uint32_t n,
                    uint32_t key_lo, uint32_t key_hi, rbgpu_set **out) {
  SETTLE(in);
  if (!out) return fail(RB_EINVAL, "null out");
  if (key_lo > key_hi || key_hi > 65536) return fail(RB_EINVAL, "bad key range [%u, %u)", key_lo, key_hi);
  *out = nullptr;
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if (!in || in->ctx != ctx) return fail(RB_EINVAL, "bad input set");
  if (sem < RB_FAST_OR || sem > RB_BUFFER_PQ_XOR) return fail(RB_EINVAL, "bad semantics %d", sem);
  rc = ensure_h_begin(in);
  if (rc) return rc;
  std::vector<uint32_t> mem;
  if (members) {
    mem.assign(members, members + n);
    for (uint32_t m : mem)
      if (m >= in->nb) return fail(RB_EINVAL, "member %u out of range", m);
  } else {
    if (n > in->nb) return fail(RB_EINVAL, "n exceeds the set");
    mem.resize(n);
    for (uint32_t i = 0; i < n; ++i) mem[i] = i;
  }
  if (sem == RB_PQ_XOR || sem == RB_PQ_OR || sem >= RB_BUFFER_PQ_OR) {
    if (key_lo != 0 || key_hi != 65536) return fail(RB_EINVAL, "priorityqueue_or/xor have no key-range shards");
    switch (sem) {
    case RB_PQ_XOR: return pq_xor(ctx, in, mem, out, false);
    case RB_BUFFER_PQ_XOR: return pq_xor(ctx, in, mem, out, true);
    case RB_PQ_OR: return pq_or(ctx, in, mem, out, kSizeLong);
    case RB_BUFFER_PQ_OR: return pq_or(ctx, in, mem, out, kSizeSerialized);
    default: return pq_or(ctx, in, mem, out, kSizeImmutable);
    }
  }
  return wide_run(ctx, sem, in, mem, key_lo, key_hi, out);
}

int rbgpu_wide_cardinality(rbgpu_ctx *ctx, int op, const rbgpu_set *in, const uint32_t *members, uint32_t n,
                           uint64_t *out) {
  SETTLE(in);
  if (!out) return fail(RB_EINVAL, "null out");
  if (op != RB_AND && op != RB_OR) return fail(RB_EINVAL, "wide cardinality supports AND and OR");
  rbgpu_set *r = nullptr;
  int rc = rbgpu_wide(ctx, op == RB_AND ? RB_WORKSHY_AND : RB_FAST_OR, in, members, n, &r);
  if (rc) return rc;
  rc = rbgpu_set_cardinalities(r, out);
  rbgpu_set_free(r);
  return rc;
}

} // extern "C"
