// pairwise_call.hip — the host side of the pairwise calls: the small-batch path (one launch) and the general
// pipeline (segments, tasks, task kernels, compaction), their entry points and the probe hook.
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

namespace {
// ---------------------------------------------------------------- pairwise
// Merge-path segment length: 256 merged keys per thread for large batches; shorter when the batch's
// expected key count would leave fewer than ~128K walking threads (the walk is latency-bound).
static uint32_t pairwise_seg_keys(const rbgpu_set *a, const rbgpu_set *b, uint64_t np) {
  const double per = (double)a->nc / std::max<uint32_t>(a->nb, 1) + (double)b->nc / std::max<uint32_t>(b->nb, 1);
  const double est = per * (double)np;
  uint32_t seg = 256;
  while (seg > 8 && est / seg < 131072.0) seg >>= 1;
  return seg;
}
// Small batches (kernels.hpp: <= kSmallPairs pairs of <= kSmallPairKeys keys, <= kSmallSlots merged
// keys, no Run container over 8 KiB to copy): two launches and one host read-back.  Returns 1 when
// the batch does not qualify (the general pipeline runs), else an rbgpu status.
// containers of bitmap i (RB_EMPTY_BITMAP: none)
static inline uint64_t bm_conts(const rbgpu_set *s, uint32_t i) {
  return i == kEmptyBitmap ? 0 : s->h_begin[i + 1] - s->h_begin[i];
}
static int pairwise_small(rbgpu_ctx *ctx, int op, const rbgpu_set *a, const rbgpu_set *b, const uint32_t *a_idx,
                          const uint32_t *b_idx, uint32_t np, rbgpu_set **out, uint64_t *card_out, bool inplace,
                          bool keep_empty) {
  const char *dis = getenv("RBGPU_NO_SMALL_PAIRS"); // parity tests run both paths
  if ((dis && dis[0] == '1') || np == 0 || np > kSmallPairs) return 1;
  int rc = ensure_h_begin(a);
  if (!rc) rc = ensure_h_begin(b);
  if (rc) return rc;
  // per pair: first containers and counts (from the host CSR), first slot (merged keys <= na + nb), first
  // block (small_pair_nsub blocks per pair, at most ~16K blocks in all), the x1.op(x1) flag
  if (a->nc >= (1ull << 32) || b->nc >= (1ull << 32)) return 1; // 32-bit container indices in the tables
  const uint32_t cap = std::max<uint32_t>(1, std::min<uint32_t>(2048, 16384 / np));
  const bool inl = np <= kSmallInline;
  const uint64_t nid = (np + 31) / 32;
  std::vector<uint32_t> &tabv = ctx->small_tab; // [ident nid | i0 np | j0 np | nab np | slot np + 1 | blk np + 1]
  SmallTabInline *ti = inl ? &ctx->small_inline : nullptr;
  uint32_t *ident, *ti0, *tj0, *tnab, *slot, *blk;
  if (inl) {
    ident = ti->ident, ti0 = ti->i0, tj0 = ti->j0, tnab = ti->nab, slot = ti->slot, blk = nullptr;
  } else {
    tabv.assign(nid + 5ull * np + 2, 0u);
    ident = tabv.data(), ti0 = ident + nid, tj0 = ti0 + np, tnab = tj0 + np, slot = tnab + np, blk = slot + np + 1;
  }
  std::memset(ident, 0, 4 * nid);
  uint64_t acc = 0;
  uint32_t max_keys = 0;
  for (uint32_t p = 0; p < np; ++p) {
    const uint32_t ai = a_idx ? a_idx[p] : p, bi = b_idx ? b_idx[p] : p;
    const uint64_t na = bm_conts(a, ai), nb = bm_conts(b, bi), nk = na + nb;
    if (na > kSmallPairKeys || nb > kSmallPairKeys || nk > kSmallPairKeys) return 1;
    max_keys = std::max(max_keys, (uint32_t)nk);
    ti0[p] = ai == kEmptyBitmap ? 0u : (uint32_t)a->h_begin[ai];
    tj0[p] = bi == kEmptyBitmap ? 0u : (uint32_t)b->h_begin[bi];
    tnab[p] = (uint32_t)na | ((uint32_t)nb << 16);
    if (inplace && a == b && ai == bi && ai != kEmptyBitmap) ident[p >> 5] |= 1u << (p & 31);
    slot[p] = (uint32_t)acc;
    acc += nk;
    if (acc > kSmallSlots) return 1;
  }
  slot[np] = (uint32_t)acc;
  rc = ensure_max_runs(a);
  if (!rc) rc = ensure_max_runs(b);
  if (rc) return rc;
  if (a->max_runs > 2048 || b->max_runs > 2048) return 1; // a copy would not fit its 8 KiB slot
  const uint64_t E = acc;
  // merged keys per wave: 1, or doubled until the blocks fit the resident ones (one round of blocks)
  const uint64_t resident = small_resident_blocks();
  auto nsub = [&](uint32_t p, uint32_t kpw) { return small_pair_nsub(slot[p + 1] - slot[p], cap, kpw); };
  auto blocks_for = [&](uint32_t kpw) {
    uint64_t n = 0;
    for (uint32_t p = 0; p < np; ++p) n += nsub(p, kpw);
    return n;
  };
  uint32_t kpw = 1;
  uint64_t nblocks64 = blocks_for(1);
  while (nblocks64 > resident && kpw < 64) {
    kpw *= 2;
    nblocks64 = blocks_for(kpw);
  }
  const uint32_t nblocks = (uint32_t)nblocks64;
  for (uint32_t p = 0, k = 0; p <= np; ++p) {
    if (inl) ti->blk[p] = (uint16_t)k;
    else blk[p] = k;
    if (p < np) k += nsub(p, kpw);
  }
  rc = ensure_call_words(ctx);
  if (!rc) rc = seq_begin(ctx);
  if (rc) return rc;
  uint64_t *hout = reinterpret_cast<uint64_t *>(ctx->h_small);

  hipStream_t st = ctx->stream;
  const bool card_only = out == nullptr;
  const uint64_t E1 = std::max<uint64_t>(E, 1);
  const size_t tabb = inl ? 0 : 4 * tabv.size();
  const size_t need = aligned256(8ull * np) + aligned256(4 * E1) + aligned256(tabb) + 256;
  if (ctx->ws_pairs.reserve(need, st) != hipSuccess) return fail(RB_ENOMEM, "pair workspace");
  Workspace &W = ctx->ws_pairs;
  SmallPairArgs sa{};
  sa.A = a->view();
  sa.B = b->view();
  sa.np = np;
  SmallTabDev dt{};
  if (!inl) { // larger batches: the tables in device memory, one copy from pinned staging
    if ((rc = ensure_stage(ctx, tabb))) return rc;
    std::memcpy(ctx->h_stage, tabv.data(), tabb);
    uint32_t *d = W.take<uint32_t>(tabv.size());
    HIPCHK(hipMemcpyAsync(d, ctx->h_stage, tabb, hipMemcpyHostToDevice, st));
    dt = SmallTabDev{d, d + nid, d + nid + np, d + nid + 2ull * np, d + nid + 3ull * np, d + nid + 4ull * np + 1};
  }
  sa.pcard = card_out ? W.take<uint64_t>(np) : nullptr;
  uint32_t *xpos = W.take<uint32_t>(E1);
  sa.smeta = ctx->d_small_slots;
  sa.ctr = ctx->d_small_ctr;

  SetPtr res;
  if (!card_only) {
    if ((rc = make_set(ctx, np, E, E * kBitmapBytes, res))) return rc;
    sa.arena = res->payload;
  }
  // kernel events only when asked for (RBGPU_SMALL_KERNEL_TIMES=1, the bench's breakdown): the call is a
  // few tens of microseconds
  const char *kt = getenv("RBGPU_SMALL_KERNEL_TIMES");
  const bool ktimes = kt && kt[0] == '1';
  stats_begin(ctx, false);
  if (ktimes) HIPCHK(hipEventRecord(ctx->ev[1], st));
  sa.E = (uint32_t)E;
  sa.xpos = xpos;
  sa.rbegin = res ? res->begin : nullptr;
  if (res) sa.out = OutView{res->key, res->type, res->card, res->nruns, res->off};
  sa.hout = reinterpret_cast<uint64_t *>(ctx->d_small);
  sa.seq = ++ctx->small_seq;
  sa.lazy = is_lazy_op(op) ? op : 0;
  sa.inplace = inplace;
  sa.keep_empty = keep_empty;
  launch_pair_small(is_lazy_op(op) ? (int)RB_OR : op, card_only, sa, ti, dt, max_keys, nblocks, st);
  if (ktimes) HIPCHK(hipEventRecord(ctx->ev[2], st));
  if (card_out) HIPCHK(hipMemcpyAsync(card_out, sa.pcard, 8ull * np, hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(ctx->ev[5], st));
  // The last block writes the result words to host memory and then the call's sequence number
  // (wait_call_seq); per-pair cardinalities come back by a copy, so those calls wait for the stream.
  bool seen = false;
  if ((rc = seq_end(ctx, sa.seq, !card_out, "small-batch pairwise", &seen))) return rc;
  // the result words, written by the last block straight into host memory
  uint64_t *w = ctx->words;
  for (int i = 0; i < kStatWords; ++i) w[i] = 0;
  w[0] = hout[1];           // input bytes with key arrays
  w[6] = hout[1] - hout[2]; // container input bytes
  w[1] = hout[3];           // output bytes
  w[7] = hout[4];           // result cardinality
  const uint64_t nres = hout[0];
  const KernelSpan spans[1] = {{"k_pair_small", 6, 1, E}};
  rc = stats_fill(ctx, E, nres, spans, ktimes ? 1 : 0, !seen);
  ctx->stats_pending = seen;
  ctx->stats_pending_k = seen && ktimes;
  if (rc) return rc;
  ctx->last.result_containers = nres;
  if (res) {
    res->nc = nres;
    res->end_seq = seen ? sa.seq : 0;
    *out = res.release();
  }
  return RB_OK;
}

// tasks bound up to which pairwise_impl reserves the task workspace before the totals are read back
// (58 B per task: 464 MiB at the cap; the bound a.nc + b.nc can far exceed the real count — an AND of
// mostly disjoint keys — and the workspace stays grown, so the cap is set just above config 2's 6.1M)
constexpr uint64_t kEarlyEmitTasks = 1ull << 23;

// One general-pipeline call: its arguments and what each phase leaves for the next.
struct PairCall {
  rbgpu_ctx *ctx;
  int op;
  const rbgpu_set *a, *b;
  const uint32_t *a_idx, *b_idx;
  uint32_t npairs;
  rbgpu_set **out;
  uint64_t *card_out;
  PairOpts o;
  hipStream_t st = nullptr;
  uint64_t np = 0;
  bool card_only = false;
  int kop = 0;   // the kernels' op (lazy roles run as OR, TaskMeta::lazy)
  int slot = -1; // asynchronous calls: the pinned word the result count lands in (SlotGuard)
  // per pair (ws_pairs)
  uint32_t *d_aidx = nullptr, *d_bidx = nullptr;
  uint64_t *nseg_p = nullptr, *seg_begin = nullptr, *pcard = nullptr, *ptmp = nullptr;
  bool host_segs = false, ident_segs = false;
  uint32_t seg_keys = 0;
  PairArgs pa{};
  uint64_t ns = 0, nblk = 0;
  // per segment (ws_segs)
  uint32_t *seg_pair = nullptr;
  uint64_t *cnt = nullptr; // per segment, packed (pack_seg_counts)
  PairCountArrays bt{}, bs{};
  uint64_t *task_begin = nullptr, *rseg = nullptr, *bk = nullptr, *bks = nullptr, *d_tot = nullptr;
  // per task (ws_tasks)
  TaskMeta tm{};
  TaskRec *light = nullptr, *heavy = nullptr;
  unsigned long long *queue = nullptr;
  bool early = false, conc = false;
  uint64_t tbound = 0, ntasks = 0, nlight = 0, nheavy = 0, small_base = 0, arena = 0;
  SetPtr res;
  bool tailed = false;
  CallTail tail{};
};

int check_pair_args(const PairCall &c) {
  const rbgpu_set *a = c.a, *b = c.b;
  if ((c.op < RB_AND || c.op > RB_ANDNOT) && !is_lazy_op(c.op)) return fail(RB_EINVAL, "bad op %d", c.op);
  if (!a || !b) return fail(RB_EINVAL, "null set");
  if (a->ctx != c.ctx || b->ctx != c.ctx) return fail(RB_EINVAL, "sets belong to another context");
  if (!c.a_idx && c.npairs > a->nb) return fail(RB_EINVAL, "npairs exceeds bitmaps of a");
  if (!c.b_idx && c.npairs > b->nb) return fail(RB_EINVAL, "npairs exceeds bitmaps of b");
  for (uint32_t i = 0; c.a_idx && i < c.npairs; ++i)
    if (c.a_idx[i] >= a->nb && c.a_idx[i] != kEmptyBitmap) return fail(RB_EINVAL, "a_idx[%u] out of range", i);
  for (uint32_t i = 0; c.b_idx && i < c.npairs; ++i)
    if (c.b_idx[i] >= b->nb && c.b_idx[i] != kEmptyBitmap) return fail(RB_EINVAL, "b_idx[%u] out of range", i);
  return RB_OK;
}

// a pinned word for an asynchronous call's result count; none free: the call completes synchronously
int take_async_slot(PairCall &c) {
  rbgpu_ctx *ctx = c.ctx;
  if (!ctx->h_async) {
    if (hipHostMalloc((void **)&ctx->h_async, kAsyncSlots * sizeof(uint64_t)) != hipSuccess)
      return fail(RB_ENOMEM, "pinned result-count slots");
    for (int i = kAsyncSlots - 1; i >= 0; --i) ctx->async_free.push_back(i);
  }
  if (!ctx->async_free.empty()) {
    c.slot = ctx->async_free.back();
    ctx->async_free.pop_back();
  }
  return RB_OK;
}

// ---- per pair: indices, merge-path segment counts and their scan, pair cardinalities
int stage_pairs(PairCall &c) {
  rbgpu_ctx *ctx = c.ctx;
  const rbgpu_set *a = c.a, *b = c.b;
  const uint64_t np = c.np;
  hipStream_t st = c.st;
  size_t need = 2 * aligned256(np * 4) + 3 * aligned256((np + 1) * 8) + aligned256(scan_tmp_words(np + 1) * 8);
  if (ctx->ws_pairs.reserve(need, st) != hipSuccess) return fail(RB_ENOMEM, "pair workspace");
  Workspace &W = ctx->ws_pairs;
  c.d_aidx = c.a_idx ? W.take<uint32_t>(np) : nullptr;
  c.d_bidx = c.b_idx ? W.take<uint32_t>(np) : nullptr;
  c.nseg_p = W.take<uint64_t>(np + 1), c.seg_begin = W.take<uint64_t>(np + 1);
  c.pcard = W.take<uint64_t>(np + 1);
  c.ptmp = W.take<uint64_t>(std::max<uint64_t>(scan_tmp_words(np + 1), 1));
  // small batches: the merge-path segment counts come from the host CSR copies (no count kernel,
  // scan and host read-back before the segment phase)
  c.host_segs = np && np <= 4096 && !ensure_h_begin(a) && !ensure_h_begin(b);
  c.seg_keys = pairwise_seg_keys(a, b, np);
  if (c.d_aidx || c.d_bidx || c.host_segs) { // through pinned staging: a pageable copy would block the host
    const size_t bytes = np * 4 * ((c.d_aidx != nullptr) + (c.d_bidx != nullptr)) + (c.host_segs ? (np + 1) * 8 : 0);
    if (const int rc = ensure_stage(ctx, bytes)) return rc;
    uint8_t *h = ctx->h_stage;
    if (c.d_aidx) {
      std::memcpy(h, c.a_idx, np * 4);
      HIPCHK(hipMemcpyAsync(c.d_aidx, h, np * 4, hipMemcpyHostToDevice, st));
      h += np * 4;
    }
    if (c.d_bidx) {
      std::memcpy(h, c.b_idx, np * 4);
      HIPCHK(hipMemcpyAsync(c.d_bidx, h, np * 4, hipMemcpyHostToDevice, st));
      h += np * 4;
    }
    if (c.host_segs) {
      uint64_t *sb = reinterpret_cast<uint64_t *>(h), acc = 0;
      for (uint64_t p = 0; p < np; ++p) { // k_seg_count's formula
        const uint32_t ai = c.a_idx ? c.a_idx[p] : (uint32_t)p, bi = c.b_idx ? c.b_idx[p] : (uint32_t)p;
        const uint64_t nk = bm_conts(a, ai) + bm_conts(b, bi);
        sb[p] = acc;
        acc += (nk + c.seg_keys - 1) / c.seg_keys + (nk == 0);
      }
      sb[np] = acc;
      HIPCHK(hipMemcpyAsync(c.seg_begin, sb, (np + 1) * 8, hipMemcpyHostToDevice, st));
    }
  }
  if (c.card_out && np) HIPCHK(hipMemsetAsync(c.pcard, 0, np * 8, st));
  return RB_OK;
}

// the segment count ns: from the host CSR, the identity, or the count kernel, its scan and a read-back
int count_segments(PairCall &c) {
  rbgpu_ctx *ctx = c.ctx;
  const rbgpu_set *a = c.a, *b = c.b;
  const uint64_t np = c.np;
  hipStream_t st = c.st;
  c.pa = PairArgs{c.op, a->view(), b->view(), c.d_aidx, c.d_bidx, c.npairs, c.seg_begin, nullptr, 0, c.seg_keys,
                  c.o.inplace, a == b, a->nc, b->nc};
  uint64_t *const tot = ctx->h_pinned;
  // one segment per pair when no pair can exceed seg_keys merged keys (config 2: <= 8 keys per
  // pair): seg_begin is the identity and the count kernel, its scan and the read-back are skipped
  c.ident_segs = !c.host_segs && np && !c.a_idx && !c.b_idx && !ensure_max_keys(a) && !ensure_max_keys(b) &&
                 (uint64_t)(a->max_keys + b->max_keys) <= c.seg_keys;
  if (c.host_segs) {
    c.ns = reinterpret_cast<const uint64_t *>(ctx->h_stage +
                                              np * 4 * ((c.d_aidx != nullptr) + (c.d_bidx != nullptr)))[np];
  } else if (c.ident_segs) {
    c.ns = np;
  } else {
    launch_seg_count(c.pa, c.nseg_p, st);
    scan_exclusive(c.nseg_p, c.seg_begin, np, c.ptmp, st);
    HIPCHK(hipMemcpyAsync(tot + 6, c.seg_begin + np, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    LAUNCHCHK();
    c.ns = np ? tot[6] : 0;
  }
  return RB_OK;
}

// ---- per segment: counts, block totals and their scans, result counts / offsets
int scan_segments(PairCall &c) {
  rbgpu_ctx *ctx = c.ctx;
  const uint64_t ns = c.ns;
  hipStream_t st = c.st;
  const uint64_t nblk = c.nblk = pair_blocks(ns);
  const size_t need = aligned256(ns * 4) + 3 * aligned256((ns + 1) * 8) + 10 * aligned256((nblk + 1) * 8) + 4 * 256;
  Workspace &G = ctx->ws_segs;
  if (G.reserve(need, st) != hipSuccess) return fail(RB_ENOMEM, "segment workspace");
  c.seg_pair = G.take<uint32_t>(std::max<uint64_t>(ns, 1));
  c.cnt = G.take<uint64_t>(ns + 1);
  c.bt = PairCountArrays{G.take<uint64_t>(nblk + 1), G.take<uint64_t>(nblk + 1), G.take<uint64_t>(nblk + 1),
                         G.take<uint64_t>(nblk + 1)};
  c.bs = PairCountArrays{G.take<uint64_t>(nblk + 1), G.take<uint64_t>(nblk + 1), G.take<uint64_t>(nblk + 1),
                         G.take<uint64_t>(nblk + 1)};
  c.task_begin = G.take<uint64_t>(ns + 1), c.rseg = G.take<uint64_t>(ns + 1);
  c.bk = G.take<uint64_t>(nblk + 1), c.bks = G.take<uint64_t>(nblk + 1);
  c.d_tot = G.take<uint64_t>(4);
  // one segment per pair: no segment maps at all (the kernels take segment p as pair p)
  if (!c.ident_segs) launch_seg_fill(c.pa, c.seg_begin, c.seg_pair, st);
  c.pa.seg_pair = c.ident_segs ? nullptr : c.seg_pair;
  c.pa.nseg = ns;
  launch_pair_count(c.pa, c.cnt, c.bt, ctx->d_stats, st);
  if (ns) {
    const uint64_t *scan_in[4] = {c.bt.task, c.bt.light, c.bt.big, c.bt.small};
    uint64_t *scan_out[4] = {c.bs.task, c.bs.light, c.bs.big, c.bs.small};
    scan_blocks_multi(scan_in, scan_out, 4, nblk, c.d_tot, st);
  }
  HIPCHK(hipMemcpyAsync(ctx->h_pinned, c.d_tot, 4 * 8, hipMemcpyDeviceToHost, st));
  return RB_OK;
}

// one record array (the light records, then the heavy ones) and the per-task metadata, for nt tasks
int take_tasks(PairCall &c, uint64_t nt) {
  const uint64_t nt1 = std::max<uint64_t>(nt, 1);
  const size_t tneed = aligned256(nt1 * sizeof(TaskRec)) + aligned256(nt1) + 2 * aligned256(nt1 * 8) +
                       aligned256(kQueueWords * 8) + 256;
  Workspace &T = c.ctx->ws_tasks;
  if (T.reserve(tneed, c.st) != hipSuccess) return fail(RB_ENOMEM, "task workspace (%llu tasks)", (unsigned long long)nt);
  c.light = T.take<TaskRec>(nt1);
  c.tm.type = T.take<uint8_t>(nt1);
  c.tm.res = T.take<uint64_t>(nt1);
  c.tm.slot = T.take<uint64_t>(nt1);
  c.queue = T.take<unsigned long long>(kQueueWords); // light-task chunk counters (<= 32, 128 B apart)
  return RB_OK;
}

// The task totals on the host, the task records (emitted early, or late behind ev[1]'s predecessor) and the result.
// Early emission: with identity pairing every container of A and of B takes at most one task, so
// a.nc + b.nc bounds the task count before the totals are on the host.  The task workspace is then
// sized by that bound and the emit kernel reads the totals on the device: it runs while the host
// waits for the totals, allocates the result and launches the task kernels.  Otherwise the host
// reads the totals first (the bound is the segments' key capacity, too loose to reserve).
// light tasks come from a shared chunk queue (a second light launch takes over the heavy kernel's
// CUs when it finishes)
int emit_tasks(PairCall &c) {
  rbgpu_ctx *ctx = c.ctx;
  const rbgpu_set *a = c.a, *b = c.b;
  hipStream_t st = c.st;
  uint64_t *const tot = ctx->h_pinned;
  int rc;
  const uint64_t seg_cap = c.ns * (uint64_t)c.seg_keys;
  c.tbound = !c.d_aidx && !c.d_bidx ? std::min<uint64_t>(a->nc + b->nc, seg_cap) : seg_cap;
  c.early = !c.o.probe && c.ns && c.tbound <= kEarlyEmitTasks;
  c.tm.lazy = is_lazy_op(c.op) ? c.op : 0;
  c.tm.inplace = c.o.inplace;
  c.tm.keep_empty = c.o.keep_empty;
  if (c.early) {
    if ((rc = take_tasks(c, c.tbound))) return rc;
    HIPCHK(hipEventRecord(ctx->ev_tot, st));
    launch_pair_emit(c.pa, c.cnt, c.bs, 0, c.light, nullptr, c.tm, c.task_begin, c.d_tot, c.tbound, c.queue, st);
    HIPCHK(hipEventSynchronize(ctx->ev_tot));
  } else {
    HIPCHK(hipStreamSynchronize(st));
  }
  LAUNCHCHK();
  if (!c.ns) tot[0] = tot[1] = tot[2] = tot[3] = 0;
  c.ntasks = tot[0], c.nlight = tot[1], c.nheavy = c.ntasks - c.nlight;
  const uint64_t nbig_t = tot[2], small_t = tot[3];
  c.small_base = nbig_t * kBitmapBytes;
  c.arena = c.card_only ? 0 : c.small_base + small_t;
  if (c.arena >= kSlotOffsetLimit) { // a task slot holds 40-bit arena offsets
    (void)hipStreamSynchronize(st);
    return fail(RB_ENOMEM, "pairwise: result arena of %llu bytes", (unsigned long long)c.arena);
  }
  if (c.early && c.ntasks > c.tbound) { // never expected: the emit dropped the records past the bound
    (void)hipStreamSynchronize(st);
    return fail(RB_EDEVICE, "pairwise: %llu tasks exceed the bound %llu", (unsigned long long)c.ntasks,
                (unsigned long long)c.tbound);
  }
  if (!c.early && (rc = take_tasks(c, c.ntasks))) return rc;
  c.heavy = c.light + c.nlight;
  if (!c.card_only && (rc = make_set(ctx, c.npairs, c.ntasks, c.arena, c.res))) {
    (void)hipStreamSynchronize(st); // the early emit may still write the workspace
    return rc;
  }
  // the light and heavy task kernels run concurrently (heavy on the side stream, 1 block per CU;
  // light 2 blocks per CU: 2 x 128 + 256 VGPRs per SIMD)
  c.conc = !c.o.probe && c.nlight && c.nheavy &&
           c.nlight + c.nheavy >= 65536; // small batches: the cross-stream waits cost more than the overlap
  // the emit zeroes the queue counters before ev[1]: the side stream waits on ev[1] before its light launch
  if (!c.early)
    launch_pair_emit(c.pa, c.cnt, c.bs, c.small_base, c.light, c.heavy, c.tm, c.task_begin, nullptr, 0, c.queue, st);
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  return RB_OK;
}

// the measurement probes in place of the task kernels; the call ends here
int run_probe(PairCall &c) {
  rbgpu_ctx *ctx = c.ctx;
  const rbgpu_set *a = c.a, *b = c.b;
  hipStream_t st = c.st;
  const int probe = c.o.probe;
  {
    Scratch w(ctx->pool);
    uint32_t *sink = nullptr;
    const unsigned blocks = 256 * 4;
    if (!w.get(sink, blocks * 256ull)) return fail(RB_ENOMEM, "probe sink");
    launch_probe(c.op, probe, a->payload, b->payload, a->payload_bytes, c.light, c.nlight, sink, blocks, st);
    if (probe == 1) launch_probe(c.op, probe, a->payload, b->payload, 0, c.heavy, c.nheavy, sink, blocks, st);
    HIPCHK(hipEventRecord(ctx->ev[2], st));
    HIPCHK(hipStreamSynchronize(st));
    LAUNCHCHK();
  }
  c.res.reset();
  const KernelSpan spans[1] = {{probe == 1 ? "k_probe_tasks" : "k_probe_stream", 6, -1, c.ntasks}};
  const int rc = stats_end(ctx, c.ntasks, 0, spans, 1);
  if (probe == 2) ctx->last.main_kernel_bytes = ctx->last.kernel_bytes[0] = a->payload_bytes / 8192 * 8192;
  return rc;
}

int run_tasks(PairCall &c) {
  rbgpu_ctx *ctx = c.ctx;
  hipStream_t st = c.st;
  uint8_t *arena = c.res ? c.res->payload : nullptr;
  if (c.conc) {
    HIPCHK(hipStreamWaitEvent(ctx->side, ctx->ev[1], 0));
    launch_pairwise_concurrent(c.kop, c.card_only, c.a->payload, c.b->payload, c.light, c.nlight, c.heavy, c.nheavy,
                               arena, c.tm, st, ctx->side, ctx->ev[2], ctx->ev_side[0], ctx->ev_side[1], c.queue);
    HIPCHK(hipEventRecord(ctx->ev_side[2], ctx->side));
    HIPCHK(hipStreamWaitEvent(st, ctx->ev_side[2], 0));
  } else {
    launch_pairwise(c.kop, c.card_only, c.a->payload, c.b->payload, c.light, c.nlight, c.heavy, c.nheavy, arena, c.tm,
                    st, ctx->ev[2]);
  }
  HIPCHK(hipEventRecord(ctx->ev[3], st));
  return RB_OK;
}

int compact_results(PairCall &c) {
  rbgpu_ctx *ctx = c.ctx;
  hipStream_t st = c.st;
  rbgpu_set *res = c.res.get();
  const uint64_t np = c.np, ns = c.ns;
  int rc;
  launch_compact_count(c.task_begin, ns, c.tm.type, c.bk, st);
  // the block totals' scan total is the result container count: stats word 8, read back with the
  // counters by stats_end
  if (ns) {
    const uint64_t *kin[1] = {c.bk};
    uint64_t *kout[1] = {c.bks};
    scan_blocks_multi(kin, kout, 1, c.nblk, ctx->d_stats + 8 * kStripes, st);
  }
  OutView ov{};
  if (res) ov = OutView{res->key, res->type, res->card, res->nruns, res->off};
  // one segment per pair: the compaction writes the result CSR itself; else per segment, mapped below
  uint64_t *rb_direct = res && c.ident_segs ? res->begin : nullptr;
  // RBGPU_CALL_TAIL=1: a synchronous call whose compaction is its last kernel returns on that kernel's tail
  // (CallTail): the last block hands the summed counters to host-visible words, so no counters copy, memset or
  // stream wait.  Off by default: measured slower on config 2 (4.384 vs 4.333 ms per AND step, three interleaved
  // pairs, profiles/r06/tail) — the host phase did not shrink and the next call's light kernel ran ~35 us longer.
  const char *ct = getenv("RBGPU_CALL_TAIL"); // the parity test runs both forms
  c.tailed = ct && ct[0] == '1' && c.slot < 0 && res && c.ident_segs && !c.card_out && ns;
  if (c.tailed) {
    if ((rc = ensure_call_words(ctx)) || (rc = seq_begin(ctx))) {
      (void)hipStreamSynchronize(st);
      return rc;
    }
    c.tail = CallTail{ctx->d_small_ctr + 48, reinterpret_cast<uint64_t *>(ctx->d_small) + kTailWord, ++ctx->small_seq};
  }
  launch_compact_write(c.task_begin, ns, c.tm, c.bks, ov, c.pa.seg_pair, c.card_out ? c.pcard : nullptr, ctx->d_stats,
                       res && !c.ident_segs ? c.rseg : nullptr, rb_direct, st, c.tail);
  if (res && np && !c.ident_segs) launch_pair_rbegin(c.seg_begin, c.npairs, c.rseg, res->begin, nullptr, st);
  else if (res && !np) HIPCHK(hipMemsetAsync(res->begin, 0, 8, st));
  if (c.card_out && np) HIPCHK(hipMemcpyAsync(c.card_out, c.pcard, np * 8, hipMemcpyDeviceToHost, st));
  return RB_OK;
}

// asynchronous: the result count (stats word 8, written by the compaction's scan) into the pinned slot, the
// counters zeroed for the next call, and the completion event the result settles on
int finish_async(PairCall &c) {
  rbgpu_ctx *ctx = c.ctx;
  hipStream_t st = c.st;
  const int prc = c.np ? (hipMemcpyAsync(ctx->h_async + c.slot, ctx->d_stats + 8 * kStripes, 8, hipMemcpyDeviceToHost, st)
                              ? RB_EDEVICE : RB_OK)
                       : (ctx->h_async[c.slot] = 0, RB_OK);
  hipEvent_t done = nullptr;
  if (prc || hipMemsetAsync(ctx->d_stats, 0, kStatWords * kStripes * sizeof(uint64_t), st) ||
      hipEventCreateWithFlags(&done, hipEventDisableTiming) || hipEventRecord(done, st) ||
      (c.o.ext && hipStreamWaitEvent(c.o.ext, done, 0)) ||
      hipGetLastError()) {
    if (done) (void)hipEventDestroy(done);
    (void)hipStreamSynchronize(st);
    return fail(RB_EDEVICE, "asynchronous pairwise: enqueue failed");
  }
  // the inputs stay allocated until the call is done with them: set_release waits for this
  for (const rbgpu_set *in : {c.a, c.b}) {
    rbgpu_set *m = const_cast<rbgpu_set *>(in);
    if ((!m->read_done && hipEventCreateWithFlags(&m->read_done, hipEventDisableTiming)) ||
        hipEventRecord(m->read_done, st)) {
      (void)hipStreamSynchronize(st);
      c.res->pending = done;
      c.res->pend_slot = c.slot;
      c.slot = -1;
      c.res.reset();
      return fail(RB_EDEVICE, "asynchronous pairwise: enqueue failed");
    }
  }
  ctx->stats_clean = true;
  c.res->pending = done;
  c.res->pend_slot = c.slot;
  c.slot = -1; // the result owns it now
  *c.out = c.res.release();
  return RB_OK;
}

// synchronous: the counters back through stats_end, or through the compaction's tail (RBGPU_CALL_TAIL)
int finish_sync(PairCall &c) {
  rbgpu_ctx *ctx = c.ctx;
  const uint64_t ntasks = c.ntasks, nlight = c.nlight, nheavy = c.nheavy;
  int rc;
  KernelSpan spans[3] = {{"k_pair_tasks<light>", 2, 4, nlight}, {"k_pair_tasks<heavy>", 3, 5, nheavy}, {"", -1, -1, 0}};
  int nspans = 2;
  if (c.conc) { // [0] the concurrent task phase (both kernels' bytes over the union of their spans), then each
    spans[0] = KernelSpan{"k_pair_tasks<light>||<heavy>", 2, 4, ntasks, ctx->ev[1], ctx->ev[3], 3, 5};
    spans[1] = KernelSpan{"k_pair_tasks<light>", 2, 4, nlight, ctx->ev[1], ctx->ev[2]};
    spans[2] = KernelSpan{"k_pair_tasks<heavy>", 3, 5, nheavy, ctx->ev_side[0], ctx->ev_side[1]};
    nspans = 3;
  }
  if (c.tailed) {
    HIPCHK(hipEventRecord(ctx->ev[5], c.st));
    bool seen = false;
    if ((rc = seq_end(ctx, c.tail.seq, true, "pairwise compaction", &seen, kTailWord + kStatWords))) return rc;
    const uint64_t *hw = reinterpret_cast<const uint64_t *>(ctx->h_small) + kTailWord;
    for (int i = 0; i < kStatWords; ++i) ctx->words[i] = hw[i];
    ctx->stats_clean = true; // the tail zeroed the counters
    rc = stats_fill(ctx, ntasks, 0, spans, nspans, !seen);
    if (seen) { // the kernel times when the stats are asked for (rbgpu_get_stats)
      ctx->stats_pending = true;
      ctx->stats_pending_k = false;
      for (int i = 0; i < nspans; ++i) ctx->pend_spans[i] = spans[i];
      ctx->pend_n = nspans;
      ctx->pend_tasks = ntasks;
      c.res->end_seq = c.tail.seq;
    }
  } else {
    rc = stats_end(ctx, ntasks, 0, spans, nspans);
  }
  if (rc) return rc;
  const uint64_t nres = c.np ? ctx->words[8] : 0;
  ctx->last.result_containers = nres;
  if (c.res) {
    c.res->nc = nres;
    *c.out = c.res.release();
  }
  if (c.o.ext) { // the caller's later work on its stream comes after this call's
    HIPCHK(hipEventRecord(ctx->ev_ext, ctx->stream));
    HIPCHK(hipStreamWaitEvent(c.o.ext, ctx->ev_ext, 0));
  }
  return RB_OK;
}
} // namespace

namespace rbg {
int pairwise_impl(rbgpu_ctx *ctx, int op, const rbgpu_set *a, const rbgpu_set *b, const uint32_t *a_idx,
                  const uint32_t *b_idx, uint32_t npairs, rbgpu_set **out, uint64_t *card_out, const PairOpts &o) {
  int rc = check_ctx(ctx);
  if (rc) return rc;
  PairCall c{ctx, op, a, b, a_idx, b_idx, npairs, out, card_out, o};
  if ((rc = check_pair_args(c))) return rc;
  hipStream_t &ext = c.o.ext;
  if (ext == ctx->stream) ext = nullptr;
  if (ext) { // the caller's earlier work on its stream comes first
    HIPCHK(hipEventRecord(ctx->ev_ext, ext));
    HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_ext, 0));
  }
  if (!o.probe) { // small batches complete before the return, asynchronous call or not
    rc = pairwise_small(ctx, op, a, b, a_idx, b_idx, npairs, out, card_out, o.inplace, o.keep_empty);
    if (rc == RB_OK && ext) {
      // the host returned on the last block's sequence word, before the kernel's end (and its L2 write-back):
      // the caller's later work on its stream waits for that end, as after the general path below
      HIPCHK(hipEventRecord(ctx->ev_ext, ctx->stream));
      HIPCHK(hipStreamWaitEvent(ext, ctx->ev_ext, 0));
    }
    if (rc != 1) return rc;
  }
  struct SlotGuard { // an error return gives the slot back
    rbgpu_ctx *c;
    int &slot;
    ~SlotGuard() {
      if (slot >= 0) c->async_free.push_back(slot);
    }
  } slot_guard{ctx, c.slot};
  if (o.async && out && (rc = take_async_slot(c))) return rc;
  c.card_only = out == nullptr;
  c.kop = is_lazy_op(op) ? (int)RB_OR : op;
  c.st = ctx->stream;
  c.np = npairs;
  if ((rc = stage_pairs(c))) return rc;
  stats_begin(ctx);
  if ((rc = count_segments(c)) || (rc = scan_segments(c)) || (rc = emit_tasks(c))) return rc;
  if (o.probe) return run_probe(c);
  if ((rc = run_tasks(c)) || (rc = compact_results(c))) return rc;
  return c.slot >= 0 ? finish_async(c) : finish_sync(c);
}
} // namespace rbg

static double us_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}

extern "C" {

int rbgpu_pairwise(rbgpu_ctx *ctx, int op, const rbgpu_set *a, const rbgpu_set *b, const uint32_t *a_idx,
                   const uint32_t *b_idx, uint32_t npairs, rbgpu_set **out) {
  SETTLE(a, b);
  const auto t0 = std::chrono::steady_clock::now();
  if (!out) return fail(RB_EINVAL, "null out");
  *out = nullptr;
  const int rc = pairwise_impl(ctx, op, a, b, a_idx, b_idx, npairs, out, nullptr, PairOpts{});
  if (!rc) ctx->last.call_us = us_since(t0);
  return rc;
}

int rbgpu_pairwise_async(rbgpu_ctx *ctx, int op, const rbgpu_set *a, const rbgpu_set *b, const uint32_t *a_idx,
                         const uint32_t *b_idx, uint32_t npairs, void *stream, rbgpu_set **out) {
  SETTLE(a, b);
  if (!out) return fail(RB_EINVAL, "null out");
  *out = nullptr;
  PairOpts o;
  o.async = true;
  o.ext = reinterpret_cast<hipStream_t>(stream);
  return pairwise_impl(ctx, op, a, b, a_idx, b_idx, npairs, out, nullptr, o);
}

int rbgpu_pairwise_cardinality(rbgpu_ctx *ctx, int op, const rbgpu_set *a, const rbgpu_set *b, const uint32_t *a_idx,
                               const uint32_t *b_idx, uint32_t npairs, uint64_t *out) {
  SETTLE(a, b);
  const auto t0 = std::chrono::steady_clock::now();
  if (!out && npairs) return fail(RB_EINVAL, "null out");
  const int rc = pairwise_impl(ctx, op, a, b, a_idx, b_idx, npairs, nullptr, out, PairOpts{});
  if (!rc) ctx->last.call_us = us_since(t0);
  return rc;
}

int rbgpu_pairwise_inplace(rbgpu_ctx *ctx, int op, const rbgpu_set *a, const rbgpu_set *b, const uint32_t *a_idx,
                           const uint32_t *b_idx, uint32_t npairs, rbgpu_set **out) {
  SETTLE(a, b);
  const auto t0 = std::chrono::steady_clock::now();
  if (!out) return fail(RB_EINVAL, "null out");
  *out = nullptr;
  if (op < RB_AND || op > RB_ANDNOT) return fail(RB_EINVAL, "bad op %d", op);
  PairOpts o;
  o.inplace = true;
  const int rc = pairwise_impl(ctx, op, a, b, a_idx, b_idx, npairs, out, nullptr, o);
  if (!rc) ctx->last.call_us = us_since(t0);
  return rc;
}

// Measurement hook (not part of rbgpu.h): runs the pairwise setup, then a read-only probe kernel
// in place of the task kernel (mode 1: the task kernel's payload loads; 2: a streaming read of
// a's arena).  The probe's time is in rbgpu_get_stats().main_kernel_ms.
int rbgpu_internal_probe(rbgpu_ctx *ctx, int op, const rbgpu_set *a, const rbgpu_set *b, uint32_t npairs, int mode) {
  SETTLE(a, b);
  if (mode != 1 && mode != 2) return fail(RB_EINVAL, "probe mode");
  rbgpu_set *res = nullptr;
  PairOpts o;
  o.probe = mode;
  return pairwise_impl(ctx, op, a, b, nullptr, nullptr, npairs, &res, nullptr, o);
}

// Test hook (not part of rbgpu.h): pool blocks handed out and not yet released (DevPool::outstanding).  With every
// set freed it is back at its reading after rbgpu_open: anything else is a leak or a double release.
int64_t rbgpu_internal_pool_outstanding(rbgpu_ctx *ctx) { return ctx ? ctx->pool.outstanding : -1; }

} // extern "C"
namespace rbg {
int pairwise_call(rbgpu_ctx *ctx, int op, const rbgpu_set *a, const rbgpu_set *b, const uint32_t *a_idx,
                  const uint32_t *b_idx, uint32_t npairs, rbgpu_set **out, bool inplace, bool keep_empty) {
  *out = nullptr;
  PairOpts o;
  o.inplace = inplace;
  o.keep_empty = keep_empty;
  return pairwise_impl(ctx, op, a, b, a_idx, b_idx, npairs, out, nullptr, o);
}
} // namespace rbg
