// context.hip — the context's lifetime, the last error, call accounting (stats_*) and the one-launch sequence
// protocol (seq_*) of librbgpu (include/rbgpu.h).
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
thread_local std::string g_err;
} // namespace

namespace rbg {
int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
int check_ctx(rbgpu_ctx *ctx) {
  if (!ctx) return fail(RB_EINVAL, "null context");
  HIPCHK(hipSetDevice(ctx->device));
  (void)hipGetLastError(); // LAUNCHCHK reports only what this call launches
  return RB_OK;
}
// through pinned staging: a pageable copy would block the host
int ensure_stage(rbgpu_ctx *ctx, size_t bytes) {
  if (bytes <= ctx->h_stage_cap) return RB_OK;
  if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
  ctx->h_stage = nullptr;
  ctx->h_stage_cap = 0;
  if (hipHostMalloc((void **)&ctx->h_stage, bytes) != hipSuccess) return fail(RB_ENOMEM, "pinned staging");
  ctx->h_stage_cap = bytes;
  return RB_OK;
}
void ctx_unref(rbgpu_ctx *ctx) {
  if (--ctx->refs > 0) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->side) (void)hipStreamSynchronize(ctx->side);
  for (auto &e : ctx->ev) (void)hipEventDestroy(e);
  for (auto &e : ctx->ev_side) (void)hipEventDestroy(e);
  (void)hipEventDestroy(ctx->ev_tot);
  if (ctx->ev_ext) (void)hipEventDestroy(ctx->ev_ext);
  (void)hipFree(ctx->d_stats);
  (void)hipHostFree(ctx->h_pinned);
  (void)hipHostFree(ctx->h_stats);
  if (ctx->h_async) (void)hipHostFree(ctx->h_async);
  if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
  if (ctx->h_small) (void)hipHostFree(ctx->h_small);
  if (ctx->d_small_ctr) (void)hipFree(ctx->d_small_ctr);
  if (ctx->d_small_slots) (void)hipFree(ctx->d_small_slots);
  ctx->pool.clear();
  ctx->ws_pairs.destroy();
  ctx->ws_tasks.destroy();
  ctx->ws_segs.destroy();
  (void)hipStreamDestroy(ctx->stream);
  if (ctx->side) (void)hipStreamDestroy(ctx->side);
  delete ctx;
}
// The counters are zeroed right behind their read-back in stats_end (the memset runs while the host
// waits anyway), so the next call starts its kernels without one; a call that did not reach
// stats_end leaves them dirty and the next stats_begin zeroes them.
void stats_begin(rbgpu_ctx *ctx, bool zero) {
  ctx->stats_pending = false;
  if (zero && !ctx->stats_clean)
    (void)hipMemsetAsync(ctx->d_stats, 0, kStatWords * kStripes * sizeof(uint64_t), ctx->stream);
  ctx->stats_clean = false;
  (void)hipEventRecord(ctx->ev[0], ctx->stream);
}
int stats_end(rbgpu_ctx *ctx, uint64_t tasks, uint64_t result_containers, const KernelSpan *k, int n,
              const uint64_t *d_src) {
  HIPCHK(hipEventRecord(ctx->ev[5], ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->h_stats, d_src ? d_src : ctx->d_stats, kStatWords * kStripes * sizeof(uint64_t),
                        hipMemcpyDeviceToHost, ctx->stream));
  if (!d_src) HIPCHK(hipMemsetAsync(ctx->d_stats, 0, kStatWords * kStripes * sizeof(uint64_t), ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  LAUNCHCHK();
  if (!d_src) ctx->stats_clean = true;
  uint64_t *w = ctx->words;
  for (int i = 0; i < kStatWords; ++i) {
    w[i] = 0;
    for (int j = 0; j < kStripes; ++j) w[i] += ctx->h_stats[i * kStripes + j];
  }
  return stats_fill(ctx, tasks, result_containers, k, n);
}
int stats_fill(rbgpu_ctx *ctx, uint64_t tasks, uint64_t result_containers, const KernelSpan *k, int n, bool timed) {
  ctx->stats_pending = false;
  ctx->pend_n = 0;
  const uint64_t *w = ctx->words;
  rb_stats &s = ctx->last;
  s = rb_stats{};
  s.tasks = tasks;
  s.input_bytes = w[0];
  s.output_bytes = w[1];
  s.result_cardinality = w[7];
  s.result_containers = result_containers;
  float ms = 0;
  s.total_ms = timed && hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[5]) == hipSuccess ? ms : 0.0;
  s.n_kernels = (uint32_t)std::min(n, 4);
  int best = -1;
  for (int i = 0; i < (int)s.n_kernels; ++i) {
    std::snprintf(s.kernel_name[i], sizeof s.kernel_name[i], "%s", k[i].name);
    hipEvent_t e0 = k[i].e0 ? k[i].e0 : ctx->ev[1 + i], e1 = k[i].e1 ? k[i].e1 : ctx->ev[2 + i];
    s.kernel_ms[i] = timed && hipEventElapsedTime(&ms, e0, e1) == hipSuccess ? ms : 0.0;
    s.kernel_bytes[i] = (k[i].in_word >= 0 ? w[k[i].in_word] : 0) + (k[i].out_word >= 0 ? w[k[i].out_word] : 0) +
                        (k[i].in2 >= 0 ? w[k[i].in2] : 0) + (k[i].out2 >= 0 ? w[k[i].out2] : 0);
    s.kernel_items[i] = k[i].items;
    if (best < 0 || s.kernel_ms[i] > s.kernel_ms[best]) best = i;
  }
  if (best >= 0) {
    s.main_kernel_ms = s.kernel_ms[best];
    s.main_kernel_bytes = s.kernel_bytes[best];
    std::snprintf(s.main_kernel, sizeof s.main_kernel, "%s", s.kernel_name[best]);
  }
  return RB_OK;
}
// Host-visible result words a one-launch call's last block writes (8 words: [5] = the call's sequence
// number, written last) and the device counters it resets (pairwise_small, the fused BSI compare).
int ensure_call_words(rbgpu_ctx *ctx) {
  if (!ctx->h_small) {
    if (hipHostMalloc((void **)&ctx->h_small, 256, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
      return fail(RB_ENOMEM, "host-visible result words");
    if (hipHostGetDevicePointer((void **)&ctx->d_small, ctx->h_small, 0) != hipSuccess) {
      (void)hipHostFree(ctx->h_small);
      ctx->h_small = nullptr;
      return fail(RB_EDEVICE, "host-visible result words have no device address");
    }
  }
  if (!ctx->d_small_ctr) { // block tickets and counters of the one-launch kernels; each call's last block resets its own
    if (hipMalloc((void **)&ctx->d_small_ctr, 512) != hipSuccess) return fail(RB_ENOMEM, "block counters");
    if (hipMemset(ctx->d_small_ctr, 0, 512) != hipSuccess) return fail(RB_EDEVICE, "block counters");
  }
  if (!ctx->d_small_slots) { // every word kSlotUnset (all ones) between calls: each call's compaction resets its own
    if (hipMalloc((void **)&ctx->d_small_slots, 16ull * kSmallSlots) != hipSuccess) return fail(RB_ENOMEM, "slot words");
    if (hipMemset(ctx->d_small_slots, 0xFF, 16ull * kSmallSlots) != hipSuccess) return fail(RB_EDEVICE, "slot words");
  }
  return RB_OK;
}
// Spins (bounded) until the call's last block has written `seq` after its result words: the host returns
// without waiting for the kernel's end to be signalled (it has no work left by then, and later calls on the
// stream are ordered behind it).  false: not seen in time — the caller waits for the stream, which also
// reports a fault.
bool wait_call_seq(rbgpu_ctx *ctx, uint64_t seq, int word) {
  const volatile uint64_t *flag = reinterpret_cast<const volatile uint64_t *>(ctx->h_small) + word;
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t it = 0;; ++it) {
    if (__atomic_load_n(const_cast<const uint64_t *>(flag), __ATOMIC_ACQUIRE) == seq) return true;
    if ((it & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) return false;
  }
}
int seq_begin(rbgpu_ctx *ctx) {
  if (ctx->seq_settled >= ctx->seq_recorded) return RB_OK;
  const hipError_t q = hipEventQuery(ctx->ev[5]);
  if (q == hipSuccess) {
    ctx->seq_settled = ctx->seq_recorded;
    return RB_OK;
  }
  if (q == hipErrorNotReady) return RB_OK; // still running: this call's work queues behind it
  (void)hipGetLastError();
  return fail(RB_EDEVICE, "an earlier one-launch call's kernel failed after the call returned: %s", hipGetErrorString(q));
}
int seq_end(rbgpu_ctx *ctx, uint64_t seq, bool poll, const char *what, bool *seen, int word) {
  *seen = false;
  ctx->seq_recorded = seq; // ctx->ev[5], recorded by the caller behind the kernel, marks its end
  const bool s = poll && wait_call_seq(ctx, seq, word);
  const hipError_t e1 = s ? hipSuccess : hipStreamSynchronize(ctx->stream), e2 = hipGetLastError();
  if (e1 != hipSuccess || e2 != hipSuccess)
    return fail(RB_EDEVICE, "%s kernel failed: %s", what, hipGetErrorString(e1 != hipSuccess ? e1 : e2));
  if (!s) {
    ctx->seq_settled = seq;
    const uint64_t got = __atomic_load_n(reinterpret_cast<const uint64_t *>(ctx->h_small) + word, __ATOMIC_ACQUIRE);
    if (got != seq) { // no block saw itself last: the counters are not this call's, and nor are the words
      (void)hipMemsetAsync(ctx->d_small_ctr, 0, 512, ctx->stream);
      if (ctx->d_small_slots) (void)hipMemsetAsync(ctx->d_small_slots, 0xFF, 16ull * kSmallSlots, ctx->stream);
      (void)hipStreamSynchronize(ctx->stream);
      return fail(RB_EDEVICE, "%s: the kernel ended without handing over call %llu's result words (found %llu)", what,
                  (unsigned long long)seq, (unsigned long long)got);
    }
  }
  *seen = s;
  return RB_OK;
}
int seq_settle(rbgpu_ctx *ctx, uint64_t seq) {
  if (!seq || seq <= ctx->seq_settled) return RB_OK;
  const hipError_t e = hipEventSynchronize(ctx->ev[5]); // recorded behind call seq or a later one
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(RB_EDEVICE, "one-launch kernel failed: %s", hipGetErrorString(e));
  }
  ctx->seq_settled = ctx->seq_recorded;
  return RB_OK;
}
} // namespace rbg

// ===================================================================== C ABI
extern "C" {

const char *rbgpu_last_error(void) { return g_err.c_str(); }

int rbgpu_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int rbgpu_open(int device, rbgpu_ctx **out) {
  if (!out) return fail(RB_EINVAL, "null out");
  *out = nullptr;
  int n = rbgpu_device_count();
  if (device < 0 || device >= n) return fail(RB_EDEVICE, "no HIP device %d (found %d)", device, n);
  HIPCHK(hipSetDevice(device));
  rbgpu_ctx *c = new rbgpu_ctx;
  c->device = device;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc((void **)&c->d_stats, kStatWords * kStripes * sizeof(uint64_t)) != hipSuccess ||
      hipHostMalloc((void **)&c->h_stats, kStatWords * kStripes * sizeof(uint64_t)) != hipSuccess ||
      hipHostMalloc((void **)&c->h_pinned, 16 * sizeof(uint64_t)) != hipSuccess) {
    delete c;
    return fail(RB_EDEVICE, "context creation failed on device %d", device);
  }
  for (auto &e : c->ev) (void)hipEventCreate(&e);
  for (auto &e : c->ev_side) (void)hipEventCreate(&e);
  (void)hipEventCreate(&c->ev_tot);
  (void)hipEventCreateWithFlags(&c->ev_ext, hipEventDisableTiming);
  // every source file's code object now, not inside the first call of each kind: HIP loads a code object at
  // the first launch of one of its kernels (~1 ms each), which otherwise lands in that call's time and in a
  // set's first-use setup (rbgpu_set_setup_parts)
  for (auto w : {warm_pairwise, warm_scan, warm_wide, warm_wide_runs, warm_wide_xor, warm_bsi, warm_codec, warm_setops,
                 warm_generate, warm_values, warm_build, warm_range, warm_bsi_arith})
    w(c->stream);
  if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess) {
    rbgpu_close(c);
    return fail(RB_EDEVICE, "context creation failed on device %d (kernel load)", device);
  }
  *out = c;
  return RB_OK;
}

void rbgpu_close(rbgpu_ctx *ctx) {
  // sets still alive keep the context (stream, pool) alive until they are freed
  if (!ctx || ctx->closed) return;
  ctx->closed = true;
  ctx_unref(ctx);
}

int rbgpu_synchronize(rbgpu_ctx *ctx) {
  int rc = check_ctx(ctx);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  LAUNCHCHK();
  return RB_OK;
}

int rbgpu_get_stats(rbgpu_ctx *ctx, rb_stats *out) {
  if (!ctx || !out) return fail(RB_EINVAL, "null argument");
  if (ctx->stats_pending) { // a small batch returned before its end was signalled: its times now
    ctx->stats_pending = false;
    float ms = 0.f;
    const hipError_t e = hipEventSynchronize(ctx->ev[5]);
    if (e != hipSuccess) { // the kernel faulted after its last block handed the result over
      (void)hipGetLastError();
      return fail(RB_EDEVICE, "the last call's kernel failed after the call returned: %s", hipGetErrorString(e));
    }
    ctx->seq_settled = std::max(ctx->seq_settled, ctx->seq_recorded); // ev[5] follows the last one-launch kernel
    if (ctx->pend_n) { // a general-pipeline call's spans (CallTail): the same accounting as stats_end, now timed
      const rb_stats keep = ctx->last;
      KernelSpan spans[4];
      const int n = ctx->pend_n;
      for (int i = 0; i < n; ++i) spans[i] = ctx->pend_spans[i];
      (void)stats_fill(ctx, ctx->pend_tasks, keep.result_containers, spans, n, true);
      ctx->last.call_us = keep.call_us;
    } else {
      if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[5]) == hipSuccess) ctx->last.total_ms = ms;
      if (ctx->stats_pending_k && hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]) == hipSuccess)
        ctx->last.kernel_ms[0] = ctx->last.main_kernel_ms = ms;
    }
  }
  *out = ctx->last;
  return RB_OK;
}

} // extern "C"
