// set.hip — device-resident sets: allocation and release, derived metadata, upload / download, the metadata
// queries and the thin entry points of serialize, values, lookup and build (include/rbgpu.h).
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

namespace rbg {
int set_alloc(rbgpu_ctx *ctx, rbgpu_set *s, uint32_t nb, uint64_t nc, uint64_t payload) {
  s->ctx = ctx;
  ctx->refs++;
  s->nb = nb;
  s->nc = nc;
  s->payload_bytes = payload;
  DevPool &p = ctx->pool;
  const uint64_t ncap = std::max<uint64_t>(nc, 1);
  if (p.alloc((void **)&s->begin, (nb + 1) * sizeof(uint64_t)) != hipSuccess ||
      p.alloc((void **)&s->key, ncap * 2) != hipSuccess || p.alloc((void **)&s->type, ncap) != hipSuccess ||
      p.alloc((void **)&s->card, ncap * 4) != hipSuccess || p.alloc((void **)&s->nruns, ncap * 2) != hipSuccess ||
      p.alloc((void **)&s->off, ncap * 8) != hipSuccess ||
      p.alloc((void **)&s->payload, std::max<uint64_t>(payload, 16)) != hipSuccess) {
    // give back what was taken and the context reference: make_set only deletes s on failure
    set_release(s);
    return fail(RB_ENOMEM, "device allocation of a %u-bitmap / %llu-container set failed", nb,
                (unsigned long long)nc);
  }
  return RB_OK;
}
void set_release(rbgpu_set *s) {
  if (!s || !s->ctx) return;
  (void)settle(s); // an asynchronous result's kernels may still write its buffers
  if (s->read_done) { // ... and a pending call that takes this set as an input may still read them
    (void)hipEventSynchronize(s->read_done);
    (void)hipEventDestroy(s->read_done);
    s->read_done = nullptr;
  }
  DevPool &p = s->ctx->pool;
  p.release(s->begin);
  p.release(s->key);
  p.release(s->type);
  p.release(s->card);
  p.release(s->nruns);
  p.release(s->off);
  p.release(s->payload);
  p.release(s->mrec);
  p.release(s->krec);
  p.release(s->bsi_table);
  p.release(s->bsi_klist);
  p.release(s->cpre);
  rbgpu_ctx *ctx = s->ctx;
  s->ctx = nullptr;
  ctx_unref(ctx);
}
int make_set(rbgpu_ctx *ctx, uint32_t nb, uint64_t nc, uint64_t payload, SetPtr &out) {
  rbgpu_set *s = new rbgpu_set;
  const int rc = set_alloc(ctx, s, nb, nc, payload);
  if (rc) {
    delete s;
    return rc;
  }
  out.reset(s);
  return RB_OK;
}
int settle(const rbgpu_set *cs) {
  if (cs && cs->failed) return fail(RB_EDEVICE, "the asynchronous call that produced this set failed");
  if (!cs || !cs->pending) return RB_OK;
  rbgpu_set *s = const_cast<rbgpu_set *>(cs);
  rbgpu_ctx *ctx = s->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  const hipError_t e = hipEventSynchronize(s->pending);
  (void)hipEventDestroy(s->pending);
  s->pending = nullptr;
  // the slot is only read when the call completed; a failed call leaves the set failed (sticky), not a
  // set whose container count is whatever the pinned word held
  s->nc = e == hipSuccess ? ctx->h_async[s->pend_slot] : 0;
  ctx->async_free.push_back(s->pend_slot);
  s->pend_slot = -1;
  if (e != hipSuccess) {
    s->failed = true;
    return fail(RB_EDEVICE, "asynchronous call failed: %s", hipGetErrorString(e));
  }
  return RB_OK;
}
int ensure_h_begin(const rbgpu_set *cs) {
  rbgpu_set *s = const_cast<rbgpu_set *>(cs);
  if (s->h_begin.size() == (size_t)s->nb + 1) return RB_OK;
  s->h_begin.resize((size_t)s->nb + 1);
  HIPCHK(hipSetDevice(s->ctx->device));
  HIPCHK(hipMemcpyAsync(s->h_begin.data(), s->begin, (s->nb + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                        s->ctx->stream));
  HIPCHK(hipStreamSynchronize(s->ctx->stream));
  LAUNCHCHK();
  return RB_OK;
}
// One word reduced on the device (reduce(d, stream) launches the kernel on the zeroed word d) and read back.
template <class F> static int reduce_word(rbgpu_ctx *ctx, const char *what, uint64_t &m, const F &reduce) {
  HIPCHK(hipSetDevice(ctx->device));
  Scratch w(ctx->pool);
  uint64_t *d = nullptr;
  if (!w.get(d, 1)) return fail(RB_ENOMEM, "%s", what);
  HIPCHK(hipMemsetAsync(d, 0, 8, ctx->stream));
  reduce(d, ctx->stream);
  HIPCHK(hipMemcpyAsync(ctx->h_pinned + 7, d, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  LAUNCHCHK();
  m = ctx->h_pinned[7];
  return RB_OK;
}
// Sets are immutable, so the largest per-bitmap container count is computed once (host CSR if it
// is already here, else one reduction kernel + read-back) and cached.
int ensure_max_keys(const rbgpu_set *cs) {
  rbgpu_set *s = const_cast<rbgpu_set *>(cs);
  if (s->max_keys >= 0) return RB_OK;
  uint64_t m = 0;
  if (s->h_begin.size() == (size_t)s->nb + 1) {
    for (uint32_t i = 0; i < s->nb; ++i) m = std::max<uint64_t>(m, s->h_begin[i + 1] - s->h_begin[i]);
  } else if (s->nb) {
    const int rc = reduce_word(s->ctx, "max-keys word", m,
                               [&](uint64_t *d, hipStream_t st) { launch_max_span(s->begin, s->nb, d, st); });
    if (rc) return rc;
  }
  s->max_keys = (int64_t)m;
  return RB_OK;
}
int ensure_max_runs(const rbgpu_set *cs) {
  rbgpu_set *s = const_cast<rbgpu_set *>(cs);
  if (s->max_runs >= 0) return RB_OK;
  uint64_t m = 0;
  if (s->nc) {
    const int rc = reduce_word(s->ctx, "max-runs word", m, [&](uint64_t *d, hipStream_t st) {
      launch_max_runs(s->type, s->nruns, s->nc, d, st);
    });
    if (rc) return rc;
  }
  s->max_runs = (int64_t)m;
  return RB_OK;
}
int ensure_dense(const rbgpu_set *cs) {
  rbgpu_set *s = const_cast<rbgpu_set *>(cs);
  if (s->dense_lo != -2) return RB_OK;
  int rc = ensure_h_begin(s);
  if (rc) return rc;
  s->dense_lo = s->dense_hi = -1;
  if (!s->nb) return RB_OK;
  const uint64_t cnt = s->h_begin[1] - s->h_begin[0];
  if (!cnt) return RB_OK;
  for (uint32_t b = 1; b < s->nb; ++b)
    if (s->h_begin[b + 1] - s->h_begin[b] != cnt) return RB_OK;
  HIPCHK(hipSetDevice(s->ctx->device));
  uint16_t k0 = 0;
  Scratch w(s->ctx->pool);
  uint32_t *d = nullptr;
  if (!w.get(d, 1)) return fail(RB_ENOMEM, "dense-check word");
  hipStream_t st = s->ctx->stream;
  HIPCHK(hipMemcpyAsync(&k0, s->key + s->h_begin[0], 2, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  uint32_t bad = 1;
  if ((uint64_t)k0 + cnt <= 65536) {
    {
      DeriveTimer t(s, 0);
      HIPCHK(hipMemsetAsync(d, 0, 4, st));
      launch_dense_check(s->view(), s->nb, k0, (uint32_t)cnt, d, st);
    }
    HIPCHK(hipMemcpyAsync(&bad, d, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    LAUNCHCHK();
  }
  s->derive_bytes += 2ull * s->nc; // the keys
  s->part_bytes[0] += 2ull * s->nc;
  if (!bad) {
    s->dense_lo = k0;
    s->dense_hi = (int64_t)k0 + (int64_t)cnt;
  }
  return RB_OK;
}
int ensure_mrec(const rbgpu_set *cs) {
  rbgpu_set *s = const_cast<rbgpu_set *>(cs);
  if (s->mrec) return RB_OK;
  if (s->payload_bytes >= kRecMaxPayload) return fail(RB_EINVAL, "packed records hold 40-bit payload offsets");
  HIPCHK(hipSetDevice(s->ctx->device));
  Scratch w(s->ctx->pool);
  uint64_t *m = nullptr;
  if (!w.get(m, s->nc)) return fail(RB_ENOMEM, "packed records");
  {
    DeriveTimer t(s, 1);
    launch_pack_records(s->view(), s->nc, m, s->ctx->stream);
  }
  if (hipGetLastError() != hipSuccess) return fail(RB_EDEVICE, "packed-record kernel failed");
  s->mrec = w.keep(m);
  s->derive_bytes += 24ull * s->nc; // 16 B of metadata read, an 8-B record written per container
  s->part_bytes[1] += 24ull * s->nc;
  return RB_OK;
}
// naive_xor's key-major 4-B records of keys [a, b) into k (the set's whole dense range laid out from dense_lo).
// (Round 6 also built them in two key chunks on the side stream beside the first call's kernel: the build slowed
// the kernel beside it about as much as it hid, profiles/r06/xor/krec_overlap.)
// Member m's container at key x is begin[m] + x - dense_lo: the set's own device begin array, no host table
// copied up (a pageable 32 KiB copy cost ~0.8 ms inside the timed setup).  From mrec when the set already has it
// (12 B per container), else from the SoA itself (the run count and the offset, 10 B read, a 4-B record
// written: k_records_direct).  Returns the bytes it moves.
uint64_t build_krec_range(const rbgpu_set *s, uint32_t *k, uint32_t a, uint32_t b, hipStream_t st) {
  const SetView v = s->view();
  uint32_t *dst = k + (uint64_t)(a - (uint32_t)s->dense_lo) * s->nb;
  if (s->mrec) {
    launch_records_transpose(s->mrec, v.begin, (uint64_t)s->dense_lo, s->nb, a, b, dst, st);
    return 12ull * s->nb * (b - a);
  }
  // two containers per load: member m's first container begin[m] at an even index and the arrays aligned for it
  bool even_bases = !((uintptr_t)v.nruns & 3) && !((uintptr_t)v.off & 15) && !((a - (uint32_t)s->dense_lo) & 1);
  for (uint32_t m = 0; m < s->nb && even_bases; ++m) even_bases = !(s->h_begin[m] & 1);
  launch_records_direct(v, v.begin, (uint64_t)s->dense_lo, s->nb, a, b, dst, st, even_bases);
  return 14ull * s->nb * (b - a);
}
int ensure_krec(const rbgpu_set *cs) {
  rbgpu_set *s = const_cast<rbgpu_set *>(cs);
  if (s->krec) return RB_OK;
  int rc = ensure_dense(s);
  if (rc) return rc;
  if (s->dense_lo < 0) return fail(RB_EINVAL, "key-major records need a dense set");
  HIPCHK(hipSetDevice(s->ctx->device));
  Scratch w(s->ctx->pool);
  uint32_t *k = nullptr;
  if (!w.get(k, s->nc)) return fail(RB_ENOMEM, "key-major records");
  uint64_t bytes;
  {
    DeriveTimer t(s, 2);
    bytes = build_krec_range(s, k, (uint32_t)s->dense_lo, (uint32_t)s->dense_hi, s->ctx->stream);
  }
  if (hipGetLastError() != hipSuccess) return fail(RB_EDEVICE, "key-major record kernel failed");
  s->krec = w.keep(k);
  s->derive_bytes += bytes;
  s->part_bytes[2] += bytes;
  return RB_OK;
}
// Upload a validated host SoA, re-laid out: Bitmaps first (8 KiB aligned), then the rest (16 B).
int upload_host(rbgpu_ctx *ctx, const HostSoA &h, rbgpu_set **out) {
  const uint64_t nc = h.nc();
  std::vector<uint64_t> off(nc);
  uint64_t nbig = 0, small = 0;
  for (uint64_t i = 0; i < nc; ++i) {
    if (h.type[i] == RB_BITMAP) ++nbig;
    else small += round16(payload_bytes(h.type[i], h.card[i], h.nruns[i]));
  }
  uint64_t bi = 0, so = nbig * kBitmapBytes;
  for (uint64_t i = 0; i < nc; ++i) {
    if (h.type[i] == RB_BITMAP) off[i] = (bi++) * kBitmapBytes;
    else {
      off[i] = so;
      so += round16(payload_bytes(h.type[i], h.card[i], h.nruns[i]));
    }
  }
  const uint64_t total = nbig * kBitmapBytes + small;
  // a run count only on Run containers: workShyAnd's SoA reads and naive_xor's records take "nruns > 0" for
  // "a Run", so an Array / Bitmap entry's count (which the format ignores) is stored as 0
  std::vector<uint16_t> nruns(h.nruns.begin(), h.nruns.begin() + nc);
  for (uint64_t i = 0; i < nc; ++i)
    if (h.type[i] != RB_RUN) nruns[i] = 0;
  std::vector<uint8_t> staged(std::max<uint64_t>(total, 16), 0);
  for (uint64_t i = 0; i < nc; ++i)
    std::memcpy(staged.data() + off[i], h.payload.data() + h.off[i], payload_bytes(h.type[i], h.card[i], h.nruns[i]));
  SetPtr s;
  const int rc = make_set(ctx, h.nb, nc, total, s);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  auto cp = [&](void *dst, const void *src, size_t n) {
    return n ? hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st) : hipSuccess;
  };
  if (cp(s->begin, h.begin.data(), (h.nb + 1) * 8) || cp(s->key, h.key.data(), nc * 2) ||
      cp(s->type, h.type.data(), nc) || cp(s->card, h.card.data(), nc * 4) || cp(s->nruns, nruns.data(), nc * 2) ||
      cp(s->off, off.data(), nc * 8) || cp(s->payload, staged.data(), total) || hipStreamSynchronize(st))
    return fail(RB_EDEVICE, "host-to-device upload failed");
  s->h_begin = h.begin;
  *out = s.release();
  return RB_OK;
}

// Download bitmaps [first, first+count) into a HostSoA with compact 16-B aligned payloads.
int download_host(const rbgpu_set *s, uint32_t first, uint32_t count, HostSoA &h) {
  rbgpu_ctx *ctx = s->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  int rc = ensure_h_begin(s);
  if (rc) return rc;
  const uint64_t lo = s->h_begin[first], hi = s->h_begin[first + count], n = hi - lo;
  hipStream_t st = ctx->stream;
  h.nb = count;
  h.begin.resize(count + 1);
  for (uint32_t i = 0; i <= count; ++i) h.begin[i] = s->h_begin[first + i] - lo;
  h.key.resize(n);
  h.type.resize(n);
  h.card.resize(n);
  h.nruns.resize(n);
  h.off.resize(n);
  std::vector<uint64_t> soff(n);
  if (n) {
    HIPCHK(hipMemcpyAsync(h.key.data(), s->key + lo, n * 2, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h.type.data(), s->type + lo, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h.card.data(), s->card + lo, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h.nruns.data(), s->nruns + lo, n * 2, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(soff.data(), s->off + lo, n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    LAUNCHCHK();
  }
  std::vector<uint64_t> bytes(n);
  uint64_t total = 0;
  for (uint64_t i = 0; i < n; ++i) {
    bytes[i] = payload_bytes(h.type[i], h.card[i], h.nruns[i]);
    h.off[i] = total;
    total += round16(bytes[i]);
  }
  h.payload.assign(std::max<uint64_t>(total, 16), 0);
  if (n) {
    Scratch w(ctx->pool);
    uint64_t *d_soff, *d_doff, *d_bytes;
    uint8_t *d_stage;
    if (!w.get(d_soff, n) || !w.get(d_doff, n) || !w.get(d_bytes, n) || !w.get(d_stage, total))
      return fail(RB_ENOMEM, "download staging allocation failed");
    HIPCHK(hipMemcpyAsync(d_soff, soff.data(), n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_doff, h.off.data(), n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_bytes, bytes.data(), n * 8, hipMemcpyHostToDevice, st));
    launch_gather(s->payload, d_soff, d_bytes, d_stage, d_doff, n, st);
    HIPCHK(hipMemcpyAsync(h.payload.data(), d_stage, total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    LAUNCHCHK();
  }
  return RB_OK;
}
int read_meta(const rbgpu_set *s, uint64_t lo, uint64_t n, std::vector<uint8_t> &type, std::vector<uint16_t> &nruns,
              std::vector<uint32_t> &card, std::vector<uint16_t> *key) {
  hipStream_t st = s->ctx->stream;
  type.resize(n);
  nruns.resize(n);
  card.resize(n);
  if (key) key->resize(n);
  if (!n) return RB_OK;
  if (key) HIPCHK(hipMemcpyAsync(key->data(), s->key + lo, n * 2, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(type.data(), s->type + lo, n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(nruns.data(), s->nruns + lo, n * 2, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(card.data(), s->card + lo, n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  LAUNCHCHK();
  return RB_OK;
}
// Only the min/max shortcut answers of a key-range BSI shard come here (a copy of ebM or foundSet,
// restricted); the containers stay bytes-identical.
int set_key_subset(const rbgpu_set *s, uint32_t key_lo, uint32_t key_hi, rbgpu_set **out) {
  HostSoA h;
  int rc = download_host(s, 0, 1, h);
  if (rc) return rc;
  HostSoA r;
  r.nb = 1;
  r.begin.assign(2, 0);
  for (uint64_t i = 0; i < h.nc(); ++i) {
    if (h.key[i] < key_lo || h.key[i] >= key_hi) continue;
    const uint64_t bytes = payload_bytes(h.type[i], h.card[i], h.nruns[i]);
    r.key.push_back(h.key[i]);
    r.type.push_back(h.type[i]);
    r.card.push_back(h.card[i]);
    r.nruns.push_back(h.nruns[i]);
    r.off.push_back(r.payload.size());
    r.payload.insert(r.payload.end(), h.payload.begin() + h.off[i], h.payload.begin() + h.off[i] + round16(bytes));
  }
  r.begin[1] = r.key.size();
  return upload_host(s->ctx, r, out);
}

// Bitmaps idx[0..n) of s as a new set, in that order (a device-resident copy through the host; the
// containers stay bytes-identical, empty ones included).
int set_gather(const rbgpu_set *s, const uint32_t *idx, uint32_t n, rbgpu_set **out) {
  for (uint32_t i = 0; i < n; ++i)
    if (idx[i] >= s->nb) return fail(RB_EINVAL, "bitmap %u out of range", idx[i]);
  HostSoA h;
  int rc = s->nb ? download_host(s, 0, s->nb, h) : RB_OK;
  if (rc) return rc;
  HostSoA r;
  r.nb = n;
  r.begin.assign(1, 0);
  for (uint32_t k = 0; k < n; ++k) {
    for (uint64_t i = h.begin[idx[k]]; i < h.begin[idx[k] + 1]; ++i) {
      const uint64_t bytes = payload_bytes(h.type[i], h.card[i], h.nruns[i]);
      r.key.push_back(h.key[i]);
      r.type.push_back(h.type[i]);
      r.card.push_back(h.card[i]);
      r.nruns.push_back(h.nruns[i]);
      r.off.push_back(r.payload.size());
      r.payload.insert(r.payload.end(), h.payload.begin() + h.off[i], h.payload.begin() + h.off[i] + round16(bytes));
    }
    r.begin.push_back(r.key.size());
  }
  return upload_host(s->ctx, r, out);
}
} // namespace rbg

extern "C" {

// RBGPU_HOST_CODEC=1 selects the host parser / writer (format.cpp) instead of codec.hip — an A/B
// switch for tests; both give identical sets, bytes and error codes.
static bool host_codec() {
  const char *e = std::getenv("RBGPU_HOST_CODEC");
  return e && e[0] == '1';
}

int rbgpu_set_from_serialized(rbgpu_ctx *ctx, const uint8_t *const *bufs, const uint64_t *lens, uint32_t n,
                              rbgpu_set **out) {
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if (!out || (n && (!bufs || !lens))) return fail(RB_EINVAL, "null argument");
  if (host_codec()) {
    HostSoA h;
    std::string err;
    for (uint32_t i = 0; i < n; ++i) {
      rc = parse_serialized(bufs[i], lens[i], h, err);
      if (rc) return fail(rc, "bitmap %u: %s", i, err.c_str());
    }
    return upload_host(ctx, h, out);
  }
  // one host-to-device copy of the concatenated bytes, parsed on the GPU
  std::vector<uint64_t> off(n + 1ull, 0);
  for (uint32_t i = 0; i < n; ++i) off[i + 1] = off[i] + lens[i];
  const uint64_t total = off[n];
  uint8_t *pin = nullptr, *d_in = nullptr;
  uint64_t *d_off = nullptr;
  Scratch w(ctx->pool);
  if (hipHostMalloc((void **)&pin, std::max<uint64_t>(total, 4) + 8 * (n + 1ull)) != hipSuccess)
    return fail(RB_ENOMEM, "pinned staging of %llu bytes", (unsigned long long)total);
  for (uint32_t i = 0; i < n; ++i)
    if (lens[i]) std::memcpy(pin + off[i], bufs[i], lens[i]);
  uint8_t *pin_off = pin + std::max<uint64_t>(total, 4);
  std::memcpy(pin_off, off.data(), 8 * (n + 1ull));
  if (!w.get(d_in, ((total + 3) & ~3ull) + 4) || !w.get(d_off, n + 1ull)) {
    (void)hipHostFree(pin);
    return fail(RB_ENOMEM, "device staging of %llu bytes", (unsigned long long)total);
  }
  hipStream_t st = ctx->stream;
  if ((total && hipMemcpyAsync(d_in, pin, total, hipMemcpyHostToDevice, st)) ||
      hipMemcpyAsync(d_off, pin_off, 8 * (n + 1ull), hipMemcpyHostToDevice, st)) {
    (void)hipStreamSynchronize(st);
    (void)hipHostFree(pin);
    return fail(RB_EDEVICE, "host-to-device copy failed");
  }
  rc = deserialize_device(ctx, d_in, total, d_off, n, out);
  (void)hipStreamSynchronize(st);
  (void)hipHostFree(pin);
  return rc;
}

int rbgpu_set_from_serialized_device(rbgpu_ctx *ctx, const uint8_t *d_bytes, const uint64_t *offsets, uint32_t n,
                                     rbgpu_set **out) {
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if (!out || !offsets || (n && !d_bytes)) return fail(RB_EINVAL, "null argument");
  for (uint32_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return fail(RB_EINVAL, "offsets not monotone at %u", i);
  Scratch w(ctx->pool);
  uint64_t *d_off = nullptr;
  if (!w.get(d_off, n + 1ull)) return fail(RB_ENOMEM, "offsets");
  hipStream_t st = ctx->stream;
  if (hipMemcpyAsync(d_off, offsets, 8 * (n + 1ull), hipMemcpyHostToDevice, st))
    return fail(RB_EDEVICE, "host-to-device copy failed");
  rc = deserialize_device(ctx, d_bytes, offsets[n], d_off, n, out);
  (void)hipStreamSynchronize(st);
  return rc;
}

int rbgpu_set_from_soa(rbgpu_ctx *ctx, const rb_soa *soa, rbgpu_set **out) {
  return rbg::set_from_soa(ctx, soa, out, false);
}
}  // extern "C"

namespace rbg {
// allow_empty: an empty Array (card 0, no payload) or Run (card 0, no runs) is kept — the containers a
// Roaring64Bitmap xor leaves under their keys, read back from its own serialized form (set64.hip)
int set_from_soa(rbgpu_ctx *ctx, const rb_soa *soa, rbgpu_set **out, bool allow_empty) {
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if (!soa || !out) return fail(RB_EINVAL, "null argument");
  HostSoA h;
  h.nb = soa->n_bitmaps;
  h.begin.assign(soa->begin, soa->begin + soa->n_bitmaps + 1);
  if (h.begin[0] != 0 || h.begin[h.nb] != soa->n_containers) return fail(RB_EINVAL, "bad CSR begin array");
  const uint64_t nc = soa->n_containers;
  h.key.assign(soa->key, soa->key + nc);
  h.type.assign(soa->type, soa->type + nc);
  h.card.assign(soa->card, soa->card + nc);
  h.nruns.assign(soa->nruns, soa->nruns + nc);
  h.off.resize(nc);
  std::string err;
  for (uint32_t b = 0; b < h.nb; ++b) {
    if (h.begin[b + 1] < h.begin[b]) return fail(RB_EINVAL, "bad CSR begin array");
    for (uint64_t i = h.begin[b]; i < h.begin[b + 1]; ++i)
      if (i > h.begin[b] && h.key[i] <= h.key[i - 1]) return fail(RB_EINVAL, "bitmap %u: keys not increasing", b);
  }
  for (uint64_t i = 0; i < nc; ++i) {
    const uint64_t bytes = payload_bytes(h.type[i], h.card[i], h.nruns[i]);
    if (soa->offset[i] + bytes > soa->payload_bytes) return fail(RB_EINVAL, "container %llu payload out of range", (unsigned long long)i);
    const bool empty_ok = allow_empty && h.card[i] == 0 && h.type[i] != RB_BITMAP && h.nruns[i] == 0;
    rc = empty_ok ? RB_OK : validate_container(h.type[i], h.card[i], h.nruns[i], soa->payload + soa->offset[i], err);
    if (rc) return fail(rc, "container %llu: %s", (unsigned long long)i, err.c_str());
    h.off[i] = soa->offset[i];
  }
  h.payload.assign(soa->payload, soa->payload + soa->payload_bytes);
  return upload_host(ctx, h, out);
}
}  // namespace rbg

extern "C" {

void rbgpu_set_free(rbgpu_set *set) {
  if (!set) return;
  set_release(set);
  delete set;
}
uint32_t rbgpu_set_bitmap_count(const rbgpu_set *s) { return s ? s->nb : 0; }
uint64_t rbgpu_set_container_count(const rbgpu_set *s) { return s && !settle(s) ? s->nc : 0; }
uint64_t rbgpu_set_payload_capacity(const rbgpu_set *s) { return s ? s->payload_bytes : 0; }

int rbgpu_set_cardinalities(const rbgpu_set *s, uint64_t *out) {
  SETTLE(s);
  if (!s || !out) return fail(RB_EINVAL, "null argument");
  rbgpu_ctx *ctx = s->ctx;
  int rc = check_ctx(ctx);
  if (rc) return rc;
  Scratch w(ctx->pool);
  uint64_t *d;
  if (!w.get(d, s->nb)) return fail(RB_ENOMEM, "alloc");
  launch_bitmap_cards(s->view(), s->nb, d, ctx->stream);
  HIPCHK(hipMemcpyAsync(out, d, s->nb * 8ull, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  LAUNCHCHK();
  return RB_OK;
}

int rbgpu_set_download(const rbgpu_set *s, uint32_t first, uint32_t count, rb_soa *soa) {
  SETTLE(s);
  if (!s || !soa) return fail(RB_EINVAL, "null argument");
  if ((uint64_t)first + count > s->nb) return fail(RB_EINVAL, "bitmap range out of bounds");
  HostSoA h;
  int rc = download_host(s, first, count, h);
  if (rc) return rc;
  if (!soa->key) { // size query
    soa->n_bitmaps = count;
    soa->n_containers = h.nc();
    soa->payload_bytes = h.payload.size();
    return RB_OK;
  }
  if (soa->n_containers < h.nc() || soa->payload_bytes < h.payload.size())
    return fail(RB_EINVAL, "rb_soa buffers too small");
  soa->n_bitmaps = count;
  soa->n_containers = h.nc();
  soa->payload_bytes = h.payload.size();
  std::memcpy(soa->begin, h.begin.data(), (count + 1) * 8ull);
  std::memcpy(soa->key, h.key.data(), h.nc() * 2);
  std::memcpy(soa->type, h.type.data(), h.nc());
  std::memcpy(soa->card, h.card.data(), h.nc() * 4);
  std::memcpy(soa->nruns, h.nruns.data(), h.nc() * 2);
  std::memcpy(soa->offset, h.off.data(), h.nc() * 8);
  std::memcpy(soa->payload, h.payload.data(), h.payload.size());
  return RB_OK;
}

int rbgpu_set_serialized_sizes(const rbgpu_set *s, uint64_t *out) {
  SETTLE(s);
  if (!s || !out) return fail(RB_EINVAL, "null argument");
  int rc = check_ctx(s->ctx);
  if (rc) return rc;
  rc = ensure_h_begin(s);
  if (rc) return rc;
  // sizes need only metadata: download types / cards / nruns
  std::vector<uint8_t> type;
  std::vector<uint16_t> nruns;
  std::vector<uint32_t> card;
  if ((rc = read_meta(s, 0, s->nc, type, nruns, card))) return rc;
  for (uint32_t b = 0; b < s->nb; ++b) {
    const uint64_t lo = s->h_begin[b], hi = s->h_begin[b + 1], k = hi - lo;
    bool hasrun = false;
    uint64_t bytes = 0;
    for (uint64_t i = lo; i < hi; ++i) {
      hasrun |= type[i] == RB_RUN;
      bytes += serialized_container_bytes(type[i], card[i], nruns[i]);
    }
    out[b] = serialized_header_bytes(hasrun, k) + bytes;
  }
  return RB_OK;
}

int rbgpu_set_summaries(const rbgpu_set *s, uint32_t first, uint32_t count, rb_bitmap_summary *out) {
  SETTLE(s);
  if (!s || (count && !out)) return fail(RB_EINVAL, "null argument");
  if ((uint64_t)first + count > s->nb) return fail(RB_EINVAL, "bitmap range out of bounds");
  int rc = check_ctx(s->ctx);
  if (rc) return rc;
  rc = ensure_h_begin(s);
  if (rc) return rc;
  const uint64_t lo = s->h_begin[first], n = s->h_begin[first + count] - lo;
  std::vector<uint16_t> nruns;
  std::vector<uint8_t> type;
  std::vector<uint32_t> card;
  if ((rc = read_meta(s, lo, n, type, nruns, card))) return rc;
  for (uint32_t b = 0; b < count; ++b) {
    rb_bitmap_summary &o = out[b];
    o = rb_bitmap_summary{};
    o.size_in_bytes = 8;
    for (uint64_t i = s->h_begin[first + b] - lo; i < s->h_begin[first + b + 1] - lo; ++i) {
      o.cardinality += card[i];
      o.n_containers += 1;
      o.n_run_containers += type[i] == RB_RUN;
      o.payload_bytes += serialized_container_bytes(type[i], card[i], nruns[i]);
      // 2 key bytes + Container.getSizeInBytes: Array 2c + 4, Bitmap 8192, Run 4r + 4
      o.size_in_bytes += 2 + (type[i] == RB_BITMAP ? 8192ull : type[i] == RB_ARRAY ? 2ull * card[i] + 4 : 4ull * nruns[i] + 4);
    }
  }
  return RB_OK;
}

int rbgpu_set_type_stats(const rbgpu_set *s, uint64_t *out) {
  SETTLE(s);
  if (!s || !out) return fail(RB_EINVAL, "null argument");
  int rc = check_ctx(s->ctx);
  if (rc) return rc;
  const uint64_t n = s->nc;
  std::vector<uint16_t> nruns;
  std::vector<uint8_t> type;
  std::vector<uint32_t> card;
  if ((rc = read_meta(s, 0, n, type, nruns, card))) return rc;
  std::fill(out, out + 6, 0ull);
  for (uint64_t i = 0; i < n; ++i) {
    const int t = type[i] <= RB_RUN ? type[i] : RB_RUN;
    out[t] += 1;
    out[3 + t] += serialized_container_bytes(t, card[i], nruns[i]);
  }
  return RB_OK;
}


int rbgpu_set_range_counts(const rbgpu_set *s, const uint32_t *members, uint32_t n, uint32_t key_lo, uint32_t key_hi,
                           uint64_t *out) {
  SETTLE(s);
  if (!s || (n && !out)) return fail(RB_EINVAL, "null argument");
  if (key_lo > key_hi || key_hi > 65536u) return fail(RB_EINVAL, "key range [%u, %u) outside [0, 65536]", key_lo, key_hi);
  if (!members && n != s->nb) return fail(RB_EINVAL, "without a member list n must be the bitmap count");
  for (uint32_t i = 0; members && i < n; ++i)
    if (members[i] >= s->nb) return fail(RB_EINVAL, "member %u out of range", members[i]);
  int rc = check_ctx(s->ctx);
  if (rc) return rc;
  if (!n) return RB_OK;
  HIPCHK(hipSetDevice(s->ctx->device));
  Scratch w(s->ctx->pool);
  uint32_t *d_m = nullptr;
  uint64_t *d_out = nullptr;
  if ((members && !w.get(d_m, n)) || !w.get(d_out, n)) return fail(RB_ENOMEM, "range counts");
  hipStream_t st = s->ctx->stream;
  if (members) HIPCHK(hipMemcpyAsync(d_m, members, 4ull * n, hipMemcpyHostToDevice, st));
  launch_range_counts(s->begin, s->key, d_m, n, key_lo, key_hi, d_out, st);
  HIPCHK(hipMemcpyAsync(out, d_out, 8ull * n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  LAUNCHCHK();
  return RB_OK;
}

int rbgpu_set_key_bytes(const rbgpu_set *s, uint64_t *out) {
  SETTLE(s);
  if (!s || !out) return fail(RB_EINVAL, "null argument");
  int rc = check_ctx(s->ctx);
  if (rc) return rc;
  const uint64_t n = s->nc;
  std::vector<uint16_t> key, nruns;
  std::vector<uint8_t> type;
  std::vector<uint32_t> card;
  if ((rc = read_meta(s, 0, n, type, nruns, card, &key))) return rc;
  std::fill(out, out + 65536, 0ull);
  for (uint64_t i = 0; i < n; ++i) out[key[i]] += serialized_container_bytes(type[i], card[i], nruns[i]) + 16;
  return RB_OK;
}

int rbgpu_set_serialize(const rbgpu_set *s, uint32_t first, uint32_t count, uint8_t *dst, uint64_t cap,
                        uint64_t *offsets) {
  SETTLE(s);
  if (!s || (count && !dst)) return fail(RB_EINVAL, "null argument");
  if ((uint64_t)first + count > s->nb) return fail(RB_EINVAL, "bitmap range out of bounds");
  int rc = check_ctx(s->ctx);
  if (rc) return rc;
  if (!host_codec()) return serialize_device(s, first, count, dst, cap, offsets, true);
  HostSoA h;
  rc = download_host(s, first, count, h);
  if (rc) return rc;
  uint64_t pos = 0;
  for (uint32_t b = 0; b < count; ++b) {
    const uint64_t k = serialized_size(h, b);
    if (pos + k > cap) return fail(RB_EINVAL, "destination buffer too small (%llu needed)", (unsigned long long)(pos + k));
    if (offsets) offsets[b] = pos;
    serialize_bitmap(h, b, dst + pos);
    pos += k;
  }
  if (offsets) offsets[count] = pos;
  return RB_OK;
}

int rbgpu_set_serialize_device(const rbgpu_set *s, uint32_t first, uint32_t count, uint8_t *d_dst, uint64_t cap,
                               uint64_t *offsets) {
  SETTLE(s);
  if (!s || (count && !d_dst)) return fail(RB_EINVAL, "null argument");
  if ((uint64_t)first + count > s->nb) return fail(RB_EINVAL, "bitmap range out of bounds");
  int rc = check_ctx(s->ctx);
  if (rc) return rc;
  return serialize_device(s, first, count, d_dst, cap, offsets, false);
}

// ---------------------------------------------------------------- value read-out (values.hip)
static int set_values_call(const rbgpu_set *s, uint32_t first, uint32_t count, uint32_t *dst, uint64_t cap,
                           uint64_t *offsets, bool host_dst) {
  SETTLE(s);
  if (!s || !offsets) return fail(RB_EINVAL, "null argument");
  if ((uint64_t)first + count > s->nb) return fail(RB_EINVAL, "bitmap range out of bounds");
  const int rc = check_ctx(s->ctx);
  if (rc) return rc;
  return set_values(s, first, count, dst, cap, offsets, host_dst);
}

int rbgpu_set_values(const rbgpu_set *s, uint32_t first, uint32_t count, uint32_t *dst, uint64_t cap,
                     uint64_t *offsets) {
  return set_values_call(s, first, count, dst, cap, offsets, true);
}

int rbgpu_set_values_device(const rbgpu_set *s, uint32_t first, uint32_t count, uint32_t *d_dst, uint64_t cap,
                            uint64_t *offsets) {
  return set_values_call(s, first, count, d_dst, cap, offsets, false);
}

// the batched lookups' arguments: every bitmap[i] names a bitmap of the set (checked here, before any launch)
static int set_lookup_call(const rbgpu_set *s, int kind, const uint32_t *bitmap, const void *queries, uint64_t n,
                           void *out, uint8_t *found) {
  SETTLE(s);
  if (!s) return fail(RB_EINVAL, "null set");
  if (n && (!queries || !out || (kind == kLookupSelect && !found))) return fail(RB_EINVAL, "null argument");
  if (n && !bitmap && !s->nb) return fail(RB_EINVAL, "the set holds no bitmap 0");
  if (bitmap)
    for (uint64_t i = 0; i < n; ++i)
      if (bitmap[i] >= s->nb)
        return fail(RB_EINVAL, "bitmap[%llu] = %u: the set holds %u bitmaps", (unsigned long long)i, bitmap[i], s->nb);
  const int rc = check_ctx(s->ctx);
  if (rc) return rc;
  return set_lookup(s, kind, bitmap, queries, n, out, found);
}

int rbgpu_set_contains(const rbgpu_set *s, const uint32_t *bitmap, const uint32_t *values, uint64_t n, uint8_t *out) {
  return set_lookup_call(s, kLookupContains, bitmap, values, n, out, nullptr);
}

int rbgpu_set_rank(const rbgpu_set *s, const uint32_t *bitmap, const uint32_t *values, uint64_t n, uint64_t *out) {
  return set_lookup_call(s, kLookupRank, bitmap, values, n, out, nullptr);
}

int rbgpu_set_select(const rbgpu_set *s, const uint32_t *bitmap, const uint64_t *j, uint64_t n, uint32_t *out,
                     uint8_t *found) {
  return set_lookup_call(s, kLookupSelect, bitmap, j, n, out, found);
}

// ---------------------------------------------------------------- building from values (build.hip)
static int set_from_values_call(rbgpu_ctx *ctx, const uint32_t *values, const uint64_t *offsets, uint32_t n,
                                uint32_t flags, rbgpu_set **out, bool host_src) {
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if (!out) return fail(RB_EINVAL, "null out");
  *out = nullptr;
  if (flags & ~(uint32_t)RB_BUILD_RUN_OPTIMIZE) return fail(RB_EINVAL, "unknown build flags 0x%x", flags);
  if (n && !offsets) return fail(RB_EINVAL, "null offsets");
  for (uint32_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return fail(RB_EINVAL, "offsets not monotone at %u", i);
  const uint64_t base = n ? offsets[0] : 0, total = n ? offsets[n] - base : 0;
  if (total && !values) return fail(RB_EINVAL, "null values");
  if (!host_src || !total) return build_set_values(ctx, values, offsets, n, flags, out);
  Scratch w(ctx->pool);
  uint32_t *d_values = nullptr;
  if (!w.get(d_values, total)) return fail(RB_ENOMEM, "staging of %llu values", (unsigned long long)total);
  std::vector<uint64_t> rel((size_t)n + 1);
  for (uint32_t i = 0; i <= n; ++i) rel[i] = offsets[i] - base;
  if (hipMemcpyAsync(d_values, values + base, total * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    return fail(RB_EDEVICE, "host-to-device copy failed");
  rc = build_set_values(ctx, d_values, rel.data(), n, flags, out);
  (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

int rbgpu_set_from_values(rbgpu_ctx *ctx, const uint32_t *values, const uint64_t *offsets, uint32_t n, uint32_t flags,
                          rbgpu_set **out) {
  return set_from_values_call(ctx, values, offsets, n, flags, out, true);
}

int rbgpu_set_from_values_device(rbgpu_ctx *ctx, const uint32_t *d_values, const uint64_t *offsets, uint32_t n,
                                 uint32_t flags, rbgpu_set **out) {
  return set_from_values_call(ctx, d_values, offsets, n, flags, out, false);
}

static int bsi_from_pairs_call(rbgpu_ctx *ctx, const uint32_t *cols, const uint64_t *vals, uint64_t n, uint32_t flags,
                               rbgpu_set **out, uint64_t *min_value, uint64_t *max_value, bool host_src) {
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if (!out) return fail(RB_EINVAL, "null out");
  *out = nullptr;
  if (flags & ~(uint32_t)RB_BUILD_RUN_OPTIMIZE) return fail(RB_EINVAL, "unknown build flags 0x%x", flags);
  if (n && (!cols || !vals)) return fail(RB_EINVAL, "null pairs");
  if (!host_src || !n) return build_bsi_pairs(ctx, cols, vals, n, flags, out, min_value, max_value);
  Scratch w(ctx->pool);
  uint32_t *d_cols = nullptr;
  uint64_t *d_vals = nullptr;
  if (!w.get(d_cols, n) || !w.get(d_vals, n)) return fail(RB_ENOMEM, "staging of %llu pairs", (unsigned long long)n);
  if (hipMemcpyAsync(d_cols, cols, n * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      hipMemcpyAsync(d_vals, vals, n * 8, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    rc = fail(RB_EDEVICE, "host-to-device copy failed");
  else rc = build_bsi_pairs(ctx, d_cols, d_vals, n, flags, out, min_value, max_value);
  (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

int rbgpu_bsi_from_pairs(rbgpu_ctx *ctx, const uint32_t *cols, const uint64_t *vals, uint64_t n, uint32_t flags,
                         rbgpu_set **out, uint64_t *min_value, uint64_t *max_value) {
  return bsi_from_pairs_call(ctx, cols, vals, n, flags, out, min_value, max_value, true);
}

int rbgpu_bsi_from_pairs_device(rbgpu_ctx *ctx, const uint32_t *d_cols, const uint64_t *d_vals, uint64_t n,
                                uint32_t flags, rbgpu_set **out, uint64_t *min_value, uint64_t *max_value) {
  return bsi_from_pairs_call(ctx, d_cols, d_vals, n, flags, out, min_value, max_value, false);
}

int rbgpu_set_wait(const rbgpu_set *s) {
  if (!s) return fail(RB_EINVAL, "null argument");
  const int rc = settle(s);
  return rc ? rc : seq_settle(s->ctx, s->end_seq);
}

int rbgpu_set_device_view(const rbgpu_set *s, rb_device_view *out) {
  if (!s || !out) return fail(RB_EINVAL, "null argument");
  if (s->failed) return fail(RB_EDEVICE, "the asynchronous call that produced this set failed");
  *out = rb_device_view{s->nb, s->pending ? RB_UNKNOWN_COUNT : s->nc, s->payload_bytes, s->begin, s->key, s->type,
                        s->card, s->nruns, s->off, s->payload};
  return RB_OK;
}

int rbgpu_set_run_optimize(const rbgpu_set *in, rbgpu_set **out, uint8_t *any_run) {
  SETTLE(in);
  if (!in || !out) return fail(RB_EINVAL, "null argument");
  *out = nullptr;
  rbgpu_ctx *ctx = in->ctx;
  int rc = check_ctx(ctx);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  SetPtr res;
  if ((rc = make_set(ctx, in->nb, in->nc, in->payload_bytes, res))) return rc;
  Scratch w(ctx->pool);
  uint8_t *d_any = nullptr;
  if (any_run && in->nb && !w.get(d_any, in->nb)) return fail(RB_ENOMEM, "runOptimize flags");
  const uint64_t n = in->nc;
  auto copy = [&](void *d, const void *s, uint64_t b) { return b ? hipMemcpyAsync(d, s, b, hipMemcpyDeviceToDevice, st) : hipSuccess; };
  if (copy(res->begin, in->begin, 8ull * (in->nb + 1)) || copy(res->key, in->key, 2 * n) ||
      copy(res->card, in->card, 4 * n) || copy(res->off, in->off, 8 * n))
    return fail(RB_EDEVICE, "runOptimize metadata copy");
  stats_begin(ctx);
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  launch_run_optimize(in->view(), n, res->type, res->nruns, res->payload, in->nb, d_any, st);
  HIPCHK(hipEventRecord(ctx->ev[2], st));
  if (d_any) HIPCHK(hipMemcpyAsync(any_run, d_any, in->nb, hipMemcpyDeviceToHost, st));
  const KernelSpan spans[1] = {{"k_run_optimize", 0, 1, n}};
  if ((rc = stats_end(ctx, n, n, spans, 1))) return rc;
  res->h_begin = in->h_begin;
  *out = res.release();
  return RB_OK;
}

int rbgpu_set_setup_stats(const rbgpu_set *s, double *ms, uint64_t *bytes) {
  if (!s || !ms || !bytes) return fail(RB_EINVAL, "null argument");
  *ms = s->derive_ms;
  *bytes = s->derive_bytes;
  return RB_OK;
}

int rbgpu_set_setup_parts(const rbgpu_set *s, double *ms, uint64_t *bytes) {
  if (!s || !ms || !bytes) return fail(RB_EINVAL, "null argument");
  for (int i = 0; i < 4; ++i) {
    ms[i] = s->part_ms[i];
    bytes[i] = s->part_bytes[i];
  }
  return RB_OK;
}

int rbgpu_set_extract(const rbgpu_set *s, uint32_t first, uint32_t count, rbgpu_set **out) {
  SETTLE(s);
  if (!s || !out) return fail(RB_EINVAL, "null argument");
  *out = nullptr;
  if ((uint64_t)first + count > s->nb) return fail(RB_EINVAL, "bitmap range out of bounds");
  HostSoA h;
  int rc = download_host(s, first, count, h);
  if (rc) return rc;
  return upload_host(s->ctx, h, out);
}

} // extern "C"
