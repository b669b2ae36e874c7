// entry.hip — thin C entry points (argument checks) of the BSI calls (bsi.hip) and the generators (generate.hip).
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

// Kernel-study hook (not part of rbgpu.h): config-2 generator type mix, cumulative per mille
// {filter Array, filter Array+Bitmap, posting Array, posting Array+Bitmap}.
void rbgpu_internal_set_mix(int fa, int fab, int pa, int pab) {
  const int m[4] = {fa, fab, pa, pab};
  set_mix(m);
}

// ---------------------------------------------------------------- bit-sliced index
int rbgpu_bsi_compare_keys(rbgpu_ctx *ctx, const rbgpu_set *bsi, int op, uint64_t start_or_value, uint64_t end,
                           uint64_t min_value, uint64_t max_value, const rbgpu_set *found, uint32_t key_lo,
                           uint32_t key_hi, rbgpu_set **out) {
  SETTLE(bsi, found);
  if (!out) return fail(RB_EINVAL, "null out");
  *out = nullptr;
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if (!bsi || bsi->ctx != ctx) return fail(RB_EINVAL, "bad bsi set");
  if (bsi->nb < 1 || bsi->nb > 65) return fail(RB_EINVAL, "a bsi set holds 0..64 slices and the existence bitmap");
  if (found && (found->ctx != ctx || found->nb != 1)) return fail(RB_EINVAL, "foundSet must be a one-bitmap set");
  if (op < RB_BSI_EQ || op > RB_BSI_RANGE) return fail(RB_EINVAL, "not support operation!");
  if (key_lo > key_hi || key_hi > 65536) return fail(RB_EINVAL, "bad key range [%u, %u)", key_lo, key_hi);
  rc = ensure_h_begin(bsi);
  if (rc) return rc;
  return bsi_compare(ctx, bsi, op, start_or_value, end, min_value, max_value, found, key_lo, key_hi, out);
}

int rbgpu_bsi_compare(rbgpu_ctx *ctx, const rbgpu_set *bsi, int op, uint64_t start_or_value, uint64_t end,
                      uint64_t min_value, uint64_t max_value, const rbgpu_set *found, rbgpu_set **out) {
  return rbgpu_bsi_compare_keys(ctx, bsi, op, start_or_value, end, min_value, max_value, found, 0, 65536, out);
}

// the aggregates' arguments: a bsi set of 1..65 bitmaps, found a one-bitmap set of the same context or NULL
static int check_bsi_agg(rbgpu_ctx *ctx, const rbgpu_set *bsi, const rbgpu_set *found) {
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if (!bsi || bsi->ctx != ctx) return fail(RB_EINVAL, "bad bsi set");
  if (bsi->nb < 1 || bsi->nb > 65) return fail(RB_EINVAL, "a bsi set holds 0..64 slices and the existence bitmap");
  if (found && (found->ctx != ctx || found->nb != 1)) return fail(RB_EINVAL, "foundSet must be a one-bitmap set");
  return ensure_h_begin(bsi);
}

int rbgpu_bsi_slice_counts(rbgpu_ctx *ctx, const rbgpu_set *bsi, const rbgpu_set *found, uint32_t key_lo,
                           uint32_t key_hi, uint64_t *counts) {
  SETTLE(bsi, found);
  if (!counts) return fail(RB_EINVAL, "null counts");
  int rc = check_bsi_agg(ctx, bsi, found);
  if (rc) return rc;
  if (key_lo > key_hi || key_hi > 65536) return fail(RB_EINVAL, "bad key range [%u, %u)", key_lo, key_hi);
  return bsi_slice_counts(ctx, bsi, found, key_lo, key_hi, counts);
}

// SUM_i counts[i] << i (mod 2^64) and counts[nbits]
static void bsi_weighted_sum(const uint64_t *counts, uint32_t nbits, uint64_t *sum, uint64_t *count) {
  uint64_t s = 0;
  for (uint32_t i = 0; i < nbits; ++i) s += counts[i] << i;
  *sum = s;
  *count = counts[nbits];
}

int rbgpu_bsi_sum(rbgpu_ctx *ctx, const rbgpu_set *bsi, const rbgpu_set *found, uint64_t *sum, uint64_t *count) {
  if (!sum || !count) return fail(RB_EINVAL, "null out");
  uint64_t counts[65] = {};
  const int rc = rbgpu_bsi_slice_counts(ctx, bsi, found, 0, 65536, counts);
  if (rc) return rc;
  bsi_weighted_sum(counts, bsi->nb - 1, sum, count);
  return RB_OK;
}

int rbgpu_bsi_topk(rbgpu_ctx *ctx, const rbgpu_set *bsi, const rbgpu_set *found, uint64_t k, rbgpu_set **out) {
  SETTLE(bsi, found);
  if (!out) return fail(RB_EINVAL, "null out");
  *out = nullptr;
  const int rc = check_bsi_agg(ctx, bsi, found);
  if (rc) return rc;
  return bsi_topk(ctx, bsi, found, k, out);
}

// the export's arguments (rbgpu_bsi_slice_counts' checks, and outputs that come as a pair)
static int bsi_values_call(rbgpu_ctx *ctx, const rbgpu_set *bsi, const rbgpu_set *found, uint32_t key_lo,
                           uint32_t key_hi, uint32_t *cols, uint64_t *vals, uint64_t cap, uint64_t *count,
                           bool host_dst) {
  SETTLE(bsi, found);
  if (!count) return fail(RB_EINVAL, "null count");
  *count = 0;
  int rc = check_bsi_agg(ctx, bsi, found);
  if (rc) return rc;
  if (key_lo > key_hi || key_hi > 65536) return fail(RB_EINVAL, "bad key range [%u, %u)", key_lo, key_hi);
  if (!cols != !vals) return fail(RB_EINVAL, "cols and vals come together (both null: the count only)");
  return bsi_values(ctx, bsi, found, key_lo, key_hi, cols, vals, cap, count, host_dst);
}

int rbgpu_bsi_values(rbgpu_ctx *ctx, const rbgpu_set *bsi, const rbgpu_set *found, uint32_t key_lo, uint32_t key_hi,
                     uint32_t *cols, uint64_t *vals, uint64_t cap, uint64_t *count) {
  return bsi_values_call(ctx, bsi, found, key_lo, key_hi, cols, vals, cap, count, true);
}

int rbgpu_bsi_values_device(rbgpu_ctx *ctx, const rbgpu_set *bsi, const rbgpu_set *found, uint32_t key_lo,
                            uint32_t key_hi, uint32_t *d_cols, uint64_t *d_vals, uint64_t cap, uint64_t *count) {
  return bsi_values_call(ctx, bsi, found, key_lo, key_hi, d_cols, d_vals, cap, count, false);
}

int rbgpu_bsi_get_values(rbgpu_ctx *ctx, const rbgpu_set *bsi, const uint32_t *columns, uint64_t n, uint64_t *values,
                         uint8_t *exists) {
  SETTLE(bsi);
  const int rc = check_bsi_agg(ctx, bsi, nullptr);
  if (rc) return rc;
  if (n && !columns) return fail(RB_EINVAL, "null columns");
  return bsi_get_values(ctx, bsi, columns, n, values, exists);
}

int rbgpu_generate_bsi(rbgpu_ctx *ctx, uint32_t nslices, uint64_t nrows, uint64_t seed, rbgpu_set **out) {
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if (!out) return fail(RB_EINVAL, "null out");
  *out = nullptr;
  return generate_bsi(ctx, nslices, nrows, seed, 0, 65536, out);
}

int rbgpu_generate_bsi_keys(rbgpu_ctx *ctx, uint32_t nslices, uint64_t nrows, uint64_t seed, uint32_t key_lo,
                            uint32_t key_hi, rbgpu_set **out) {
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if (!out) return fail(RB_EINVAL, "null out");
  *out = nullptr;
  return generate_bsi(ctx, nslices, nrows, seed, key_lo, key_hi, out);
}

// ---------------------------------------------------------------- range mutations (range.hip)
static int range_op_call(rbgpu_ctx *ctx, int op, bool inplace, const rbgpu_set *in, const uint32_t *members,
                         const uint64_t *start, const uint64_t *end, uint32_t n, rbgpu_set **out) {
  if (!out) return fail(RB_EINVAL, "null out");
  *out = nullptr; // before anything can fail: no path leaves the caller's word as it was
  SETTLE(in);
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if (!in || in->ctx != ctx) return fail(RB_EINVAL, "bad input set");
  if (op < RB_RANGE_ADD || op > RB_RANGE_FLIP) return fail(RB_EINVAL, "unknown range op %d", op);
  if (n && (!start || !end)) return fail(RB_EINVAL, "null range arrays");
  if (!members && n != in->nb) return fail(RB_EINVAL, "without a member list n must be the bitmap count");
  for (uint32_t i = 0; i < n; ++i) {
    if (members && members[i] >= in->nb)
      return fail(RB_EINVAL, "members[%u] = %u: the set holds %u bitmaps", i, members[i], in->nb);
    // rangeSanityCheck (RoaringBitmap.java:204-213)
    if (start[i] > 0xFFFFFFFFull)
      return fail(RB_EINVAL, "rangeStart=%llu should be in [0, 0xffffffff]", (unsigned long long)start[i]);
    if (end[i] > (1ull << 32))
      return fail(RB_EINVAL, "rangeEnd=%llu should be in [0, 0xffffffff + 1]", (unsigned long long)end[i]);
  }
  return range_op(ctx, op, inplace, in, members, start, end, n, out);
}

int rbgpu_set_range_op(rbgpu_ctx *ctx, int op, const rbgpu_set *in, const uint32_t *members, const uint64_t *start,
                       const uint64_t *end, uint32_t n, rbgpu_set **out) {
  return range_op_call(ctx, op, false, in, members, start, end, n, out);
}

int rbgpu_set_range_op_inplace(rbgpu_ctx *ctx, int op, const rbgpu_set *in, const uint32_t *members,
                               const uint64_t *start, const uint64_t *end, uint32_t n, rbgpu_set **out) {
  return range_op_call(ctx, op, true, in, members, start, end, n, out);
}

// ---------------------------------------------------------------- generator
int rbgpu_generate(rbgpu_ctx *ctx, int workload, uint32_t n, uint64_t seed, rbgpu_set **a, rbgpu_set **b) {
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if (!a) return fail(RB_EINVAL, "null out");
  *a = nullptr;
  if (b) *b = nullptr;
  if (workload == RB_WL_FILTER_POSTING && !b) return fail(RB_EINVAL, "filter/posting workload needs two outputs");
  return generate_sets(ctx, workload, n, seed, 0, 65536, a, b);
}

int rbgpu_generate_keys(rbgpu_ctx *ctx, int workload, uint32_t n, uint64_t seed, uint32_t key_lo, uint32_t key_hi,
                        rbgpu_set **a) {
  int rc = check_ctx(ctx);
  if (rc) return rc;
  if (!a) return fail(RB_EINVAL, "null out");
  *a = nullptr;
  if (workload == RB_WL_FILTER_POSTING) return fail(RB_EINVAL, "key ranges apply to the wide workloads");
  return generate_sets(ctx, workload, n, seed, key_lo, key_hi, a, nullptr);
}

} // extern "C"
