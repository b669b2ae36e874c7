// lookup.hpp — point probes of one container, straight from its payload (shared by the BSI value read-back,
// bsi.hip, and the set read-out, values.hip).
#pragma once
#include "common.hpp"

namespace rbg {

// first index i of the sorted u16 array a[0, n) with a[i] >= x (n: none)
__device__ __forceinline__ uint32_t lower_bound_u16(const uint16_t *a, uint32_t n, uint32_t x) {
  uint32_t lo = 0;
  while (n) {
    const uint32_t h = n >> 1;
    if (a[lo + h] < x) {
      lo += h + 1;
      n -= h + 1;
    } else {
      n = h;
    }
  }
  return lo;
}
// first run i of the run list r[0, n) (start | length - 1 << 16; ascending, disjoint) that ends at or after x
__device__ __forceinline__ uint32_t first_run_ending_from(const uint32_t *r, uint32_t n, uint32_t x) {
  uint32_t lo = 0;
  while (n) {
    const uint32_t h = n >> 1, q = r[lo + h];
    if ((q & 0xFFFF) + (q >> 16) < x) {
      lo += h + 1;
      n -= h + 1;
    } else {
      n = h;
    }
  }
  return lo;
}
// x in the container?  Bitmap: one word; Array: a search over the values; Run: a search over the runs' ends, then
// the start.  Straight from the payload, whatever its size (a Run of more than 2047 runs included).
__device__ __forceinline__ bool container_has(int type, const uint8_t *p, uint32_t card, uint32_t nruns, uint32_t x) {
  if (type == kBitmap) return (reinterpret_cast<const uint32_t *>(p)[x >> 5] >> (x & 31)) & 1u;
  if (type == kArray) {
    const uint16_t *a = reinterpret_cast<const uint16_t *>(p);
    const uint32_t i = lower_bound_u16(a, card, x);
    return i < card && a[i] == x;
  }
  const uint32_t *r = reinterpret_cast<const uint32_t *>(p);
  const uint32_t i = first_run_ending_from(r, nruns, x);
  return i < nruns && (r[i] & 0xFFFF) <= x;
}

} // namespace rbg
