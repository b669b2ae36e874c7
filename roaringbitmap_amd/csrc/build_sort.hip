// build_sort.hip — the two device sorts of the value build (build.hip), in a translation unit of their own so
// that build.hip's resource record lists the project's kernels only.  rocprim's LSD radix sort is stable: among
// equal keys the input order stands, which is what lets the BSI build keep the last value given for a column.
#include <cstring> // before rocprim: its headers use std::memcpy without including it

#include <rocprim/device/device_radix_sort.hpp>

#include "kernels.hpp"

namespace rbg {

// Keys on bits [begin_bit, end_bit).  tmp = null: *tmp_bytes receives the scratch size and nothing is launched.
hipError_t build_sort_keys(void *tmp, size_t *tmp_bytes, const uint64_t *in, uint64_t *out, uint64_t n,
                           unsigned begin_bit, unsigned end_bit, hipStream_t st) {
  return rocprim::radix_sort_keys(tmp, *tmp_bytes, in, out, (size_t)n, begin_bit, end_bit, st);
}

// (column, value) pairs by column, stable.
hipError_t build_sort_pairs(void *tmp, size_t *tmp_bytes, const uint32_t *kin, uint32_t *kout, const uint64_t *vin,
                            uint64_t *vout, uint64_t n, hipStream_t st) {
  return rocprim::radix_sort_pairs(tmp, *tmp_bytes, kin, kout, vin, vout, (size_t)n, 0u, 32u, st);
}

} // namespace rbg
