// vr_primitives.h -- the device-wide sorts and scans of the volume and mesh operations (vr_primitives.hip): rocPRIM's radix
// sorts and prefix sums behind plain functions, compiled once.  Each takes device scratch of at least what its _temp_bytes
// query returns (0: rocPRIM refused the query); nothing here allocates or waits.  A null pointer, n == 0, and bits == 0 or
// above the key's width: hipErrorInvalidValue.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vr {

// stable radix sorts of (key, value) pairs over the key bits [0, bits)
size_t sort_pairs64_temp_bytes(uint64_t n, uint32_t bits);
size_t sort_pairs32_temp_bytes(uint64_t n, uint32_t bits);
hipError_t launch_sort_pairs64(void *temp, size_t temp_bytes, const uint64_t *key_in, uint64_t *key_out, const uint32_t *value_in,
                               uint32_t *value_out, uint64_t n, uint32_t bits, hipStream_t st);
hipError_t launch_sort_pairs32(void *temp, size_t temp_bytes, const uint32_t *key_in, uint32_t *key_out, const uint32_t *value_in,
                               uint32_t *value_out, uint64_t n, uint32_t bits, hipStream_t st);
// radix sort of 64-bit keys alone over the key bits [0, bits)
size_t sort_keys64_temp_bytes(uint64_t n, uint32_t bits);
hipError_t launch_sort_keys64(void *temp, size_t temp_bytes, const uint64_t *key_in, uint64_t *key_out, uint64_t n, uint32_t bits,
                              hipStream_t st);
// sums of n uint32 in place (their total stays below 2^32), inclusive or exclusive; the query: the larger of the two needs
size_t scan32_temp_bytes(uint64_t n);
hipError_t launch_scan32(uint32_t *data, uint64_t n, bool inclusive, void *temp, size_t temp_bytes, hipStream_t st);
// exclusive sums of n uint64 in place
size_t scan64_temp_bytes(uint64_t n);
hipError_t launch_scan64(uint64_t *data, uint64_t n, void *temp, size_t temp_bytes, hipStream_t st);

}  // namespace vr
