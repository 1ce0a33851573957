// vr_primitives.hip -- the five device-wide primitives the volume and mesh operations share (vr_primitives.h): the only file
// that includes rocPRIM, so each of its sorts and scans is instantiated once and lives in one code object.  One translation
// unit: nothing here reads a voxel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "vr_code_unit.h"
#include "vr_primitives.h"

namespace vr {

size_t sort_pairs64_temp_bytes(uint64_t n, uint32_t bits)
{
    size_t bytes = 0;
    uint64_t *k = nullptr;
    uint32_t *v = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, bytes, (const uint64_t *)k, k, (const uint32_t *)v, v, (size_t)n, 0u, bits) != hipSuccess) return 0;
    return bytes;
}

size_t sort_pairs32_temp_bytes(uint64_t n, uint32_t bits)
{
    size_t bytes = 0;
    uint32_t *k = nullptr, *v = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, bytes, (const uint32_t *)k, k, (const uint32_t *)v, v, (size_t)n, 0u, bits) != hipSuccess) return 0;
    return bytes;
}

hipError_t launch_sort_pairs64(void *temp, size_t temp_bytes, const uint64_t *key_in, uint64_t *key_out, const uint32_t *value_in,
                               uint32_t *value_out, uint64_t n, uint32_t bits, hipStream_t st)
{
    if (!temp || !key_in || !key_out || !value_in || !value_out || n == 0 || bits == 0 || bits > 64) return hipErrorInvalidValue;
    return rocprim::radix_sort_pairs(temp, temp_bytes, key_in, key_out, value_in, value_out, (size_t)n, 0u, bits, st);
}

hipError_t launch_sort_pairs32(void *temp, size_t temp_bytes, const uint32_t *key_in, uint32_t *key_out, const uint32_t *value_in,
                               uint32_t *value_out, uint64_t n, uint32_t bits, hipStream_t st)
{
    if (!temp || !key_in || !key_out || !value_in || !value_out || n == 0 || bits == 0 || bits > 32) return hipErrorInvalidValue;
    return rocprim::radix_sort_pairs(temp, temp_bytes, key_in, key_out, value_in, value_out, (size_t)n, 0u, bits, st);
}

size_t sort_keys64_temp_bytes(uint64_t n, uint32_t bits)
{
    size_t bytes = 0;
    uint64_t *k = nullptr;
    if (rocprim::radix_sort_keys(nullptr, bytes, (const uint64_t *)k, k, (size_t)n, 0u, bits) != hipSuccess) return 0;
    return bytes;
}

hipError_t launch_sort_keys64(void *temp, size_t temp_bytes, const uint64_t *key_in, uint64_t *key_out, uint64_t n, uint32_t bits,
                              hipStream_t st)
{
    if (!temp || !key_in || !key_out || n == 0 || bits == 0 || bits > 64) return hipErrorInvalidValue;
    return rocprim::radix_sort_keys(temp, temp_bytes, key_in, key_out, (size_t)n, 0u, bits, st);
}

size_t scan32_temp_bytes(uint64_t n)
{
    size_t a = 0, b = 0;
    uint32_t *none = nullptr;
    if (rocprim::exclusive_scan(nullptr, a, none, none, 0u, (size_t)n, rocprim::plus<uint32_t>()) != hipSuccess) return 0;
    if (rocprim::inclusive_scan(nullptr, b, none, none, (size_t)n, rocprim::plus<uint32_t>()) != hipSuccess) return 0;
    return a > b ? a : b;
}

hipError_t launch_scan32(uint32_t *data, uint64_t n, bool inclusive, void *temp, size_t temp_bytes, hipStream_t st)
{
    if (!data || !temp || n == 0) return hipErrorInvalidValue;
    if (inclusive) return rocprim::inclusive_scan(temp, temp_bytes, data, data, (size_t)n, rocprim::plus<uint32_t>(), st);
    return rocprim::exclusive_scan(temp, temp_bytes, data, data, 0u, (size_t)n, rocprim::plus<uint32_t>(), st);
}

size_t scan64_temp_bytes(uint64_t n)
{
    size_t bytes = 0;
    uint64_t *none = nullptr;
    if (rocprim::exclusive_scan(nullptr, bytes, none, none, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>()) != hipSuccess) return 0;
    return bytes;
}

hipError_t launch_scan64(uint64_t *data, uint64_t n, void *temp, size_t temp_bytes, hipStream_t st)
{
    if (!data || !temp || n == 0) return hipErrorInvalidValue;
    return rocprim::exclusive_scan(temp, temp_bytes, data, data, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), st);
}

namespace {
VR_CODE_UNIT(primitives, , "sort and scan", WARM_LOAD_SHADER)
}  // namespace

}  // namespace vr
