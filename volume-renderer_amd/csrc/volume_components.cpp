// volume_components.cpp -- connected components of the resident volume and the selection as a bit plane (vr_label_components,
// vr_extract_components)
#include <vector>

#include "volume_ops.h"
#include "vr_components.h"
#include "vr_primitives.h"

namespace vr {

// Tile pass, seam pass, flatten, the scan of the root counts; then -- the number of components known -- the labels and the records.
Labelling label_components(const DeviceQueue &q, const ResidentVolume &V, int32_t iso, float iso_s, int index_bits, float &ms)
{
    ComponentsJob J = {};
    J.volume = V.data; J.bytes_per_voxel = V.bytes_per_voxel; J.layout = V.layout;
    J.nx = V.nx; J.ny = V.ny; J.nz = V.nz;
    J.iso_s = iso_s;
    const uint64_t nvox = component_voxels(J), words = component_words(J);
    const bool fits32 = nvox < 0xffffffffull;
    if (index_bits == 32 && !fits32) throw std::invalid_argument("labelComponents: 32-bit parents cannot number this volume's voxels");
    J.index_bits = index_bits ? index_bits : (fits32 ? 32 : 64);
    DeviceBuffer<uint32_t> labels, error;
    DeviceBuffer<uint64_t> parent64, bits, scan;
    DeviceBuffer<uint8_t> temp;
    const size_t temp_bytes = scan64_temp_bytes(words + 1);
    labels.allocOrNoMemory(nvox, "labelComponents: hipMalloc(labels)");
    if (J.index_bits == 64) parent64.allocOrNoMemory(nvox, "labelComponents: hipMalloc(parents)");
    bits.allocOrNoMemory(words, "labelComponents: hipMalloc(root bits)");
    scan.allocOrNoMemory(words + 1, "labelComponents: hipMalloc(root counts)");
    temp.allocOrNoMemory(temp_bytes ? temp_bytes : 16, "labelComponents: hipMalloc(scan scratch)");
    error.allocOrNoMemory(1, "labelComponents: hipMalloc(error word)");
    J.labels = labels.get();
    J.parent = J.index_bits == 64 ? (void *)parent64.get() : (void *)labels.get();
    J.bits = bits.get(); J.scan = scan.get(); J.error = error.get();
    hipError_t e = hipMemsetAsync(J.error, 0, sizeof(uint32_t), q.stream);
    if (e == hipSuccess) e = hipEventRecord(q.ev0, q.stream);
    if (e == hipSuccess) e = launch_components_tiles(J, q.stream);
    if (e == hipSuccess) e = launch_components_seams(J, q.stream);
    if (e == hipSuccess) e = launch_components_flatten(J, q.stream);
    if (e == hipSuccess) e = launch_scan64(J.scan, words + 1, temp.get(), temp_bytes, q.stream);
    q.check(q.finishTimed(e, ms), "component kernels (union-find)");
    auto kernelsOk = [&] {
        uint32_t flags = 0;
        q.check(hipMemcpy(&flags, J.error, sizeof(flags), hipMemcpyDeviceToHost), "hipMemcpy(D2H error word)");
        if (flags) throw HipError(hipErrorUnknown, "labelComponents: a union-find loop hit its iteration cap (flags " + std::to_string(flags) + ")");
    };
    kernelsOk();
    uint64_t n = 0;
    q.check(hipMemcpy(&n, J.scan + words, sizeof(n), hipMemcpyDeviceToHost), "hipMemcpy(D2H component count)");
    if (n > 0xfffffffeull)
        throw RefusalWithMessage("labelComponents: more than 2^32 - 2 components",
                                 "The volume has " + std::to_string(n) + " connected components at this iso value: more than 32-bit labels number. "
                                 "Smooth the volume or choose another iso value.");
    DeviceBuffer<uint64_t> voxels, first;
    DeviceBuffer<int32_t> bbox;
    std::vector<uint64_t> h_voxels((size_t)n), h_first((size_t)n);
    std::vector<int32_t> h_bbox((size_t)n * 6);
    if (n > 0) {
        voxels.allocOrNoMemory(n, "labelComponents: hipMalloc(voxel counts)");
        first.allocOrNoMemory(n, "labelComponents: hipMalloc(first voxels)");
        bbox.allocOrNoMemory(n * 6, "labelComponents: hipMalloc(boxes)");
        J.voxels = voxels.get(); J.first_voxel = first.get(); J.bbox = bbox.get();
    }
    e = hipEventRecord(q.ev0, q.stream);
    if (e == hipSuccess) e = launch_components_labels(J, n, q.stream);
    if (e == hipSuccess && n > 0) e = launch_components_records(J, q.stream);
    q.check(q.finishTimed(e, ms), "component kernels (labels)");
    kernelsOk();
    if (n > 0) {
        q.check(hipMemcpy(h_voxels.data(), J.voxels, n * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy(D2H voxel counts)");
        q.check(hipMemcpy(h_first.data(), J.first_voxel, n * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy(D2H first voxels)");
        q.check(hipMemcpy(h_bbox.data(), J.bbox, n * 6 * sizeof(int32_t), hipMemcpyDeviceToHost), "hipMemcpy(D2H boxes)");
    }
    Labelling L;
    L.labels = std::move(labels);
    L.records.adopt(iso, iso_s, std::move(h_voxels), std::move(h_first), std::move(h_bbox));
    return L;
}

// a small kernel over the labels; no component at all: the empty plane
DeviceBuffer<uint64_t> selection_plane(const DeviceQueue &q, const Labelling &L, float &ms)
{
    const uint64_t nvox = L.labels.size(), words = (nvox + 63) / 64;
    const std::vector<uint8_t> &sel = L.records.selected;
    DeviceBuffer<uint64_t> plane;
    DeviceBuffer<uint8_t> selected;
    plane.allocOrNoMemory(words, "extractComponents: hipMalloc(selection plane)");
    hipError_t e = hipSuccess;
    if (sel.empty()) {
        e = hipMemsetAsync(plane.get(), 0, plane.bytes(), q.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(q.stream);
        q.check(e, "hipMemset(selection plane)");
    } else {
        selected.allocOrNoMemory(sel.size(), "extractComponents: hipMalloc(selection)");
        e = hipMemcpyAsync(selected.get(), sel.data(), sel.size(), hipMemcpyHostToDevice, q.stream);
        if (e == hipSuccess) e = hipEventRecord(q.ev0, q.stream);
        if (e == hipSuccess) e = launch_components_plane(L.labels.get(), selected.get(), nvox, plane.get(), q.stream);
        q.check(q.finishTimed(e, ms), "selection kernel");
    }
    return plane;
}

}  // namespace vr
