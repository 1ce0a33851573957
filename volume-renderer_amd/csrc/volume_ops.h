// volume_ops.h -- the computations on the resident volume and the resident mesh outside a frame, as free functions: each sees a
// queue and its inputs, allocates what it needs, launches its kernels and returns its result by value.  RendererCore's members
// (volume_ops.cpp) validate, call, and adopt the result only after the function has returned: a call that throws leaves the
// previous mesh or labelling as it was.  One file per algorithm: volume_smooth.cpp, volume_rank.cpp, mesh_extract.cpp, mesh_simplify.cpp,
// mesh_smooth.cpp, volume_components.cpp.
#pragma once
#include <stdexcept>
#include <string>

#include "component_records.h"
#include "device_buffer.h"
#include "resident_mesh.h"
#include "volume_copies.h"

namespace vr {

// the stream the kernels go to and the two events that time a stretch of them (the ones render() times frames with)
struct DeviceQueue {
    hipStream_t stream;
    hipEvent_t ev0, ev1;
    // ends a stretch that began with ev0 recorded: records ev1 unless `e` says a launch failed, waits for the stream either way,
    // and adds the elapsed time to `ms`
    hipError_t finishTimed(hipError_t e, float &ms) const
    {
        if (e == hipSuccess) e = hipEventRecord(ev1, stream);
        const hipError_t es = hipStreamSynchronize(stream);
        if (e == hipSuccess) e = es;
        float t = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&t, ev0, ev1);
        ms += t;
        return e;
    }
    void check(hipError_t e, const std::string &what) const { hipCheck(e, what); }
};

// a refusal the GUI is told about: what() is the error's text, `message` the text the handle queues under "Error!"
struct RefusalWithMessage : std::invalid_argument {
    std::string message;
    RefusalWithMessage(const std::string &what, std::string m) : std::invalid_argument(what), message(std::move(m)) {}
};

// device scratch of the sorts and scans that grows when a later one needs more; `what`: the allocation's error text
struct GrowingScratch {
    DeviceBuffer<uint8_t> buf;
    const char *what;
    explicit GrowingScratch(const char *w) : what(w) {}
    void atLeast(size_t bytes) { if (buf.bytes() < bytes || !buf) buf.allocOrNoMemory(bytes ? bytes : 16, what); }
    void *get() const { return buf.get(); }
    size_t bytes() const { return buf.bytes(); }
};

inline uint32_t bitWidth(uint64_t m) { uint32_t b = 0; while (m) { b++; m >>= 1; } return b; }   // bits the numbers 0 .. m need

// the labelling: the records on the host, one label per voxel (linear order) on the device
struct Labelling {
    ComponentRecords records;
    DeviceBuffer<uint32_t> labels;
    void clear() { labels.reset(); records.clear(); }
};

// Gaussian smoothing's passes, src -> dst (both allocVolume storage of V's dimensions, type and layout); ms: set to the passes' time
void smooth_passes(const DeviceQueue &q, const ResidentVolume &V, const void *src, void *dst, const float sigma[3], uint64_t workspace_limit, float &ms);
// the rank filter's passes (rank_schedule.h), src -> dst like smooth_passes; op and r3 pass rank_arguments_ok and are not the identity
void rank_passes(const DeviceQueue &q, const ResidentVolume &V, const void *src, void *dst, int op, const int r3[3], float &ms);
// the isosurface iso_s (stored units) of V; selected: launch_components_plane's bits or nullptr; ms: kernel time so far, added to
ResidentMesh extract_mesh(const DeviceQueue &q, const ResidentVolume &V, const float spacing[3], uint64_t workspace_limit, int32_t iso, float iso_s,
                          const uint64_t *selected, float &ms);
ResidentMesh simplify_mesh(const DeviceQueue &q, const ResidentMesh &M, float cell, float &ms);
// new positions and normals for M's triangles (both empty: nothing to do), and the number of fixed vertices
struct SmoothedMesh { DeviceBuffer<float> positions, normals; uint32_t n_fixed = 0; };
SmoothedMesh smooth_mesh(const DeviceQueue &q, const ResidentMesh &M, int iterations, float lambda, float mu, int fix_boundary, float &build_ms, float &iterate_ms);
// index_bits: 0 automatic (32 below 2^32 - 1 voxels, else 64), 32, 64
Labelling label_components(const DeviceQueue &q, const ResidentVolume &V, int32_t iso, float iso_s, int index_bits, float &ms);
// the labelling's selection as one bit per voxel
DeviceBuffer<uint64_t> selection_plane(const DeviceQueue &q, const Labelling &L, float &ms);

}  // namespace vr
