// renderer_core.h -- host side of the MI355X ray-march path.
//
// Mirrors the reference's RendererCore (include/RendererCore.h:9-44): same member
// and method names, same call semantics, with the OpenGL objects replaced by HIP
// allocations and the compute-shader dispatch replaced by vr::launch_raymarch.
// Members the reference keeps private-but-friend (RendererGUI pokes them directly,
// include/RendererCore.h:18) are public here; vr_capi.cpp is the "friend".
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "camera.h"
#include "device_buffer.h"
#include "launch_plan.h"
#include "launch_tuner.h"
#include "tile_tables.h"
#include "mesh_files.h"
#include "volume_copies.h"
#include "volume_ops.h"
#include "vr_frame.h"

namespace vr {

struct NoDeviceError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// which of the four frame kernels a frame runs: the first-hit isosurface and the reslice mode exclude each other and come before
// everything else; Shaded: gradient-lit compositing is on and the frame is not MIP; RayMarch: composite or MIP (vr_kernels.hip)
enum class FrameMode { RayMarch, Isosurface, Reslice, Shaded };

class RendererCore {
public:
    explicit RendererCore(int device);      // device < 0: host-only (no HIP calls ever)
    ~RendererCore();
    RendererCore(const RendererCore &) = delete;
    RendererCore &operator=(const RendererCore &) = delete;

    void setup();                            // src/RendererCore.cpp:34-44
    void render();                           // src/RendererCore.cpp:138-163 (timed, blocking)
    void renderAsync();                      // same launch, no events / no host sync
    void synchronize();

    // ---- reference-named members (private+friend in the reference)
    void setAlpha();                         // :56-60
    void setMinVal();                        // :62-71
    void setMaxVal();                        // :73-82
    void setMIP();                           // :84-88
    void setUniforms();                      // :100-110
    void setInitialCameraRotation();         // :90-98
    void setupFBO();                         // :184-219
    void setupUBO(bool is_update = false);   // :221-240
    void readVolumeData(std::string fn);     // :242-447
    bool checkRawInfFile(std::string fn);    // :46-54
    bool saveImage(std::string fn, std::string ext);  // :165-182
    void readPixelsRGBA8(uint8_t *rgba8, size_t n_bytes);   // the own target converted on the device: 4x fewer bytes over PCIe
    // Presentation (replaces the on-GPU blit of src/RendererCore.cpp:158-162 for a display that is not this GPU): the frame
    // in `src_frame` (device RGBA32F, fb_w x fb_h; nullptr = this handle's target) is converted to RGBA8 on the launch
    // stream and copied to one of TWO pinned host buffers on a copy stream; returns the frame enqueued by the PREVIOUS call
    // (complete by now: its copy ran under the kernel that followed it), or this one after a wait on the first call.
    const uint8_t *presentRGBA8(const void *src_frame);
    bool loadShader(std::string fn, bool reload);     // :112-136

    Camera main_cam;
    std::vector<float> histogram;
    std::string loaded_dataset, loaded_shader, msg, title;
    float alpha_scale = 1, kerneltime_sum = 0;
    int workgroups_x = 0, workgroups_y = 0, datasize_bytes = -1, min_val = 0, max_val = 0, max_dataset_val = 0,
        min_dataset_val = 0;
    bool use_mip = false, rotate_to_bottom = false, rotate_to_top = false;
    float voxel_size[3] = {1.0f, 1.0f, 1.0f};
    int tex3D_dim[3] = {0, 0, 0};
    int window_size[2] = {0, 0}, framebuffer_size[2] = {0, 0};

    // ---- additions (no reference equivalent)
    void setVolume(const void *host, int nx, int ny, int nz, int bytes, float sx, float sy, float sz);
    void generateSynthetic(int kind, int nx, int ny, int nz, int bytes, uint32_t param);
    void readVolume(void *host, size_t bytes);
    void setLayout(int layout);
    void setQuirks(uint32_t q);               // workgroups_x/y + window uniforms only (camera, messages untouched)
    void setTransferFunction(const int32_t *iso, const float *rgba4, int n);
    void getTransferLut(float *lut1024) const;
    void countSamples(uint64_t *total, uint32_t *per_pixel, size_t n_pixels);
    void readPixels(float *rgba, size_t n_floats);
    void *framebufferDevice() const { return ext_fb_ ? ext_fb_ : d_fb_.get(); }
    void setStream(hipStream_t s) { user_stream_ = s; }
    hipStream_t streamHandle() const { return stream(); }     // the stream the next launch goes to
    bool greyMode() const { return tf_lut_.empty() && frameMode() != FrameMode::Isosurface; }   // r == g == b in every pixel (no transfer function, no isosurface; reslice and shaded composite frames without one are grey)
    void prepareForLaunch() { (void)prepareLaunch(); }   // certification, tile order, packed copy: host work a timed launch should not carry
    void setExternalFramebuffer(void *p) { ext_fb_ = p; }
    void setRowRange(int b, int e) { row_begin_ = b; row_end_ = e; }
    void setRowStripes(int rows, int index, int count);
    void setFramebufferCompact(bool on) { fb_compact_ = on; }
    void setFramebufferFormat(int fmt);      // 0 RGBA32F, 1 (grey, alpha) float2 -- external targets, grey modes
    int localRows() const;   // rows this handle renders (stripe padding included)
    void computeHistogram(float out[256]);
    // best-of-`reps` streaming read of the resident volume; returns GB/s (1e9 bytes per second)
    double measureStreamRead(int reps);
    void assembleShards(const void *gathered, void *frame, int n, int local_rows, int stripe_rows, int channels, void *hip_stream);
    const char *lastKernelName() const { return last_kernel_; }
    // settled entries of the measured work model as a flat blob (vr_export_choices / vr_import_choices): a handle that imports what
    // another handle -- or an earlier process -- measured starts every known configuration on its settled kernel, with no trial frames.
    // A blob is only accepted on the device model and library build it was measured with (returns 0 entries otherwise).
    size_t exportChoices(void *buf, size_t capacity);           // bytes the blob needs; written when capacity suffices
    int importChoices(const void *buf, size_t bytes);           // entries accepted
    int lastLaunchChoice() const { return last_choice_; }     // 1 relay, 2 pipelined loop, 4 short batches, tri_slab << 3, 256: the work model is still exploring this configuration
    size_t lastPacked12Bytes() const { return last_packed12_bytes_; }
    size_t lastApronBytes() const { return last_apron_bytes_; }
    // device memory this handle holds right now, summed from its buffers: the volume being rendered; the optional speed copies
    // (12-bit packed copy, apron copies); every other device buffer (targets, tables, skip grid, staging, the loaded volume, the mesh)
    void residentBytes(uint64_t &volume, uint64_t &copies, uint64_t &other) const;
    // upper bound on the optional copies' total bytes (vr_set_copy_budget).  kCopyBudgetAuto: allowed while the device keeps
    // VolumeCopies::kReserveBytes (and a tenth of its memory) free after the allocation.  Lowering it frees copies that no longer fit.
    static constexpr uint64_t kCopyBudgetAuto = VolumeCopies::kBudgetAuto;
    void setCopyBudget(uint64_t bytes);
    uint64_t copyBudget() const { return copies_.budget(); }
    // The ray-ordered sample stream of a still view (vr_set_ray_stream; vr_stream.hip): NEAREST frames of the
    // fast kernel's modes, with skipping off, are replayed from a copy of the voxels their samples read while the ray geometry
    // (launch_plan.h: rayGeometryKey) stands still.  0 off; 1 automatic: from the 64th consecutive launch of one geometry on,
    // and never on a launch the measured choice wants timed or tried; 2 build at the next eligible launch.  Frames are the same
    // bits either way.  Building blocks once on an 8-byte read-back; the stream counts as a copy (residentBytes, setCopyBudget).
    void setRayStream(int mode);
    int rayStreamMode() const { return ray_stream_mode_; }
    uint64_t rayStreamBytes() const { return copies_.rayStreamBytes(); }
    uint64_t rayStreamElements() const { return copies_.rayStreamElements(); }
    uint64_t rayStreamBuilds() const { return copies_.rayStreamBuilds(); }
    // The stream's format (vr_set_ray_stream_pack; vr_stream_pack.h): 0 never packs, 1 (default) packs a 16-bit volume whose exact
    // range spans at most 4095 when the stream would be larger unpacked than the last-level cache, 2 packs whenever that range
    // allows.  12 bits per sample instead of 16, the same frames bit for bit; a new mode rebuilds the stream.
    void setRayStreamPack(int mode);
    int rayStreamPack() const { return copies_.rayStreamPack(); }
    // The hybrid classification of replayed frames (vr_set_ray_stream_table; vr_stream.h: streamTableEligible): 0 never, 1
    // (default) where eligible on a packed stream whose samples are larger than kStreamTableMinBytes, 2 wherever eligible.  The same
    // frames bit for bit; the stream is not rebuilt.  rayStreamTableUsed: whether the last replayed frame took it.
    void setRayStreamTable(int mode);
    int rayStreamTable() const { return ray_stream_table_; }
    bool rayStreamTableUsed() const { return last_stream_table_; }
    bool hasDevice() const { return device_ >= 0; }
    void warmTrilinear();                    // pre-load the staged TRILINEAR kernel's code objects (once)
    // first-hit isosurface mode (vr_set_isosurface): while on, frames are the shaded surface and its depth, whatever the MIP /
    // composite settings, which are kept for when it is switched off.  iso in the window's units (vr_set_window).
    void setIsosurface(bool enable, int32_t iso);   // enable while reslicing: std::invalid_argument
    bool isosurfaceEnabled() const { return iso_enable_; }
    void readDepth(float *depth, size_t n_floats);   // the last iso frame's depth target (rows x fb_w floats, indexed like the colour target)
    // multi-planar reslice mode (vr_set_reslice): while on, frames are the plane's (slab-reduced) values, windowed; the MIP /
    // composite settings and the camera are kept for when it is switched off.  geom: o, du, dv, dw in voxel index coordinates.
    // enable = false ignores the other arguments; a bad mode / n / geometry, or the isosurface mode being on: std::invalid_argument
    void setReslice(bool enable, const float *geom12, int mode, int n);
    bool resliceEnabled() const { return reslice_enable_; }
    void readResliceValues(float *values, size_t n_floats);   // the last reslice frame's values target (as readDepth)
    // gradient-lit compositing (vr_set_shading): an option of the composite mode -- MIP, isosurface and reslice frames ignore it
    // and keep it.  enable = false ignores the other arguments; a coefficient that is non-finite or < 0, or a shininess outside
    // 1, 2, 4, ..., 128: std::invalid_argument, the state unchanged
    void setShading(bool enable, float ambient, float diffuse, float specular, int shininess);
    void getShading(int *enable, float *ambient, float *diffuse, float *specular, int *shininess) const;
    // Gaussian smoothing of the resident volume (vr_smooth_volume): always computed from the volume AS LOADED, which stays
    // resident beside the smoothed one (d_loaded_); (0, 0, 0) drops the smoothed volume.  A sigma that is not finite or outside
    // [0, 8]: std::invalid_argument; a device allocation that fails: DeviceMemoryError; either way nothing changes.
    void smoothVolume(float sigma_x, float sigma_y, float sigma_z);
    void getSmoothing(float sigma3[3]) const { for (int a = 0; a < 3; a++) sigma3[a] = smooth_sigma_[a]; }
    float lastSmoothMs() const { return last_smooth_ms_; }   // HIP-event time of the last smoothVolume's passes (first launch to last; 0: none ran)
    // upper bound on the bytes of ONE of smoothVolume's two fp32 plane buffers (vr_set_smoothing_workspace); 0: automatic -- the
    // whole volume's planes where they fit in 2 GiB and in the free device memory, z slabs of the volume otherwise
    uint64_t smooth_workspace_limit = 0;
    // grey-level morphology and the median of the resident volume (vr_rank_filter_volume; vr_rank.hip).  The
    // volume being rendered is always G(R(loaded)): R this filter, G smoothVolume's sigmas, both computed again from the volume as
    // loaded by either call.  op outside 0 .. 5 or a radius outside 0 .. 8 (0 .. 1 for the median): std::invalid_argument; a
    // device allocation that fails: DeviceMemoryError; either way nothing changes.  OFF or a box of one voxel reads back (OFF, 0, 0, 0).
    void rankFilterVolume(int op, int rx, int ry, int rz);
    void getRankFilter(int *op, int r3[3]) const { if (op) *op = rank_op_; for (int a = 0; a < 3 && r3; a++) r3[a] = rank_r_[a]; }
    float lastRankMs() const { return last_rank_ms_; }       // HIP-event time of the last rank filter passes (first launch to last; 0: none ran)
    // extraction of the isosurface s = iso of the volume being rendered as an indexed triangle mesh (vr_extract_isosurface;
    // vr_mesh.hip).  The mesh is a snapshot on the device: it stays until the next extraction, freeMesh or the handle's end, and
    // loading or smoothing another volume leaves it alone.  No volume: std::runtime_error; more than 2^32 - 1 vertices or
    // triangles: a queued message and std::invalid_argument; an allocation that fails: DeviceMemoryError; in each case the
    // previous mesh stays.  No rendering state changes.
    void extractIsosurface(int32_t iso, uint64_t *n_vertices, uint64_t *n_triangles);
    bool hasMesh() const { return mesh_.valid; }
    void meshInfo(int32_t *iso, uint64_t *n_vertices, uint64_t *n_triangles) const;
    void readMesh(float *positions, float *normals, uint32_t *triangles, uint64_t vertex_capacity, uint64_t triangle_capacity);
    void saveMesh(const std::string &fn, const std::string &ext);   // "stl" (binary) | "ply" (binary little endian)
    void freeMesh();
    float lastMeshMs() const { return last_mesh_ms_; }   // HIP-event time of the last extraction's kernels (the counting pass plus the emitting pass)
    // upper bound on the bytes of extractIsosurface's per-voxel arrays (vr_set_mesh_workspace; 9 bytes a voxel); 0: automatic --
    // 2 GiB or what the device has free; the extraction runs in z slabs that fit
    uint64_t mesh_workspace_limit = 0;
    // simplification of the resident mesh by vertex clustering on cubic cells of edge `cell` (vr_simplify_mesh; vr_simplify.hip;
    // DESIGN.md section 1.7): replaces the mesh, whichever extraction made it, by its simplification.  A cell that is not a
    // normal number above 0, no mesh: std::invalid_argument; a coordinate / cell of 2^21 or more: a queued message and
    // std::invalid_argument; an allocation that fails: DeviceMemoryError; in each case the previous mesh stays.  No rendering
    // state changes and the labelling is kept.
    void simplifyMesh(float cell, uint64_t *n_vertices, uint64_t *n_triangles);
    // the cell of the simplification that made the resident mesh (0: an extraction did) and the counts of the mesh it was given
    void meshSimplification(float *cell, uint64_t *source_vertices, uint64_t *source_triangles) const;
    float lastSimplifyMs() const { return last_simplify_ms_; }   // HIP-event time of the last simplification's kernels and device sorts
    // smoothing of the resident mesh (vr_smooth_mesh; vr_meshsmooth.hip): `iterations` times a Jacobi step
    // towards the mean of the distinct neighbours with factor lambda, then one with factor mu (skipped when mu == 0); the normals
    // are recomputed from the result; the triangles stay.  With fix_boundary the ends of edges with one triangle do not move.
    // iterations outside [0, 1000], lambda outside (0, 1], mu outside [-2, 0], no mesh: std::invalid_argument; 6 T > 2^32 - 1: a
    // queued message and std::invalid_argument; an allocation that fails: DeviceMemoryError; in each case the previous mesh stays.
    // Calls accumulate: n then m iterations are n + m.  No rendering state changes and the labelling is kept.
    void smoothMesh(int iterations, float lambda, float mu, int fix_boundary);
    // the arguments of the last successful smoothMesh on the resident mesh and its number of fixed vertices; all 0 on a new mesh
    void meshSmoothing(int *iterations, float *lambda, float *mu, int *fix_boundary, uint64_t *fixed_vertices) const;
    // HIP-event times of the last successful smoothMesh: building the graph, and the steps and normals (0: nothing was launched)
    float lastMeshSmoothBuildMs() const { return last_mesh_smooth_build_ms_; }
    float lastMeshSmoothIterateMs() const { return last_mesh_smooth_iterate_ms_; }
    // connected components of the inside voxels (s >= iso) of the volume being rendered under the 14-neighbourhood of the
    // extraction's edge directions (vr_label_components; vr_components.hip).  The labels stay on the device
    // (4 bytes a voxel, under `other`), the records come to the host, where the selection is made.  Unlike the mesh the labelling
    // belongs to the voxels: loading, generating or smoothing a volume drops it; the layout, the window and the quirks do not (it
    // keeps its own iso_s).  No volume: std::runtime_error; more than 2^32 - 2 components: a queued message and
    // std::invalid_argument; an allocation that fails: DeviceMemoryError; a capped loop in a kernel: HipError; in each case the
    // previous labelling stays.  No rendering state changes.
    void labelComponents(int32_t iso, uint64_t *n_components);
    bool hasComponents() const { return comp_.records.valid; }
    void componentsInfo(int32_t *iso, uint64_t *n_components, uint64_t *n_inside, uint64_t *n_selected) const { comp_.records.info(iso, n_components, n_inside, n_selected); }
    void readComponents(uint64_t *voxels, uint64_t *first_voxel, int32_t *bbox6, uint8_t *selected, uint64_t capacity) const { comp_.records.read(voxels, first_voxel, bbox6, selected, capacity); }
    void readLabels(uint32_t *labels, uint64_t n_voxels);
    uint32_t componentAt(int i, int j, int k);
    // selected: voxels >= min_voxels and, when keep_largest > 0, among the keep_largest first by (voxels descending, label ascending)
    uint64_t selectComponents(uint64_t min_voxels, uint64_t keep_largest) { return comp_.records.select(min_voxels, keep_largest); }
    uint64_t selectComponentList(const uint32_t *labels, uint64_t n) { return comp_.records.selectList(labels, n); }   // exactly these; a label of 0 or above n_components: std::invalid_argument, nothing changes
    // extractIsosurface at the labelling's iso value with INSIDE meaning "inside and its component selected": replaces the mesh
    void extractComponents(uint64_t *n_vertices, uint64_t *n_triangles);
    void freeComponents();
    void setComponentIndexBits(int bits);    // aid for tests: 0 automatic (32 below 2^32 - 1 voxels, else 64), 32, 64
    float lastComponentsMs() const { return last_comp_ms_; }   // HIP-event time of the last labelling's kernels

    int filter = 0, accum = 0, skip_empty = 0;
    int layout = 1;          // VR_LAYOUT_BRICKED: the faster HBM layout is the default (vr_set_layout)
    uint32_t quirks = 2u;   // VR_QUIRK_DEFAULT
    int force_generic = 0;
    int pack12 = 1;                          // 1: keep a 12-bit packed copy for the fast kernel when the data allow (vr_set_pack12)
    int tri_apron = 1;                       // 1: keep an apron copy (5x4x4-stored bricks) for the TRILINEAR kernel (vr_set_trilinear_copy)
    int tile_order = 1;      // 1: longest-first tile schedule, 0: arithmetic order
    int autotune = 1;        // 1: kernel variant 0 measures its candidate kernels on the first frames of a configuration and keeps the fastest (vr_set_autotune)
    std::string last_error;

private:
    // the values the kernel sees: the reference's GL uniform state (set by set*())
    struct Uniforms {
        float alpha_scale = 1;
        float voxel_size[3] = {1, 1, 1};
        int min_val = 0, max_val = 0, is_MIP = 0, view_top = 0, view_bottom = 0;
    } u_;
    std::vector<float> cam_block_;           // the "UBO" contents (21 floats)
    bool cs_program_ = false;                // cs_programID != 0
    static constexpr uint32_t kQuirkTruncGrid = 1u << 0, kQuirkU16Offset = 1u << 1;   // VR_QUIRK_*

    int device_ = -1;
    hipStream_t own_stream_ = nullptr, user_stream_ = nullptr;
    Event ev0_, ev1_;
    DeviceBuffer<uint8_t> d_vol_;            // the volume the kernels render: as loaded, or rank-filtered and / or smoothed
    DeviceBuffer<uint8_t> d_loaded_;         // while d_vol_ is a filtered volume: the loaded one (same dimensions, type and layout)
    float smooth_sigma_[3] = {0.0f, 0.0f, 0.0f};
    float last_smooth_ms_ = 0.0f;
    int rank_op_ = 0, rank_r_[3] = {0, 0, 0};
    float last_rank_ms_ = 0.0f;
    // the one place that renders G(R(loaded)) for a new (op, r3, sigma): computes, swaps in, scans the ranges, adopts the state
    void applyVolumeFilters(const char *who, int op, const int r3[3], const float sigma[3]);
    ResidentMesh mesh_;                      // the extracted mesh with its simplification and smoothing records (resident_mesh.h)
    float last_mesh_ms_ = 0.0f, last_simplify_ms_ = 0.0f;
    float last_mesh_smooth_build_ms_ = 0.0f, last_mesh_smooth_iterate_ms_ = 0.0f;
    // the shared body of extractIsosurface and extractComponents; selected: selection_plane's bits or nullptr; ms: kernel time so far
    void extractMesh(int32_t iso, float iso_s, const uint64_t *selected, float ms, uint64_t *n_vertices, uint64_t *n_triangles);
    Labelling comp_;                         // the labelling: records on the host (component_records.h), labels on the device
    int comp_index_bits_ = 0;                // setComponentIndexBits
    float last_comp_ms_ = 0.0f;
    DeviceQueue queue() const { return {stream(), ev0_, ev1_}; }   // what the algorithms of volume_ops.h launch on and time with
    // runs one of them: a RefusalWithMessage queues its message for the GUI and goes on as it is
    template <class F>
    auto queueingRefusals(F &&call) -> decltype(call())
    {
        try {
            return call();
        } catch (const RefusalWithMessage &r) {
            setMessage("Error!", r.message);
            throw;
        }
    }
    // geometry and voxel type of the volume that is RESIDENT (set only after a successful upload).
    // tex3D_dim / datasize_bytes above are GUI inputs of readVolumeData, like the reference's fields;
    // the reference's shader reads textureSize() of the uploaded texture (VolumeRenderer.cs:62), not them.
    int res_dims_[3] = {0, 0, 0};
    int res_bytes_ = 0;
    int vol_layout_ = 0;
    DeviceBuffer<float4> d_fb_;
    void *ext_fb_ = nullptr;                 // borrowed
    DeviceBuffer<float4> d_tf_;
    DeviceBuffer<uint32_t> d_spp_;
    DeviceBuffer<unsigned> d_scratch_;       // 4 + 256 words (+ slack)
    std::vector<float> tf_lut_;              // 256 x RGBA, empty = grey ramp
    bool tf_grey_ = false;                   // every entry of tf_lut_ has r == g == b bit for bit
    int exact_min_ = 0, exact_max_ = 65535;   // exact voxel range of the resident volume
    int row_begin_ = 0, row_end_ = -1;
    bool iso_enable_ = false;
    int32_t iso_value_ = 0;
    DeviceBuffer<float> d_depth_;            // depth target of the iso frames (+inf where no surface; allocated on the first one)
    int depth_rows_ = -1, depth_w_ = 0;      // rows x width the last iso frame's depth is indexed by (-1: no iso frame yet)
    float storedIso(int32_t iso) const;      // an iso value in stored voxel units (the +1000 of VR_QUIRK_U16_OFFSET included)
    float isoStored() const { return storedIso(iso_value_); }   // ... the isosurface mode's
    bool reslice_enable_ = false;
    float reslice_geom_[12] = {};            // o, du, dv, dw (vr_reslice.h: ResliceGeom)
    int reslice_mode_ = 0, reslice_n_ = 1;   // VR_SLAB_*, slab samples
    DeviceBuffer<float> d_values_;           // values target of the reslice frames (NaN where no sample; allocated on the first one)
    int values_rows_ = -1, values_w_ = 0;    // rows x width the last reslice frame's values are indexed by (-1: no reslice frame yet)
    bool shade_enable_ = false;
    float shade_k_[3] = {0.15f, 0.65f, 0.2f};   // ambient, diffuse, specular (the isosurface mode's constants)
    int shade_shininess_ = 16;
    FrameMode frameMode() const   // of the next frame
    {
        if (iso_enable_) return FrameMode::Isosurface;
        if (reslice_enable_) return FrameMode::Reslice;
        return (shade_enable_ && u_.is_MIP != 1) ? FrameMode::Shaded : FrameMode::RayMarch;
    }
    int stripe_rows_ = 0, stripe_index_ = 0, stripe_count_ = 1;
    bool fb_compact_ = false;
    int fb_format_ = 0;
    std::map<uint32_t, bool> cert_cache_;    // divisor bits -> certified
    DeviceBuffer<uint8_t> d_rgba8_;          // RGBA8 staging of the target (readPixelsRGBA8)
    static constexpr int kPresentSlots = 3;  // the frame handed out by call n (slot (n - 1) % 3) is written again by call n + 2: valid until the next-but-one call
    DeviceBuffer<uint8_t> d_present_[kPresentSlots];   // presentRGBA8: device staging per slot (all of one size, or all empty)
    PinnedBuffer h_present_[kPresentSlots];  // ... and pinned host frames
    Event present_converted_[kPresentSlots], present_copied_[kPresentSlots];
    hipStream_t present_stream_ = nullptr;
    int present_count_ = 0;                  // frames enqueued so far
    void releasePresent();
    VolumeCopies copies_;                    // the packed copy, the apron copies and the skip grid: built lazily from d_vol_, dropped with its voxels
    ResidentVolume residentVolume() const { return {d_vol_.get(), res_dims_[0], res_dims_[1], res_dims_[2], res_bytes_, vol_layout_, exact_min_, exact_max_, stream()}; }
    size_t last_packed12_bytes_ = 0, last_apron_bytes_ = 0;   // packed copy / apron copies used by the last launch (0 = none)
    void refreshPacked12(FrameParams &P, LaunchConfig &L);
    void refreshApron(const FrameParams &P, LaunchConfig &L);
    void refreshSkipGrid(FrameParams &P, LaunchConfig &L);
    void refuseIsoGreyAlpha() const;
    bool ensureSkipGrid();                   // build the dilated cell-max grid if it is not resident; false = the volume is too large for it
    // everything one launch needs, decided before it (prepareLaunch) and handed to it (launchKernel)
    struct PreparedLaunch {
        FrameParams P;                       // (both zeroed by buildFrame)
        LaunchConfig L;
        float4 *fb = nullptr;                // the colour target
        FrameMode mode = FrameMode::RayMarch;
        const uint16_t *skip_grid = nullptr; // the isosurface and the shaded kernel: the grid they skip on (nullptr = no skipping) ...
        int skip_thresh = 0;                 // ... and the shaded kernel's threshold (the ray-march kernels carry theirs in P and L)
        LaunchTuner::Pick pick;              // the tuner's decision (measure: the launch is a measurement)
        bool stream_eligible = false;        // a frame the ray-ordered sample stream could replay (rayStreamEligible) ...
        RayGeometryKey stream_key;           // ... and its geometry
        bool replay = false;                 // engageRayStream: this launch reads the stream
    };
    int ray_stream_mode_ = 1;
    int ray_stream_table_ = 1;               // vr_set_ray_stream_table
    bool last_stream_table_ = false;         // the last replayed frame classified a share of its samples through the table
    uint64_t volume_generation_ = 0;        // counts the writers of d_vol_ (dropDerived)
    bool still_key_valid_ = false;
    RayGeometryKey still_key_;               // the geometry of the last eligible launch ...
    int still_launches_ = 0;                 // ... and how many consecutive launches have had it
    void engageRayStream(PreparedLaunch &F, const uint32_t *spp);   // counts the launch; builds / selects the stream by the mode's rule
    hipError_t launchKernel(const PreparedLaunch &F, uint32_t *spp);   // the ray-march, the iso, the reslice or the shaded kernel
    TileTables tiles_;                       // the work-ordered block -> tile tables the specialised kernels walk
    const char *last_kernel_ = "";
    bool tslab_warm_ = false;
    // ---- measured work model (kernel variant 0; launch_tuner.h): the tuner decides which candidate kernel a launch runs, this
    // class enumerates the candidates and times the measurement launches (HIP events on the launch stream, polled without blocking)
    LaunchTuner tuner_;
    static constexpr int kTuneSlots = 12;    // asynchronous measurements that may be in flight (a burst of renderAsync calls)
    struct TuneSlot { Event ev0, ev1; uint64_t key = 0, gen = 0; int cand = -1; };   // cand: the candidate VALUE (bit set), not its index in the entry's shuffled order
    TuneSlot tune_slot_[kTuneSlots];
    int tune_head_ = 0, tune_count_ = 0;     // ring of in-flight slots: oldest at tune_head_
    int last_choice_ = 0;                    // candidate bits of the last launch (vr_get_launch_choice)
    void tuneChoose(PreparedLaunch &F);
    void tuneCollect();
    void noMeasuredChoice() { last_choice_ = 0; }   // a frame of a mode with one kernel (isosurface, reslice, shaded)

    hipStream_t stream() const { return user_stream_ ? user_stream_ : own_stream_; }
    void requireDevice(const char *what) const;
    void check(hipError_t e, const std::string &what) const { hipCheck(e, what); }
    void warmUnits(int group);               // one empty launch per code object of a WarmGroup (vr_code_unit.h)
    void freeVolume();
    void dropDerived();                      // everything built from the voxels of d_vol_: packed copy, apron copies, skip grid, the tile order under skipping
    void allocVolume(int nx, int ny, int nz, int bytes, int layout);
    DeviceBuffer<uint8_t> allocVolumeBuffer(int nx, int ny, int nz, int bytes, int layout);   // allocVolume's storage contract: zeroed brick padding, the slack slab
    size_t storageVoxels(int nx, int ny, int nz, int layout) const;
    void afterVolumeLoaded(const std::string &name);
    void scanDatasetRange();
    bool certifyDivisor(float b);
    void buildFrame(FrameParams &P, LaunchConfig &L);
    PreparedLaunch prepareLaunch();
    void setSkipCells(FrameParams &P) const;
    void growFloatTarget(DeviceBuffer<float> &d, int fill, const char *name);
    void launch(uint32_t *spp, bool blocking);   // blocking: timed into kerneltime_sum (render)
    void updateWorkgroups();
    void setMessage(const std::string &t, const std::string &m) { title = t; msg = m; }
};

}  // namespace vr
