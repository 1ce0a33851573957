// renderer_core.cpp -- see renderer_core.h.  Host side of the ray-march path:
// owns the HBM objects (volume, RGBA32F target, transfer-function table), turns the
// reference's uniform/UBO state into the kernel's FrameParams and launches it.
// Compiled with -ffp-contract=off: buildFrame() repeats the fp32 operations of the
// shader's main() (VolumeRenderer.cs:62-83,109) in the shader's order.
#include "renderer_core.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

#include "launch_plan.h"
#include "tile_schedule.h"
#include "volume_io.h"
#include "vr_code_unit.h"
#include "vr_iso.h"
#include "vr_reslice.h"
#include "vr_shade.h"
#include "vr_smooth.h"
#include "vr_components.h"
#include "vr_mesh.h"
#include "vr_simplify.h"
#include "vr_kernels.h"
#include "vr_stream.h"

namespace vr {

namespace {
constexpr int kLocalSize = 16;   // layout(local_size_x = 16, local_size_y = 16), VolumeRenderer.cs:3
}  // namespace

RendererCore::RendererCore(int device) : main_cam(30), histogram(256, 0.0f), device_(device)
{
    if (device_ >= 0) {
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess || n <= 0) throw NoDeviceError("no HIP device available");
        if (device_ >= n) throw NoDeviceError("HIP device ordinal out of range");
        check(hipSetDevice(device_), "hipSetDevice");
        check(hipStreamCreateWithFlags(&own_stream_, hipStreamNonBlocking), "hipStreamCreate");
        ev0_.create(); ev1_.create();
        for (TuneSlot &s : tune_slot_) { s.ev0.create(); s.ev1.create(); }
        d_scratch_.alloc(264, "scratch");
    }
}

RendererCore::~RendererCore()
{
    if (device_ >= 0) {
        (void)hipSetDevice(device_);
        (void)hipStreamSynchronize(stream());
        if (present_stream_) { (void)hipStreamSynchronize(present_stream_); (void)hipStreamDestroy(present_stream_); }
        if (own_stream_) (void)hipStreamDestroy(own_stream_);
    }
}   // (the buffers and events release themselves after this body: nothing is in flight, and releasing them needs no stream)

void RendererCore::requireDevice(const char *what) const
{
    if (device_ < 0) throw NoDeviceError(std::string(what) + ": host-only handle, no HIP device");
    hipCheck(hipSetDevice(device_), "hipSetDevice");
}

// ---------------------------------------------------------------- setup / FBO / UBO
void RendererCore::setup()
{
    setupFBO();
}

void RendererCore::setupFBO()
{
    if (framebuffer_size[0] <= 0 || framebuffer_size[1] <= 0)
        throw std::runtime_error("Framebuffer not complete. Error code: zero-sized framebuffer");
    if (device_ < 0) return;   // host-only handle: nothing to allocate
    requireDevice("setupFBO");
    const size_t n = (size_t)framebuffer_size[0] * (size_t)framebuffer_size[1];
    d_fb_.alloc(n, "framebuffer");
    check(hipMemsetAsync(d_fb_.get(), 0, n * sizeof(float4), stream()), "hipMemset(framebuffer)");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
}

void RendererCore::setupUBO(bool)
{
    cam_block_.clear();
    main_cam.setUBO(cam_block_);
}

// ---------------------------------------------------------------- uniforms
void RendererCore::setAlpha()
{
    if (cs_program_) u_.alpha_scale = alpha_scale;
}

void RendererCore::setMinVal()
{
    if (cs_program_) u_.min_val = (datasize_bytes == 2 && (quirks & kQuirkU16Offset)) ? min_val + 1000 : min_val;
}

void RendererCore::setMaxVal()
{
    if (cs_program_) u_.max_val = (datasize_bytes == 2 && (quirks & kQuirkU16Offset)) ? max_val + 1000 : max_val;
}

void RendererCore::setMIP()
{
    if (cs_program_) u_.is_MIP = use_mip ? 1 : 0;
}

void RendererCore::setInitialCameraRotation()
{
    if (cs_program_) {
        main_cam.resetCamera();
        main_cam.is_changed = true;
        u_.view_top = rotate_to_top ? 1 : 0;
        u_.view_bottom = rotate_to_bottom ? 1 : 0;
    }
}

void RendererCore::setUniforms()
{
    if (cs_program_) {
        u_.voxel_size[0] = voxel_size[0];
        u_.voxel_size[1] = voxel_size[1];
        u_.voxel_size[2] = voxel_size[2];
    }
    setAlpha();
    setMinVal();
    setMaxVal();
    setMIP();
    setInitialCameraRotation();
}

bool RendererCore::loadShader(std::string fn, bool reload)
{
    // The kernel is compiled into this library; `fn` is only recorded so the GUI's
    // "shader loaded" state (RendererGUI.cpp:150) behaves the same.
    if (reload) fn = loaded_shader;
    if (fn.empty()) {
        setMessage("Error!", "Failed to open Shader file.");
        loaded_shader.clear();
        return false;
    }
    const size_t idx = fn.find_last_of('/');
    loaded_shader = idx == std::string::npos ? fn : fn.substr(idx + 1);
    cs_program_ = true;
    updateWorkgroups();
    // the reference compiles + links the shader here (:112-118); the HIP code objects are loaded now
    // instead of by the first render() (a cold first launch costs ~16 ms)
    if (device_ >= 0) {
        requireDevice("loadShader");
        warmUnits(WARM_LOAD_SHADER);
        check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
        tslab_warm_ = false;
        if (filter == 1) warmTrilinear();
    }
    u_.alpha_scale = alpha_scale;
    if (!loaded_dataset.empty()) {
        setUniforms();
        main_cam.resetCamera();
        main_cam.is_changed = true;
    }
    setMessage("Shader Loaded!", "Shader Loaded Successfully!");
    return true;
}

void RendererCore::updateWorkgroups()
{
    if (quirks & kQuirkTruncGrid) {
        workgroups_x = window_size[0] / kLocalSize;   // src/RendererCore.cpp:121-122
        workgroups_y = window_size[1] / kLocalSize;
    } else {
        workgroups_x = (window_size[0] + kLocalSize - 1) / kLocalSize;
        workgroups_y = (window_size[1] + kLocalSize - 1) / kLocalSize;
    }
}

void RendererCore::setQuirks(uint32_t q)
{
    quirks = q;
    setMinVal(); setMaxVal();                 // Q10 changes what the kernel sees as the window
    if (cs_program_) updateWorkgroups();      // Q1 changes the dispatch grid; nothing else is touched
}

// ---------------------------------------------------------------- volume
size_t RendererCore::storageVoxels(int nx, int ny, int nz, int lay) const
{
    if (lay == 0) return (size_t)nx * (size_t)ny * (size_t)nz;
    return (size_t)bricksX(nx) * (size_t)bricksY(ny) * (size_t)bricksZ(nz) * 64u;
}

void RendererCore::freeVolume()
{
    d_vol_.reset(); d_loaded_.reset();
    smooth_sigma_[0] = smooth_sigma_[1] = smooth_sigma_[2] = 0.0f;
    rank_op_ = 0; rank_r_[0] = rank_r_[1] = rank_r_[2] = 0;
    res_dims_[0] = res_dims_[1] = res_dims_[2] = 0; res_bytes_ = 0;
    dropDerived();
    freeComponents();                                                    // the labelling belongs to the voxels that just went
}

void RendererCore::dropDerived()
{
    tiles_.invalidateSkipOrder();                                        // (an order built on the old volume's visibility)
    copies_.dropAll();
    volume_generation_++;                                                // new voxels: no ray-ordered sample stream of the old ones is this volume's
    still_key_valid_ = false;
    still_launches_ = 0;
}

DeviceBuffer<uint8_t> RendererCore::allocVolumeBuffer(int nx, int ny, int nz, int bytes, int lay)
{
    // + one x/y slab of slack so a one-past-the-edge index can never fault
    const size_t need = (storageVoxels(nx, ny, nz, lay) + (size_t)nx * (size_t)ny + 256) * (size_t)bytes;
    DeviceBuffer<uint8_t> p(need, "volume");
    if (lay != 0) check(hipMemsetAsync(p.get(), 0, need, stream()), "hipMemset(volume)");
    return p;
}

void RendererCore::allocVolume(int nx, int ny, int nz, int bytes, int lay)
{
    requireDevice("volume upload");
    freeVolume();
    d_vol_ = allocVolumeBuffer(nx, ny, nz, bytes, lay);
    vol_layout_ = lay;
}

void RendererCore::setVolume(const void *host, int nx, int ny, int nz, int bytes, float sx, float sy, float sz)
{
    if (!host || nx <= 0 || ny <= 0 || nz <= 0 || (bytes != 1 && bytes != 2))
        throw std::invalid_argument("setVolume: bad dimensions or datasize_bytes");
    requireDevice("setVolume");
    // nx*ny*nz*bytes must not wrap (three ints of up to 2^31 each): bound it at 2^48 bytes by division
    if ((uint64_t)nx > (1ull << 48) / (uint64_t)ny / (uint64_t)nz / (uint64_t)bytes)
        throw std::invalid_argument("setVolume: volume too large");
    const size_t lin_bytes = (size_t)nx * (size_t)ny * (size_t)nz * (size_t)bytes;
    const uint32_t bnx = bricksX(nx), bny = bricksY(ny);
    if (layout == 0) {
        allocVolume(nx, ny, nz, bytes, 0);
        check(hipMemcpyAsync(d_vol_.get(), host, lin_bytes, hipMemcpyHostToDevice, stream()), "hipMemcpy(volume)");
    } else {
        DeviceBuffer<uint8_t> staging(lin_bytes, "staging");
        hipError_t e = hipMemcpyAsync(staging.get(), host, lin_bytes, hipMemcpyHostToDevice, stream());
        if (e == hipSuccess) {
            allocVolume(nx, ny, nz, bytes, 1);
            e = launch_relayout(staging.get(), d_vol_.get(), bytes, (uint32_t)nx, (uint32_t)ny, (uint32_t)nz, bnx, bny, 0, stream());
        }
        if (e == hipSuccess) e = hipStreamSynchronize(stream());
        check(e, "volume relayout");
    }
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
    res_dims_[0] = nx; res_dims_[1] = ny; res_dims_[2] = nz; res_bytes_ = bytes;   // what is resident now
    tex3D_dim[0] = nx; tex3D_dim[1] = ny; tex3D_dim[2] = nz;
    voxel_size[0] = sx; voxel_size[1] = sy; voxel_size[2] = sz;
    datasize_bytes = bytes;
    afterVolumeLoaded("<memory>");
}

void RendererCore::generateSynthetic(int kind, int nx, int ny, int nz, int bytes, uint32_t param)
{
    if (nx <= 0 || ny <= 0 || nz <= 0 || (bytes != 1 && bytes != 2) || (kind != 0 && kind != 1 && kind != 2) ||
        (kind == 0 && bytes != 1) || (kind == 2 && bytes != 2))
        throw std::invalid_argument("generateSynthetic: bad arguments");
    if ((uint64_t)nx > (1ull << 48) / (uint64_t)ny / (uint64_t)nz / (uint64_t)bytes)
        throw std::invalid_argument("generateSynthetic: volume too large");
    requireDevice("generateSynthetic");
    allocVolume(nx, ny, nz, bytes, layout);
    check(launch_gen_volume(d_vol_.get(), bytes, kind, (uint32_t)nx, (uint32_t)ny, (uint32_t)nz, param, layout,
                            bricksX(nx), bricksY(ny), stream()),
          "gen_volume_kernel");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
    res_dims_[0] = nx; res_dims_[1] = ny; res_dims_[2] = nz; res_bytes_ = bytes;   // what is resident now
    tex3D_dim[0] = nx; tex3D_dim[1] = ny; tex3D_dim[2] = nz;
    voxel_size[0] = voxel_size[1] = voxel_size[2] = 1.0f;
    datasize_bytes = bytes;
    afterVolumeLoaded(kind == 0 ? "<synthetic sphere>" : (kind == 1 ? "<synthetic noise ball>" : "<synthetic noise ball + 1000>"));
}

void RendererCore::readVolume(void *host, size_t bytes)
{
    requireDevice("readVolume");
    if (!d_vol_) throw std::runtime_error("readVolume: no dataset loaded");
    const size_t lin_bytes = (size_t)res_dims_[0] * res_dims_[1] * res_dims_[2] * (size_t)res_bytes_;
    if (!host || bytes < lin_bytes) throw std::invalid_argument("readVolume: buffer too small");
    if (vol_layout_ == 0) {
        check(hipMemcpyAsync(host, d_vol_.get(), lin_bytes, hipMemcpyDeviceToHost, stream()), "hipMemcpy(D2H volume)");
        check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
        return;
    }
    DeviceBuffer<uint8_t> staging(lin_bytes, "staging");
    hipError_t e = launch_relayout(d_vol_.get(), staging.get(), res_bytes_, (uint32_t)res_dims_[0], (uint32_t)res_dims_[1],
                                   (uint32_t)res_dims_[2], bricksX(res_dims_[0]),
                                   bricksY(res_dims_[1]), 1, stream());
    if (e == hipSuccess) e = hipMemcpyAsync(host, staging.get(), lin_bytes, hipMemcpyDeviceToHost, stream());
    if (e == hipSuccess) e = hipStreamSynchronize(stream());
    check(e, "readVolume");
}

void RendererCore::setLayout(int lay)
{
    if (lay != 0 && lay != 1) throw std::invalid_argument("setLayout: unknown layout");
    layout = lay;
    if (!d_vol_ || vol_layout_ == lay) return;
    requireDevice("setLayout");
    const int nx = res_dims_[0], ny = res_dims_[1], nz = res_dims_[2], bytes = res_bytes_;
    // the rendered volume and, beside a smoothed one, the loaded volume: both into new storage, then moved in together
    // (a failure leaves the handle as it was: `fresh` frees itself, which waits for the kernels); the smoothing is not computed again
    DeviceBuffer<uint8_t> fresh[2], *old[2] = {&d_vol_, &d_loaded_};
    hipError_t e = hipSuccess;
    for (int b = 0; b < 2 && e == hipSuccess; b++) {
        if (!*old[b]) continue;
        fresh[b] = allocVolumeBuffer(nx, ny, nz, bytes, lay);
        e = launch_relayout(old[b]->get(), fresh[b].get(), bytes, (uint32_t)nx, (uint32_t)ny, (uint32_t)nz, bricksX(nx), bricksY(ny), lay == 0 ? 1 : 0, stream());
    }
    const hipError_t es = hipStreamSynchronize(stream());
    check(e == hipSuccess ? es : e, "relayout");
    d_vol_ = std::move(fresh[0]); d_loaded_ = std::move(fresh[1]);
    vol_layout_ = lay;
    dropDerived();
}

// min/max scan of src/RendererCore.cpp:360-384 as a device reduction
void RendererCore::scanDatasetRange()
{
    // scratch: [0..1] reference-style min/max (index 8390640 skipped), [2..3] exact min/max
    const unsigned init[4] = {0xffffffffu, 0u, 0xffffffffu, 0u};
    check(hipMemcpyAsync(d_scratch_.get(), init, sizeof(init), hipMemcpyHostToDevice, stream()), "hipMemcpy(scratch)");
    check(launch_stats(d_vol_.get(), res_bytes_, (uint32_t)res_dims_[0], (uint32_t)res_dims_[1], (uint32_t)res_dims_[2],
                       vol_layout_, bricksX(res_dims_[0]), bricksY(res_dims_[1]), 0, 1.0f,
                       d_scratch_.get(), d_scratch_.get() + 4, stream()),
          "stats_kernel");
    unsigned mm[4];
    check(hipMemcpyAsync(mm, d_scratch_.get(), sizeof(mm), hipMemcpyDeviceToHost, stream()), "hipMemcpy(scratch)");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
    exact_min_ = (int)mm[2];
    exact_max_ = (int)mm[3];
    if (res_bytes_ == 2) {
        // reference initial values: max_value = -1, min_value = 9000000
        const int mx = mm[1] == 0u && mm[0] == 0xffffffffu ? -1 : (int)mm[1];
        const int mn = mm[0] == 0xffffffffu ? 9000000 : (int)mm[0];
        max_val = max_dataset_val = mx;
        min_val = min_dataset_val = mn;
    } else {
        min_val = min_dataset_val = 0;
        max_val = max_dataset_val = 255;
    }
}

void RendererCore::computeHistogram(float out[256])
{
    requireDevice("histogram");
    if (!d_vol_) throw std::runtime_error("histogram: no dataset loaded");
    check(hipMemsetAsync(d_scratch_.get(), 0, sizeof(unsigned) * 264, stream()), "hipMemset(scratch)");
    check(launch_stats(d_vol_.get(), res_bytes_, (uint32_t)res_dims_[0], (uint32_t)res_dims_[1], (uint32_t)res_dims_[2],
                       vol_layout_, bricksX(res_dims_[0]), bricksY(res_dims_[1]), 1,
                       (float)max_dataset_val, d_scratch_.get(), d_scratch_.get() + 4, stream()),
          "stats_kernel");
    unsigned counts[256];
    check(hipMemcpyAsync(counts, d_scratch_.get() + 4, sizeof(counts), hipMemcpyDeviceToHost, stream()), "hipMemcpy(hist)");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
    // src/RendererCore.cpp:361,400-405: the normaliser starts from the dataset max
    // (16-bit) or -1 (8-bit) and is raised to the largest bin count
    double max_value = res_bytes_ == 2 ? (double)max_dataset_val : -1.0;
    for (int i = 1; i < 256; i++) max_value = std::max(max_value, (double)counts[i]);
    // a volume of zeros (X, the voxel the range scan skips, apart): the normaliser is 0 and the reference's own arithmetic is
    // undefined; every bin is 0 here (deviations)
    const bool empty = !(max_value > 0.0);
    for (int i = 0; i < 256; i++) {
        histogram[i] = (i == 0 || empty) ? 0.0f : (float)counts[i] * 100.0f / (float)max_value;
        out[i] = histogram[i];
    }
}

// the receiving rank's half of the multi-process gather (vr_assemble_shards): de-interleave + (grey, alpha) expansion
void RendererCore::assembleShards(const void *gathered, void *frame, int n, int local_rows, int stripe_rows, int channels, void *hip_stream)
{
    requireDevice("assembleShards");
    if (!gathered || !frame) throw std::invalid_argument("assembleShards: null buffer");
    if (framebuffer_size[0] <= 0 || framebuffer_size[1] <= 0) throw std::runtime_error("assembleShards: setup() has not run");
    if (n < 1 || local_rows < 1 || stripe_rows < 0 || (channels != 2 && channels != 4)) throw std::invalid_argument("assembleShards: bad shard geometry");
    // every frame row must exist in the gather buffer
    const long long rows_held = stripe_rows == 0 ? (long long)n * local_rows
                                                 : (long long)(local_rows / stripe_rows) * n * stripe_rows;
    if (rows_held < framebuffer_size[1] || (stripe_rows > 0 && local_rows % stripe_rows != 0)) throw std::invalid_argument("assembleShards: the shards do not cover the frame");
    check(launch_assemble(gathered, static_cast<float4 *>(frame), framebuffer_size[0], framebuffer_size[1], n, local_rows, stripe_rows, channels,
                          hip_stream ? static_cast<hipStream_t>(hip_stream) : stream()), "assemble kernel");
}

double RendererCore::measureStreamRead(int reps)
{
    requireDevice("measureStreamRead");
    if (!d_vol_) throw std::runtime_error("measureStreamRead: no dataset loaded");
    const uint64_t bytes = (uint64_t)storageVoxels(res_dims_[0], res_dims_[1], res_dims_[2], vol_layout_) * (uint64_t)res_bytes_ & ~15ull;
    Event a, b; a.create(); b.create();
    double best_ms = 1e30;
    hipError_t e = hipMemsetAsync(d_scratch_.get(), 0, sizeof(unsigned), stream());
    for (int r = 0; r < std::max(reps, 1) + 1 && e == hipSuccess; r++) {      // first pass warms up
        e = hipEventRecord(a, stream());
        if (e == hipSuccess) e = launch_stream_read(d_vol_.get(), bytes, d_scratch_.get(), stream());
        if (e == hipSuccess) e = hipEventRecord(b, stream());
        if (e == hipSuccess) e = hipEventSynchronize(b);
        float ms = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
        if (r > 0 && (double)ms < best_ms) best_ms = (double)ms;
    }
    check(e, "stream_read_kernel");
    return (double)bytes / (best_ms * 1e-3) / 1e9;
}

void RendererCore::afterVolumeLoaded(const std::string &name)
{
    scanDatasetRange();
    setMessage("File Loaded!", "File Loaded Successfully!");
    if (!loaded_shader.empty()) {
        setUniforms();
        main_cam.resetCamera();
        main_cam.is_changed = true;
    }
    const size_t idx = name.find_last_of('/');
    loaded_dataset = idx == std::string::npos ? name : name.substr(idx + 1);
}

bool RendererCore::checkRawInfFile(std::string fn)
{
    std::ifstream inf_file(fn + ".inf");
    return bool(inf_file);
}

void RendererCore::readVolumeData(std::string fn)
{
    if (fn.size() < 3) { setMessage("Error!", "Failed to Open RAW file..."); return; }
    if (datasize_bytes != 1 && datasize_bytes != 2) {
        setMessage("Error!", "Select the data size (UINT8/UINT16) before loading a dataset.");
        return;
    }
    const std::string ext = fn.substr(fn.length() - 3, 3);
    std::vector<uint8_t> voxels;
    int dims[3];
    float spacing[3];
    if (ext == "raw") {
        if (checkRawInfFile(fn)) {
            RawInf inf;
            std::string t, m;
            if (!parseRawInf(fn + ".inf", inf, t, m)) { setMessage(t, m); return; }
            for (int i = 0; i < 3; i++) { dims[i] = inf.dims[i]; spacing[i] = inf.spacing[i]; }
        } else {
            // no sidecar: use the values typed into the GUI and write one (:304-317)
            for (int i = 0; i < 3; i++) { dims[i] = tex3D_dim[i]; spacing[i] = voxel_size[i]; }
            writeRawInf(fn + ".inf", dims, spacing);
        }
        const uint64_t len = (uint64_t)std::max(dims[0], 0) * (uint64_t)std::max(dims[1], 0) * (uint64_t)std::max(dims[2], 0);
        {
            std::ifstream probe(fn, std::ios::binary);
            if (!probe) { setMessage("Error!", "Failed to Open RAW file..."); return; }
        }
        if (len == 0) {
            setMessage("Invalid Data Size!",
                       "Texture Dimensions shouldn't contain any zeroes. Please provide a valid .raw.inf file.");
            return;
        }
        if (!readRawFile(fn, len * (uint64_t)datasize_bytes, voxels)) {
            setMessage("Error!", "Failed to Open RAW file...");
            return;
        }
    } else {
        PvmVolume pvm;
        std::string err;
        if (!readPVMvolume(fn, pvm, err)) { setMessage("Error!", "Error reading PVM file"); last_error = err; return; }
        dims[0] = (int)pvm.width; dims[1] = (int)pvm.height; dims[2] = (int)pvm.depth;
        spacing[0] = pvm.scalex; spacing[1] = pvm.scaley; spacing[2] = pvm.scalez;
        if ((int)pvm.components != datasize_bytes) {
            // the reference reinterprets the payload with the GUI-selected size and
            // reads out of bounds when they disagree; refuse instead
            setMessage("Error!", "Error reading PVM file");
            last_error = "PVM component count does not match datasize_bytes";
            return;
        }
        voxels.swap(pvm.data);   // Q9: 16-bit payload bytes are taken in host order, no swap (:347,368,393)
    }
    std::cout << "Dataset dimensions: " << dims[0] << ", " << dims[1] << ", " << dims[2] << std::endl;
    std::cout << "Dataset Aspect ratio: " << spacing[0] << ", " << spacing[1] << ", " << spacing[2] << std::endl;
    const int bytes = datasize_bytes;
    setVolume(voxels.data(), dims[0], dims[1], dims[2], bytes, spacing[0], spacing[1], spacing[2]);
    const size_t idx = fn.find_last_of('/');
    loaded_dataset = idx == std::string::npos ? fn : fn.substr(idx + 1);
}

// ---------------------------------------------------------------- transfer function
void RendererCore::setTransferFunction(const int32_t *iso, const float *rgba4, int n)
{
    if (n == 0) {
        tf_lut_.clear();
        return;
    }
    std::vector<float> lut;
    if (!iso || !rgba4 || !buildSplineLUT(iso, rgba4, n, lut))
        throw std::invalid_argument("setTransferFunction: need >= 2 knots with ascending iso values");
    tf_lut_.swap(lut);
    tf_grey_ = true;                         // r == g == b bit for bit in every entry (the reference's black -> white ramp always is)
    for (size_t e = 0; e < tf_lut_.size() / 4 && tf_grey_; e++)
        tf_grey_ = std::memcmp(&tf_lut_[4 * e], &tf_lut_[4 * e + 1], sizeof(float)) == 0 && std::memcmp(&tf_lut_[4 * e], &tf_lut_[4 * e + 2], sizeof(float)) == 0;
    if (device_ >= 0) {
        requireDevice("setTransferFunction");
        d_tf_.ensure(256, "tf");
        check(hipMemcpyAsync(d_tf_.get(), tf_lut_.data(), 256 * sizeof(float4), hipMemcpyHostToDevice, stream()), "hipMemcpy(tf)");
        check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
    }
}

void RendererCore::getTransferLut(float *lut) const
{
    if (tf_lut_.empty()) {
        for (int i = 0; i < 256; i++) lut[4 * i] = lut[4 * i + 1] = lut[4 * i + 2] = lut[4 * i + 3] = (float)i / 255.0f;
    } else {
        std::memcpy(lut, tf_lut_.data(), sizeof(float) * 1024);
    }
}

// ---------------------------------------------------------------- render
void RendererCore::setRowStripes(int rows, int index, int count)
{
    if (count < 1 || index < 0 || index >= count || (count > 1 && rows < 1))
        throw std::invalid_argument("setRowStripes: bad stripe spec");
    stripe_rows_ = rows; stripe_index_ = index; stripe_count_ = count;
}

int RendererCore::localRows() const
{
    const int h = framebuffer_size[1];
    if (stripe_count_ > 1) {
        const int total = (h + stripe_rows_ - 1) / stripe_rows_;
        const int mine = (total - stripe_index_ + stripe_count_ - 1) / stripe_count_;
        return mine * stripe_rows_;
    }
    const int b = std::max(0, row_begin_), e = row_end_ < 0 ? h : std::min(row_end_, h);
    return std::max(0, e - b);
}

bool RendererCore::certifyDivisor(float b)
{
    uint32_t bits;
    std::memcpy(&bits, &b, 4);
    auto it = cert_cache_.find(bits);
    if (it != cert_cache_.end()) return it->second;
    bool ok = false;
    if (std::isfinite(b) && b > 1e-30f && b < 1e30f) {
        const float r = 1.0f / b;
        check(hipMemsetAsync(d_scratch_.get(), 0, sizeof(unsigned), stream()), "hipMemset(scratch)");
        check(launch_certify_div(b, r, d_scratch_.get(), stream()), "certify_div_kernel");
        unsigned bad = 1;
        check(hipMemcpyAsync(&bad, d_scratch_.get(), sizeof(unsigned), hipMemcpyDeviceToHost, stream()), "hipMemcpy(scratch)");
        check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
        ok = (bad == 0);
    }
    cert_cache_[bits] = ok;
    return ok;
}

void RendererCore::buildFrame(FrameParams &P, LaunchConfig &L)
{
    std::memset(&P, 0, sizeof(P));
    std::memset(&L, 0, sizeof(L));
    if (cam_block_.size() != 21 || main_cam.is_changed) setupUBO(true);
    std::memcpy(P.cam, cam_block_.data(), sizeof(float) * 21);
    P.img_w = framebuffer_size[0];
    P.img_h = framebuffer_size[1];
    P.row_begin = std::max(0, row_begin_);
    P.row_end = row_end_ < 0 ? P.img_h : std::min(row_end_, P.img_h);
    if (quirks & kQuirkTruncGrid) {
        P.col_lim = (P.img_w / kLocalSize) * kLocalSize;
        P.row_lim = (P.img_h / kLocalSize) * kLocalSize;
    } else {
        P.col_lim = P.img_w;
        P.row_lim = P.img_h;
    }
    P.stripe_rows = stripe_count_ > 1 ? stripe_rows_ : 1;
    P.stripe_index = stripe_index_;
    P.stripe_count = stripe_count_;
    P.fb_compact = fb_compact_ ? 1 : 0;
    P.fb_format = (fb_format_ == 1 && ext_fb_) ? 1 : 0;
    const int nx = res_dims_[0], ny = res_dims_[1], nz = res_dims_[2];
    P.nx = nx; P.ny = ny; P.nz = nz;
    P.fdim[0] = (float)nx; P.fdim[1] = (float)ny; P.fdim[2] = (float)nz;
    P.bnx = (int)bricksX(nx); P.bny = (int)bricksY(ny); P.bnz = (int)bricksZ(nz);
    // ---- main(): VolumeRenderer.cs:65-83
    int max_dim = std::max(nx, ny);
    max_dim = std::max(max_dim, nz);
    const bool swz = (u_.view_bottom == 1 || u_.view_top == 1);
    const float d0 = (float)nx, d1 = swz ? (float)nz : (float)ny, d2 = swz ? (float)ny : (float)nz;
    const float s0 = u_.voxel_size[0], s1 = swz ? u_.voxel_size[2] : u_.voxel_size[1],
                s2 = swz ? u_.voxel_size[1] : u_.voxel_size[2];
    const float fmax_dim = (float)max_dim;
    const float pm[3] = {(d0 / fmax_dim) * s0, (d1 / fmax_dim) * s1, (d2 / fmax_dim) * s2};
    for (int i = 0; i < 3; i++) {
        P.half[i] = pm[i] / 2.0f;
        P.pmin[i] = 0.0f - P.half[i];
        P.pmax[i] = pm[i] - P.half[i];
        P.ext[i] = P.pmax[i] + P.half[i];
        P.rext[i] = 1.0f / P.ext[i];
    }
    // ---- step_size: VolumeRenderer.cs:109 (composite, .xzy) / :146 (MIP, .xyz)
    const float e0 = P.pmax[0] - P.pmin[0], e1 = P.pmax[1] - P.pmin[1], e2 = P.pmax[2] - P.pmin[2];
    // length(vec3) = sqrt of the dot summed from the last component to the first, as the reference's GL executes it
    // (oracle/ref_gl/probe_arith.py); .xzy in rayMarchVolume, .xyz in MIP
    const float num = std::sqrt((e2 * e2 + e1 * e1) + e0 * e0);
    const float fx = (float)nx, fy = (float)ny, fz = (float)nz;
    // (the isosurface mode marches the composite mode's positions, whatever the MIP switch says)
    const bool iso = frameMode() == FrameMode::Isosurface;
    const float den = (u_.is_MIP == 1 && !iso) ? std::sqrt((fz * fz + fy * fy) + fx * fx) : std::sqrt((fy * fy + fz * fz) + fx * fx);
    P.step = num / den;
    P.alpha_scale = u_.alpha_scale;
    P.min_val = u_.min_val; P.max_val = u_.max_val;
    P.fmin = (float)u_.min_val; P.fmax = (float)u_.max_val;
    P.fden = (float)(u_.max_val - u_.min_val);
    P.rden = P.fden != 0.0f ? 1.0f / P.fden : 0.0f;
    P.view_top = u_.view_top; P.view_bottom = u_.view_bottom;
    P.max_steps = 10000;   // VolumeRenderer.cs:115
    P.accum = accum;
    P.tf_len = tf_lut_.empty() ? 0 : 256;
    P.skip_empty = skip_empty;

    L.bytes_per_voxel = res_bytes_;
    L.filter = filter;
    L.mip = iso ? 0 : u_.is_MIP;
    L.layout = vol_layout_;
    L.generic = force_generic == 1 ? 1 : 0;
    // kernel variants 6 .. 11: TRILINEAR on the LDS-staged kernel wherever it is eligible, in one of its shapes (0: see launch_plan.h, firstGuess)
    L.tri_slab = (force_generic >= 6 && force_generic <= 11) ? force_generic - 5 : 0;
    L.pipelined = 0;
    L.short_batches = 0;
    // 32-bit voxel offsets with 24-bit multiplies (VoxelAddr) whenever the volume allows
    {
        // VoxelAddr: the strides carry minus the part of the in-brick term the split axis repeats
        const uint64_t bsy = 64ull * (uint64_t)P.bnx - (BRICK_LY ? (uint64_t)(BRICK_X * BRICK_Y) : 0ull);
        const uint64_t bsz = 64ull * (uint64_t)P.bnx * (uint64_t)P.bny - (BRICK_LZ ? 64ull : 0ull);
        P.bstride_y = (uint32_t)bsy;
        P.bstride_z = (uint32_t)bsz;
        const uint64_t storage = storageVoxels(nx, ny, nz, vol_layout_);
        const uint64_t lim24 = 1ull << 24;
        bool small = storage < (1ull << 32) && (uint64_t)nx < lim24 && (uint64_t)ny < lim24 && (uint64_t)nz < lim24;
        if (vol_layout_ == 0) small = small && (uint64_t)ny * (uint64_t)nz < lim24;
        else small = small && bsy < lim24 && bsz < lim24;
        const uint64_t bytes = storage * (uint64_t)res_bytes_;
        if (bytes >= (1ull << 32)) small = false;
        L.big_offsets = small ? 0 : 1;
        L.vol_bytes32 = small ? (uint32_t)bytes : 0u;
        const int64_t width = (int64_t)u_.max_val - (int64_t)u_.min_val + 1;
        // LDS classification table: 4096 (c,a) entries, or with a transfer function one index byte per
        // window value behind the 256-entry RGBA table (vr_kernels.hip: FAST_TF_WINDOW_MAX)
        L.use_lut = (width >= 2 && width <= (tf_lut_.empty() ? 4096 : FAST_TF_WINDOW_MAX) && (tf_lut_.empty() || tf_lut_.size() / 4 <= 256)) ? 1 : 0;
        L.lut_noclamp = (exact_min_ >= u_.min_val && exact_max_ <= u_.max_val) ? 1 : 0;
        // a grey transfer function under NEAREST composite whose window fits the grey-ramp kernels' (c, a) table is folded
        // into that table: the launch runs on the MODE 0 instances (vr_kernels.hip: raymarch_fast_kernel, LUT build)
        P.tf_grey = (!tf_lut_.empty() && tf_grey_ && filter == 0 && u_.is_MIP != 1 && L.use_lut != 0 && width <= 4096) ? 1 : 0;   // (NEAREST only: the fold lives in the fast / relay kernels' tables)
        auto is_pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
        L.pow2_dims = (is_pow2(nx) && is_pow2(ny) && is_pow2(nz)) ? 1 : 0;
    }
    // division strategy: unit extents need no division at all; other divisors use the
    // 3-op Markstein quotient only after an exhaustive on-device certification
    const bool unit = P.ext[0] == 1.0f && P.ext[1] == 1.0f && P.ext[2] == 1.0f;
    if (unit) L.divmode_tc = DIV_UNIT;
    else L.divmode_tc = (certifyDivisor(P.ext[0]) && certifyDivisor(P.ext[1]) && certifyDivisor(P.ext[2])) ? DIV_CERT : DIV_EXACT;
    L.divmode_win = (P.fden > 0.0f && certifyDivisor(P.fden)) ? DIV_CERT : DIV_EXACT;
}

void RendererCore::setFramebufferFormat(int fmt)
{
    if (fmt != 0 && fmt != 1) throw std::invalid_argument("setFramebufferFormat: unknown format");
    fb_format_ = fmt;
}

// everything a launch needs that may touch the host or synchronise (certification, skip grid,
// tile order, packed copy): done BEFORE the timed region of render()
// an isosurface frame is RGBA: a (grey, alpha) target is refused -- before the device checks, it is a configuration error
void RendererCore::refuseIsoGreyAlpha() const
{
    if (frameMode() == FrameMode::Isosurface && fb_format_ == 1 && ext_fb_)
        throw std::invalid_argument("render: the (grey, alpha) target format needs a grey mode (the isosurface mode is not one)");
}

// the skip grid's cells per axis of the resident volume (after ensureSkipGrid() has passed: no limit check here)
void RendererCore::setSkipCells(FrameParams &P) const
{
    uint32_t c[3];
    size_t cells;
    (void)skipGridCells(res_dims_[0], res_dims_[1], res_dims_[2], c, cells);
    P.cnx = (int32_t)c[0]; P.cny = (int32_t)c[1]; P.cnz = (int32_t)c[2];
}

// a per-pixel float target beside the colour one (depth, values): grown to this frame's rows x width; a new allocation is filled
// with the bit pattern `fill` (pixels no later frame writes read as "nothing here")
void RendererCore::growFloatTarget(DeviceBuffer<float> &d, int fill, const char *name)
{
    const int rows = std::max(localRows(), framebuffer_size[1]);
    const size_t n = (size_t)rows * (size_t)framebuffer_size[0];
    if (!d.ensure(std::max<size_t>(n, 1), name)) return;
    check(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d.get()), fill, n, stream()), (std::string("hipMemset(") + name + ")").c_str());
}

RendererCore::PreparedLaunch RendererCore::prepareLaunch()
{
    refuseIsoGreyAlpha();
    requireDevice("render");
    if (!cs_program_) throw std::runtime_error("render: no shader loaded (call loadShader first)");
    if (!d_vol_) throw std::runtime_error("render: no dataset loaded");
    PreparedLaunch F;
    FrameParams &P = F.P;
    LaunchConfig &L = F.L;
    F.fb = ext_fb_ ? reinterpret_cast<float4 *>(ext_fb_) : d_fb_.get();
    if (!F.fb) throw std::runtime_error("render: setup() has not allocated the framebuffer");
    if (fb_format_ == 1 && ext_fb_ && !tf_lut_.empty())
        throw std::invalid_argument("render: the (grey, alpha) target format needs a grey mode (no transfer function)");
    F.mode = frameMode();
    if (F.mode == FrameMode::RayMarch && filter == 1) warmTrilinear();   // (a caller that set the public field directly; a no-op once done)
    buildFrame(P, L);
    if (F.mode != FrameMode::RayMarch) {
        // the isosurface, reslice and gradient-lit composite kernels (vr_iso.hip, vr_reslice.hip, vr_shade.hip): one kernel each, no
        // measured choice (nothing explored, settled or evicted), no tile table or speed copies
        P.skip_empty = 0;
        int thresh = 0;
        const float *tf = tf_lut_.empty() ? nullptr : tf_lut_.data();
        if (F.mode == FrameMode::Isosurface) {
            // the skip grid when skipping is on and some cell lies below the iso value
            if (skip_empty && ensureSkipGrid() && (float)copies_.skipGridMin() < isoStored()) F.skip_grid = copies_.skipGrid();
            growFloatTarget(d_depth_, 0x7f800000, "depth");   // +inf
            depth_rows_ = (ext_fb_ && fb_compact_) ? localRows() : framebuffer_size[1];
            depth_w_ = framebuffer_size[0];
        } else if (F.mode == FrameMode::Reslice) {
            growFloatTarget(d_values_, 0x7fc00000, "values");   // quiet NaN
            values_rows_ = (ext_fb_ && fb_compact_) ? localRows() : framebuffer_size[1];
            values_w_ = framebuffer_size[0];
        } else if (skip_empty && zeroAlphaThreshold(P, u_.min_val, u_.max_val, tf, filter == 1, thresh) && ensureSkipGrid() && thresh >= (int)copies_.skipGridMin()) {
            // shaded: the skip grid when skipping is on and some cell classifies to alpha 0 (the composite mode's threshold rule:
            // NEAREST per value, TRILINEAR the table's whole leading zero-alpha run)
            F.skip_grid = copies_.skipGrid();
            F.skip_thresh = thresh;
        }
        if (F.skip_grid) setSkipCells(P);
        noMeasuredChoice();
        return F;
    }
    refreshSkipGrid(P, L);
    // the tile tables, then the first guess of a launch that walks one
    const TileTableNeeds needs = tileTableNeeds(P, L, force_generic);
    const int rows = launch_local_rows(P);
    if (tile_order && needs.any && rows > 0) {
        tiles_.refresh(P, L, rows, needs.tall, needs.small, needs.skip_order ? L.skip_grid : nullptr, exact_max_, stream());
        firstGuess(P, L, force_generic, tiles_.active(), tiles_.longest());
    }
    refreshPacked12(P, L);
    refreshApron(P, L);
    halfLayerFallback(P, L, force_generic);
    // the specialised kernels gather from the packed copy when their address tables fit (vr_kernels.hip: dispatch_fast3)
    last_packed12_bytes_ = (L.packed12 && P.nx + P.ny + P.nz <= 3072) ? (size_t)L.packed12_bytes : 0;
    tuneChoose(F);
    F.stream_eligible = rayStreamEligible(P, L, skip_empty);
    if (F.stream_eligible) F.stream_key = rayGeometryKey(P, L, volume_generation_);
    return F;
}

void RendererCore::setRayStream(int mode)
{
    if (mode < 0 || mode > 2) throw std::invalid_argument("setRayStream: unknown mode");
    ray_stream_mode_ = mode;                                             // (0 keeps a valid stream: it is used again if the geometry still stands when the mode returns)
}

void RendererCore::setRayStreamPack(int mode)
{
    if (mode < 0 || mode > 2) throw std::invalid_argument("setRayStreamPack: unknown mode");
    copies_.setRayStreamPack(mode);                                      // (another mode: the stream is stale, its allocation is kept)
}

void RendererCore::setRayStreamTable(int mode)
{
    if (mode < 0 || mode > 2) throw std::invalid_argument("setRayStreamTable: unknown mode");
    ray_stream_table_ = mode;                                            // (the stream holds the same voxels: nothing is rebuilt)
}

// The ray-ordered sample stream (vr_stream.hip): counts this launch's geometry and decides whether the launch replays.  A launch
// that cannot replay (another mode or filter, skipping, no tile table) or whose geometry differs from the last one's makes the
// stream stale at once; its allocation is kept for the next build.  Mode 1: replay from the kRayStreamStillLaunches-th
// consecutive launch of one geometry on, and not on a launch the measured choice wants timed or tried -- that launch runs the
// gather kernel it asks for, and the count goes on; a forced kernel variant (vr_set_kernel_variant) runs that kernel.  Mode 2:
// the next eligible launch builds.  A countSamples launch counts but neither builds nor replays.  The build
// (VolumeCopies::ensureRayStream) blocks on one 8-byte read-back; it happens here, before render()'s timed stretch.  A camera
// that moves every frame pays the key comparison and nothing else.
void RendererCore::engageRayStream(PreparedLaunch &F, const uint32_t *spp)
{
    F.replay = false;
    if (!F.stream_eligible) {
        still_key_valid_ = false;
        still_launches_ = 0;
        copies_.invalidateRayStream();
        return;
    }
    if (still_key_valid_ && F.stream_key == still_key_) {
        still_launches_++;
    } else {
        still_key_ = F.stream_key;
        still_key_valid_ = true;
        still_launches_ = 1;
        copies_.invalidateRayStream();
    }
    if (spp != nullptr) return;
    const bool wanted = ray_stream_mode_ == 2 ||
                        (ray_stream_mode_ == 1 && force_generic == 0 && still_launches_ >= kRayStreamStillLaunches && !F.pick.measure && !F.pick.trial);
    if (!wanted) return;
    F.replay = copies_.ensureRayStream(residentVolume(), F.P, F.L);
}

// the LDS-staged TRILINEAR kernel's seven code objects (vr_tslab.hip), loaded when TRILINEAR is selected -- vr_set_filter,
// or vr_load_shader with the filter already set -- not by the first frame that needs one of them (round-4 advisor: the
// measured choice tries several shapes mid-interaction, each of which would pay a lazy decompress + load)
void RendererCore::warmUnits(int group)
{
    const char *family = nullptr;
    const hipError_t e = launch_warm_units((WarmGroup)group, stream(), &family);
    check(e, family ? std::string("module pre-load (") + family + ")" : std::string("module pre-load: a kernel unit without its VR_CODE_UNIT line"));
}

void RendererCore::warmTrilinear()
{
    if (device_ < 0 || tslab_warm_ || !cs_program_) return;
    requireDevice("warmTrilinear");
    warmUnits(WARM_TRILINEAR);
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
    tslab_warm_ = true;
}

// one frame: prepare, launch, and where the launch is a measurement of the work model hand its time to the tuner.  The
// reference brackets glDispatchCompute with a GL_TIME_ELAPSED query and blocks on its result (src/RendererCore.cpp:149-153):
// `blocking` is that shape with HIP events (the dispatch only: all host-side preparation happens first), and measures whatever
// the tuner asks for.  Otherwise a measurement takes a TuneSlot while one is free -- events read later without blocking
// (tuneCollect) -- and a countSamples launch never measures
void RendererCore::launch(uint32_t *spp, bool blocking)
{
    PreparedLaunch F = prepareLaunch();
    engageRayStream(F, spp);
    const LaunchTuner::Pick &pick = F.pick;
    const bool measure = pick.measure && !F.replay && spp == nullptr && (blocking || tune_count_ < kTuneSlots);   // (a forced replay is no measurement of the gather kernel)
    TuneSlot &slot = tune_slot_[(tune_head_ + tune_count_) % kTuneSlots];
    const hipEvent_t e0 = blocking ? ev0_ : slot.ev0, e1 = blocking ? ev1_ : slot.ev1;
    if (blocking || measure) check(hipEventRecord(e0, stream()), "hipEventRecord");
    check(launchKernel(F, spp), "raymarch launch");
    if (blocking || measure) check(hipEventRecord(e1, stream()), "hipEventRecord");
    if (blocking) {
        check(hipEventSynchronize(e1), "hipEventSynchronize");
        float ms = 0.0f;
        check(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
        kerneltime_sum += ms;
        if (measure) { tuner_.issued(pick.key, pick.gen, pick.cand); tuner_.record(pick.key, pick.gen, pick.cand, ms); }
    } else if (measure) {
        slot.key = pick.key; slot.cand = pick.cand; slot.gen = pick.gen;
        tune_count_++;
        tuner_.issued(pick.key, pick.gen, pick.cand);                    // counted only now that its events are on the stream
    }
}

// ---- the measured work model (launch_tuner.cpp): the results of the measurement launches whose events have completed
void RendererCore::tuneCollect()
{
    while (tune_count_ > 0) {                                            // the stream completes them in order
        TuneSlot &s = tune_slot_[tune_head_];
        const hipError_t q = hipEventQuery(s.ev1);
        if (q == hipErrorNotReady) { (void)hipGetLastError(); return; }
        tune_head_ = (tune_head_ + 1) % kTuneSlots;
        tune_count_--;
        if (q != hipSuccess) { (void)hipGetLastError(); continue; }
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, s.ev0, s.ev1) == hipSuccess) tuner_.record(s.key, s.gen, s.cand, ms);
        else (void)hipGetLastError();
    }
}

// ---- settled choices as a blob.  The reference dispatches ONE shader per frame and never tries anything
// (src/RendererCore.cpp:138-163); with an imported table neither does this library for the configurations the table knows.
#ifndef VR_BUILD_ID
#define VR_BUILD_ID 0ull
#endif
namespace {
void choiceDeviceName(int device, char (&out)[64])
{
    // the device MODEL as a string of attributes, not hipDeviceProp_t::name: under rocprofv3 hipGetDeviceProperties came back
    // without a name (round 6: the profiled bench run rejected the blob the run before it had written), attribute queries do not differ
    std::memset(out, 0, sizeof(out));
    if (device < 0) return;
    int cus = 0, clk = 0, l2 = 0, bus = 0, major = 0, minor = 0;
    size_t mem = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    (void)hipDeviceGetAttribute(&clk, hipDeviceAttributeClockRate, device);
    (void)hipDeviceGetAttribute(&l2, hipDeviceAttributeL2CacheSize, device);
    (void)hipDeviceGetAttribute(&bus, hipDeviceAttributeMemoryBusWidth, device);
    (void)hipDeviceGetAttribute(&major, hipDeviceAttributeComputeCapabilityMajor, device);
    (void)hipDeviceGetAttribute(&minor, hipDeviceAttributeComputeCapabilityMinor, device);
    (void)hipDeviceTotalMem(&mem, device);
    (void)hipGetLastError();
    std::snprintf(out, sizeof(out), "cc%d.%d cu%d clk%d l2_%d bus%d mem%zuG", major, minor, cus, clk / 1000, l2 >> 10, bus, mem >> 30);
}
}  // namespace

// (the blob's layout -- ChoiceHeader, ChoiceRecord -- and what an import accepts: launch_tuner.h / launch_tuner.cpp)
size_t RendererCore::exportChoices(void *buf, size_t capacity)
{
    tuneCollect();                                                       // measurements whose events have completed since the last launch count
    char device[64];
    choiceDeviceName(device_, device);
    return tuner_.exportChoices(buf, capacity, (uint64_t)VR_BUILD_ID, device);
}

int RendererCore::importChoices(const void *buf, size_t bytes)
{
    char device[64];
    choiceDeviceName(device_, device);
    return tuner_.importChoices(buf, bytes, (uint64_t)VR_BUILD_ID, device);
}

// the measured choice of this launch: the candidate kernels it could run (launch_plan.cpp), the tuner's pick among them
// (launch_tuner.cpp) applied to L
void RendererCore::tuneChoose(PreparedLaunch &F)
{
    tuneCollect();
    const int prior = choiceBits(F.L);                                   // the heuristics' choice (what buildFrame / firstGuess left in L)
    last_choice_ = prior;
    if (!autotune || force_generic != 0 || !F.L.tile_table) return;
    int cand[LaunchTuner::kTuneCand];
    const int n = launchCandidates(F.P, F.L, prior, cand);
    if (n < 2) return;
    const uint64_t key = launchTuneKey(F.P, F.L, launch_local_rows(F.P), tiles_.active(), prior);
    F.pick = tuner_.choose(key, cand, n, tune_count_, kTuneSlots);
    if (!F.pick.decided) return;                                         // only passing through: L and last_choice_ stay the heuristics'
    applyChoice(F.L, F.pick.cand);
    last_choice_ = F.pick.cand | (F.pick.trial ? 256 : 0);               // bit 8: a trial frame of a configuration still being explored
}

// 12-bit packed copy (vr_set_pack12, default on): when the voxels of a bricked u16 volume span at most 4096
// values (max - min <= 4095: 12-bit CT data whatever its offset -- the reference's own +1000 convention,
// src/RendererCore.cpp:66-67, stores 1000 .. 5095 -- and BASELINE's synthetic volume) the fast kernel's prefix
// gathers from a lossless copy of (voxel - min) with 1.5 bytes per voxel: the launch is bound by the number of
// cache lines it moves, and this is 25 % fewer.  The minimum is folded into the window limits and
// the table bias the kernel already carries (FrameParams::pk12_base), so the sample loop is the same code.  The
// u16 volume stays resident for every other kernel and for the checked head / tail of each ray.
void RendererCore::refreshPacked12(FrameParams &P, LaunchConfig &L)
{
    L.packed12 = nullptr;
    L.packed12_bytes = 0;
    P.pk12_base = 0;
    if (!pack12 || res_bytes_ != 2 || vol_layout_ != 1 || L.big_offsets || exact_max_ - exact_min_ > 4095) return;
    if (!fast_path_eligible(P, L)) return;
    const size_t voxels = storageVoxels(res_dims_[0], res_dims_[1], res_dims_[2], 1);
    const size_t bytes = voxels / 2 * 3;
    if (bytes + 16 >= (1ull << 32)) return;
    if (!copies_.ensurePacked12(residentVolume(), voxels, bytes)) return;   // (a refusal is not asked again every frame; vr_set_copy_budget / the next volume re-arm it)
    L.packed12 = copies_.packed12();
    L.packed12_bytes = (uint32_t)copies_.packed12Bytes();
    P.pk12_base = copies_.packed12Base();
}

// TRILINEAR's apron copy (vr_set_trilinear_copy, default on; vr_device.h: build_axis_tables_apron): the bricked
// volume once more with every 4x4x4 brick stored as 5x4x4, so that the two x taps of a sample are one load for
// every lane.  Built on first use from the resident volume, dropped with it; +25 % of the volume's bytes.
// Purely a speed device (2.27 -> ~1.8 ms on cfg3): the copy holds the same voxels, frames are bit-identical.
void RendererCore::refreshApron(const FrameParams &P, LaunchConfig &L)
{
    L.apron = nullptr;
    L.apron_y = L.apron_x = nullptr;
    L.apron_bytes = 0;
    last_apron_bytes_ = 0;
    if (!tri_apron || vol_layout_ != 1 || !(tri_path_candidate(P, L) || tri_slab_candidate(P, L))) return;
    const uint64_t bytes = apron_voxels(res_dims_[0], res_dims_[1], res_dims_[2]) * (uint64_t)res_bytes_;
    if (bytes + 16 >= (1ull << 32) && !tri_slab_candidate(P, L)) return;   // the batched kernel gathers through a 32-bit buffer descriptor
    if (!copies_.ensureApron(residentVolume(), bytes)) return;          // an optimisation only
    L.apron = copies_.apron();
    L.apron_bytes = (uint64_t)copies_.apronBytes();
    last_apron_bytes_ = copies_.apronBytes();
    // Half layers of the staged kernel (vr_tslab.hip, 16-bit volumes): two more copies with the bricks' planes along y / x
    // slowest, so that half a brick along any major axis is 80 contiguous bytes.  Built the first time a view is oblique
    // to the volume axes (or kernel variants 8 / 9 ask for them); +2 x 1.25 volumes of HBM.
    // Only when a launch can use them (round-4 advisor): the staged kernel must be able to run (it walks the tile table),
    // and either a half-layer shape is forced (variants 8 / 9) or the automatic choice may pick one -- the heuristic's first
    // guess for an oblique view, or a candidate of the measured choice.  Both or none: a lone copy is freed again.
    const bool oblique = viewAxisAlignment(P) < kTriWholeLayerAlignment;
    const bool half_layers_possible = (force_generic >= 8 && force_generic <= 9) || (force_generic == 11 && oblique) ||
                                      (force_generic == 0 && oblique && (L.tri_slab >= 3 || autotune));
    const bool want_perm = res_bytes_ == 2 && tri_slab_candidate(P, L) && L.tile_table != nullptr && half_layers_possible;
    if (want_perm) (void)copies_.ensureApronPerm(residentVolume(), bytes);   // (a refusal is re-armed by vr_set_copy_budget and by the next volume)
    if (copies_.hasApronPerm()) {
        L.apron_y = copies_.apronPerm(0);
        L.apron_x = copies_.apronPerm(1);
        last_apron_bytes_ += 2 * copies_.apronBytes();
    }
}

void RendererCore::setCopyBudget(uint64_t bytes)
{
    copies_.setBudget(bytes);                                            // a new budget re-arms what an old one refused
    if (device_ < 0 || bytes == kCopyBudgetAuto) return;
    requireDevice("setCopyBudget");
    copies_.trimToBudget(stream());
}

void RendererCore::residentBytes(uint64_t &volume, uint64_t &copies, uint64_t &other) const
{
    volume = d_vol_.bytes();
    copies = copies_.copiesBytes();
    other = d_fb_.bytes() + d_tf_.bytes() + d_spp_.bytes() + d_scratch_.bytes() + d_depth_.bytes() + d_values_.bytes() + copies_.skipGridBytes() +
            d_loaded_.bytes() + mesh_.bytes() + comp_.labels.bytes() + d_rgba8_.bytes() + tiles_.bytes();
    for (const auto &q : d_present_) other += q.bytes();
}

// Exact empty-space skipping (vr_set_skip_empty): the fast kernel may skip a batch of
// samples only if every voxel it could touch classifies to (0,0,0,0), so compositing it
// cannot change dest.  "Classifies to zero" is a prefix of the window: voxel <= min_val maps
// to v = 0 (grey ramp / MIP); with a transfer function the prefix is as long as its leading
// zero-opacity entries.  The grid holds, per 8^3-voxel cell, the maximum over the cell and
// its 26 neighbours.
void RendererCore::refreshSkipGrid(FrameParams &P, LaunchConfig &L)
{
    L.skip_grid = nullptr;
    L.skip_grid_bytes = 0;
    P.skip_empty = 0;
    // TRILINEAR on the LDS-staged kernel skips whole brick layers of a tile (vr_tslab.hip: SKIP): same grid, same threshold --
    // an interpolated value never exceeds its largest tap, and the classification of everything <= thresh is exactly zero
    const bool staged_tri = filter == 1 && tri_slab_candidate(P, L);
    if (!skip_empty || !(fast_path_eligible(P, L) || staged_tri)) return;
    if (!staged_tri && !nearestBatchWithinCells(P)) return;
    int thresh;
    if (!zeroAlphaThreshold(P, u_.min_val, u_.max_val, tf_lut_.empty() ? nullptr : tf_lut_.data(), staged_tri, thresh)) return;
    if (!ensureSkipGrid()) return;
    // nothing to skip at this threshold (a window that starts at the data's floor): the launch takes the instances without
    // skipping -- theirs are the leaner loops (staged TRILINEAR 3.8 %, its tiles on global taps 20 %, the NEAREST kernels a
    // workgroup of occupancy).  A host comparison against the grid's smallest cell: no device work, no synchronisation per frame.
    if (thresh < (int)copies_.skipGridMin()) return;
    P.skip_empty = 1;
    P.skip_thresh = thresh;
    setSkipCells(P);
    L.skip_grid = copies_.skipGrid();
    L.skip_grid_bytes = (uint32_t)((size_t)P.cnx * P.cny * P.cnz * sizeof(uint16_t));
}

bool RendererCore::ensureSkipGrid()
{
    uint32_t c[3];
    size_t cells;
    if (!skipGridCells(res_dims_[0], res_dims_[1], res_dims_[2], c, cells)) return false;
    copies_.ensureSkipGrid(residentVolume(), cells);
    return true;
}

void RendererCore::render()
{
    launch(nullptr, true);
}

hipError_t RendererCore::launchKernel(const PreparedLaunch &F, uint32_t *spp)
{
    const FrameParams &P = F.P;
    const LaunchConfig &L = F.L;
    switch (F.mode) {
    case FrameMode::Reslice: {
        ResliceArgs A;
        std::memcpy(&A.g, reslice_geom_, sizeof(A.g));
        A.mode = reslice_mode_;
        A.n = reslice_n_;
        A.hu_offset = (datasize_bytes == 2 && (quirks & kQuirkU16Offset)) ? 1 : 0;
        A.values = d_values_.get();
        return launch_reslice(P, L, A, d_vol_.get(), d_tf_.get(), F.fb, spp, stream(), &last_kernel_);
    }
    case FrameMode::Shaded: {
        ShadeArgs A;
        A.ambient = shade_k_[0]; A.diffuse = shade_k_[1]; A.specular = shade_k_[2];
        A.spec_squarings = 0;
        while ((1 << A.spec_squarings) < shade_shininess_) A.spec_squarings++;
        A.skip_grid = F.skip_grid;
        A.skip_thresh = F.skip_thresh;
        return launch_raymarch_shade(P, L, A, d_vol_.get(), d_tf_.get(), F.fb, spp, stream(), &last_kernel_);
    }
    case FrameMode::Isosurface: {
        IsoArgs A;
        A.iso_s = isoStored();
        A.depth = d_depth_.get();
        A.skip_grid = F.skip_grid;
        return launch_raymarch_iso(P, L, A, d_vol_.get(), d_tf_.get(), F.fb, spp, stream(), &last_kernel_);
    }
    case FrameMode::RayMarch: break;
    }
    if (F.replay && spp == nullptr) {
        RayStreamView S = copies_.rayStream();
        // the hybrid classification: wherever eligible (mode 2), or -- automatic -- on a packed stream larger than the
        // last-level cache, where it was measured to gain (vr_stream.h: kStreamTableMinBytes)
        const uint64_t sample_bytes = streamSampleBytes(S.format, L.bytes_per_voxel, copies_.rayStreamElements());
        const bool automatic = S.format == kStreamPack12 && sample_bytes > kStreamTableMinBytes;
        S.table = (ray_stream_table_ == 2 || (ray_stream_table_ == 1 && automatic)) ? 1 : 0;
        last_stream_table_ = S.table != 0 && streamTableEligible(P, L, S);
        return launch_raymarch_stream(P, L, d_tf_.get(), F.fb, S, stream(), &last_kernel_);
    }
    return launch_raymarch(P, L, d_vol_.get(), d_tf_.get(), F.fb, spp, stream(), &last_kernel_);
}

// iso_s = float(iso + 1000) for 16-bit data under VR_QUIRK_U16_OFFSET (the window's own offset, setMinVal), float(iso) otherwise
float RendererCore::storedIso(int32_t iso) const
{
    const bool offset = datasize_bytes == 2 && (quirks & kQuirkU16Offset);
    return (float)((int64_t)iso + (offset ? 1000 : 0));
}

void RendererCore::readDepth(float *depth, size_t n_floats)
{
    requireDevice("readDepth");
    if (depth_rows_ < 0 || !d_depth_) throw std::invalid_argument("readDepth: no isosurface frame has been rendered");
    const size_t n = (size_t)depth_rows_ * (size_t)depth_w_;
    if (!depth || n_floats < n) throw std::invalid_argument("readDepth: buffer too small");
    check(hipMemcpyAsync(depth, d_depth_.get(), n * sizeof(float), hipMemcpyDeviceToHost, stream()), "hipMemcpy(D2H depth)");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
}

void RendererCore::setIsosurface(bool enable, int32_t iso)
{
    if (enable && reslice_enable_) throw std::invalid_argument("setIsosurface: the reslice mode is on (switch it off first)");
    iso_enable_ = enable;
    iso_value_ = iso;
}

void RendererCore::setReslice(bool enable, const float *geom12, int mode, int n)
{
    if (!enable) { reslice_enable_ = false; return; }
    if (iso_enable_) throw std::invalid_argument("setReslice: the isosurface mode is on (switch it off first)");
    if (mode < 0 || mode > 2) throw std::invalid_argument("setReslice: unknown slab mode");
    if (n < 1 || n > 1024) throw std::invalid_argument("setReslice: slab samples outside 1..1024");
    if (!geom12) throw std::invalid_argument("setReslice: no geometry");
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(geom12[i])) throw std::invalid_argument("setReslice: non-finite geometry");
    std::memcpy(reslice_geom_, geom12, sizeof(reslice_geom_));
    reslice_mode_ = mode;
    reslice_n_ = n;
    reslice_enable_ = true;
}

void RendererCore::setShading(bool enable, float ambient, float diffuse, float specular, int shininess)
{
    if (!enable) { shade_enable_ = false; return; }
    for (float k : {ambient, diffuse, specular})
        if (!std::isfinite(k) || k < 0.0f) throw std::invalid_argument("setShading: a coefficient is non-finite or negative");
    if (shininess < 1 || shininess > 128 || (shininess & (shininess - 1)) != 0)
        throw std::invalid_argument("setShading: shininess outside 1, 2, 4, ..., 128");
    shade_k_[0] = ambient; shade_k_[1] = diffuse; shade_k_[2] = specular;
    shade_shininess_ = shininess;
    shade_enable_ = true;
}

void RendererCore::getShading(int *enable, float *ambient, float *diffuse, float *specular, int *shininess) const
{
    if (enable) *enable = shade_enable_ ? 1 : 0;
    if (ambient) *ambient = shade_k_[0];
    if (diffuse) *diffuse = shade_k_[1];
    if (specular) *specular = shade_k_[2];
    if (shininess) *shininess = shade_shininess_;
}

void RendererCore::readResliceValues(float *values, size_t n_floats)
{
    // (before the device check: a handle that never rendered a reslice frame has no values, with or without a device)
    if (values_rows_ < 0 || !d_values_) throw std::invalid_argument("readResliceValues: no reslice frame has been rendered");
    requireDevice("readResliceValues");
    const size_t n = (size_t)values_rows_ * (size_t)values_w_;
    if (!values || n_floats < n) throw std::invalid_argument("readResliceValues: buffer too small");
    check(hipMemcpyAsync(values, d_values_.get(), n * sizeof(float), hipMemcpyDeviceToHost, stream()), "hipMemcpy(D2H values)");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
}

void RendererCore::renderAsync()
{
    launch(nullptr, false);
}

void RendererCore::synchronize()
{
    requireDevice("synchronize");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
}

void RendererCore::countSamples(uint64_t *total, uint32_t *per_pixel, size_t n_pixels)
{
    refuseIsoGreyAlpha();
    requireDevice("countSamples");
    const size_t n = (size_t)framebuffer_size[0] * (size_t)framebuffer_size[1];
    if (per_pixel && n_pixels < n) throw std::invalid_argument("countSamples: per_pixel buffer too small");
    d_spp_.ensure(n, "spp");
    check(hipMemsetAsync(d_spp_.get(), 0, n * sizeof(uint32_t), stream()), "hipMemset(spp)");
    launch(d_spp_.get(), false);
    std::vector<uint32_t> host(n);
    check(hipMemcpyAsync(host.data(), d_spp_.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream()), "hipMemcpy(spp)");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
    uint64_t sum = 0;
    for (uint32_t v : host) sum += v;
    if (total) *total = sum;
    if (per_pixel) std::memcpy(per_pixel, host.data(), n * sizeof(uint32_t));
}

void RendererCore::readPixels(float *rgba, size_t n_floats)
{
    requireDevice("readPixels");
    const size_t n = (size_t)framebuffer_size[0] * (size_t)framebuffer_size[1] * 4;
    if (!rgba || n_floats < n) throw std::invalid_argument("readPixels: buffer too small");
    if (ext_fb_ && (fb_compact_ || fb_format_ == 1))
        throw std::invalid_argument("readPixels: the external target is compact and/or (grey, alpha): it does not hold fb_w x fb_h RGBA32F pixels");
    const void *src = framebufferDevice();
    if (!src) throw std::runtime_error("readPixels: no framebuffer");
    check(hipMemcpyAsync(rgba, src, n * sizeof(float), hipMemcpyDeviceToHost, stream()), "hipMemcpy(D2H framebuffer)");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
}

void RendererCore::readPixelsRGBA8(uint8_t *rgba8, size_t n_bytes)
{
    requireDevice("readPixelsRGBA8");
    const size_t n = (size_t)framebuffer_size[0] * (size_t)framebuffer_size[1];
    if (!rgba8 || n_bytes < n * 4) throw std::invalid_argument("readPixelsRGBA8: buffer too small");
    if (ext_fb_ && (fb_compact_ || fb_format_ == 1))
        throw std::invalid_argument("readPixelsRGBA8: the external target is compact and/or (grey, alpha): it does not hold fb_w x fb_h RGBA32F pixels");
    const void *src = framebufferDevice();
    if (!src) throw std::runtime_error("readPixelsRGBA8: no framebuffer");
    d_rgba8_.ensure(n * 4, "rgba8");
    check(launch_to_rgba8(src, d_rgba8_.get(), n, stream()), "to_rgba8_kernel");
    check(hipMemcpyAsync(rgba8, d_rgba8_.get(), n * 4, hipMemcpyDeviceToHost, stream()), "hipMemcpy(D2H rgba8)");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
}

void RendererCore::releasePresent()
{
    if (present_stream_) (void)hipStreamSynchronize(present_stream_);
    for (int s = 0; s < kPresentSlots; s++) {
        d_present_[s].reset(); h_present_[s].reset(); present_converted_[s].reset(); present_copied_[s].reset();
    }
    if (present_stream_) { (void)hipStreamDestroy(present_stream_); present_stream_ = nullptr; }
    present_count_ = 0;
}

const uint8_t *RendererCore::presentRGBA8(const void *src_frame)
{
    requireDevice("presentRGBA8");
    const size_t n = (size_t)framebuffer_size[0] * (size_t)framebuffer_size[1];
    if (n == 0) throw std::runtime_error("presentRGBA8: setup() has not sized the framebuffer");
    if (!src_frame) {
        if (ext_fb_ && (fb_compact_ || fb_format_ == 1))
            throw std::invalid_argument("presentRGBA8: the external target is compact and/or (grey, alpha): it does not hold fb_w x fb_h RGBA32F pixels");
        src_frame = framebufferDevice();
        if (!src_frame) throw std::runtime_error("presentRGBA8: no framebuffer");
    }
    if (d_present_[kPresentSlots - 1].size() != n * 4) {     // (the last slot: a set-up that threw half way is done again)
        releasePresent();
        check(hipStreamCreateWithFlags(&present_stream_, hipStreamNonBlocking), "hipStreamCreate(present)");
        for (int s = 0; s < kPresentSlots; s++) {
            h_present_[s].alloc(n * 4, "hipHostMalloc(present)");
            present_converted_[s].create(hipEventDisableTiming); present_copied_[s].create(hipEventDisableTiming);
            d_present_[s].alloc(n * 4, "present");
        }
    }
    // three slots: call n converts and copies into slot n % 3 and hands out slot (n - 1) % 3, which call n + 1 leaves alone and
    // call n + 2 overwrites -- the pointer stays valid until the next-but-one call, as include/vr_core.h promises (round-3
    // advisor: with two slots it was the next call)
    const int s = present_count_ % kPresentSlots;
    // the slot's previous copy (three frames ago) must have left its staging buffer before it is overwritten
    if (present_count_ >= kPresentSlots) check(hipStreamWaitEvent(stream(), present_copied_[s], 0), "hipStreamWaitEvent");
    check(launch_to_rgba8(src_frame, d_present_[s].get(), n, stream()), "to_rgba8_kernel");
    check(hipEventRecord(present_converted_[s], stream()), "hipEventRecord");
    check(hipStreamWaitEvent(present_stream_, present_converted_[s], 0), "hipStreamWaitEvent");
    check(hipMemcpyAsync(h_present_[s].get(), d_present_[s].get(), n * 4, hipMemcpyDeviceToHost, present_stream_), "hipMemcpy(D2H present)");
    check(hipEventRecord(present_copied_[s], present_stream_), "hipEventRecord");
    const int ready = present_count_ == 0 ? s : (s + kPresentSlots - 1) % kPresentSlots;   // the previous frame; the first call waits for its own
    present_count_++;
    check(hipEventSynchronize(present_copied_[ready]), "hipEventSynchronize");
    return h_present_[ready].get();
}

// src/RendererCore.cpp:165-182: RGB8 read-back of the target, written top row first
// (stbi_flip_vertically_on_write).  glReadPixels' float->unorm8 conversion is
// round(clamp(c,0,1)*255).
bool RendererCore::saveImage(std::string fn, std::string ext)
{
    const int w = framebuffer_size[0], h = framebuffer_size[1];
    std::vector<float> rgba((size_t)w * h * 4);
    readPixels(rgba.data(), rgba.size());
    const int stride = w * 3;
    std::vector<uint8_t> rgb((size_t)stride * h);
    for (int y = 0; y < h; y++) {
        const float *src = &rgba[(size_t)(h - 1 - y) * w * 4];
        uint8_t *dst = &rgb[(size_t)y * stride];
        for (int x = 0; x < w; x++)
            for (int c = 0; c < 3; c++) {
                float v = src[4 * x + c];
                v = v != v ? 0.0f : std::fmin(std::fmax(v, 0.0f), 1.0f);
                dst[3 * x + c] = (uint8_t)std::floor(v * 255.0f + 0.5f);
            }
    }
    if (ext == ".png") return writePNG(fn, w, h, rgb.data(), stride);
    if (ext == ".bmp") return writeBMP(fn, w, h, rgb.data(), stride);
    if (ext == ".ppm") return writePPM(fn, w, h, rgb.data(), stride);
    if (ext == ".jpg") return writeJPEG(fn, w, h, rgb.data(), stride, 100);   // :176-177
    return false;
}

}  // namespace vr
