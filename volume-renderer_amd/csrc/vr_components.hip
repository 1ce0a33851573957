// vr_components.hip -- connected components of the inside voxels (s >= iso) of the resident volume under the 14-neighbourhood
// of the extraction's seven edge directions (vr_label_components).  The definition, step by step, is in include/vr_core.h and
// DESIGN.md section 1.6; tests/components_ref/components_ref.c restates it on the CPU and tests/test_components_gpu.py holds
// these kernels to it bit for bit.
//
// Its own translation units (VR_COMP_TU = 0: 8-bit volumes, 1: 16-bit volumes), like vr_mesh.hip.
// Union-find, a fixed number of launches whatever the shape of the components:
//   tiles:   one workgroup per 32x8x4 tile (a whole number of bricks; a wavefront writes whole 128-byte lines of parents), four
//            voxels along x per thread.  Union-find over the tile in LDS on tile-local indices x + 32 * (y + 8 * z), which order
//            the tile's voxels like their linear indices; every inside voxel's parent is then written as the linear index of its
//            tile-local root.  A tile with no inside voxel, or with nothing else, skips the unions.
//   seams:   the voxels on a tile's +x, +y, +z faces union with their inside neighbours in the directions that leave the tile.
//            What is united are the two voxels' parents (the tile-local roots); a lane whose pair of parents equals the lane
//            before it, or its own previous direction's, leaves the union to that one.
//            The higher root is always hooked under the lower one with an agent-scope atomic min whose returned value is checked:
//            parents only ever decrease, so a component's final root is its voxel of lowest linear index whatever the order of
//            arrival.  Every parent read while others may write it is a relaxed agent-scope atomic load.
//   flatten: parent = root; one bit per voxel says "root", and the roots of every 64 voxels are counted.
//   (host)   rocPRIM's exclusive scan of the counts: a root's rank is its word's offset plus the root bits below it.
//   labels:  label = rank of the root + 1; the root writes its component's first voxel and an empty record.
//   records: voxel counts and boxes.  Runs of equal labels along x are folded in registers, then per workgroup (8192 voxels) in
//            an LDS table keyed by label, then ONE set of integer atomics per (workgroup, component) goes to memory: a percolating
//            component costs nvox / 8192 adds on its address, not nvox.  Integer only: independent of the order.
// Every find / union loop is capped; a cap that is hit sets a bit in the job's error word and the host fails the call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_code_unit.h"
#include "vr_components.h"
#include "vr_frame.h"

#ifndef VR_COMP_TU
#error "VR_COMP_TU: the unit number comes from the build"
#endif

namespace vr {

namespace {

constexpr uint32_t kTileX = 32, kTileY = 8, kTileZ = 4, kTileVoxels = kTileX * kTileY * kTileZ, kTileThreads = kTileVoxels / 4;   // sixteen bricks
static_assert(kTileX % BRICK_X == 0 && kTileY % BRICK_Y == 0 && kTileZ % BRICK_Z == 0 && kTileX == 32 && kTileY == 8, "tiles are whole bricks");
constexpr uint32_t kNoneLocal = 0xffffffffu;

struct CompArgs {
    const void *vol;
    uint32_t nx, ny, nz, bnx, bny, tnx, tny;
    int32_t layout;
    float iso_s;
    uint64_t nvox, nwords, ntiles;
    void *parent;
    uint64_t *bits, *scan;
    uint32_t *labels, *error;
    uint64_t *voxels, *first;
    int32_t *bbox;
};

__device__ __forceinline__ uint64_t stored_index(const CompArgs &A, uint32_t i, uint32_t j, uint32_t k)
{
    if (A.layout == 0) return (uint64_t)i + (uint64_t)A.nx * ((uint64_t)j + (uint64_t)A.ny * (uint64_t)k);
    const uint64_t brick = (uint64_t)(i >> BRICK_LX) + (uint64_t)A.bnx * ((uint64_t)(j >> BRICK_LY) + (uint64_t)A.bny * (uint64_t)(k >> BRICK_LZ));
    return brick * 64u + ((i & (BRICK_X - 1u)) | ((j & (BRICK_Y - 1u)) << BRICK_LX) | ((k & (BRICK_Z - 1u)) << (BRICK_LX + BRICK_LY)));
}

__device__ __forceinline__ uint64_t linear_index(const CompArgs &A, uint32_t i, uint32_t j, uint32_t k)
{
    return (uint64_t)i + (uint64_t)A.nx * ((uint64_t)j + (uint64_t)A.ny * (uint64_t)k);
}

// Grids are two-dimensional, kGridRow workgroups a row, so that no dimension's thread count reaches 2^32 (2048^3 voxels make
// 2^25 workgroups of 256); a kernel's workgroup number is block_id(), and the last row's surplus workgroups find nothing to do.
// A row is short enough that a test volume of 2^25 voxels gives every kernel a second one.
constexpr uint32_t kGridRow = 1u << 12;
__device__ __forceinline__ uint64_t block_id() { return (uint64_t)blockIdx.y * gridDim.x + blockIdx.x; }

__device__ __forceinline__ uint32_t corner_of_dir(int d)   // e_d as bits x | y << 1 | z << 2
{
    constexpr uint32_t bits = 1u | 2u << 3 | 4u << 6 | 3u << 9 | 5u << 12 | 6u << 15 | 7u << 18;
    return bits >> (3 * d) & 7u;
}

// ------------------------------------------------------------------ union-find in LDS (the tile pass)
__device__ __forceinline__ uint32_t lds_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ uint32_t lds_find(const uint32_t *par, uint32_t x)
{
    // parents strictly decrease along a chain: at most kTileVoxels links
    for (uint32_t it = 0; it < kTileVoxels; it++) {
        const uint32_t p = lds_load(par + x);
        if (p == x || p >= kTileVoxels) break;
        x = p;
    }
    return x;
}

__device__ __forceinline__ void lds_union(uint32_t *par, uint32_t a, uint32_t b)
{
    // every retry lowers max(a, b): at most kTileVoxels of them
    for (uint32_t it = 0; it < kTileVoxels; it++) {
        a = lds_find(par, a);
        b = lds_find(par, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicMin(par + hi, lo);
        if (old == hi) return;                           // hi was a root and hangs under lo now
        a = old; b = lo;                                 // hi had a parent already: that one and lo still have to meet
    }
}

struct TileAt { uint32_t i0, j0, k0; };                 // a tile's first voxel

__device__ __forceinline__ TileAt tile_at(const CompArgs &A, uint64_t tile)
{
    uint32_t b = (uint32_t)tile;                         // (job_ok: below 2^31 tiles)
    const uint32_t tx = b % A.tnx;
    b /= A.tnx;
    return {tx * kTileX, (b % A.tny) * kTileY, (b / A.tny) * kTileZ};
}

template <typename VoxelT, typename IdxT>
__global__ __launch_bounds__(kTileThreads) void comp_tile_kernel(const CompArgs A)
{
    __shared__ uint32_t par[kTileVoxels];
    if (block_id() >= A.ntiles) return;
    const TileAt T = tile_at(A, block_id());
    const uint32_t t = threadIdx.x, x0 = (t & 7u) * 4u, y = t >> 3 & 7u, z = t >> 6;      // this thread's voxels: x0 .. x0 + 3
    const uint32_t l0 = x0 + kTileX * (y + kTileY * z);
    const uint32_t i0 = T.i0 + x0, j = T.j0 + y, k = T.k0 + z;
    const bool row = j < A.ny && k < A.nz;
    uint32_t valid = 0, inside = 0;                      // bit q: voxel x0 + q
    if (row && i0 < A.nx) {
        const VoxelT *vol = static_cast<const VoxelT *>(A.vol);
        if (A.layout != 0 && BRICK_X == 4) {             // the four voxels are one row of a brick (its padding included): one load
            struct alignas(4 * sizeof(VoxelT)) Row { VoxelT v[4]; };
            const Row r = *reinterpret_cast<const Row *>(vol + stored_index(A, i0, j, k));
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) {
                if (i0 + q >= A.nx) continue;
                valid |= 1u << q;
                inside |= (uint32_t)((float)r.v[q] >= A.iso_s) << q;
            }
        } else {
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) {
                if (i0 + q >= A.nx) continue;
                valid |= 1u << q;
                inside |= (uint32_t)((float)vol[stored_index(A, i0 + q, j, k)] >= A.iso_s) << q;
            }
        }
    }
    // the thread's own run along x needs no atomics: a voxel behind an inside voxel starts under that one's root
    uint32_t root = kNoneLocal;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
        root = (inside >> q & 1u) ? (root == kNoneLocal ? l0 + q : root) : kNoneLocal;
        par[l0 + q] = root;
    }
    const int some = __syncthreads_or(inside != 0), all = __syncthreads_and(inside == 0xfu);
    if (some && !all) {
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            if (!(inside >> q & 1u)) continue;
#pragma unroll
            for (int d = 0; d < 7; d++) {
                const uint32_t e = corner_of_dir(d), dx = e & 1u, dy = e >> 1 & 1u, dz = e >> 2;
                if (d == 0 && q < 3) continue;           // joined above
                if (x0 + q + dx >= kTileX || y + dy >= kTileY || z + dz >= kTileZ) continue;
                const uint32_t nb = l0 + q + dx + kTileX * dy + kTileX * kTileY * dz;
                if (lds_load(par + nb) != kNoneLocal) lds_union(par, l0 + q, nb);
            }
        }
    }
    __syncthreads();
    if (!valid) return;
    IdxT out[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
        out[q] = ~(IdxT)0;
        if (inside >> q & 1u) {
            const uint32_t r = all ? 0u : lds_find(par, l0 + q);
            out[q] = (IdxT)linear_index(A, T.i0 + (r & (kTileX - 1u)), T.j0 + (r >> 5 & (kTileY - 1u)), T.k0 + (r >> 8));
        }
    }
    IdxT *dst = static_cast<IdxT *>(A.parent) + linear_index(A, i0, j, k);
    if ((A.nx & 3u) == 0) {                              // every row starts 4 voxels aligned and ends on a whole quad
        struct alignas(4 * sizeof(IdxT)) Quad { IdxT v[4]; };
        *reinterpret_cast<Quad *>(dst) = Quad{{out[0], out[1], out[2], out[3]}};
    } else {
#pragma unroll
        for (uint32_t q = 0; q < 4; q++)
            if (valid >> q & 1u) dst[q] = out[q];
    }
}

#if VR_COMP_TU == 0
// ------------------------------------------------------------------ union-find in memory (the seam pass, flatten)
constexpr uint32_t kFindCap = 1u << 20, kUnionCap = 1u << 12;
// the +x face, the rest of the +y face, the rest of the +z face
constexpr uint32_t kSeamX = kTileY * kTileZ, kSeamY = (kTileX - 1) * kTileZ, kSeamZ = (kTileX - 1) * (kTileY - 1);
constexpr uint32_t kSeamVoxels = kSeamX + kSeamY + kSeamZ, kSeamThreads = (kSeamVoxels + 63) / 64 * 64;
constexpr uint32_t kRecThreads = 512, kRecChunks = 16, kRecSlots = 1024;   // records: 16 x 512 voxels a workgroup, a 1024-slot table

__device__ __forceinline__ void raise(const CompArgs &A, uint32_t bit) { atomicOr(A.error, bit); }

template <typename IdxT>
__device__ __forceinline__ IdxT par_load(const IdxT *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <typename IdxT>
__device__ __forceinline__ IdxT par_min(IdxT *p, IdxT v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x; Halve: every visited voxel is pointed at its grandparent on the way (an atomic min: parents only decrease)
template <typename IdxT, bool Halve>
__device__ __forceinline__ IdxT find_root(const CompArgs &A, IdxT x, bool &ok)
{
    IdxT *par = static_cast<IdxT *>(A.parent);
    for (uint32_t it = 0; it < kFindCap; it++) {
        const IdxT p = par_load(par + x);
        if (p == x) return x;
        if (p >= (IdxT)A.nvox) { raise(A, kComponentsBadParent); ok = false; return x; }
        const IdxT gp = par_load(par + p);
        if (gp == p) return p;
        if (gp >= (IdxT)A.nvox) { raise(A, kComponentsBadParent); ok = false; return x; }
        if (Halve) (void)par_min(par + x, gp);
        x = gp;
    }
    raise(A, kComponentsFindCap);
    ok = false;
    return x;
}

template <typename IdxT>
__device__ __forceinline__ void unite(const CompArgs &A, IdxT a, IdxT b)
{
    IdxT *par = static_cast<IdxT *>(A.parent);
    bool ok = true;
    for (uint32_t it = 0; it < kUnionCap; it++) {
        a = find_root<IdxT, true>(A, a, ok);
        b = find_root<IdxT, true>(A, b, ok);
        if (!ok || a == b) return;
        const IdxT hi = a > b ? a : b, lo = a > b ? b : a;
        const IdxT old = par_min(par + hi, lo);
        if (old == hi) return;                           // hi was a root and hangs under lo now
        a = old; b = lo;                                 // hi had a parent already: that one and lo still have to meet
    }
    raise(A, kComponentsUnionCap);
}

template <typename IdxT>
__global__ __launch_bounds__(kSeamThreads) void comp_seam_kernel(const CompArgs A)
{
    const uint32_t f = threadIdx.x, lane = f & 63u;
    uint32_t x, y, z;
    if (f < kSeamX) { x = kTileX - 1; y = f % kTileY; z = f / kTileY; }
    else if (f < kSeamX + kSeamY) { const uint32_t q = f - kSeamX; x = q % (kTileX - 1); y = kTileY - 1; z = q / (kTileX - 1); }
    else { const uint32_t q = f - kSeamX - kSeamY; x = q % (kTileX - 1); y = q / (kTileX - 1); z = kTileZ - 1; }
    if (block_id() >= A.ntiles) return;
    const TileAt T = tile_at(A, block_id());
    const uint32_t i = T.i0 + x, j = T.j0 + y, k = T.k0 + z;
    const IdxT *par = static_cast<const IdxT *>(A.parent);
    const IdxT none = ~(IdxT)0;
    IdxT pv = none;                                      // the voxel's parent: its tile-local root
    if (f < kSeamVoxels && i < A.nx && j < A.ny && k < A.nz) pv = par_load(par + linear_index(A, i, j, k));
    if (__syncthreads_or(pv != none) == 0) return;
    IdxT last = none;
    for (int d = 0; d < 7; d++) {                        // every lane walks the seven directions: the shuffles below need them all
        const uint32_t e = corner_of_dir(d), dx = e & 1u, dy = e >> 1 & 1u, dz = e >> 2;
        IdxT pq = none;
        if (pv != none && (x + dx >= kTileX || y + dy >= kTileY || z + dz >= kTileZ) &&      // (inside the tile: the tile pass joined them)
            i + dx < A.nx && j + dy < A.ny && k + dz < A.nz)
            pq = par_load(par + linear_index(A, i + dx, j + dy, k + dz));
        const unsigned long long before_v = __shfl_up((unsigned long long)pv, 1), before_q = __shfl_up((unsigned long long)pq, 1);
        if (pq == none || pq == last) continue;
        last = pq;
        if (lane != 0 && before_v == (unsigned long long)pv && before_q == (unsigned long long)pq) continue;   // the lane before unites the same two
        unite<IdxT>(A, pv, pq);
    }
}

template <typename IdxT>
__global__ __launch_bounds__(256) void comp_flatten_kernel(const CompArgs A)
{
    const uint64_t g = block_id() * 256u + threadIdx.x;
    IdxT *par = static_cast<IdxT *>(A.parent);
    const IdxT none = ~(IdxT)0;
    bool root = false;
    if (g < A.nvox) {
        const IdxT p = par_load(par + g);
        if (p != none) {
            bool ok = true;
            const IdxT r = find_root<IdxT, false>(A, (IdxT)g, ok);
            if (ok && r != p) __hip_atomic_store(par + g, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            root = ok && r == (IdxT)g;
        }
    }
    const uint64_t mask = __ballot(root);
    const uint64_t w = g >> 6;
    if ((threadIdx.x & 63u) == 0 && w < A.nwords) {
        A.bits[w] = mask;
        A.scan[w] = (uint64_t)__popcll(mask);
    }
    if (g == 0) A.scan[A.nwords] = 0;
}

template <typename IdxT>
__global__ __launch_bounds__(256) void comp_label_kernel(const CompArgs A)
{
    const uint64_t g = block_id() * 256u + threadIdx.x;
    if (g >= A.nvox) return;
    const IdxT p = static_cast<const IdxT *>(A.parent)[g];
    uint32_t label = 0;
    if (p != ~(IdxT)0) {
        const uint64_t w = (uint64_t)p >> 6;
        label = (uint32_t)(A.scan[w] + (uint64_t)__popcll(A.bits[w] & ((1ull << ((uint32_t)p & 63u)) - 1ull))) + 1u;
        if ((uint64_t)p == g) {
            const uint64_t c = label - 1u;
            A.first[c] = g;
            A.voxels[c] = 0;
            int32_t *bb = A.bbox + 6 * c;
            bb[0] = bb[1] = bb[2] = INT32_MAX;
            bb[3] = bb[4] = bb[5] = -1;
        }
    }
    A.labels[g] = label;                                 // with 32-bit parents this is parent[g]: nobody else reads it
}

// ------------------------------------------------------------------ records
__device__ __forceinline__ void record_add(const CompArgs &A, uint32_t label, uint32_t count, const uint32_t lo[3], const uint32_t hi[3])
{
    const uint64_t c = label - 1u;
    atomicAdd(reinterpret_cast<unsigned long long *>(A.voxels + c), (unsigned long long)count);
    int32_t *bb = A.bbox + 6 * c;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        atomicMin(bb + a, (int32_t)lo[a]);
        atomicMax(bb + 3 + a, (int32_t)hi[a]);
    }
}

__global__ __launch_bounds__(kRecThreads) void comp_record_kernel(const CompArgs A)
{
    __shared__ uint32_t hkey[kRecSlots], hcnt[kRecSlots], hlo[3][kRecSlots], hhi[3][kRecSlots];
    for (uint32_t s = threadIdx.x; s < kRecSlots; s += kRecThreads) {
        hkey[s] = 0; hcnt[s] = 0;
        for (int a = 0; a < 3; a++) { hlo[a][s] = 0xffffffffu; hhi[a][s] = 0; }
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const bool small = A.nvox <= 0xffffffffull;
    for (uint32_t c = 0; c < kRecChunks; c++) {
        const uint64_t g = (block_id() * kRecChunks + c) * kRecThreads + threadIdx.x;
        const bool have = g < A.nvox;
        const uint32_t label = have ? A.labels[g] : 0u;
        uint32_t i = 0;
        uint64_t row = 0;
        if (have) {
            if (small) { const uint32_t r = (uint32_t)g / A.nx; row = r; i = (uint32_t)g - r * A.nx; }
            else { row = g / A.nx; i = (uint32_t)(g - row * A.nx); }
        }
        // a run: equal labels on consecutive lanes of one row; its first lane speaks for it
        const uint32_t before = __shfl_up(label, 1);
        const bool brk = lane == 0 || before != label || i == 0;
        const uint64_t brks = __ballot(brk);
        if (!brk || label == 0) continue;
        const uint64_t rest = lane == 63 ? 0ull : brks >> (lane + 1);
        const uint32_t len = rest ? (uint32_t)__ffsll((unsigned long long)rest) : 64u - lane;
        uint32_t j, k;
        if (small) { k = (uint32_t)row / A.ny; j = (uint32_t)row - k * A.ny; }
        else { k = (uint32_t)(row / A.ny); j = (uint32_t)(row - (uint64_t)k * A.ny); }
        const uint32_t lo[3] = {i, j, k}, hi[3] = {i + len - 1, j, k};
        uint32_t s = (label * 2654435761u) >> 22, tries = 0;
        for (; tries < kRecSlots; tries++) {
            const uint32_t prev = atomicCAS(&hkey[s], 0u, label);
            if (prev == 0u || prev == label) break;
            s = (s + 1) & (kRecSlots - 1);
        }
        if (tries == kRecSlots) { record_add(A, label, len, lo, hi); continue; }   // the table is full: straight to memory
        atomicAdd(&hcnt[s], len);
#pragma unroll
        for (int a = 0; a < 3; a++) { atomicMin(&hlo[a][s], lo[a]); atomicMax(&hhi[a][s], hi[a]); }
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < kRecSlots; s += kRecThreads) {
        if (hkey[s] == 0) continue;
        const uint32_t lo[3] = {hlo[0][s], hlo[1][s], hlo[2][s]}, hi[3] = {hhi[0][s], hhi[1][s], hhi[2][s]};
        record_add(A, hkey[s], hcnt[s], lo, hi);
    }
}

__global__ __launch_bounds__(256) void comp_plane_kernel(const uint32_t *labels, const uint8_t *selected, uint64_t nvox, uint64_t nwords, uint64_t *plane)
{
    const uint64_t g = block_id() * 256u + threadIdx.x;
    bool on = false;
    if (g < nvox) {
        const uint32_t label = labels[g];
        on = label != 0 && selected[label - 1u] != 0;
    }
    const uint64_t mask = __ballot(on);
    if ((threadIdx.x & 63u) == 0 && (g >> 6) < nwords) plane[g >> 6] = mask;
}

#endif

CompArgs make_args(const ComponentsJob &J)
{
    CompArgs A = {};
    A.vol = J.volume;
    A.nx = (uint32_t)J.nx; A.ny = (uint32_t)J.ny; A.nz = (uint32_t)J.nz;
    A.bnx = (uint32_t)((J.nx + BRICK_X - 1) / BRICK_X); A.bny = (uint32_t)((J.ny + BRICK_Y - 1) / BRICK_Y);
    A.tnx = (A.nx + kTileX - 1) / kTileX; A.tny = (A.ny + kTileY - 1) / kTileY;
    A.layout = J.layout;
    A.iso_s = J.iso_s;
    A.nvox = component_voxels(J); A.nwords = component_words(J);
    A.ntiles = (uint64_t)A.tnx * A.tny * ((A.nz + kTileZ - 1) / kTileZ);
    A.parent = J.parent; A.bits = J.bits; A.scan = J.scan;
    A.labels = J.labels; A.error = J.error;
    A.voxels = J.voxels; A.first = J.first_voxel; A.bbox = J.bbox;
    return A;
}

dim3 grid_of(uint64_t blocks) { return blocks <= kGridRow ? dim3((uint32_t)blocks) : dim3(kGridRow, (uint32_t)((blocks + kGridRow - 1) / kGridRow)); }

template <typename VoxelT>
hipError_t launch_tiles_type(const ComponentsJob &J, hipStream_t st)
{
    const CompArgs A = make_args(J);
    const dim3 grid = grid_of(A.ntiles);
    if (J.index_bits == 32) hipLaunchKernelGGL((comp_tile_kernel<VoxelT, uint32_t>), grid, dim3(kTileThreads), 0, st, A);
    else hipLaunchKernelGGL((comp_tile_kernel<VoxelT, uint64_t>), grid, dim3(kTileThreads), 0, st, A);
    return hipGetLastError();
}

}  // namespace

VR_CODE_UNIT(components, VR_COMP_TU, "components", WARM_LOAD_SHADER)

#if VR_COMP_TU == 1
hipError_t launch_components_tiles_u16(const ComponentsJob &J, hipStream_t st) { return launch_tiles_type<uint16_t>(J, st); }
#else
// the unit of 8-bit volumes also carries the entry points and the kernels that never read a voxel
hipError_t launch_components_tiles_u8(const ComponentsJob &J, hipStream_t st) { return launch_tiles_type<uint8_t>(J, st); }
hipError_t launch_components_tiles_u16(const ComponentsJob &J, hipStream_t st);

namespace {

// every launch's preconditions: a volume, an index width that holds every voxel number beside the sentinel, grids that fit
bool job_ok(const ComponentsJob &J, bool labelled)
{
    if (!J.volume || !J.parent || !J.bits || !J.scan || !J.labels || !J.error || J.nx < 1 || J.ny < 1 || J.nz < 1 ||
        (J.bytes_per_voxel != 1 && J.bytes_per_voxel != 2) || (J.layout != 0 && J.layout != 1) || (J.index_bits != 32 && J.index_bits != 64))
        return false;
    const uint64_t n = component_voxels(J);
    if (J.index_bits == 32 && n >= 0xffffffffull) return false;
    if (n > (1ull << 35)) return false;                  // at most 2^27 workgroups of 256: 2^15 grid rows of 2^12
    return !labelled || (J.voxels && J.first_voxel && J.bbox);
}

dim3 linear_grid(const ComponentsJob &J) { return grid_of((component_words(J) * 64 + 255) / 256); }

}  // namespace

hipError_t launch_components_tiles(const ComponentsJob &J, hipStream_t st)
{
    if (!job_ok(J, false)) return hipErrorInvalidValue;
    return J.bytes_per_voxel == 1 ? launch_components_tiles_u8(J, st) : launch_components_tiles_u16(J, st);
}

hipError_t launch_components_seams(const ComponentsJob &J, hipStream_t st)
{
    if (!job_ok(J, false)) return hipErrorInvalidValue;
    const CompArgs A = make_args(J);
    const dim3 grid = grid_of(A.ntiles);
    if (J.index_bits == 32) hipLaunchKernelGGL(comp_seam_kernel<uint32_t>, grid, dim3(kSeamThreads), 0, st, A);
    else hipLaunchKernelGGL(comp_seam_kernel<uint64_t>, grid, dim3(kSeamThreads), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_components_flatten(const ComponentsJob &J, hipStream_t st)
{
    if (!job_ok(J, false)) return hipErrorInvalidValue;
    const CompArgs A = make_args(J);
    if (J.index_bits == 32) hipLaunchKernelGGL(comp_flatten_kernel<uint32_t>, linear_grid(J), dim3(256), 0, st, A);
    else hipLaunchKernelGGL(comp_flatten_kernel<uint64_t>, linear_grid(J), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_components_labels(const ComponentsJob &J, uint64_t n_components, hipStream_t st)
{
    if (!job_ok(J, n_components > 0) || n_components > 0xfffffffeull) return hipErrorInvalidValue;
    const CompArgs A = make_args(J);
    if (J.index_bits == 32) hipLaunchKernelGGL(comp_label_kernel<uint32_t>, linear_grid(J), dim3(256), 0, st, A);
    else hipLaunchKernelGGL(comp_label_kernel<uint64_t>, linear_grid(J), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_components_records(const ComponentsJob &J, hipStream_t st)
{
    if (!job_ok(J, true)) return hipErrorInvalidValue;
    const CompArgs A = make_args(J);
    const uint64_t per = (uint64_t)kRecThreads * kRecChunks;
    hipLaunchKernelGGL(comp_record_kernel, grid_of((A.nvox + per - 1) / per), dim3(kRecThreads), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_components_plane(const uint32_t *labels, const uint8_t *selected, uint64_t n_voxels, uint64_t *plane, hipStream_t st)
{
    if (!labels || !selected || !plane || n_voxels == 0 || n_voxels > (1ull << 35)) return hipErrorInvalidValue;
    const uint64_t words = (n_voxels + 63) / 64;
    hipLaunchKernelGGL(comp_plane_kernel, grid_of((words * 64 + 255) / 256), dim3(256), 0, st, labels, selected, n_voxels, words, plane);
    return hipGetLastError();
}
#endif

}  // namespace vr
