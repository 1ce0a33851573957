// vr_mesh.hip -- extraction of the isosurface s = iso of the resident volume as an indexed triangle mesh
// (vr_extract_isosurface): marching tetrahedra on the Kuhn split of every voxel cell.  The definition, step by step, is in
// include/vr_core.h and DESIGN.md section 1.5; tests/mesh_ref/mesh_ref.c restates it on the CPU and
// tests/test_mesh_gpu.py holds these kernels to it bit for bit.
//
// Its own translation units (VR_MESH_TU = 0: 8-bit volumes, 1: 16-bit volumes), like vr_smooth.hip.
// Shape: three launches per z slab, one thread per voxel, no atomics (the mesh is the same bytes on every run).
//   count: per voxel, the directions whose edge carries a vertex (a mask byte) and, packed into one 64-bit word, the number of
//          those vertices (low half) and of the triangles of the cell the voxel is the origin of (high half).
//   scan:  the exclusive scan (vr_primitives.h) of the words, in place: both offsets at once.  The totals are known before the mesh is allocated.
//   emit:  the voxel's vertices at its vertex offset, its cell's triangles at its triangle offset.  The index of a vertex on
//          edge (A, d) is A's offset plus the number of A's active directions below d.
// Every voxel is read straight from the volume (eight corner loads per thread, neighbours served by the caches): no LDS
// staging yet.  Voxel addresses are 64-bit; slab-relative voxel numbers are 32-bit (a slab has at most 2^28 voxels).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_code_unit.h"
#include "vr_frame.h"
#include "vr_mesh.h"

#ifndef VR_MESH_TU
#error "VR_MESH_TU: the unit number comes from the build"
#endif

#if VR_MESH_TU == 0
#include <cstring>
#endif

namespace vr {

namespace {

// ------------------------------------------------------------------ the case table, built from rules 7 to 9 of the definition
// slot = (owner corner of the cell, bits x | y << 1 | z << 2) << 3 | direction d: the edge (cell + corner, d) the vertex lies on
struct CaseTable {
    uint8_t ntri[6][16];
    uint8_t slot[6][16][6];
    uint16_t swapped[6];                                 // bit m: rule 9 swapped the entry (t, m)
};

constexpr CaseTable make_case_table()
{
    CaseTable T = {};
    const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    const int dir_of_bits[8] = {-1, 0, 1, 3, 2, 4, 5, 6};   // e_0 .. e_6 = 100, 010, 001, 110, 101, 011, 111 (x first)
    for (int t = 0; t < 6; t++) {
        const int c[4] = {0, 1 << perm[t][0], (1 << perm[t][0]) | (1 << perm[t][1]), 7};
        for (int m = 1; m < 15; m++) {
            int in[4] = {}, out[4] = {}, ni = 0, no = 0;
            for (int n = 0; n < 4; n++) {
                if (m >> n & 1) in[ni++] = n;
                else out[no++] = n;
            }
            int tri[2][3][2] = {}, nt = 1;               // [triangle][vertex] = the two corners of its edge
            if (ni == 1) {
                for (int v = 0; v < 3; v++) { tri[0][v][0] = in[0]; tri[0][v][1] = out[v]; }
            } else if (ni == 3) {
                for (int v = 0; v < 3; v++) { tri[0][v][0] = out[0]; tri[0][v][1] = in[v]; }
            } else {
                const int a = in[0], b = in[1], cc = out[0], d = out[1];
                const int q[2][3][2] = {{{a, cc}, {a, d}, {b, d}}, {{a, cc}, {b, d}, {b, cc}}};
                nt = 2;
                for (int k = 0; k < 2; k++)
                    for (int v = 0; v < 3; v++) { tri[k][v][0] = q[k][v][0]; tri[k][v][1] = q[k][v][1]; }
            }
            // rule 9 on the first triangle: twice the edge midpoints, and (mean of O - mean of I) times |O| |I|
            int p[3][3] = {}, w[3] = {};
            for (int v = 0; v < 3; v++)
                for (int ax = 0; ax < 3; ax++) p[v][ax] = (c[tri[0][v][0]] >> ax & 1) + (c[tri[0][v][1]] >> ax & 1);
            for (int ax = 0; ax < 3; ax++) {
                int so = 0, si = 0;
                for (int n = 0; n < no; n++) so += c[out[n]] >> ax & 1;
                for (int n = 0; n < ni; n++) si += c[in[n]] >> ax & 1;
                w[ax] = so * ni - si * no;
            }
            const int u[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
            const int v2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
            const int dot = (u[1] * v2[2] - u[2] * v2[1]) * w[0] + (u[2] * v2[0] - u[0] * v2[2]) * w[1] + (u[0] * v2[1] - u[1] * v2[0]) * w[2];
            const bool swap = dot < 0;
            if (swap) T.swapped[t] = (uint16_t)(T.swapped[t] | (1u << m));
            T.ntri[t][m] = (uint8_t)nt;
            for (int k = 0; k < nt; k++)
                for (int v = 0; v < 3; v++) {
                    const int src = swap && v > 0 ? 3 - v : v;
                    const int n0 = tri[k][src][0] < tri[k][src][1] ? tri[k][src][0] : tri[k][src][1];
                    const int n1 = tri[k][src][0] < tri[k][src][1] ? tri[k][src][1] : tri[k][src][0];
                    T.slot[t][m][3 * k + v] = (uint8_t)(c[n0] << 3 | dir_of_bits[c[n1] ^ c[n0]]);
                }
        }
    }
    return T;
}

constexpr CaseTable kHostCases = make_case_table();
// rule 9's check value: the even permutations swap exactly m in {2, 5, 8, 10, 11, 14}, the odd ones the other eight cases
constexpr uint16_t kEvenSwaps = 1u << 2 | 1u << 5 | 1u << 8 | 1u << 10 | 1u << 11 | 1u << 14, kAllCases = 0x7ffe;
static_assert(kHostCases.swapped[0] == kEvenSwaps && kHostCases.swapped[3] == kEvenSwaps && kHostCases.swapped[4] == kEvenSwaps, "rule 9, even permutations");
static_assert(kHostCases.swapped[1] == (kAllCases ^ kEvenSwaps) && kHostCases.swapped[2] == (kAllCases ^ kEvenSwaps) &&
              kHostCases.swapped[5] == (kAllCases ^ kEvenSwaps), "rule 9, odd permutations");

__constant__ CaseTable kCases = make_case_table();

struct MeshArgs {
    const void *vol;
    uint32_t nx, ny, nz, bnx, bny;
    int32_t layout;
    float iso_s, sx, sy, sz;
    int32_t z0, z1, zs;                                  // owned planes [z0, z1), planes of the arrays [z0, zs)
    uint64_t *scan;
    uint8_t *mask;
    float *pos, *nrm;
    uint32_t *tri;
    uint32_t vbase, tbase;
    const uint64_t *selected;                            // SelectedInside only: one bit per voxel in linear order
};

__device__ __forceinline__ uint64_t voxel_index(const MeshArgs &A, uint32_t i, uint32_t j, uint32_t k)
{
    if (A.layout == 0) return (uint64_t)i + (uint64_t)A.nx * ((uint64_t)j + (uint64_t)A.ny * (uint64_t)k);
    const uint64_t brick = (uint64_t)(i >> BRICK_LX) + (uint64_t)A.bnx * ((uint64_t)(j >> BRICK_LY) + (uint64_t)A.bny * (uint64_t)(k >> BRICK_LZ));
    return brick * 64u + ((i & (BRICK_X - 1u)) | ((j & (BRICK_Y - 1u)) << BRICK_LX) | ((k & (BRICK_Z - 1u)) << (BRICK_LX + BRICK_LY)));
}

// s at a voxel inside the volume
template <typename VoxelT>
__device__ __forceinline__ float load_s(const MeshArgs &A, uint32_t i, uint32_t j, uint32_t k)
{
    return (float)static_cast<const VoxelT *>(A.vol)[voxel_index(A, i, j, k)];
}

// the eight corners of the cell at (i, j, k), corner bits x | y << 1 | z << 2; a corner outside the volume repeats the edge voxel
// (callers look at `exists` before they use it)
template <typename VoxelT>
__device__ __forceinline__ void load_corners(const MeshArgs &A, uint32_t i, uint32_t j, uint32_t k, float s[8], uint32_t &exists)
{
    const uint32_t hx = i + 1 < A.nx, hy = j + 1 < A.ny, hz = k + 1 < A.nz;
    exists = 0;
#pragma unroll
    for (uint32_t c = 0; c < 8; c++) {
        const uint32_t ok = ((c & 1) == 0 || hx) && ((c & 2) == 0 || hy) && ((c & 4) == 0 || hz);
        exists |= ok << c;
        s[c] = load_s<VoxelT>(A, i + ((c & 1) & hx), j + ((c >> 1 & 1) & hy), k + ((c >> 2 & 1) & hz));
    }
}

// Step 2's INSIDE as a template parameter of the two kernels that evaluate it.  PlainInside: s >= iso_s (vr_extract_isosurface).
// SelectedInside: the voxel's bit in the plane that launch_components_plane wrote -- inside at the labelling's iso value AND its
// component selected (vr_extract_components).  in8: the bits of the cell's eight corners as load_corners reads them.
struct PlainInside {
    static __device__ __forceinline__ uint32_t in8(const MeshArgs &A, uint32_t, uint32_t, uint32_t, const float s[8])
    {
        uint32_t bits = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) bits |= (uint32_t)(s[c] >= A.iso_s) << c;
        return bits;
    }
};

struct SelectedInside {
    static __device__ __forceinline__ uint32_t in8(const MeshArgs &A, uint32_t i, uint32_t j, uint32_t k, const float[8])
    {
        const uint32_t hx = i + 1 < A.nx, hy = j + 1 < A.ny, hz = k + 1 < A.nz;
        uint32_t bits = 0;
#pragma unroll
        for (uint32_t c = 0; c < 8; c++) {
            const uint64_t v = (uint64_t)(i + ((c & 1) & hx)) + (uint64_t)A.nx * ((uint64_t)(j + ((c >> 1 & 1) & hy)) + (uint64_t)A.ny * (uint64_t)(k + ((c >> 2 & 1) & hz)));
            bits |= (uint32_t)(A.selected[v >> 6] >> (v & 63u) & 1u) << c;
        }
        return bits;
    }
};

__device__ __forceinline__ uint32_t corner_of_dir(int d)   // e_d as corner bits
{
    constexpr uint32_t bits = 1u | 2u << 3 | 4u << 6 | 3u << 9 | 5u << 12 | 6u << 15 | 7u << 18;
    return bits >> (3 * d) & 7u;
}

// the inside corners of tetrahedron t as the mask m, from the cell's eight inside bits
__device__ __forceinline__ uint32_t tet_mask(uint32_t in8, int t)
{
    // c_1 and c_2 of the permutations xyz, xzy, yxz, yzx, zxy, zyx as corner bits
    constexpr uint32_t c1 = 1u | 1u << 3 | 2u << 6 | 2u << 9 | 4u << 12 | 4u << 15;
    constexpr uint32_t c2 = 3u | 5u << 3 | 3u << 6 | 6u << 9 | 5u << 12 | 6u << 15;
    const uint32_t a = c1 >> (3 * t) & 7u, b = c2 >> (3 * t) & 7u;
    return (in8 & 1u) | (in8 >> a & 1u) << 1 | (in8 >> b & 1u) << 2 | (in8 >> 7 & 1u) << 3;
}

__device__ __forceinline__ void decode(const MeshArgs &A, uint32_t g, uint32_t &i, uint32_t &j, uint32_t &k)
{
    const uint32_t row = g / A.nx;
    i = g - row * A.nx;
    const uint32_t pl = row / A.ny;
    j = row - pl * A.ny;
    k = (uint32_t)A.z0 + pl;
}

// ------------------------------------------------------------------ count
template <typename VoxelT, typename Inside>
__global__ __launch_bounds__(256) void mesh_count_kernel(const MeshArgs A)
{
    const uint32_t n = A.nx * A.ny * (uint32_t)(A.zs - A.z0);
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g > n) return;
    if (g == n) { A.scan[n] = 0; return; }
    uint32_t i, j, k;
    decode(A, g, i, j, k);
    float s[8];
    uint32_t exists;
    load_corners<VoxelT>(A, i, j, k, s, exists);
    const uint32_t in8 = Inside::in8(A, i, j, k, s);
    // direction d leads to corner corner_of_dir(d): a vertex where that voxel exists and lies on the other side
    const uint32_t differs = (in8 ^ (0u - (in8 & 1u))) & exists & 0xfeu;
    uint32_t mk = 0;
#pragma unroll
    for (int d = 0; d < 7; d++) mk |= (differs >> corner_of_dir(d) & 1u) << d;
    uint32_t nt = 0;
    if (exists == 0xffu && (int32_t)k < A.z1 && in8 != 0 && in8 != 0xffu) {
#pragma unroll
        for (int t = 0; t < 6; t++) {
            const int pc = __popc(tet_mask(in8, t));
            nt += pc == 2 ? 2u : (pc == 1 || pc == 3 ? 1u : 0u);
        }
    }
    A.mask[g] = (uint8_t)mk;
    A.scan[g] = (uint64_t)nt << 32 | (uint64_t)__popc(mk);
}

// ------------------------------------------------------------------ emit
// g(V): the NEAREST central difference with clamped neighbours
template <typename VoxelT>
__device__ __forceinline__ void gradient(const MeshArgs &A, uint32_t i, uint32_t j, uint32_t k, float g[3])
{
    g[0] = load_s<VoxelT>(A, min(i + 1, A.nx - 1), j, k) - load_s<VoxelT>(A, i > 0 ? i - 1 : 0, j, k);
    g[1] = load_s<VoxelT>(A, i, min(j + 1, A.ny - 1), k) - load_s<VoxelT>(A, i, j > 0 ? j - 1 : 0, k);
    g[2] = load_s<VoxelT>(A, i, j, min(k + 1, A.nz - 1)) - load_s<VoxelT>(A, i, j, k > 0 ? k - 1 : 0);
}

template <typename VoxelT, typename Inside>
__global__ __launch_bounds__(256) void mesh_emit_kernel(const MeshArgs A)
{
    const uint32_t plane = A.nx * A.ny;
    const uint32_t n = plane * (uint32_t)(A.z1 - A.z0);
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n) return;
    const uint64_t word = A.scan[g];
    const uint32_t mk = A.mask[g];
    const uint32_t ntri = (uint32_t)(A.scan[g + 1] >> 32) - (uint32_t)(word >> 32);
    if (mk == 0 && ntri == 0) return;
    uint32_t i, j, k;
    decode(A, g, i, j, k);
    float s[8];
    uint32_t exists;
    load_corners<VoxelT>(A, i, j, k, s, exists);

    if (mk != 0) {
        float ga[3];
        gradient<VoxelT>(A, i, j, k, ga);
        uint32_t vi = A.vbase + (uint32_t)word;
        const float fa[3] = {(float)i, (float)j, (float)k}, sp[3] = {A.sx, A.sy, A.sz};
#pragma unroll
        for (int d = 0; d < 7; d++) {
            if (!(mk >> d & 1u)) continue;
            const uint32_t e = corner_of_dir(d);
            const float f = (A.iso_s - s[0]) / (s[e] - s[0]);
            float gb[3];
            gradient<VoxelT>(A, i + (e & 1u), j + (e >> 1 & 1u), k + (e >> 2 & 1u), gb);
            float p[3], v[3];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                p[a] = (e >> a & 1u) ? (fa[a] + f) * sp[a] : fa[a] * sp[a];
                const float G = ga[a] + f * (gb[a] - ga[a]);
                v[a] = -(G / sp[a]);
            }
            const float dot = (v[2] * v[2] + v[1] * v[1]) + v[0] * v[0];
            float nn[3] = {0.0f, 0.0f, 0.0f};
            if (dot != 0.0f) {
                const float rn = 1.0f / sqrtf(dot);
                nn[0] = v[0] * rn; nn[1] = v[1] * rn; nn[2] = v[2] * rn;
            }
            float *po = A.pos + 3ull * vi, *no = A.nrm + 3ull * vi;
            po[0] = p[0]; po[1] = p[1]; po[2] = p[2];
            no[0] = nn[0]; no[1] = nn[1]; no[2] = nn[2];
            vi++;
        }
    }

    if (ntri != 0) {
        const uint32_t in8 = Inside::in8(A, i, j, k, s);
        // first vertex and active directions of the seven voxels that own the cell's edges (corner 7 owns none of them)
        uint32_t first[7], act[7];
#pragma unroll
        for (uint32_t c = 0; c < 7; c++) {
            const uint32_t gc = g + (c & 1u) + (c >> 1 & 1u) * A.nx + (c >> 2 & 1u) * plane;
            first[c] = A.vbase + (uint32_t)A.scan[gc];
            act[c] = A.mask[gc];
        }
        uint32_t *to = A.tri + 3ull * (A.tbase + (uint32_t)(word >> 32));
        for (int t = 0; t < 6; t++) {
            const uint32_t m = tet_mask(in8, t);
            const int nt = kCases.ntri[t][m];
            for (int q = 0; q < 3 * nt; q++) {
                const uint32_t sl = kCases.slot[t][m][q], c = sl >> 3, d = sl & 7u;
                uint32_t fc = first[0], ac = act[0];
#pragma unroll
                for (uint32_t cc = 1; cc < 7; cc++)
                    if (c == cc) { fc = first[cc]; ac = act[cc]; }
                *to++ = fc + (uint32_t)__popc(ac & ((1u << d) - 1u));
            }
        }
    }
}

template <typename VoxelT, typename Inside>
hipError_t launch_mesh_pred(const MeshSlab &S, bool emit, hipStream_t st)
{
    MeshArgs A = {};
    A.vol = S.volume;
    A.nx = (uint32_t)S.nx; A.ny = (uint32_t)S.ny; A.nz = (uint32_t)S.nz;
    A.bnx = (uint32_t)((S.nx + BRICK_X - 1) / BRICK_X); A.bny = (uint32_t)((S.ny + BRICK_Y - 1) / BRICK_Y);
    A.layout = S.layout;
    A.iso_s = S.iso_s; A.sx = S.spacing[0]; A.sy = S.spacing[1]; A.sz = S.spacing[2];
    A.z0 = S.z0; A.z1 = S.z1; A.zs = S.z0 + mesh_scan_planes(S);
    A.scan = S.scan; A.mask = S.mask;
    A.pos = S.positions; A.nrm = S.normals; A.tri = S.triangles;
    A.vbase = (uint32_t)S.vertex_base; A.tbase = (uint32_t)S.triangle_base;
    A.selected = S.selected;
    const uint64_t plane = (uint64_t)S.nx * (uint64_t)S.ny;
    if (!emit) {
        const uint64_t threads = plane * (uint64_t)(A.zs - A.z0) + 1;
        hipLaunchKernelGGL((mesh_count_kernel<VoxelT, Inside>), dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st, A);
    } else {
        const uint64_t threads = plane * (uint64_t)(A.z1 - A.z0);
        hipLaunchKernelGGL((mesh_emit_kernel<VoxelT, Inside>), dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st, A);
    }
    return hipGetLastError();
}

template <typename VoxelT>
hipError_t launch_mesh_type(const MeshSlab &S, bool emit, hipStream_t st)
{
    return S.selected ? launch_mesh_pred<VoxelT, SelectedInside>(S, emit, st) : launch_mesh_pred<VoxelT, PlainInside>(S, emit, st);
}

}  // namespace

VR_CODE_UNIT(mesh, VR_MESH_TU, "extraction", WARM_LOAD_SHADER)

#if VR_MESH_TU == 1
hipError_t launch_mesh_u16(const MeshSlab &S, bool emit, hipStream_t st) { return launch_mesh_type<uint16_t>(S, emit, st); }
#else
// the unit of 8-bit volumes also carries the entry points
hipError_t launch_mesh_u8(const MeshSlab &S, bool emit, hipStream_t st) { return launch_mesh_type<uint8_t>(S, emit, st); }
hipError_t launch_mesh_u16(const MeshSlab &S, bool emit, hipStream_t st);

namespace {

// every launch's preconditions: the slab lies in the volume and is small enough for 32-bit voxel numbers and partial sums
bool slab_ok(const MeshSlab &S, bool emit)
{
    if (!S.volume || !S.scan || !S.mask || S.nx < 2 || S.ny < 2 || S.nz < 2 || (S.bytes_per_voxel != 1 && S.bytes_per_voxel != 2) ||
        (S.layout != 0 && S.layout != 1) || S.z0 < 0 || S.z1 <= S.z0 || S.z1 > S.nz)
        return false;
    if (mesh_scan_words(S) - 1 > kMeshMaxSlabVoxels) return false;
    return !emit || (S.vertex_base <= 0xffffffffull && S.triangle_base <= 0xffffffffull);
}

}  // namespace

hipError_t launch_mesh_count(const MeshSlab &S, hipStream_t st)
{
    if (!slab_ok(S, false)) return hipErrorInvalidValue;
    return S.bytes_per_voxel == 1 ? launch_mesh_u8(S, false, st) : launch_mesh_u16(S, false, st);
}

hipError_t launch_mesh_emit(const MeshSlab &S, hipStream_t st)
{
    if (!slab_ok(S, true)) return hipErrorInvalidValue;
    return S.bytes_per_voxel == 1 ? launch_mesh_u8(S, true, st) : launch_mesh_u16(S, true, st);
}
#endif

}  // namespace vr
