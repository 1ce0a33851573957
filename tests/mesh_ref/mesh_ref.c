/* TEST INFRASTRUCTURE ONLY -- plain scalar C99 restatement of vr_extract_isosurface (include/vr_core.h, the ten steps):
   marching tetrahedra on the Kuhn split of every voxel cell.  Build with -ffp-contract=off -fno-fast-math: every step is one
   correctly rounded fp32 operation in the order the header gives.

   mesh_extract works on the cells of an index box [c0, c1) per axis (the whole volume: 0 .. dim - 1).  Its vertices are those
   of the voxels [c0, c1] per axis, its triangles those of the box's cells, both in the global order (steps 6 and 10) and with
   global coordinates; vertex indices count from the box's first vertex.  Where no voxel outside the box owns a vertex, that
   IS the whole volume's mesh.  Call it with NULL arrays for the counts, then again with arrays that hold them. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* step 3: e_0 .. e_6 */
static const int DIRS[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};
/* step 7: the permutations xyz, xzy, yxz, yzx, zxy, zyx */
static const int PERMS[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

/* the case table: per (t, m) the triangles' vertices as (corner n, corner m') pairs of tetrahedron corners, n < m' */
static int g_ready = 0;
static int g_corner[6][4][3];          /* c_0 .. c_3 of tetrahedron t, relative to the cell */
static int g_ntri[6][16];
static int g_edge[6][16][6][2];
static int g_swapped[6][16];

static void set_tri(int tri[3][2], int a0, int b0, int a1, int b1, int a2, int b2)
{
    tri[0][0] = a0; tri[0][1] = b0; tri[1][0] = a1; tri[1][1] = b1; tri[2][0] = a2; tri[2][1] = b2;
}

static void build_table(void)
{
    if (g_ready) return;
    for (int t = 0; t < 6; t++) {
        for (int a = 0; a < 3; a++) {
            g_corner[t][0][a] = 0;
            g_corner[t][1][a] = a == PERMS[t][0];
            g_corner[t][2][a] = a == PERMS[t][0] || a == PERMS[t][1];
            g_corner[t][3][a] = 1;
        }
        for (int m = 0; m < 16; m++) {
            int I[4], O[4], ni = 0, no = 0, tri[2][3][2];
            for (int n = 0; n < 4; n++) {
                if (m & (1 << n)) I[ni++] = n;
                else O[no++] = n;
            }
            g_ntri[t][m] = 0;
            g_swapped[t][m] = 0;
            if (ni == 0 || ni == 4) continue;
            if (ni == 1) {                               /* (aO_0, aO_1, aO_2), a = I_0 */
                set_tri(tri[0], I[0], O[0], I[0], O[1], I[0], O[2]);
                g_ntri[t][m] = 1;
            } else if (ni == 3) {                        /* (aI_0, aI_1, aI_2), a = O_0 */
                set_tri(tri[0], O[0], I[0], O[0], I[1], O[0], I[2]);
                g_ntri[t][m] = 1;
            } else {                                     /* (ac, ad, bd), (ac, bd, bc) */
                set_tri(tri[0], I[0], O[0], I[0], O[1], I[1], O[1]);
                set_tri(tri[1], I[0], O[0], I[1], O[1], I[1], O[0]);
                g_ntri[t][m] = 2;
            }
            /* step 9, in double on the edge midpoints of the first triangle */
            double v[3][3], mo[3] = {0, 0, 0}, mi[3] = {0, 0, 0};
            for (int q = 0; q < 3; q++)
                for (int a = 0; a < 3; a++) v[q][a] = 0.5 * (g_corner[t][tri[0][q][0]][a] + g_corner[t][tri[0][q][1]][a]);
            for (int a = 0; a < 3; a++) {
                for (int n = 0; n < no; n++) mo[a] += g_corner[t][O[n]][a] / (double)no;
                for (int n = 0; n < ni; n++) mi[a] += g_corner[t][I[n]][a] / (double)ni;
            }
            double u[3], w[3];
            for (int a = 0; a < 3; a++) { u[a] = v[1][a] - v[0][a]; w[a] = v[2][a] - v[0][a]; }
            const double cr[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
            const double dot = cr[0] * (mo[0] - mi[0]) + cr[1] * (mo[1] - mi[1]) + cr[2] * (mo[2] - mi[2]);
            g_swapped[t][m] = dot < 0.0;
            for (int k = 0; k < g_ntri[t][m]; k++)
                for (int q = 0; q < 3; q++) {
                    const int src = g_swapped[t][m] && q > 0 ? 3 - q : q;
                    const int n0 = tri[k][src][0], n1 = tri[k][src][1];
                    g_edge[t][m][3 * k + q][0] = n0 < n1 ? n0 : n1;
                    g_edge[t][m][3 * k + q][1] = n0 < n1 ? n1 : n0;
                }
        }
    }
    g_ready = 1;
}

/* bit m of the result: step 9 swapped the entry (t, m) */
int mesh_case_swapped(int t)
{
    build_table();
    int bits = 0;
    for (int m = 0; m < 16; m++) bits |= g_swapped[t][m] << m;
    return bits;
}

typedef struct {
    const void *vol;
    int bytes, dim[3];
} Volume;

static float S(const Volume *V, int i, int j, int k)
{
    const size_t at = (size_t)i + (size_t)V->dim[0] * ((size_t)j + (size_t)V->dim[1] * (size_t)k);
    return V->bytes == 1 ? (float)((const uint8_t *)V->vol)[at] : (float)((const uint16_t *)V->vol)[at];
}

static void gradient(const Volume *V, const int p[3], float g[3])
{
    for (int a = 0; a < 3; a++) {
        int hi[3] = {p[0], p[1], p[2]}, lo[3] = {p[0], p[1], p[2]};
        hi[a] = p[a] + 1 < V->dim[a] - 1 ? p[a] + 1 : V->dim[a] - 1;
        lo[a] = p[a] - 1 > 0 ? p[a] - 1 : 0;
        g[a] = S(V, hi[0], hi[1], hi[2]) - S(V, lo[0], lo[1], lo[2]);
    }
}

static int dir_index(const int e[3])
{
    for (int d = 0; d < 7; d++)
        if (DIRS[d][0] == e[0] && DIRS[d][1] == e[1] && DIRS[d][2] == e[2]) return d;
    return -1;
}

int mesh_extract(const void *vol, int bytes, int nx, int ny, int nz, float iso_s, const float *spacing, const int *c0, const int *c1,
                 float *pos, float *nrm, uint32_t *tri, uint64_t vcap, uint64_t tcap, uint64_t *n_vertices, uint64_t *n_triangles)
{
    build_table();
    if (!vol || (bytes != 1 && bytes != 2) || nx < 1 || ny < 1 || nz < 1 || !spacing || !n_vertices || !n_triangles) return -1;
    const Volume V = {vol, bytes, {nx, ny, nz}};
    *n_vertices = *n_triangles = 0;
    if (nx < 2 || ny < 2 || nz < 2) return 0;            /* step 1: no cells */
    int b0[3] = {0, 0, 0}, b1[3] = {nx - 1, ny - 1, nz - 1};
    for (int a = 0; a < 3 && c0 && c1; a++) {
        if (c0[a] < 0 || c1[a] > V.dim[a] - 1 || c0[a] >= c1[a]) return -1;
        b0[a] = c0[a]; b1[a] = c1[a];
    }
    /* the voxels b0 .. b1 (inclusive): first vertex index and active directions of each */
    const size_t wx = (size_t)(b1[0] - b0[0] + 1), wy = (size_t)(b1[1] - b0[1] + 1), wz = (size_t)(b1[2] - b0[2] + 1);
    uint64_t *first = (uint64_t *)malloc(wx * wy * wz * sizeof(uint64_t));
    uint8_t *active = (uint8_t *)malloc(wx * wy * wz);
    if (!first || !active) { free(first); free(active); return -2; }
    uint64_t nv = 0, nt = 0;
    for (int k = b0[2]; k <= b1[2]; k++)
        for (int j = b0[1]; j <= b1[1]; j++)
            for (int i = b0[0]; i <= b1[0]; i++) {       /* step 6: by the owner's linear index, then d */
                const size_t at = (size_t)(i - b0[0]) + wx * ((size_t)(j - b0[1]) + wy * (size_t)(k - b0[2]));
                const int A[3] = {i, j, k};
                const float sa = S(&V, i, j, k);
                float ga[3];
                int have_ga = 0;
                first[at] = nv;
                active[at] = 0;
                for (int d = 0; d < 7; d++) {
                    const int B[3] = {i + DIRS[d][0], j + DIRS[d][1], k + DIRS[d][2]};
                    if (B[0] >= nx || B[1] >= ny || B[2] >= nz) continue;
                    const float sb = S(&V, B[0], B[1], B[2]);
                    if ((sa >= iso_s) == (sb >= iso_s)) continue;
                    active[at] |= (uint8_t)(1 << d);
                    if (pos || nrm) {
                        if (nv >= vcap) { free(first); free(active); return -3; }
                        const float num = iso_s - sa, den = sb - sa;
                        const float f = num / den;
                        if (pos)
                            for (int a = 0; a < 3; a++) {
                                const float fa = (float)A[a];
                                float q = fa;
                                if (DIRS[d][a]) q = fa + f;
                                pos[3 * nv + a] = q * spacing[a];
                            }
                        if (nrm) {
                            float gb[3], v[3];
                            if (!have_ga) { gradient(&V, A, ga); have_ga = 1; }
                            gradient(&V, B, gb);
                            for (int a = 0; a < 3; a++) {
                                const float diff = gb[a] - ga[a];
                                const float prod = f * diff;
                                const float G = ga[a] + prod;
                                const float H = G / spacing[a];
                                v[a] = -H;
                            }
                            const float zz = v[2] * v[2], yy = v[1] * v[1], xx = v[0] * v[0];
                            const float zy = zz + yy;
                            const float dot = zy + xx;
                            if (dot == 0.0f) {
                                nrm[3 * nv] = nrm[3 * nv + 1] = nrm[3 * nv + 2] = 0.0f;
                            } else {
                                const float root = sqrtf(dot);
                                const float rn = 1.0f / root;
                                for (int a = 0; a < 3; a++) nrm[3 * nv + a] = v[a] * rn;
                            }
                        }
                    }
                    nv++;
                }
            }
    for (int k = b0[2]; k < b1[2]; k++)
        for (int j = b0[1]; j < b1[1]; j++)
            for (int i = b0[0]; i < b1[0]; i++)          /* step 10: by the cell's linear index, then t, then the case's order */
                for (int t = 0; t < 6; t++) {
                    int m = 0;
                    for (int n = 0; n < 4; n++)
                        if (S(&V, i + g_corner[t][n][0], j + g_corner[t][n][1], k + g_corner[t][n][2]) >= iso_s) m |= 1 << n;
                    for (int q = 0; q < 3 * g_ntri[t][m]; q++) {
                        const int *cn = g_corner[t][g_edge[t][m][q][0]], *cm = g_corner[t][g_edge[t][m][q][1]];
                        const int e[3] = {cm[0] - cn[0], cm[1] - cn[1], cm[2] - cn[2]};
                        const int d = dir_index(e);
                        const size_t at = (size_t)(i + cn[0] - b0[0]) + wx * ((size_t)(j + cn[1] - b0[1]) + wy * (size_t)(k + cn[2] - b0[2]));
                        if (d < 0 || !(active[at] & (1 << d))) { free(first); free(active); return -4; }   /* the table names an edge without a vertex */
                        uint64_t index = first[at];
                        for (int dd = 0; dd < d; dd++) index += (active[at] >> dd) & 1;
                        if (tri) {
                            if (nt + (uint64_t)(q / 3) >= tcap) { free(first); free(active); return -3; }
                            tri[3 * (nt + (uint64_t)(q / 3)) + (uint64_t)(q % 3)] = (uint32_t)index;
                        }
                    }
                    nt += (uint64_t)g_ntri[t][m];
                }
    free(first);
    free(active);
    *n_vertices = nv;
    *n_triangles = nt;
    return 0;
}
