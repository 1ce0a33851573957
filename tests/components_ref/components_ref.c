/* TEST INFRASTRUCTURE ONLY -- plain scalar C99 restatement of vr_label_components, vr_select_components and
   vr_extract_components (include/vr_core.h, the eight steps): a two-pass union-find over the inside voxels under the
   14-neighbourhood of the extraction's seven edge directions, the records, the selection rule, and the extraction
   (tests/mesh_ref/mesh_ref.c's ten steps, restated here) with INSIDE meaning "inside and its component selected".
   Build with -ffp-contract=off -fno-fast-math: every step is one correctly rounded fp32 operation in the order the header gives. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* step 2 (and the extraction's step 3): e_0 .. e_6 */
static const int DIRS[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};
static const int PERMS[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

typedef struct {
    const void *vol;
    int bytes, dim[3];
} Volume;

static float S(const Volume *V, int i, int j, int k)
{
    const size_t at = (size_t)i + (size_t)V->dim[0] * ((size_t)j + (size_t)V->dim[1] * (size_t)k);
    return V->bytes == 1 ? (float)((const uint8_t *)V->vol)[at] : (float)((const uint16_t *)V->vol)[at];
}

/* ------------------------------------------------------------------ labels and records */
static size_t find(size_t *parent, size_t x)
{
    size_t r = x;
    while (parent[r] != r) r = parent[r];
    while (parent[x] != r) { const size_t next = parent[x]; parent[x] = r; x = next; }
    return r;
}

/* labels: nx*ny*nz uint32, x fastest.  Returns the number of components, or -1 (bad arguments), -2 (no memory). */
int64_t comp_label(const void *vol, int bytes, int nx, int ny, int nz, float iso_s, uint32_t *labels)
{
    if (!vol || (bytes != 1 && bytes != 2) || nx < 1 || ny < 1 || nz < 1 || !labels) return -1;
    const Volume V = {vol, bytes, {nx, ny, nz}};
    const size_t n = (size_t)nx * (size_t)ny * (size_t)nz, none = (size_t)-1;
    size_t *parent = (size_t *)malloc(n * sizeof(size_t));
    if (!parent) return -2;
    /* pass 1: every inside voxel joins its inside neighbours in the seven directions; the lower root always wins, so a
       component's root is its first voxel */
    for (int k = 0; k < nz; k++)
        for (int j = 0; j < ny; j++)
            for (int i = 0; i < nx; i++) {
                const size_t at = (size_t)i + (size_t)nx * ((size_t)j + (size_t)ny * (size_t)k);
                parent[at] = S(&V, i, j, k) >= iso_s ? at : none;
            }
    for (int k = 0; k < nz; k++)
        for (int j = 0; j < ny; j++)
            for (int i = 0; i < nx; i++) {
                const size_t at = (size_t)i + (size_t)nx * ((size_t)j + (size_t)ny * (size_t)k);
                if (parent[at] == none) continue;
                for (int d = 0; d < 7; d++) {
                    const int bi = i + DIRS[d][0], bj = j + DIRS[d][1], bk = k + DIRS[d][2];
                    if (bi >= nx || bj >= ny || bk >= nz) continue;
                    const size_t b = (size_t)bi + (size_t)nx * ((size_t)bj + (size_t)ny * (size_t)bk);
                    if (parent[b] == none) continue;
                    const size_t ra = find(parent, at), rb = find(parent, b);
                    if (ra < rb) parent[rb] = ra;
                    else if (rb < ra) parent[ra] = rb;
                }
            }
    /* pass 2: step 3's numbering, by ascending first voxel */
    int64_t count = 0;
    for (size_t at = 0; at < n; at++) {
        if (parent[at] == none) { labels[at] = 0; continue; }
        const size_t r = find(parent, at);
        if (r == at) labels[at] = (uint32_t)++count;     /* a root comes before every other voxel of its component */
        else labels[at] = labels[r];
    }
    free(parent);
    return count;
}

/* step 4: the records of n components from the labels */
int comp_records(const uint32_t *labels, int nx, int ny, int nz, uint64_t n, uint64_t *voxels, uint64_t *first_voxel, int32_t *bbox6)
{
    if (!labels || nx < 1 || ny < 1 || nz < 1 || (n && (!voxels || !first_voxel || !bbox6))) return -1;
    for (uint64_t c = 0; c < n; c++) {
        voxels[c] = 0;
        first_voxel[c] = UINT64_MAX;
        for (int a = 0; a < 3; a++) { bbox6[6 * c + a] = INT32_MAX; bbox6[6 * c + 3 + a] = -1; }
    }
    for (int k = 0; k < nz; k++)
        for (int j = 0; j < ny; j++)
            for (int i = 0; i < nx; i++) {
                const uint64_t at = (uint64_t)i + (uint64_t)nx * ((uint64_t)j + (uint64_t)ny * (uint64_t)k);
                const uint32_t l = labels[at];
                if (l == 0) continue;
                if (l > n) return -3;
                const uint64_t c = l - 1;
                const int p[3] = {i, j, k};
                voxels[c]++;
                if (at < first_voxel[c]) first_voxel[c] = at;
                for (int a = 0; a < 3; a++) {
                    if (p[a] < bbox6[6 * c + a]) bbox6[6 * c + a] = p[a];
                    if (p[a] > bbox6[6 * c + 3 + a]) bbox6[6 * c + 3 + a] = p[a];
                }
            }
    return 0;
}

/* step 6: voxels >= min_voxels and, when keep_largest > 0, among the keep_largest first by (voxels descending, label ascending) */
int comp_select(const uint64_t *voxels, uint64_t n, uint64_t min_voxels, uint64_t keep_largest, uint8_t *selected)
{
    if (n && (!voxels || !selected)) return -1;
    for (uint64_t c = 0; c < n; c++) {
        uint64_t ahead = 0;                              /* components before c in the order */
        if (keep_largest > 0)
            for (uint64_t o = 0; o < n; o++)
                if (voxels[o] > voxels[c] || (voxels[o] == voxels[c] && o < c)) ahead++;
        selected[c] = voxels[c] >= min_voxels && (keep_largest == 0 || ahead < keep_largest);
    }
    return 0;
}

/* ------------------------------------------------------------------ the filtered extraction (step 7) */
static int g_ready = 0;
static int g_corner[6][4][3];
static int g_ntri[6][16];
static int g_edge[6][16][6][2];

static void set_tri(int tri[3][2], int a0, int b0, int a1, int b1, int a2, int b2)
{
    tri[0][0] = a0; tri[0][1] = b0; tri[1][0] = a1; tri[1][1] = b1; tri[2][0] = a2; tri[2][1] = b2;
}

static void build_table(void)                            /* the extraction's steps 7 to 9 */
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
            if (ni == 0 || ni == 4) continue;
            if (ni == 1) { set_tri(tri[0], I[0], O[0], I[0], O[1], I[0], O[2]); g_ntri[t][m] = 1; }
            else if (ni == 3) { set_tri(tri[0], O[0], I[0], O[0], I[1], O[0], I[2]); g_ntri[t][m] = 1; }
            else {
                set_tri(tri[0], I[0], O[0], I[0], O[1], I[1], O[1]);
                set_tri(tri[1], I[0], O[0], I[1], O[1], I[1], O[0]);
                g_ntri[t][m] = 2;
            }
            double v[3][3], mo[3] = {0, 0, 0}, mi[3] = {0, 0, 0}, u[3], w[3];
            for (int q = 0; q < 3; q++)
                for (int a = 0; a < 3; a++) v[q][a] = 0.5 * (g_corner[t][tri[0][q][0]][a] + g_corner[t][tri[0][q][1]][a]);
            for (int a = 0; a < 3; a++) {
                for (int n = 0; n < no; n++) mo[a] += g_corner[t][O[n]][a] / (double)no;
                for (int n = 0; n < ni; n++) mi[a] += g_corner[t][I[n]][a] / (double)ni;
            }
            for (int a = 0; a < 3; a++) { u[a] = v[1][a] - v[0][a]; w[a] = v[2][a] - v[0][a]; }
            const double cr[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
            const int swapped = cr[0] * (mo[0] - mi[0]) + cr[1] * (mo[1] - mi[1]) + cr[2] * (mo[2] - mi[2]) < 0.0;
            for (int k = 0; k < g_ntri[t][m]; k++)
                for (int q = 0; q < 3; q++) {
                    const int src = swapped && q > 0 ? 3 - q : q;
                    const int n0 = tri[k][src][0], n1 = tri[k][src][1];
                    g_edge[t][m][3 * k + q][0] = n0 < n1 ? n0 : n1;
                    g_edge[t][m][3 * k + q][1] = n0 < n1 ? n1 : n0;
                }
        }
    }
    g_ready = 1;
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

/* the changed predicate: inside (its label is not 0) and its component selected */
static int kept(const uint32_t *labels, const uint8_t *selected, const Volume *V, int i, int j, int k)
{
    const uint32_t l = labels[(size_t)i + (size_t)V->dim[0] * ((size_t)j + (size_t)V->dim[1] * (size_t)k)];
    return l != 0 && selected[l - 1] != 0;
}

/* Call with NULL arrays for the counts, then again with arrays that hold them.  s, f, gradients: from the raw voxels. */
int comp_extract(const void *vol, int bytes, int nx, int ny, int nz, float iso_s, const float *spacing, const uint32_t *labels,
                 const uint8_t *selected, float *pos, float *nrm, uint32_t *tri, uint64_t vcap, uint64_t tcap, uint64_t *n_vertices,
                 uint64_t *n_triangles)
{
    build_table();
    if (!vol || (bytes != 1 && bytes != 2) || nx < 1 || ny < 1 || nz < 1 || !spacing || !labels || !n_vertices || !n_triangles) return -1;
    const Volume V = {vol, bytes, {nx, ny, nz}};
    *n_vertices = *n_triangles = 0;
    if (nx < 2 || ny < 2 || nz < 2) return 0;
    const size_t n = (size_t)nx * (size_t)ny * (size_t)nz;
    uint64_t *first = (uint64_t *)malloc(n * sizeof(uint64_t));
    uint8_t *active = (uint8_t *)malloc(n);
    if (!first || !active) { free(first); free(active); return -2; }
    uint64_t nv = 0, nt = 0;
    for (int k = 0; k < nz; k++)
        for (int j = 0; j < ny; j++)
            for (int i = 0; i < nx; i++) {
                const size_t at = (size_t)i + (size_t)nx * ((size_t)j + (size_t)ny * (size_t)k);
                const int A[3] = {i, j, k};
                const float sa = S(&V, i, j, k);
                const int ka = kept(labels, selected, &V, i, j, k);
                float ga[3];
                int have_ga = 0;
                first[at] = nv;
                active[at] = 0;
                for (int d = 0; d < 7; d++) {
                    const int B[3] = {i + DIRS[d][0], j + DIRS[d][1], k + DIRS[d][2]};
                    if (B[0] >= nx || B[1] >= ny || B[2] >= nz) continue;
                    if (ka == kept(labels, selected, &V, B[0], B[1], B[2])) continue;
                    const float sb = S(&V, B[0], B[1], B[2]);
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
    for (int k = 0; k < nz - 1; k++)
        for (int j = 0; j < ny - 1; j++)
            for (int i = 0; i < nx - 1; i++)
                for (int t = 0; t < 6; t++) {
                    int m = 0;
                    for (int c = 0; c < 4; c++)
                        if (kept(labels, selected, &V, i + g_corner[t][c][0], j + g_corner[t][c][1], k + g_corner[t][c][2])) m |= 1 << c;
                    for (int q = 0; q < 3 * g_ntri[t][m]; q++) {
                        const int *cn = g_corner[t][g_edge[t][m][q][0]], *cm = g_corner[t][g_edge[t][m][q][1]];
                        const int e[3] = {cm[0] - cn[0], cm[1] - cn[1], cm[2] - cn[2]};
                        const int d = dir_index(e);
                        const size_t at = (size_t)(i + cn[0]) + (size_t)nx * ((size_t)(j + cn[1]) + (size_t)ny * (size_t)(k + cn[2]));
                        if (d < 0 || !(active[at] & (1 << d))) { free(first); free(active); return -4; }
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
