/* TEST INFRASTRUCTURE ONLY -- the CPU definition of vr_smooth_mesh (include/vr_core.h, steps 2 to 6), in plain C: two qsorts and
   nothing clever.  Built with -ffp-contract=off -fno-fast-math: every fp32 step is one correctly rounded operation.

   mesh_smooth: positions [nv][3] and triangles [nt][3] -> out_pos, out_nrm [nv][3], fixed [nv] (1: the vertex is FIXED; may be
   NULL) and *n_fixed.  iterations == 0 is the caller's business (the mesh keeps its normals): here it gives the input positions
   and the normals of step 6.
   Returns 0; 1: a parameter outside step 9's ranges; 2: 6 nt > 2^32 - 1; 3: out of memory; 4: an index >= nv. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int by_value(const void *pa, const void *pb)
{
    const uint64_t a = *(const uint64_t *)pa, b = *(const uint64_t *)pb;
    return a < b ? -1 : a > b;
}

/* step 4: one Jacobi step with factor phi, p -> q */
static void step(const float *p, float *q, uint64_t nv, const uint64_t *row, const uint32_t *nbr, const uint8_t *fixed, float phi)
{
    for (uint64_t i = 0; i < nv; i++) {
        const uint64_t k = row[i + 1] - row[i];
        for (int a = 0; a < 3; a++) {
            const float own = p[3 * i + a];
            if (fixed[i] || k == 0) { q[3 * i + a] = own; continue; }
            float acc = 0.0f;
            for (uint64_t j = row[i]; j < row[i + 1]; j++) acc = acc + p[3 * (uint64_t)nbr[j] + a];
            const float m = acc / (float)k;
            const float d = m - own;
            const float s = phi * d;
            q[3 * i + a] = own + s;
        }
    }
}

int mesh_smooth(const float *pos, const uint32_t *tri, uint64_t nv, uint64_t nt, int iterations, float lambda, float mu, int fix_boundary,
                float *out_pos, float *out_nrm, uint8_t *out_fixed, uint64_t *n_fixed)
{
    *n_fixed = 0;
    if (iterations < 0 || iterations > 1000) return 1;
    if (!isfinite(lambda) || !(lambda > 0.0f && lambda <= 1.0f)) return 1;
    if (!isfinite(mu) || !(mu >= -2.0f && mu <= 0.0f)) return 1;
    if (nt > 0xffffffffull / 6) return 2;
    for (uint64_t q = 0; q < 3 * nt; q++)
        if (tri[q] >= nv) return 4;
    if (nv == 0) return 0;
    uint64_t *pair = (uint64_t *)malloc((6 * nt + 1) * sizeof(uint64_t)), *row = (uint64_t *)calloc(nv + 1, sizeof(uint64_t));
    uint64_t *corner = (uint64_t *)malloc((3 * nt + 1) * sizeof(uint64_t));
    uint32_t *nbr = (uint32_t *)malloc((6 * nt + 1) * sizeof(uint32_t));
    uint8_t *fixed = (uint8_t *)calloc(nv, 1);
    float *p = (float *)malloc(nv * 12), *q = (float *)malloc(nv * 12), *face = (float *)malloc((nt + 1) * 12);
    int rc = 0;
    if (!pair || !row || !corner || !nbr || !fixed || !p || !q || !face) { rc = 3; goto done; }
    /* step 2: the directed pairs, sorted by (i, j); a run of equal pairs is one neighbour, its length the multiplicity */
    uint64_t np = 0;
    for (uint64_t t = 0; t < nt; t++)
        for (int e = 0; e < 3; e++) {
            const uint64_t a = tri[3 * t + e], b = tri[3 * t + (e + 1) % 3];
            if (a == b) continue;
            pair[np++] = a << 32 | b;
            pair[np++] = b << 32 | a;
        }
    qsort(pair, np, sizeof(uint64_t), by_value);
    uint64_t nn = 0;
    for (uint64_t i = 0; i < np;) {
        uint64_t run = 1;
        while (i + run < np && pair[i + run] == pair[i]) run++;
        const uint64_t a = pair[i] >> 32;
        nbr[nn++] = (uint32_t)pair[i];
        row[a + 1]++;
        if (run == 1 && fix_boundary) fixed[a] = 1;       /* step 3 (the other end is marked by the reverse pair) */
        i += run;
    }
    for (uint64_t i = 0; i < nv; i++) row[i + 1] += row[i];
    /* steps 4 and 5 */
    memcpy(p, pos, nv * 12);
    for (int it = 0; it < iterations; it++) {
        step(p, q, nv, row, nbr, fixed, lambda);
        { float *x = p; p = q; q = x; }
        if (mu == 0.0f) continue;
        step(p, q, nv, row, nbr, fixed, mu);
        { float *x = p; p = q; q = x; }
    }
    /* step 6 */
    for (uint64_t t = 0; t < nt; t++) {
        const float *p0 = p + 3 * (uint64_t)tri[3 * t], *p1 = p + 3 * (uint64_t)tri[3 * t + 1], *p2 = p + 3 * (uint64_t)tri[3 * t + 2];
        float u[3], w[3];
        for (int a = 0; a < 3; a++) { u[a] = p1[a] - p0[a]; w[a] = p2[a] - p0[a]; }
        for (int a = 0; a < 3; a++) {
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            const float left = u[b] * w[c], right = u[c] * w[b];
            face[3 * t + a] = left - right;
        }
    }
    for (uint64_t n = 0; n < 3 * nt; n++) corner[n] = (uint64_t)tri[n] << 32 | n;     /* by vertex, then by (t, corner) */
    qsort(corner, 3 * nt, sizeof(uint64_t), by_value);
    uint64_t at = 0;
    for (uint64_t i = 0; i < nv; i++) {
        float s[3] = {0.0f, 0.0f, 0.0f};
        for (; at < 3 * nt && corner[at] >> 32 == i; at++) {
            const uint64_t t = (corner[at] & 0xffffffffull) / 3;
            for (int a = 0; a < 3; a++) s[a] = s[a] + face[3 * t + a];
        }
        const float zz = s[2] * s[2], yy = s[1] * s[1], xx = s[0] * s[0];
        const float zy = zz + yy;
        const float dot = zy + xx;
        if (dot == 0.0f) {
            out_nrm[3 * i] = out_nrm[3 * i + 1] = out_nrm[3 * i + 2] = 0.0f;
        } else {
            const float root = sqrtf(dot);
            const float rn = 1.0f / root;
            for (int a = 0; a < 3; a++) out_nrm[3 * i + a] = s[a] * rn;
        }
    }
    memcpy(out_pos, p, nv * 12);
    for (uint64_t i = 0; i < nv; i++) *n_fixed += fixed[i];
    if (out_fixed) memcpy(out_fixed, fixed, nv);
done:
    free(pair); free(row); free(corner); free(nbr); free(fixed); free(p); free(q); free(face);
    return rc;
}
