/* TEST INFRASTRUCTURE ONLY -- the CPU definition of vr_simplify_mesh (include/vr_core.h, steps 1 to 5), in plain C: two qsorts
   and nothing clever.  Built with -ffp-contract=off -fno-fast-math: every fp32 step is one correctly rounded operation.

   simplify_mesh: positions / normals [nv][3], triangles [nt][3] -> out_* (capacity nv vertices, nt triangles: the output is never
   larger), *out_nv, *out_nt, and rows[v'] = the input index of output vertex v' (may be NULL).
   Returns 0; 1: cell is not a normal number above 0; 2: a quotient is not in [0, 2^21); 3: out of memory; 4: an index >= nv. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { int32_t c[3]; uint32_t dist, index; } vert_t;
typedef struct { uint32_t s[3], index; } trip_t;

static uint32_t float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static int by_cell_dist_index(const void *pa, const void *pb)
{
    const vert_t *a = (const vert_t *)pa, *b = (const vert_t *)pb;
    for (int k = 2; k >= 0; k--)
        if (a->c[k] != b->c[k]) return a->c[k] < b->c[k] ? -1 : 1;
    if (a->dist != b->dist) return a->dist < b->dist ? -1 : 1;      /* non-negative floats order like their bits */
    return a->index < b->index ? -1 : a->index > b->index;
}

static int by_set_index(const void *pa, const void *pb)
{
    const trip_t *a = (const trip_t *)pa, *b = (const trip_t *)pb;
    for (int k = 0; k < 3; k++)
        if (a->s[k] != b->s[k]) return a->s[k] < b->s[k] ? -1 : 1;
    return a->index < b->index ? -1 : a->index > b->index;
}

int simplify_mesh(const float *pos, const float *nrm, const uint32_t *tri, uint64_t nv, uint64_t nt, float cell,
                  float *out_pos, float *out_nrm, uint32_t *out_tri, uint64_t *out_nv, uint64_t *out_nt, uint32_t *rows)
{
    *out_nv = *out_nt = 0;
    if (!isnormal(cell) || !(cell > 0.0f)) return 1;
    if (nv == 0 || nt == 0) return 0;
    vert_t *verts = (vert_t *)malloc(nv * sizeof(vert_t));
    trip_t *trips = (trip_t *)malloc(nt * sizeof(trip_t));
    uint32_t *rep = (uint32_t *)malloc(nv * sizeof(uint32_t)), *renumber = (uint32_t *)malloc(nv * sizeof(uint32_t));
    uint8_t *used = (uint8_t *)calloc(nv, 1), *keep = (uint8_t *)calloc(nt, 1);
    int rc = 0;
    if (!verts || !trips || !rep || !renumber || !used || !keep) { rc = 3; goto done; }
    /* steps 2 and 3 */
    for (uint64_t v = 0; v < nv && rc == 0; v++) {
        float d[3];
        for (int a = 0; a < 3; a++) {
            const float p = pos[3 * v + a];
            const float q = p / cell;
            if (!(q >= 0.0f && q < 2097152.0f)) { rc = 2; break; }
            const int32_t c = (int32_t)floorf(q);
            const float half = (float)c + 0.5f;
            const float centre = half * cell;
            verts[v].c[a] = c;
            d[a] = p - centre;
        }
        const float zz = d[2] * d[2], yy = d[1] * d[1], xx = d[0] * d[0];
        const float zy = zz + yy;
        const float dist = zy + xx;
        verts[v].dist = float_bits(dist);
        verts[v].index = (uint32_t)v;
    }
    if (rc) goto done;
    qsort(verts, nv, sizeof(vert_t), by_cell_dist_index);
    for (uint64_t i = 0, head = 0; i < nv; i++) {
        if (i > 0 && memcmp(verts[i].c, verts[i - 1].c, sizeof(verts[i].c)) != 0) head = i;
        rep[verts[i].index] = verts[head].index;
    }
    /* step 4 */
    uint64_t n = 0;
    for (uint64_t t = 0; t < nt; t++) {
        uint32_t s[3];
        for (int k = 0; k < 3; k++) {
            if (tri[3 * t + k] >= nv) { rc = 4; goto done; }
            s[k] = rep[tri[3 * t + k]];
        }
        if (s[0] == s[1] || s[1] == s[2] || s[0] == s[2]) continue;
        if (s[0] > s[1]) { uint32_t x = s[0]; s[0] = s[1]; s[1] = x; }
        if (s[1] > s[2]) { uint32_t x = s[1]; s[1] = s[2]; s[2] = x; }
        if (s[0] > s[1]) { uint32_t x = s[0]; s[0] = s[1]; s[1] = x; }
        memcpy(trips[n].s, s, sizeof(s));
        trips[n++].index = (uint32_t)t;
    }
    qsort(trips, n, sizeof(trip_t), by_set_index);
    for (uint64_t i = 0; i < n; i++)
        if (i == 0 || memcmp(trips[i].s, trips[i - 1].s, sizeof(trips[i].s)) != 0) {
            keep[trips[i].index] = 1;
            for (int k = 0; k < 3; k++) used[trips[i].s[k]] = 1;
        }
    /* step 5 */
    uint64_t onv = 0, ont = 0;
    for (uint64_t v = 0; v < nv; v++) {
        if (!used[v]) continue;
        renumber[v] = (uint32_t)onv;
        memcpy(out_pos + 3 * onv, pos + 3 * v, 12);
        memcpy(out_nrm + 3 * onv, nrm + 3 * v, 12);
        if (rows) rows[onv] = (uint32_t)v;
        onv++;
    }
    for (uint64_t t = 0; t < nt; t++) {
        if (!keep[t]) continue;
        for (int k = 0; k < 3; k++) out_tri[3 * ont + k] = renumber[rep[tri[3 * t + k]]];
        ont++;
    }
    *out_nv = onv;
    *out_nt = ont;
done:
    free(verts); free(trips); free(rep); free(renumber); free(used); free(keep);
    return rc;
}
