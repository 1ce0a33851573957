/* TEST INFRASTRUCTURE ONLY -- the CPU definition of vr_smooth_volume (include/vr_core.h), plain C99.
 * Build with -O2 -std=c99 -ffp-contract=off -fno-fast-math: every product and every sum below is one correctly rounded fp32
 * operation and nothing is contracted into an fma.
 *
 * The weights are INPUTS (2r + 1 floats per axis, from vr_smooth_weights): the kernels and this file share them by
 * construction.  r < 0 means "no pass along this axis" (sigma == 0).
 *
 *   pass along axis a:  acc = 0.0f;  for t = -r .. r:  acc = acc + w[t + r] * in[clamp(i_a + t, 0, dim_a - 1)]
 *   order x, y, z; the first pass reads (float)voxel; intermediates stay fp32
 *   store: rintf (half to even) of the last pass, clamped to the voxel type
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static float voxel_at(const void *vol, int bytes, size_t idx)
{
    return bytes == 1 ? (float)((const uint8_t *)vol)[idx] : (float)((const uint16_t *)vol)[idx];
}

static uint32_t to_voxel(float v, int bytes)
{
    const float hi = bytes == 1 ? 255.0f : 65535.0f;
    float q = rintf(v);
    if (q < 0.0f) q = 0.0f;
    if (q > hi) q = hi;
    return (uint32_t)q;
}

/* one pass over a whole fp32 volume; stride[a] = distance of neighbours along axis a */
static void pass(const float *in, float *out, const int dim[3], int axis, const float *w, int r)
{
    const size_t stride[3] = {1, (size_t)dim[0], (size_t)dim[0] * (size_t)dim[1]};
    for (int k = 0; k < dim[2]; k++)
        for (int j = 0; j < dim[1]; j++)
            for (int i = 0; i < dim[0]; i++) {
                const int c[3] = {i, j, k};
                const size_t base = (size_t)i + stride[1] * (size_t)j + stride[2] * (size_t)k;
                float acc = 0.0f;
                for (int t = -r; t <= r; t++) {
                    const int q = clampi(c[axis] + t, 0, dim[axis] - 1);
                    const float prod = w[t + r] * in[base + ((size_t)q - (size_t)c[axis]) * stride[axis]];
                    acc = acc + prod;
                }
                out[base] = acc;
            }
}

/* whole volume, x fastest; out has the type of vol.  0 on success. */
int smooth_volume(const void *vol, int bytes, int nx, int ny, int nz, const float *wx, int rx, const float *wy, int ry,
                  const float *wz, int rz, void *out)
{
    if (!vol || !out || (bytes != 1 && bytes != 2) || nx <= 0 || ny <= 0 || nz <= 0) return 1;
    const int dim[3] = {nx, ny, nz};
    const size_t n = (size_t)nx * (size_t)ny * (size_t)nz;
    float *a = (float *)malloc(n * sizeof(float)), *b = (float *)malloc(n * sizeof(float));
    if (!a || !b) { free(a); free(b); return 2; }
    for (size_t i = 0; i < n; i++) a[i] = voxel_at(vol, bytes, i);
    const float *w[3] = {wx, wy, wz};
    const int r[3] = {rx, ry, rz};
    int passes = 0;
    for (int axis = 0; axis < 3; axis++)
        if (r[axis] >= 0 && w[axis]) {
            pass(a, b, dim, axis, w[axis], r[axis]);
            float *t = a; a = b; b = t;
            passes++;
        }
    if (passes == 0) {
        memcpy(out, vol, n * (size_t)bytes);
    } else {
        for (size_t i = 0; i < n; i++) {
            const uint32_t v = to_voxel(a[i], bytes);
            if (bytes == 1) ((uint8_t *)out)[i] = (uint8_t)v; else ((uint16_t *)out)[i] = (uint16_t)v;
        }
    }
    free(a); free(b);
    return 0;
}

/* one output voxel from its (2rx+1)(2ry+1)(2rz+1) neighbourhood: the same operations in the same order as above */
static uint32_t point(const void *vol, int bytes, const int dim[3], const float *const w[3], const int r[3], int i, int j, int k)
{
    const int ex = r[0] >= 0 && w[0], ey = r[1] >= 0 && w[1], ez = r[2] >= 0 && w[2];
    if (!ex && !ey && !ez) return (uint32_t)voxel_at(vol, bytes, (size_t)i + (size_t)dim[0] * ((size_t)j + (size_t)dim[1] * (size_t)k));
    const int ry = ey ? r[1] : 0, rz = ez ? r[2] : 0;
    float zacc = 0.0f, zlast = 0.0f;
    for (int tz = -rz; tz <= rz; tz++) {
        const int kk = clampi(k + tz, 0, dim[2] - 1);
        float yacc = 0.0f, ylast = 0.0f;
        for (int ty = -ry; ty <= ry; ty++) {
            const int jj = clampi(j + ty, 0, dim[1] - 1);
            const size_t row = (size_t)dim[0] * ((size_t)jj + (size_t)dim[1] * (size_t)kk);
            float xv;
            if (ex) {
                float acc = 0.0f;
                for (int tx = -r[0]; tx <= r[0]; tx++) {
                    const float prod = w[0][tx + r[0]] * voxel_at(vol, bytes, row + (size_t)clampi(i + tx, 0, dim[0] - 1));
                    acc = acc + prod;
                }
                xv = acc;
            } else {
                xv = voxel_at(vol, bytes, row + (size_t)i);
            }
            if (ey) { const float prod = w[1][ty + ry] * xv; yacc = yacc + prod; }
            ylast = xv;
        }
        const float yv = ey ? yacc : ylast;
        if (ez) { const float prod = w[2][tz + rz] * yv; zacc = zacc + prod; }
        zlast = yv;
    }
    return to_voxel(ez ? zacc : zlast, bytes);
}

/* n output voxels at ijk[3 * p + 0 .. 2] (inside the volume) -> out[p] */
int smooth_points(const void *vol, int bytes, int nx, int ny, int nz, const float *wx, int rx, const float *wy, int ry,
                  const float *wz, int rz, int n, const int32_t *ijk, uint32_t *out)
{
    if (!vol || !out || !ijk || (bytes != 1 && bytes != 2) || nx <= 0 || ny <= 0 || nz <= 0) return 1;
    const int dim[3] = {nx, ny, nz};
    const float *const w[3] = {wx, wy, wz};
    const int r[3] = {rx, ry, rz};
    for (int p = 0; p < n; p++) {
        const int i = ijk[3 * p], j = ijk[3 * p + 1], k = ijk[3 * p + 2];
        if (i < 0 || i >= nx || j < 0 || j >= ny || k < 0 || k >= nz) return 3;
        out[p] = point(vol, bytes, dim, w, r, i, j, k);
    }
    return 0;
}
