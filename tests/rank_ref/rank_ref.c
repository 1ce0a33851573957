/* TEST INFRASTRUCTURE ONLY -- the CPU definition of vr_rank_filter_volume (include/vr_core.h, points 1 to 3), by brute force:
   per voxel gather the clamped window, then take the minimum, the maximum, or sort and pick.  It deliberately shares nothing
   with the kernels' separable passes or their selection network.  Volumes are [z][y][x], x fastest, linear. */
#include <stdint.h>
#include <stdlib.h>

enum { RANK_OFF = 0, RANK_ERODE = 1, RANK_DILATE = 2, RANK_OPEN = 3, RANK_CLOSE = 4, RANK_MEDIAN = 5 };

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static uint32_t voxel(const void *vol, int bytes, int nx, int ny, int i, int j, int k)
{
    const size_t at = (size_t)i + (size_t)nx * ((size_t)j + (size_t)ny * (size_t)k);
    return bytes == 1 ? (uint32_t)((const uint8_t *)vol)[at] : (uint32_t)((const uint16_t *)vol)[at];
}

static int ascending(const void *a, const void *b)
{
    const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
    return x < y ? -1 : (x > y ? 1 : 0);
}

/* one single operation (ERODE, DILATE or MEDIAN) at voxel (i, j, k) */
static uint32_t single_at(const void *in, int bytes, int nx, int ny, int nz, int op, const int r[3], int i, int j, int k, uint32_t *win)
{
    int n = 0;
    for (int c = -r[2]; c <= r[2]; c++)
        for (int b = -r[1]; b <= r[1]; b++)
            for (int a = -r[0]; a <= r[0]; a++)
                win[n++] = voxel(in, bytes, nx, ny, clampi(i + a, 0, nx - 1), clampi(j + b, 0, ny - 1), clampi(k + c, 0, nz - 1));
    if (op == RANK_MEDIAN) {
        qsort(win, (size_t)n, sizeof(uint32_t), ascending);
        return win[(n - 1) / 2];
    }
    uint32_t v = win[0];
    for (int t = 1; t < n; t++) {
        if (op == RANK_ERODE && win[t] < v) v = win[t];
        if (op == RANK_DILATE && win[t] > v) v = win[t];
    }
    return v;
}

static int single_volume(const void *in, int bytes, int nx, int ny, int nz, int op, const int r[3], void *out)
{
    const size_t n = (size_t)(2 * r[0] + 1) * (size_t)(2 * r[1] + 1) * (size_t)(2 * r[2] + 1);
    uint32_t *win = (uint32_t *)malloc(n * sizeof(uint32_t));
    if (!win) return 2;
    for (int k = 0; k < nz; k++)
        for (int j = 0; j < ny; j++)
            for (int i = 0; i < nx; i++) {
                const uint32_t v = single_at(in, bytes, nx, ny, nz, op, r, i, j, k, win);
                const size_t at = (size_t)i + (size_t)nx * ((size_t)j + (size_t)ny * (size_t)k);
                if (bytes == 1) ((uint8_t *)out)[at] = (uint8_t)v;
                else ((uint16_t *)out)[at] = (uint16_t)v;
            }
    free(win);
    return 0;
}

/* 0: done; 1: refused arguments (point 4); 2: out of memory.  OFF or all radii 0 copies. */
int rank_volume(const void *in, int bytes, int nx, int ny, int nz, int op, int rx, int ry, int rz, void *out)
{
    const int r[3] = {rx, ry, rz};
    const int hi = op == RANK_MEDIAN ? 1 : 8;
    if (!in || !out || (bytes != 1 && bytes != 2) || nx <= 0 || ny <= 0 || nz <= 0 || op < RANK_OFF || op > RANK_MEDIAN) return 1;
    for (int a = 0; a < 3; a++)
        if (r[a] < 0 || r[a] > hi) return 1;
    const size_t total = (size_t)nx * (size_t)ny * (size_t)nz * (size_t)bytes;
    if (op == RANK_OFF || (rx == 0 && ry == 0 && rz == 0)) {
        for (size_t t = 0; t < total; t++) ((uint8_t *)out)[t] = ((const uint8_t *)in)[t];
        return 0;
    }
    if (op == RANK_OPEN || op == RANK_CLOSE) {
        /* the second stage reads the first stage's output and clamps at ITS edges */
        void *mid = malloc(total);
        if (!mid) return 2;
        int rc = single_volume(in, bytes, nx, ny, nz, op == RANK_OPEN ? RANK_ERODE : RANK_DILATE, r, mid);
        if (rc == 0) rc = single_volume(mid, bytes, nx, ny, nz, op == RANK_OPEN ? RANK_DILATE : RANK_ERODE, r, out);
        free(mid);
        return rc;
    }
    return single_volume(in, bytes, nx, ny, nz, op, r, out);
}

/* single operations only: the value at each of n voxels ijk[3n] = (x, y, z), each from its own window of `in` */
int rank_points(const void *in, int bytes, int nx, int ny, int nz, int op, int rx, int ry, int rz, int n, const int32_t *ijk, uint32_t *out)
{
    const int r[3] = {rx, ry, rz};
    if (!in || !out || !ijk || (bytes != 1 && bytes != 2) || (op != RANK_ERODE && op != RANK_DILATE && op != RANK_MEDIAN)) return 1;
    for (int a = 0; a < 3; a++)
        if (r[a] < 0 || r[a] > (op == RANK_MEDIAN ? 1 : 8)) return 1;
    uint32_t *win = (uint32_t *)malloc((size_t)(2 * rx + 1) * (size_t)(2 * ry + 1) * (size_t)(2 * rz + 1) * sizeof(uint32_t));
    if (!win) return 2;
    for (int t = 0; t < n; t++) {
        const int i = ijk[3 * t], j = ijk[3 * t + 1], k = ijk[3 * t + 2];
        if (i < 0 || j < 0 || k < 0 || i >= nx || j >= ny || k >= nz) { free(win); return 1; }
        out[t] = single_at(in, bytes, nx, ny, nz, op, r, i, j, k, win);
    }
    free(win);
    return 0;
}
