/*
 * shade_ref.c -- TEST INFRASTRUCTURE ONLY: scalar CPU restatement of gradient-lit compositing
 * (include/vr_core.h: vr_set_shading; volume-renderer_amd/csrc/vr_shade.hip is held to it bit for bit).
 *
 * Plain C99, built by the tests with -O2 -std=c99 -ffp-contract=off -fno-fast-math: every + - * / sqrt below is one
 * correctly rounded binary32 operation, the only fused operations are the explicit fmaf() of TRILINEAR's lerps.
 * Ray set-up, box intersection, texture-coordinate mapping, the samplers and the composite march restate oracle/vr_oracle.c
 * (its MESA model); the normal and the headlight restate tests/iso_ref/iso_ref.c.
 */
#include <math.h>
#include <stdint.h>
#include <stddef.h>

typedef struct shade_params {
    int32_t img_w, img_h, row_begin, row_end, trunc_grid;
    int32_t nx, ny, nz, bytes_per_voxel;
    const void *volume;                 /* x fastest, then y, then z */
    float cam[21];
    float voxel_size[3];
    int32_t min_val, max_val;           /* the window as the kernel sees it (after the +1000 of the u16 offset) */
    int32_t view_top, view_bottom, filter, accum, max_steps;
    const float *tf_rgba;               /* tf_len RGBA entries or NULL */
    int32_t tf_len;
    float alpha_scale;
    float ambient, diffuse, specular;   /* vr_set_shading's coefficients */
    int32_t shininess;                  /* 1, 2, 4, ..., 128 */
} shade_params;

typedef struct { float x, y, z; } v3;

static inline float gl_min(float x, float y) { return (y < x) ? y : x; }
static inline float gl_max(float x, float y) { return (x < y) ? y : x; }

typedef struct {
    float pmin[3], pmax[3], half[3], ext[3], step, fdim[3], fmin, fmax, fden;
} consts;

static void setup(const shade_params *p, consts *c)
{
    int max_dim = p->nx > p->ny ? p->nx : p->ny;
    max_dim = max_dim > p->nz ? max_dim : p->nz;
    int swz = (p->view_bottom == 1 || p->view_top == 1);
    float d0 = (float)p->nx, d1 = swz ? (float)p->nz : (float)p->ny, d2 = swz ? (float)p->ny : (float)p->nz;
    float s0 = p->voxel_size[0], s1 = swz ? p->voxel_size[2] : p->voxel_size[1], s2 = swz ? p->voxel_size[1] : p->voxel_size[2];
    float fmd = (float)max_dim;
    float pm[3] = { (d0 / fmd) * s0, (d1 / fmd) * s1, (d2 / fmd) * s2 };
    for (int i = 0; i < 3; i++) {
        c->half[i] = pm[i] / 2.0f;
        c->pmin[i] = 0.0f - c->half[i];
        c->pmax[i] = pm[i] - c->half[i];
        c->ext[i] = c->pmax[i] + c->half[i];
    }
    c->fdim[0] = (float)p->nx; c->fdim[1] = (float)p->ny; c->fdim[2] = (float)p->nz;
    /* the composite step (VolumeRenderer.cs:109): length(p_max - p_min) / length(vol_size.xzy) */
    float e0 = c->pmax[0] - c->pmin[0], e1 = c->pmax[1] - c->pmin[1], e2 = c->pmax[2] - c->pmin[2];
    float num = sqrtf((e2 * e2 + e1 * e1) + e0 * e0);
    float fx = (float)p->nx, fy = (float)p->ny, fz = (float)p->nz;
    float den = sqrtf((fy * fy + fz * fz) + fx * fx);
    c->step = num / den;
    c->fmin = (float)p->min_val; c->fmax = (float)p->max_val; c->fden = (float)(p->max_val - p->min_val);
}

static void compute_ray(const shade_params *p, float pxf, float pyf, v3 *o, v3 *d)
{
    const float *c = p->cam;
    float fw = (float)p->img_w, fh = (float)p->img_h;
    float aspect = (fw * 1.0f) / fh;
    float x = aspect * (((2.0f * pxf) / fw) - 1.0f);
    float y = ((2.0f * pyf) / fh) - 1.0f;
    float z = -c[20], w = 0.0f;
    float rs = 1.0f / sqrtf(((w * w + z * z) + y * y) + x * x);
    float dx = x * rs, dy = y * rs, dz = z * rs, dw = w * rs;
    float mx = ((c[0] * dx + c[4] * dy) + c[8] * dz) + c[12] * dw;
    float my = ((c[1] * dx + c[5] * dy) + c[9] * dz) + c[13] * dw;
    float mz = ((c[2] * dx + c[6] * dy) + c[10] * dz) + c[14] * dw;
    float mw = ((c[3] * dx + c[7] * dy) + c[11] * dz) + c[15] * dw;
    rs = 1.0f / sqrtf(((mw * mw + mz * mz) + my * my) + mx * mx);
    d->x = mx * rs; d->y = my * rs; d->z = mz * rs;
    o->x = c[16]; o->y = c[17]; o->z = c[18];
}

static int intersect(const consts *c, const v3 *o, const v3 *d, float *t_min)
{
    float tmax = INFINITY, tmin = -INFINITY;
    float ix = 1.0f / d->x, iy = 1.0f / d->y, iz = 1.0f / d->z;
    float mnx = (c->pmin[0] - o->x) * ix, mny = (c->pmin[1] - o->y) * iy, mnz = (c->pmin[2] - o->z) * iz;
    float mxx = (c->pmax[0] - o->x) * ix, mxy = (c->pmax[1] - o->y) * iy, mxz = (c->pmax[2] - o->z) * iz;
    tmin = gl_max(tmin, gl_min(mnx, mxx));
    tmax = gl_min(tmax, gl_max(mnx, mxx));
    tmin = gl_max(tmin, gl_min(mny, mxy));
    tmax = gl_min(tmax, gl_max(mny, mxy));
    if (tmax < tmin) return 0;
    tmin = gl_max(tmin, gl_min(mnz, mxz));
    tmax = gl_min(tmax, gl_max(mnz, mxz));
    *t_min = tmin;
    return tmax > gl_max(tmin, 0.0f);
}

static inline void texcoord(const shade_params *p, const consts *c, float qx, float qy, float qz, float tc[3])
{
    float ux = (qx + c->half[0]) / c->ext[0], uy = (qy + c->half[1]) / c->ext[1], uz = (qz + c->half[2]) / c->ext[2];
    float uzr = uz;
    uz = 1.0f - uz;
    if (p->view_top == 1) { tc[0] = ux; tc[1] = uzr; tc[2] = uy; }
    else if (p->view_bottom == 1) { tc[0] = ux; tc[1] = uz; tc[2] = 1.0f - uy; }
    else { tc[0] = ux; tc[1] = uy; tc[2] = uz; }
}

static inline int64_t clampi(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

static inline float voxel(const shade_params *p, int64_t i, int64_t j, int64_t k)
{
    int64_t idx = i + (int64_t)p->nx * (j + (int64_t)p->ny * k);
    if (p->bytes_per_voxel == 1) return (float)((const uint8_t *)p->volume)[idx];
    return (float)((const uint16_t *)p->volume)[idx];
}

static inline int64_t nearest_index(float tc, float fdim, int n)
{
    float f = floorf(tc * fdim);
    int64_t i = (f != f) ? 0 : (f < -9.2e18f ? INT64_MIN / 2 : (f > 9.2e18f ? INT64_MAX / 2 : (int64_t)f));
    return clampi(i, 0, n - 1);
}

/* TRILINEAR at continuous voxel coordinates (u, v, w) = tc * dim - 0.5 */
static float trilinear(const shade_params *p, float u, float v, float w)
{
    float fu = floorf(u), fv = floorf(v), fw = floorf(w);
    float ax = u - fu, ay = v - fv, az = w - fw;
    int64_t i0 = clampi((int64_t)fu, 0, p->nx - 1), i1 = clampi((int64_t)fu + 1, 0, p->nx - 1);
    int64_t j0 = clampi((int64_t)fv, 0, p->ny - 1), j1 = clampi((int64_t)fv + 1, 0, p->ny - 1);
    int64_t k0 = clampi((int64_t)fw, 0, p->nz - 1), k1 = clampi((int64_t)fw + 1, 0, p->nz - 1);
    float c000 = voxel(p, i0, j0, k0), c100 = voxel(p, i1, j0, k0), c010 = voxel(p, i0, j1, k0), c110 = voxel(p, i1, j1, k0);
    float c001 = voxel(p, i0, j0, k1), c101 = voxel(p, i1, j0, k1), c011 = voxel(p, i0, j1, k1), c111 = voxel(p, i1, j1, k1);
    float c00 = fmaf(ax, c100 - c000, c000), c10 = fmaf(ax, c110 - c010, c010);
    float c01 = fmaf(ax, c101 - c001, c001), c11 = fmaf(ax, c111 - c011, c011);
    float c0 = fmaf(ay, c10 - c00, c00), c1 = fmaf(ay, c11 - c01, c01);
    return fmaf(az, c1 - c0, c0);
}

static float sample_tc(const shade_params *p, const consts *c, const float tc[3])
{
    if (p->filter == 0)
        return voxel(p, nearest_index(tc[0], c->fdim[0], p->nx), nearest_index(tc[1], c->fdim[1], p->ny), nearest_index(tc[2], c->fdim[2], p->nz));
    return trilinear(p, tc[0] * c->fdim[0] - 0.5f, tc[1] * c->fdim[1] - 0.5f, tc[2] * c->fdim[2] - 0.5f);
}

/* the normal at continuous texture coordinates tc (vr_core.h: vr_set_shading step 3 = vr_set_isosurface step 4 at h = q_i) */
static void normal_at(const shade_params *p, const consts *c, const v3 *d, const float tc[3], float n[3])
{
    float gx, gy, gz;
    if (p->filter == 0) {
        int64_t vi = nearest_index(tc[0], c->fdim[0], p->nx), vj = nearest_index(tc[1], c->fdim[1], p->ny), vk = nearest_index(tc[2], c->fdim[2], p->nz);
        gx = voxel(p, clampi(vi + 1, 0, p->nx - 1), vj, vk) - voxel(p, clampi(vi - 1, 0, p->nx - 1), vj, vk);
        gy = voxel(p, vi, clampi(vj + 1, 0, p->ny - 1), vk) - voxel(p, vi, clampi(vj - 1, 0, p->ny - 1), vk);
        gz = voxel(p, vi, vj, clampi(vk + 1, 0, p->nz - 1)) - voxel(p, vi, vj, clampi(vk - 1, 0, p->nz - 1));
    } else {
        float u = tc[0] * c->fdim[0] - 0.5f, v = tc[1] * c->fdim[1] - 0.5f, w = tc[2] * c->fdim[2] - 0.5f;
        gx = trilinear(p, u + 1.0f, v, w) - trilinear(p, u - 1.0f, v, w);
        gy = trilinear(p, u, v + 1.0f, w) - trilinear(p, u, v - 1.0f, w);
        gz = trilinear(p, u, v, w + 1.0f) - trilinear(p, u, v, w - 1.0f);
    }
    float Gx = gx * (c->fdim[0] / c->ext[0]), Gy, Gz;
    if (p->view_top == 1) { Gy = gz * (c->fdim[2] / c->ext[1]); Gz = gy * (c->fdim[1] / c->ext[2]); }
    else if (p->view_bottom == 1) { Gy = -(gz * (c->fdim[2] / c->ext[1])); Gz = -(gy * (c->fdim[1] / c->ext[2])); }
    else { Gy = gy * (c->fdim[1] / c->ext[1]); Gz = -(gz * (c->fdim[2] / c->ext[2])); }
    float nx = -Gx, ny = -Gy, nz = -Gz;
    float dot = (nz * nz + ny * ny) + nx * nx;
    if (dot == 0.0f) {
        nx = -d->x; ny = -d->y; nz = -d->z;
    } else {
        float rn = 1.0f / sqrtf(dot);
        nx = nx * rn; ny = ny * rn; nz = nz * rn;
    }
    n[0] = nx; n[1] = ny; n[2] = nz;
}

/* one pixel: returns the sample count (the composite march's) and the composited rgba[4] */
static uint32_t shade_pixel(const shade_params *p, const consts *c, int px, int py, float rgba[4])
{
    v3 o, d;
    float t_min;
    float dest[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    uint32_t fetches = 0;
    rgba[0] = rgba[1] = rgba[2] = rgba[3] = 0.0f;
    compute_ray(p, (float)px + 0.5f, (float)py + 0.5f, &o, &d);
    if (!intersect(c, &o, &d, &t_min)) return 0;
    const float EPSILON = 0.000001f;
    float sx = o.x + d.x * t_min, sy = o.y + d.y * t_min, sz = o.z + d.z * t_min;
    float p0x = sx + d.x * EPSILON, p0y = sy + d.y * EPSILON, p0z = sz + d.z * EPSILON;
    float dsx = d.x * c->step, dsy = d.y * c->step, dsz = d.z * c->step;
    float qx = p0x, qy = p0y, qz = p0z;
    for (int i = 0; i < p->max_steps; i++) {
        if (p->accum == 1) {
            float fi = (float)i;
            qx = p0x + fi * dsx; qy = p0y + fi * dsy; qz = p0z + fi * dsz;
        }
        float tc[3];
        texcoord(p, c, qx, qy, qz, tc);
        if (tc[0] > 1.0f || tc[1] > 1.0f || tc[2] > 1.0f || tc[0] < 0.0f || tc[1] < 0.0f || tc[2] < 0.0f || dest[3] >= 0.95f) break;
        float s = sample_tc(p, c, tc);
        fetches++;
        /* 1. window and classification (the composite mode's) */
        s = gl_min(gl_max(s, c->fmin), c->fmax);
        if (c->fden == 0.0f) s = 0.0f;
        else if (s <= c->fmax && s >= c->fmin) s = (s - c->fmin) / c->fden;
        float src[4] = { s, s, s, s };
        if (p->tf_rgba && p->tf_len > 1) {
            float fi = floorf(s * (float)(p->tf_len - 1) + 0.5f);
            int idx = (int)clampi((int64_t)fi, 0, p->tf_len - 1);
            src[0] = p->tf_rgba[4 * idx]; src[1] = p->tf_rgba[4 * idx + 1]; src[2] = p->tf_rgba[4 * idx + 2]; src[3] = p->tf_rgba[4 * idx + 3];
        }
        float a = src[3] * p->alpha_scale;
        /* 2.-4. a visible sample is lit */
        if (a != 0.0f) {
            float n[3];
            normal_at(p, c, &d, tc, n);
            float dd = (n[2] * -d.z + n[1] * -d.y) + n[0] * -d.x;
            if (dd < 0.0f) dd = -dd;
            float spec = dd;
            for (int m = 1; m < p->shininess; m *= 2) spec = spec * spec;
            float lit = p->ambient + p->diffuse * dd, hl = p->specular * spec;
            for (int k = 0; k < 3; k++) src[k] = gl_min(src[k] * lit + hl, 1.0f);
        }
        /* 5. compositing (the composite mode's) */
        src[0] *= a; src[1] *= a; src[2] *= a;
        float om = 1.0f - dest[3];
        dest[0] += src[0] * om; dest[1] += src[1] * om; dest[2] += src[2] * om; dest[3] += a * om;
        if (dest[3] > 0.99f) break;
        if (p->accum == 0) { qx += dsx; qy += dsy; qz += dsz; }
    }
    rgba[0] = dest[0]; rgba[1] = dest[1]; rgba[2] = dest[2]; rgba[3] = dest[3];
    return fetches;
}

/* Renders rows [row_begin, row_end) (global rows; the Q1 grid limits when trunc_grid) into full-frame arrays: rgba h*w*4,
   spp h*w (NULL = not wanted).  Other pixels are left untouched.  Returns 0 on success. */
int shade_render(const shade_params *p, float *rgba, uint32_t *spp)
{
    if (!p || !rgba || !p->volume || p->img_w <= 0 || p->img_h <= 0 || p->nx <= 0 || p->ny <= 0 || p->nz <= 0 ||
        (p->bytes_per_voxel != 1 && p->bytes_per_voxel != 2) || p->shininess < 1 || p->shininess > 128 ||
        (p->shininess & (p->shininess - 1)) != 0)
        return 1;
    consts c;
    setup(p, &c);
    int r0 = p->row_begin < 0 ? 0 : p->row_begin, r1 = p->row_end > p->img_h ? p->img_h : p->row_end;
    int wlim = p->img_w;
    if (p->trunc_grid) {
        int hlim = (p->img_h / 16) * 16;
        if (r1 > hlim) r1 = hlim;
        wlim = (p->img_w / 16) * 16;
    }
    for (int py = r0; py < r1; py++)
        for (int px = 0; px < wlim; px++) {
            size_t pix = (size_t)py * (size_t)p->img_w + (size_t)px;
            uint32_t n = shade_pixel(p, &c, px, py, rgba + 4 * pix);
            if (spp) spp[pix] = n;
        }
    return 0;
}
