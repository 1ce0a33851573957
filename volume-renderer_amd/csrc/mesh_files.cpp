// mesh_files.cpp -- see mesh_files.h
#include "mesh_files.h"

#include <cmath>
#include <cstdio>

namespace vr {

namespace {
// the file of one save: opened here, every write checked once at the end
struct OutFile {
    const std::string &fn;
    FILE *f;
    bool ok = true;
    explicit OutFile(const std::string &name) : fn(name), f(std::fopen(name.c_str(), "wb")) { if (!f) throw IoError("saveMesh: cannot open " + fn); }
    void put(const void *p, size_t n) { ok = ok && (n == 0 || std::fwrite(p, 1, n, f) == n); }
    ~OutFile() { if (f) (void)std::fclose(f); }
    void close()
    {
        if (std::fclose(f) != 0) ok = false;
        f = nullptr;
        if (!ok) throw IoError("saveMesh: writing " + fn + " failed");
    }
};
}  // namespace

void write_stl(const std::string &fn, const float *pos, const uint32_t *tri, uint64_t nt)
{
    OutFile out(fn);
    char header[80] = "binary STL written by vr_save_mesh";
    const uint32_t count = (uint32_t)nt;
    out.put(header, sizeof(header));
    out.put(&count, 4);
    for (uint64_t t = 0; t < nt && out.ok; t++) {
        const float *p0 = &pos[3 * (size_t)tri[3 * t]], *p1 = &pos[3 * (size_t)tri[3 * t + 1]], *p2 = &pos[3 * (size_t)tri[3 * t + 2]];
        const double u[3] = {(double)p1[0] - p0[0], (double)p1[1] - p0[1], (double)p1[2] - p0[2]};
        const double v[3] = {(double)p2[0] - p0[0], (double)p2[1] - p0[1], (double)p2[2] - p0[2]};
        const double c[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
        const double len = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        float rec[12] = {};
        if (len > 0.0) for (int a = 0; a < 3; a++) rec[a] = (float)(c[a] / len);
        for (int a = 0; a < 3; a++) { rec[3 + a] = p0[a]; rec[6 + a] = p1[a]; rec[9 + a] = p2[a]; }
        const uint16_t attribute = 0;
        out.put(rec, sizeof(rec));
        out.put(&attribute, 2);
    }
    out.close();
}

void write_ply(const std::string &fn, int32_t iso, const float *pos, const float *nrm, uint64_t nv, const uint32_t *tri, uint64_t nt)
{
    OutFile out(fn);
    const std::string header = "ply\nformat binary_little_endian 1.0\ncomment isosurface at " + std::to_string(iso) +
                               ", written by vr_save_mesh\nelement vertex " + std::to_string(nv) +
                               "\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
                               "element face " + std::to_string(nt) + "\nproperty list uchar uint vertex_indices\nend_header\n";
    out.put(header.data(), header.size());
    for (uint64_t v = 0; v < nv && out.ok; v++) {
        out.put(&pos[3 * (size_t)v], 12);
        out.put(&nrm[3 * (size_t)v], 12);
    }
    const uint8_t three = 3;
    for (uint64_t t = 0; t < nt && out.ok; t++) {
        out.put(&three, 1);
        out.put(&tri[3 * (size_t)t], 12);
    }
    out.close();
}

}  // namespace vr
