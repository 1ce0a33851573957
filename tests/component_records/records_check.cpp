// TEST INFRASTRUCTURE ONLY -- drives vr::ComponentRecords (volume-renderer_amd/csrc/component_records.cpp) and the mesh file
// writers (mesh_files.cpp) through one scenario and prints what happened as one JSON line; tests/test_component_records_cpu.py
// asserts on it.  Built by that test with g++ and the address / undefined-behaviour sanitizers; needs no GPU and no HIP header.
//   records_check select | list | read
//   records_check files <directory>      writes two.stl and two.ply there
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "component_records.h"
#include "mesh_files.h"

namespace {

// ---- a JSON object, built field by field
struct Json {
    std::string s = "{";
    void key(const char *k) { if (s.size() > 1) s += ", "; s += "\""; s += k; s += "\": "; }
    void num(const char *k, long long v) { key(k); s += std::to_string(v); }
    void text(const char *k, const std::string &v) { key(k); s += "\"" + v + "\""; }
    template <class T> void list(const char *k, const std::vector<T> &v)
    {
        key(k); s += "[";
        for (size_t i = 0; i < v.size(); i++) { if (i) s += ", "; s += std::to_string((long long)v[i]); }
        s += "]";
    }
    void print() { s += "}"; std::puts(s.c_str()); }
};

vr::ComponentRecords labelled(const std::vector<uint64_t> &voxels)
{
    vr::ComponentRecords r;
    std::vector<uint64_t> v = voxels, first(voxels.size());
    std::vector<int32_t> bbox(voxels.size() * 6);
    for (size_t c = 0; c < voxels.size(); c++) {
        first[c] = 100 + c;
        for (int a = 0; a < 6; a++) bbox[6 * c + a] = (int32_t)(10 * c + a);
    }
    r.adopt(7, 1007.0f, std::move(v), std::move(first), std::move(bbox));
    return r;
}

// the name of what `call` throws, "" when it returns
template <class F> std::string thrown(F &&call)
{
    try { call(); }
    catch (const vr::IoError &) { return "IoError"; }
    catch (const std::invalid_argument &e) { return std::string("invalid_argument: ") + e.what(); }
    catch (const std::exception &) { return "other"; }
    return "";
}

// one selection on a fresh labelling: "<name>" = the selected bytes, "<name>_ret" = the return value
void selectCase(Json &j, const std::string &name, const std::vector<uint64_t> &voxels, uint64_t min_voxels, uint64_t keep_largest)
{
    vr::ComponentRecords r = labelled(voxels);
    const uint64_t ret = r.select(min_voxels, keep_largest);
    j.list(name.c_str(), r.selected);
    j.num((name + "_ret").c_str(), (long long)ret);
}

void scenarioSelect()
{
    Json j;
    const std::vector<uint64_t> six = {5, 9, 1, 9, 3, 5}, equal = {7, 7, 7, 7}, none;
    selectCase(j, "six_0_0", six, 0, 0);
    selectCase(j, "six_4_0", six, 4, 0);
    selectCase(j, "six_0_1", six, 0, 1);
    selectCase(j, "six_0_3", six, 0, 3);
    selectCase(j, "six_6_3", six, 6, 3);
    selectCase(j, "six_0_99", six, 0, 99);
    selectCase(j, "six_0_6", six, 0, 6);                 // keep_largest == n
    selectCase(j, "six_4_6", six, 4, 6);
    selectCase(j, "six_0_5", six, 0, 5);                 // keep_largest == n - 1
    selectCase(j, "six_4_5", six, 4, 5);
    selectCase(j, "equal_0_2", equal, 0, 2);
    selectCase(j, "equal_7_3", equal, 7, 3);
    selectCase(j, "six_10_0", six, 10, 0);               // min_voxels above every size
    selectCase(j, "six_10_3", six, 10, 3);
    selectCase(j, "none_0_0", none, 0, 0);               // a labelling without a component
    selectCase(j, "none_1_3", none, 1, 3);
    vr::ComponentRecords fresh = labelled(six);
    j.list("fresh", fresh.selected);                     // a new labelling selects everything
    j.num("fresh_inside", (long long)fresh.inside);
    vr::ComponentRecords unlabelled;
    j.text("unlabelled", thrown([&] { unlabelled.select(0, 0); }));
    j.print();
}

void scenarioList()
{
    Json j;
    vr::ComponentRecords r = labelled({5, 9, 1, 9, 3, 5});
    j.num("empty_ret", (long long)r.selectList(nullptr, 0));
    j.list("empty", r.selected);
    const uint32_t repeated[4] = {2, 5, 2, 2};
    j.num("repeated_ret", (long long)r.selectList(repeated, 4));
    j.list("repeated", r.selected);
    const uint32_t zero[2] = {1, 0}, above[2] = {1, 7}, last[1] = {6};
    j.text("zero", thrown([&] { r.selectList(zero, 2); }));
    j.list("after_zero", r.selected);
    j.text("above", thrown([&] { r.selectList(above, 2); }));
    j.list("after_above", r.selected);
    j.text("null_list", thrown([&] { r.selectList(nullptr, 1); }));
    j.list("after_null_list", r.selected);
    j.num("last_ret", (long long)r.selectList(last, 1));
    j.list("last", r.selected);
    vr::ComponentRecords unlabelled;
    j.text("unlabelled", thrown([&] { unlabelled.selectList(nullptr, 0); }));
    j.print();
}

void scenarioRead()
{
    Json j;
    vr::ComponentRecords r = labelled({5, 9, 1, 9, 3, 5});
    std::vector<uint64_t> voxels(6, 0), first(6, 0);
    std::vector<int32_t> bbox(36, -1);
    std::vector<uint8_t> selected(6, 9);
    j.text("small_voxels", thrown([&] { r.read(voxels.data(), nullptr, nullptr, nullptr, 5); }));
    j.text("small_selected", thrown([&] { r.read(nullptr, nullptr, nullptr, selected.data(), 5); }));
    j.list("untouched", voxels);
    j.text("all_null", thrown([&] { r.read(nullptr, nullptr, nullptr, nullptr, 0); }));
    j.text("exact", thrown([&] { r.read(voxels.data(), first.data(), bbox.data(), selected.data(), 6); }));
    j.list("voxels", voxels); j.list("first", first); j.list("bbox", bbox); j.list("selected", selected);
    int32_t iso = 0;
    uint64_t n = 0, inside = 0, n_selected = 0;
    r.select(4, 0);
    r.info(&iso, &n, &inside, &n_selected);
    j.num("iso", iso); j.num("n", (long long)n); j.num("inside", (long long)inside); j.num("n_selected", (long long)n_selected);
    r.info(nullptr, nullptr, nullptr, nullptr);
    r.clear();
    j.text("cleared_info", thrown([&] { r.info(&iso, nullptr, nullptr, nullptr); }));
    j.text("cleared_read", thrown([&] { r.read(nullptr, nullptr, nullptr, nullptr, 0); }));
    j.print();
}

// two triangles on five vertices: (0, 1, 2) has the normal (1, 1, 1) / sqrt 3, (0, 3, 4) has its corners on one line
void scenarioFiles(const std::string &dir)
{
    Json j;
    const float pos[15] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 2.5f, 0, 0, 4, 0, 0};
    const float nrm[15] = {0.25f, 0.5f, -1, 0, 1, 0, 0, 0, 1, 1, 0, 0, -0.125f, 3, 7};
    const uint32_t tri[6] = {0, 1, 2, 0, 3, 4};
    j.text("stl", thrown([&] { vr::write_stl(dir + "/two.stl", pos, tri, 2); }));
    j.text("ply", thrown([&] { vr::write_ply(dir + "/two.ply", -42, pos, nrm, 5, tri, 2); }));
    j.text("empty_stl", thrown([&] { vr::write_stl(dir + "/empty.stl", nullptr, nullptr, 0); }));
    j.text("missing_stl", thrown([&] { vr::write_stl(dir + "/no/such/two.stl", pos, tri, 2); }));
    j.text("missing_ply", thrown([&] { vr::write_ply(dir + "/no/such/two.ply", -42, pos, nrm, 5, tri, 2); }));
    j.print();
}

}  // namespace

int main(int argc, char **argv)
{
    const std::string scenario = argc > 1 ? argv[1] : "";
    if (scenario == "select") scenarioSelect();
    else if (scenario == "list") scenarioList();
    else if (scenario == "read") scenarioRead();
    else if (scenario == "files" && argc > 2) scenarioFiles(argv[2]);
    else { std::fprintf(stderr, "records_check: unknown scenario\n"); return 2; }
    return 0;
}
