// component_records.cpp -- see component_records.h
#include "component_records.h"

#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <string>

namespace vr {

void ComponentRecords::adopt(int32_t iso_value, float iso_stored, std::vector<uint64_t> &&voxels_, std::vector<uint64_t> &&first_, std::vector<int32_t> &&bbox_)
{
    voxels = std::move(voxels_); first = std::move(first_); bbox = std::move(bbox_);
    selected.assign(voxels.size(), 1);
    inside = std::accumulate(voxels.begin(), voxels.end(), (uint64_t)0);
    iso = iso_value; iso_s = iso_stored; valid = true;
}

void ComponentRecords::clear()
{
    voxels.clear(); first.clear(); bbox.clear(); selected.clear();
    inside = 0;
    valid = false;
}

void ComponentRecords::info(int32_t *iso_value, uint64_t *n_components, uint64_t *n_inside, uint64_t *n_selected) const
{
    if (!valid) throw std::invalid_argument("componentsInfo: no components have been labelled");
    if (iso_value) *iso_value = iso;
    if (n_components) *n_components = voxels.size();
    if (n_inside) *n_inside = inside;
    if (n_selected) *n_selected = (uint64_t)std::count(selected.begin(), selected.end(), (uint8_t)1);
}

void ComponentRecords::read(uint64_t *voxels_out, uint64_t *first_voxel, int32_t *bbox6, uint8_t *selected_out, uint64_t capacity) const
{
    if (!valid) throw std::invalid_argument("readComponents: no components have been labelled");
    const size_t n = voxels.size();
    if ((voxels_out || first_voxel || bbox6 || selected_out) && capacity < n) throw std::invalid_argument("readComponents: buffer too small");
    if (voxels_out) std::copy(voxels.begin(), voxels.end(), voxels_out);
    if (first_voxel) std::copy(first.begin(), first.end(), first_voxel);
    if (bbox6) std::copy(bbox.begin(), bbox.end(), bbox6);
    if (selected_out) std::copy(selected.begin(), selected.end(), selected_out);
}

uint64_t ComponentRecords::select(uint64_t min_voxels, uint64_t keep_largest)
{
    if (!valid) throw std::invalid_argument("selectComponents: no components have been labelled");
    const size_t n = voxels.size();
    std::vector<uint8_t> sel(n, 0);
    if (keep_largest == 0 || keep_largest >= n) {
        for (size_t c = 0; c < n; c++) sel[c] = voxels[c] >= min_voxels;
    } else {
        std::vector<uint32_t> order(n);
        std::iota(order.begin(), order.end(), 0u);
        auto before = [&](uint32_t a, uint32_t b) { return voxels[a] != voxels[b] ? voxels[a] > voxels[b] : a < b; };
        std::partial_sort(order.begin(), order.begin() + (size_t)keep_largest, order.end(), before);
        for (size_t q = 0; q < (size_t)keep_largest; q++) sel[order[q]] = voxels[order[q]] >= min_voxels;
    }
    selected = std::move(sel);
    return (uint64_t)std::count(selected.begin(), selected.end(), (uint8_t)1);
}

uint64_t ComponentRecords::selectList(const uint32_t *labels, uint64_t n)
{
    if (!valid) throw std::invalid_argument("selectComponentList: no components have been labelled");
    if (!labels && n > 0) throw std::invalid_argument("selectComponentList: null list");
    for (uint64_t q = 0; q < n; q++)
        if (labels[q] == 0 || labels[q] > voxels.size()) throw std::invalid_argument("selectComponentList: label " + std::to_string(labels[q]) + " does not exist");
    std::vector<uint8_t> sel(voxels.size(), 0);
    for (uint64_t q = 0; q < n; q++) sel[labels[q] - 1u] = 1;
    selected = std::move(sel);
    return (uint64_t)std::count(selected.begin(), selected.end(), (uint8_t)1);
}

}  // namespace vr
