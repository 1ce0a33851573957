// component_records.h -- the host side of a labelling (vr_label_components): the components' records
// as they came from the device, and the selection, which is made here.  No HIP: tests/component_records checks it with g++.
#pragma once
#include <stdint.h>

#include <vector>

namespace vr {

struct ComponentRecords {
    bool valid = false;                      // a labelling has succeeded (it may have no component) and was not dropped
    int32_t iso = 0;
    float iso_s = 0.0f;                      // the iso value in stored units when the labelling was made
    std::vector<uint64_t> voxels, first;     // the records, entry label - 1
    std::vector<int32_t> bbox;               // 6 each
    std::vector<uint8_t> selected;
    uint64_t inside = 0;                     // the sum of voxels

    // a new labelling: every component selected
    void adopt(int32_t iso_value, float iso_stored, std::vector<uint64_t> &&voxels_, std::vector<uint64_t> &&first_, std::vector<int32_t> &&bbox_);
    void clear();
    // each: std::invalid_argument without a labelling
    void info(int32_t *iso_value, uint64_t *n_components, uint64_t *n_inside, uint64_t *n_selected) const;
    void read(uint64_t *voxels_out, uint64_t *first_voxel, int32_t *bbox6, uint8_t *selected_out, uint64_t capacity) const;
    // selected: voxels >= min_voxels and, when 0 < keep_largest < n, among the keep_largest first by (voxels descending, label ascending)
    uint64_t select(uint64_t min_voxels, uint64_t keep_largest);
    uint64_t selectList(const uint32_t *labels, uint64_t n);   // exactly these; a label of 0 or above n_components: std::invalid_argument, nothing changes
};

}  // namespace vr
