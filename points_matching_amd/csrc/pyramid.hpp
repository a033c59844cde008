// pyramid.hpp — the device image pyramid of docs/SPEC.md S61, shared by the tracker (track_lk.hip, which builds it), the
// corner detector (corners.hip, which reads level 0) and the point descriptors (describe_points.hip, which read one level).
#pragma once
#include <cstddef>
#include <cstdint>

struct pm_pyramid {
    int device = 0;
    int w = 0, h = 0, nlev = 0;
    int lw[8] = {}, lh[8] = {};
    size_t off[8] = {};                // first byte of each level's tight plane
    size_t bytes = 0;
    uint8_t* mem = nullptr;
};
