// stage_layout.hpp — byte layout of the private device block of a host-pointer entry point (pm::StagedBlock,
// pm_common.hpp): parts in the order they are added, each at a multiple of 256 bytes.  A part of zero bytes still owns an
// address inside the block (the _dev forms are handed a non-null pointer for an empty train set), so the total of a
// layout with a part is never 0.  No HIP here: tests/stage_layout_shim.cpp builds it with the host compiler.
#pragma once
#include <cstddef>

namespace pm {

struct __attribute__((visibility("hidden"))) StageLayout {
    size_t total = 0;
    size_t add(size_t bytes)                 // the part's byte offset
    {
        const size_t off = total;
        total += bytes ? (bytes + 255) / 256 * 256 : 256;
        return off;
    }
};

}  // namespace pm
