// C face of the staging layout (csrc/stage_layout.hpp) for tests/test_stage_layout_cpu.py: n part sizes in, n offsets out.
#include <cstdint>

#include "stage_layout.hpp"

// returns the layout's total
extern "C" uint64_t stage_layout(const uint64_t* bytes, int n, uint64_t* offsets)
{
    pm::StageLayout l;
    for (int i = 0; i < n; ++i) offsets[i] = l.add(static_cast<size_t>(bytes[i]));
    return l.total;
}
