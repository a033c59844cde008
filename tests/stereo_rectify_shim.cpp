// C face of the rectification header (csrc/stereo_rectify_core.hpp, SPEC S84) for tests/test_stereo_cpu.py: the statuses of
// pm_stereo_rectify without the library.
#include "stereo_rectify_core.hpp"

extern "C" int stereo_rectify_shim(const double* R, const double* t, double* R1, double* R2, double* baseline, int* left_is_view2)
{
    if (!R || !t || !R1 || !R2 || !baseline || !left_is_view2) return PM_E_INVALID;
    if (!pm_stereo::finite12(R, t)) return PM_E_INVALID;
    return pm_stereo::rectify(R, t, R1, R2, baseline, left_is_view2);
}
