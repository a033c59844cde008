// stereo_rectify_core.hpp — SPEC S84: the two rectifying rotations of a calibrated pair from its relative pose.  Plain fp64,
// square roots and divisions, every product and sum its own operation in the order S84 writes them (the build keeps
// -ffp-contract=off), so a numpy restatement gives the same bits.  No HIP here: stereo.hip wraps it as pm_stereo_rectify and
// tests/stereo_rectify_shim.cpp builds it with the host compiler.
#pragma once
#include <cmath>

#include "pm.h"

namespace pm_stereo {

// R, t: x2 ~ R x1 + t (S35).  R1, R2: camera frame -> rectified frame, the R argument of pm_undistort* for view 1 and view 2.
// Returns PM_OK, PM_E_NO_MODEL or PM_E_UNSUPPORTED; the outputs are zero unless PM_OK.  The caller has checked the pointers
// and that the twelve inputs are finite.
inline int rectify(const double R[9], const double t[3], double R1[9], double R2[9], double* baseline, int* left_is_view2)
{
    for (int i = 0; i < 9; ++i) R1[i] = R2[i] = 0.0;
    *baseline = 0.0;
    *left_is_view2 = 0;
    double c[3];                                                     // the centre of camera 2 in camera-1 coordinates
    for (int i = 0; i < 3; ++i) c[i] = -((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]);
    const double cc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
    if (!(cc > 0.0) || !std::isfinite(cc)) return PM_E_NO_MODEL;
    if (std::fabs(c[1]) > std::fabs(c[0])) return PM_E_UNSUPPORTED;  // a vertical rig
    const double b = std::sqrt(cc);
    const double s = c[0] >= 0.0 ? 1.0 : -1.0;
    const double e1[3] = {(s * c[0]) / b, (s * c[1]) / b, (s * c[2]) / b};
    const double z[3] = {R[6], R[7], 1.0 + R[8]};                    // the sum of the two optical axes
    const double zz = (z[0] * z[0] + z[1] * z[1]) + z[2] * z[2];
    const double m[3] = {z[1] * e1[2] - z[2] * e1[1], z[2] * e1[0] - z[0] * e1[2], z[0] * e1[1] - z[1] * e1[0]};
    const double mm = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
    if (!(mm > 1e-24 * zz)) return PM_E_NO_MODEL;                    // an optical axis along the baseline, or z = 0
    const double n = std::sqrt(mm);
    const double e2[3] = {m[0] / n, m[1] / n, m[2] / n};
    const double e3[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    for (int j = 0; j < 3; ++j) {
        R1[j] = e1[j];
        R1[3 + j] = e2[j];
        R1[6 + j] = e3[j];
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R2[3 * i + j] = (R1[3 * i] * R[3 * j] + R1[3 * i + 1] * R[3 * j + 1]) + R1[3 * i + 2] * R[3 * j + 2];
    *baseline = b;
    *left_is_view2 = s < 0.0 ? 1 : 0;
    return PM_OK;
}

inline bool finite12(const double R[9], const double t[3])
{
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(R[i])) return false;
    return std::isfinite(t[0]) && std::isfinite(t[1]) && std::isfinite(t[2]);
}

}  // namespace pm_stereo
