// features_host_main.cpp — the host extractor (host/pm_features.cpp, the specification of SPEC S53-S60) as a program of its
// own that takes every argument of pm_feat::detect_and_describe: pm_cli fixes contrast and edge_r at their defaults, this
// driver does not.  Compiled from this file and host/pm_features.cpp alone (no libpm_hip.so) by tests/features_ref.py.
//
//   features_host_main IMAGE.pgm MAX_KP CONTRAST EDGE_R grad|bits OUT.bin
//
// OUT.bin: int32 n, int32 kind (0 grad, 1 bits), n x 2 float32 keypoints, then n x 128 float32 rows (grad) or n x 32 bytes
// (bits), little endian as the machine writes them.  Exit status 0, 2 on a usage error, 1 on an unreadable image or file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "pm_features.hpp"

namespace {
bool put(FILE* f, const void* p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }
}  // namespace

int main(int argc, char** argv)
{
    if (argc != 7) {
        fprintf(stderr, "usage: %s IMAGE.pgm MAX_KP CONTRAST EDGE_R grad|bits OUT.bin\n", argv[0]);
        return 2;
    }
    char* end = nullptr;
    const long max_kp = strtol(argv[2], &end, 10);
    const bool kp_ok = *argv[2] && !*end && max_kp >= 1 && max_kp <= 100000000L;
    const float contrast = strtof(argv[3], &end);
    const bool c_ok = *argv[3] && !*end;
    const float edge_r = strtof(argv[4], &end);
    const bool e_ok = *argv[4] && !*end;
    const bool grad = !strcmp(argv[5], "grad"), bits = !strcmp(argv[5], "bits");
    if (!kp_ok || !c_ok || !e_ok || !(grad || bits)) {
        fprintf(stderr, "%s: bad argument\n", argv[0]);
        return 2;
    }
    pm_feat::Image img;
    std::string err;
    if (!pm_feat::load_pnm_gray(argv[1], img, err)) {
        fprintf(stderr, "%s: %s\n", argv[0], err.c_str());
        return 1;
    }
    const pm_feat::Features ft =
        pm_feat::detect_and_describe(img, static_cast<int>(max_kp), contrast, edge_r, bits ? pm_feat::DESC_BITS : pm_feat::DESC_GRAD);
    const size_t n = static_cast<size_t>(ft.n);
    if (ft.kp_xy.size() != 2 * n || (bits ? ft.bits.size() != 32 * n : ft.desc.size() != 128 * n)) {
        fprintf(stderr, "%s: the extractor's rows do not match its count\n", argv[0]);
        return 1;
    }
    FILE* f = fopen(argv[6], "wb");
    if (!f) {
        fprintf(stderr, "%s: cannot write %s\n", argv[0], argv[6]);
        return 1;
    }
    const int head[2] = {ft.n, bits ? 1 : 0};
    bool ok = put(f, head, sizeof head) && put(f, ft.kp_xy.data(), ft.kp_xy.size() * sizeof(float));
    ok = ok && (bits ? put(f, ft.bits.data(), ft.bits.size()) : put(f, ft.desc.data(), ft.desc.size() * sizeof(float)));
    ok = (fclose(f) == 0) && ok;
    if (!ok) {
        fprintf(stderr, "%s: short write to %s\n", argv[0], argv[6]);
        return 1;
    }
    return 0;
}
