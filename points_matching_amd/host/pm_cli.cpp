// pm_cli — C++ host of the MI355X-native matcher: the counterpart of the reference's main()
// (`Points Matching/main.cpp:9-147`) for the hot path main.cpp:42-123.  It keeps the reference's
// stdout surface (main.cpp:58-59, :73, :76, :119, :123) and calls the HIP kernels only through
// the C ABI of include/pm.h.  Images come as binary PGM/PPM (no JPEG/BMP decoder in this image: `convert a.jpg a.pgm`
// or PIL does it) and go through the build-owned detector/descriptor of pm_features.cpp (the
// reference's SURF, main.cpp:22-40, is OpenCV nonfree code); descriptors and keypoints can also come from matrix files.
//
//   pm_cli --img1 left.pgm --img2 right.pgm [--max-kp 4000]        (image pair in: main.cpp:14-15, :22-40)
//   pm_cli --desc1 a.pmm --desc2 b.pmm --kp1 ka.pmm --kp2 kb.pmm   (descriptor pair in)
//          [--filter midpoint|ratio|cross|cross-ratio] [--ratio 0.8] [--iters 10000] [--thresh 1.0] [--seed 24301]
//          [--method 7point-lmeds|ransac8] [--f-scale opencv|unit] [--device 0] [--gpus N] [--quiet] [--json]
//          [--print-epilines] [--epilines out.ppm [--canvas W H] [--img2 right.pgm]] [--matcher bf|flann]
//          [--guided TAU] [--features host|device|corners] [--descriptor grad|bits]
//          [--matcher track [--lk-radius R] [--lk-levels L] [--lk-fb T]
//                           [--points dog|corners [--corner-dist D] [--corner-quality Q] [--corner-min-eig M]]]
//          [--align OUT.pgm [--align-model homography|affine|similarity]]
//   pm_cli --undistort OUT.pgm --img1 IN.pgm --camera fx,fy,cx,cy --lens k1,k2,p1,p2,k3 [--new-camera fx,fy,cx,cy] [--json]
//   pm_cli --stereo OUT.pgm --img1 L.pgm --img2 R.pgm --num-disp N [--min-disp M] [--radius R] [--uniqueness U] [--lr-check T16] [--json]
//   pm_cli --stereo OUT.pgm --img1 L.pgm --img2 R.pgm --num-disp N --sgm P1,P2 [--paths 4|8] [--min-disp M] [--uniqueness U] [--lr-check T16] [--json]
//          [--knn-hint auto|int|u8|unit]   what the caller knows about float descriptors (pm.h PM_KNN_HINT_*; default auto, and
//                                     u8 for --img1/--img2, whose extractor writes u8-valued rows): route only, same output
// --features device (with --img1/--img2): both images are uploaded and keypoints + descriptors are extracted on the GPU
// (pm_detect_describe_dev, docs/SPEC.md S53-S57); keypoints and float rows are downloaded once for the match list and
// --save-features.  The plain brute-force matcher (--filter midpoint|ratio, one GPU) then reads the u8 descriptor rows where
// the extractor left them, through DEVICE pointers (pm_bf_knn_l2_u8_dev).  Every other matcher path (--filter cross|cross-ratio,
// --matcher flann, --gpus N / --mgpu, the second pass of --guided) takes host rows by its interface and is given the
// downloaded float rows: same values, one upload more.  host (default): the C++ extractor of pm_features.cpp.  Same
// keypoints either way; descriptors may differ by one in rare elements (pm.h).
// --features corners (with --img1/--img2): on both images a pyramid, the minimum-eigenvalue corners of its level 0
// (pm_corners_dev: --max-kp corners, block radius 10, --corner-dist / --corner-quality / --corner-min-eig as for --points
// corners) and their oriented 256-bit descriptors (pm_describe_points_gather_dev at level 0, docs/SPEC.md S71-S74); from there
// the path of --features device --descriptor bits.  --descriptor grad, --matcher track|flann and --points are usage errors.
// --align OUT.pgm (with --img1/--img2 of one size, any matcher or track route, one GPU): after the correspondences the chosen
// 2-D model (--align-model homography (default) | affine | similarity: pm_ransac_homography_run_dev + pm_homography_refine_dev,
// or pm_ransac_affine_run_dev + pm_affine_refine_dev with PM_AFFINE_FULL | PM_AFFINE_PARTIAL; --iters, --thresh, --seed as
// given) takes the place of the F estimator, and pm_warp_dev (docs/SPEC.md S75-S77) pulls image 2 into the frame of image 1
// by that model as it lies on the device, with a valid mask: upload, estimate, refine and warp are enqueued on one stream and
// synchronised once.  OUT.pgm is the warped image (P5, border 0); one line is printed after the match list:
//   align: model=M inliers=N valid=V mad_before=B mad_after=A
// B and A being the mean absolute grey differences to image 1 over the V valid pixels, of image 2 as it is and warped.  No F
// is estimated, so the residual report is not printed; --json, --guided, --epilines, --print-epilines and --gpus N / --mgpu
// are usage errors with it.
// --stereo OUT.pgm (with --img1, --img2, an already rectified pair of one size, and --num-disp; docs/SPEC.md S85-S88): the
// disparity map of the left image by pm_stereo_bm (radius default 4, uniqueness 0; --lr-check T16 >= 0 adds the right map and the
// left-right check).  OUT.pgm is a 16-bit binary PGM (maxval 65535, most significant byte first) holding v - 16 * min_disp + 1
// and 0 where there is no disparity; one line
//   stereo: valid=V
// is printed (with --json the record {"stereo": {"width": W, "height": H, "n_valid": V}}) and the tool exits.
// --sgm P1,P2 with it: the map by pm_stereo_sgm instead (semi-global matching, docs/SPEC.md S89-S92; --paths 4 or 8, default 8),
// same file and same line.  --radius with --sgm, --paths without --sgm, --sgm without --stereo and a malformed P1,P2 are usage
// errors.
// Any switch of another mode with it (--undistort, --align, --guided, --epilines, --matcher, --features, --filter, ...) is a
// usage error.
// --undistort OUT.pgm (with --img1 alone, --camera and --lens; docs/SPEC.md S79-S83): the image as an ideal pinhole camera
// (--new-camera, default --camera) would have taken it, by pm_undistort_dev with border 0; OUT.pgm is written, one line
//   undistort: valid=V
// is printed (with --json the record {"undistort": {"width": W, "height": H, "n_valid": V}} instead) and the tool exits, as
// with --extract-only.  A --camera / --new-camera that is not four numbers or a --lens that is not five is a usage error.
// --descriptor bits (with --img1/--img2; default grad): 256-bit steered binary descriptors (docs/SPEC.md S58-S60) in place of
// the 128-D gradient rows: the descriptor matrices are uint8 with 32 columns, every path below matches them by Hamming
// distance, and with --features device (pm_detect_describe_bits_dev) the plain matcher reads them through
// pm_bf_knn_hamming_u8_dev where the extractor left them.  --dump-bits-pattern prints the host extractor's 256 tests
// (x1 y1 x2 y2 per line) and exits: the test surface that pins the host's copy of the S58 construction.
// --matcher flann: the reference's ACTIVE matcher object (`FlannBasedMatcher matcher;`, main.cpp:44): 4 randomised
// kd-trees, 32 checks (pm_flann_*; approximate, seeded by --seed); bf (default) is the exact matcher of main.cpp:43.
// NOTE: the default matcher DEVIATES from main.cpp:44 on purpose — the exact matcher is faster on this hardware at every
// size and reproducible (FLANN seeds its trees from C rand()); `--matcher flann` gives the reference's literal flow
// (FLANN 1-NN -> midpoint filter -> 7-point LMedS).  The image front end (--img1/--img2) is a SIFT-style detector, not
// the reference's SURF(8000) (main.cpp:22-40): no compatibility with OpenCV's keypoints is claimed.
// --matcher track (with --img1/--img2 --features device): frame-to-frame correspondences by pyramidal Lucas-Kanade tracking
// (docs/SPEC.md S61-S66) in place of descriptor matching: keypoints are detected on image 1 only and tracked into image 2 on
// the device (pm_pyramid_build_dev x 2, pm_track_lk_gather_dev); the gathered pairs feed the chosen estimator (--method) and
// the rest of the output is as before (a match record holds the keypoint's row as queryIdx, its row among the survivors as
// trainIdx and distance 0).  --lk-radius (default 10), --lk-levels (3), --lk-fb (forward-backward threshold in pixels,
// default 0 = off).  Host features, --descriptor bits, --filter, --guided, --gpus / --mgpu are usage errors with it.
// --points corners (with --matcher track; default dog = the detector above): image 1's points are minimum-eigenvalue corners
// (docs/SPEC.md S67-S70, pm_corners_dev on the first pyramid, block radius = --lk-radius, at most --max-kp of them) in place
// of the DoG keypoints: no scale space and no descriptors are computed (pm_detect_describe_dev is not called).
// --corner-dist (minimum distance in pixels, default 8), --corner-quality (relative floor, default 0.01), --corner-min-eig
// (absolute floor, default 1e-4, the tracker's).  The report keeps its fields: n1 = corners found, n2 = 0.
// --filter cross: mutual nearest neighbours (cv::BFMatcher crossCheck = true, docs/SPEC.md S41-S42): forward and reverse
// matcher pass + the fused filter in one call; cross-ratio adds the ratio test (--ratio) on the forward row.  Brute-force
// matcher on one GPU only (float and binary descriptors): with --matcher flann or --gpus / --mgpu it is a usage error.
// --guided TAU: guided matching (docs/SPEC.md S48-S50) after F is estimated: every query is matched again among the train
// keypoints within TAU pixels (Sampson) of its epipolar line under that F (guided 2-NN + the ratio test of --ratio, what
// pm_bf_match_guided_*_dev computes on device buffers), and RANSAC-F (8-point, --iters, --thresh, --seed) runs again on
// the survivors.  One more stdout line reports both match counts and both inlier counts; everything else is printed as
// without the option, for the first pass.  Single GPU only.
// --gpus N (> 1): matcher rows and hypothesis ids are sharded over N GPUs through pm_mgpu_match_ransac (RCCL behind
// the C ABI); needs --filter ratio --method ransac8 (the sharded form of the path, BASELINE config C4).
// --print-epilines / --epilines: main.cpp:127-142 — the epipolar lines of the image-1 points in image 2
// (computeCorrespondEpilines) and the two end points main.cpp:138-140 hands to cv::line; --epilines draws them in
// white over --img2 (binary PGM, as main.cpp:137 draws over img2) or over a black canvas and writes a PPM.
// --method 7point-lmeds (default) is the estimator the reference's CV_FM_7POINT call literally selects (7-point
// solver inside the LMedS loop, OpenCV's 300 iterations unless --iters is given); ransac8 is the estimator
// BASELINE.json names (normalised 8-point + Sampson, --iters defaults to 10000).
//
// .pmm file: magic "PMM1", int32 rows, int32 cols, int32 dtype (0 = float32, 1 = uint8), data
// row-major.  float32 descriptors -> BF-L2 (main.cpp:43), uint8 -> BF-Hamming.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "pm.h"
#include "pm_features.hpp"

namespace {

struct Matrix {
    int rows = 0, cols = 0, dtype = 0;
    std::vector<unsigned char> data;
    const float* f32() const { return reinterpret_cast<const float*>(data.data()); }
};

bool load_matrix(const std::string& path, Matrix& m)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "pm_cli: cannot open %s\n", path.c_str()); return false; }
    char magic[4];
    int32_t hdr[3];
    bool ok = fread(magic, 1, 4, f) == 4 && memcmp(magic, "PMM1", 4) == 0 && fread(hdr, 4, 3, f) == 3;
    if (ok) {
        m.rows = hdr[0]; m.cols = hdr[1]; m.dtype = hdr[2];
        ok = m.rows >= 0 && m.cols > 0 && (m.dtype == 0 || m.dtype == 1);
    }
    if (ok) {
        const size_t bytes = static_cast<size_t>(m.rows) * m.cols * (m.dtype == 0 ? 4 : 1);
        m.data.resize(bytes);
        ok = fread(m.data.data(), 1, bytes, f) == bytes;
    }
    fclose(f);
    if (!ok) fprintf(stderr, "pm_cli: %s is not a valid .pmm matrix\n", path.c_str());
    return ok;
}

// binary PGM (P5, maxval <= 255): what img2 of main.cpp:21 would be after a grey conversion
bool load_pgm(const std::string& path, std::vector<unsigned char>& px, int& w, int& h)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "pm_cli: cannot open %s\n", path.c_str()); return false; }
    auto token = [&](int& out) -> bool {
        int c = fgetc(f);
        for (;;) {
            while (c == ' ' || c == '\n' || c == '\r' || c == '\t') c = fgetc(f);
            if (c == '#') { while (c != '\n' && c != EOF) c = fgetc(f); continue; }
            break;
        }
        if (c < '0' || c > '9') return false;
        long v = 0;
        while (c >= '0' && c <= '9') { v = v * 10 + (c - '0'); if (v > 1000000) return false; c = fgetc(f); }
        out = static_cast<int>(v);
        return true;                                 // the single whitespace after the token has been consumed
    };
    char magic[2] = {0, 0};
    int maxv = 0;
    bool ok = fread(magic, 1, 2, f) == 2 && magic[0] == 'P' && magic[1] == '5' && token(w) && token(h) && token(maxv) &&
              w > 0 && h > 0 && maxv > 0 && maxv <= 255;
    if (ok) {
        px.resize(static_cast<size_t>(w) * h);
        ok = fread(px.data(), 1, px.size(), f) == px.size();
    }
    fclose(f);
    if (!ok) fprintf(stderr, "pm_cli: %s is not a binary 8-bit PGM\n", path.c_str());
    return ok;
}

// cv::line(img2, p1, p2, Scalar(255,255,255)) for every epipolar line (main.cpp:134-141): 8-connected Bresenham
// walk from p1 to p2, pixels outside the image skipped.  Written as a binary PPM (P6).
bool write_epiline_ppm(const std::string& path, const std::vector<unsigned char>& gray, int w, int h,
                       const std::vector<int32_t>& ends, int n)
{
    std::vector<unsigned char> rgb(static_cast<size_t>(w) * h * 3, 0);
    if (!gray.empty())
        for (size_t i = 0; i < static_cast<size_t>(w) * h; ++i) rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = gray[i];
    for (int i = 0; i < n; ++i) {
        long long x0 = ends[4 * i], y0 = ends[4 * i + 1], x1 = ends[4 * i + 2], y1 = ends[4 * i + 3];
        if (y0 == INT32_MIN || y1 == INT32_MIN) continue;              // vertical line (b == 0): no finite end points
        // clip the y range coarsely first: a nearly vertical line may have end points billions of pixels away
        const long long dx = x1 - x0, dy = y1 - y0;
        const long long adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
        const long long steps = adx > ady ? adx : ady;
        if (steps == 0) { if (x0 >= 0 && x0 < w && y0 >= 0 && y0 < h) { size_t o = 3 * (static_cast<size_t>(y0) * w + x0); rgb[o] = rgb[o + 1] = rgb[o + 2] = 255; } continue; }
        if (ady <= adx) {                                               // x-major: one pixel per column
            for (long long x = (x0 < 0 ? 0 : x0); x <= (x1 >= w ? w - 1 : x1); ++x) {
                const long long y = y0 + (2 * (x - x0) * dy + (dy >= 0 ? dx : -dx)) / (2 * dx);   // rounded, dx > 0 here
                if (y >= 0 && y < h) { size_t o = 3 * (static_cast<size_t>(y) * w + x); rgb[o] = rgb[o + 1] = rgb[o + 2] = 255; }
            }
        } else {                                                        // y-major: one pixel per row
            const long long ya = y0 < y1 ? y0 : y1, yb = y0 < y1 ? y1 : y0;
            for (long long y = (ya < 0 ? 0 : ya); y <= (yb >= h ? h - 1 : yb); ++y) {
                const long long num = 2 * (y - y0) * dx + (((y - y0) * dx >= 0) == (dy >= 0) ? dy : -dy);
                const long long x = x0 + num / (2 * dy);
                if (x >= 0 && x < w) { size_t o = 3 * (static_cast<size_t>(y) * w + x); rgb[o] = rgb[o + 1] = rgb[o + 2] = 255; }
            }
        }
    }
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { fprintf(stderr, "pm_cli: cannot write %s\n", path.c_str()); return false; }
    fprintf(f, "P6\n%d %d\n255\n", w, h);
    const bool ok = fwrite(rgb.data(), 1, rgb.size(), f) == rgb.size();
    fclose(f);
    return ok;
}

bool save_matrix(const std::string& path, const Matrix& m)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { fprintf(stderr, "pm_cli: cannot write %s\n", path.c_str()); return false; }
    const int32_t hdr[3] = {m.rows, m.cols, m.dtype};
    const bool ok = fwrite("PMM1", 1, 4, f) == 4 && fwrite(hdr, 4, 3, f) == 3 && fwrite(m.data.data(), 1, m.data.size(), f) == m.data.size();
    fclose(f);
    return ok;
}

int fail(const char* what, int rc)
{
    fprintf(stderr, "pm_cli: %s failed: %s (%s)\n", what, pm_status_string(rc), pm_last_error());
    return 1;
}

bool write_pgm(const std::string& path, const std::vector<uint8_t>& px, int w, int h)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { fprintf(stderr, "pm_cli: cannot write %s\n", path.c_str()); return false; }
    fprintf(f, "P5\n%d %d\n255\n", w, h);
    const bool ok = fwrite(px.data(), 1, px.size(), f) == px.size();
    return fclose(f) == 0 && ok;
}

// --align: the 2-D model of the correspondences and image 2 warped into the frame of image 1 by it, on the context's stream
// with one synchronisation (the first download); the PGM and the report line.
int run_align(pm_ctx* ctx, const std::string& model, const std::string& out_path, const std::string& path1, const std::string& path2,
              const std::vector<float>& xy1, const std::vector<float>& xy2, int n, pm_ransac_params prm)
{
    pm_feat::Image im1, im2;
    std::string err;
    if (!pm_feat::load_pnm_gray(path1, im1, err) || !pm_feat::load_pnm_gray(path2, im2, err)) { fprintf(stderr, "pm_cli: %s\n", err.c_str()); return 1; }
    if (im1.w != im2.w || im1.h != im2.h) { fprintf(stderr, "pm_cli: --align needs two images of one size\n"); return 1; }
    const bool homography = model == "homography";
    const int affine_model = model == "similarity" ? PM_AFFINE_PARTIAL : PM_AFFINE_FULL;
    const int min_pts = homography ? 4 : (affine_model == PM_AFFINE_PARTIAL ? 2 : 3);
    if (n < min_pts) { fprintf(stderr, "pm_cli: --align: too few correspondences (%d)\n", n); return 1; }
    const int w = im1.w, h = im1.h;
    const size_t px = static_cast<size_t>(w) * h, xyb = static_cast<size_t>(n) * 8;
    void *d_src = nullptr, *d_dst = nullptr, *d_valid = nullptr, *d_xy1 = nullptr, *d_xy2 = nullptr, *d_mask = nullptr, *d_small = nullptr;
    auto release = [&]() { for (void* p : {d_src, d_dst, d_valid, d_xy1, d_xy2, d_mask, d_small}) pm_device_free(ctx, p); };
    int rc = pm_device_alloc(ctx, px, &d_src);
    if (rc == PM_OK) rc = pm_device_alloc(ctx, px, &d_dst);
    if (rc == PM_OK) rc = pm_device_alloc(ctx, px, &d_valid);
    if (rc == PM_OK) rc = pm_device_alloc(ctx, xyb, &d_xy1);
    if (rc == PM_OK) rc = pm_device_alloc(ctx, xyb, &d_xy2);
    if (rc == PM_OK) rc = pm_device_alloc(ctx, static_cast<size_t>(n), &d_mask);
    // one block of small results: model in (72 B), refined model (72 B), key (8 B), inlier count (4 B, padded), warp info (8 B)
    if (rc == PM_OK) rc = pm_device_alloc(ctx, 256, &d_small);
    if (rc != PM_OK) { release(); return fail("device buffers of --align", rc); }
    char* small = static_cast<char*>(d_small);
    double* d_M = reinterpret_cast<double*>(small);
    double* d_Mr = reinterpret_cast<double*>(small + 72);
    uint64_t* d_key = reinterpret_cast<uint64_t*>(small + 144);
    int32_t* d_ninl = reinterpret_cast<int32_t*>(small + 152);
    pm_warp_info* d_info = reinterpret_cast<pm_warp_info*>(small + 160);
    rc = pm_device_upload(ctx, d_src, im2.px.data(), px);
    if (rc == PM_OK) rc = pm_device_upload(ctx, d_xy1, xy1.data(), xyb);
    if (rc == PM_OK) rc = pm_device_upload(ctx, d_xy2, xy2.data(), xyb);
    pm_points_view view;
    view.xy1 = static_cast<const float*>(d_xy1); view.xy2 = static_cast<const float*>(d_xy2); view.counts = nullptr;
    view.parts = 1; view.cap = n; view.pitch_xy = 0; view.pitch_cnt = 1; view.reserved = 0;
    prm.error_kind = PM_ERR_REPROJ;
    pm_warp_params wp;
    wp.flags = homography ? 0 : PM_WARP_AFFINE; wp.border_value = 0; wp.reserved[0] = wp.reserved[1] = 0;
    if (rc == PM_OK && homography) {
        rc = pm_ransac_homography_run_dev(ctx, &view, &prm, d_key, d_M, static_cast<uint8_t*>(d_mask), n, d_ninl);
        if (rc == PM_OK) rc = pm_homography_refine_dev(ctx, &view, static_cast<const uint8_t*>(d_mask), d_M, 10, d_Mr, nullptr);
    } else if (rc == PM_OK) {
        rc = pm_ransac_affine_run_dev(ctx, affine_model, &view, &prm, d_key, d_M, static_cast<uint8_t*>(d_mask), n, d_ninl);
        if (rc == PM_OK) rc = pm_affine_refine_dev(ctx, affine_model, &view, static_cast<const uint8_t*>(d_mask), d_M, d_Mr, nullptr);
    }
    if (rc == PM_OK)
        rc = pm_warp_dev(ctx, static_cast<const uint8_t*>(d_src), w, h, w, d_Mr, &wp, static_cast<uint8_t*>(d_dst), w, h, w,
                         static_cast<uint8_t*>(d_valid), d_info);
    std::vector<uint8_t> dst(px), valid(px);
    pm_warp_info info = {0, 0};
    int32_t n_inl = 0;
    if (rc == PM_OK) rc = pm_device_download(ctx, dst.data(), d_dst, px);           // the one synchronisation
    if (rc == PM_OK) rc = pm_device_download(ctx, valid.data(), d_valid, px);
    if (rc == PM_OK) rc = pm_device_download(ctx, &info, d_info, sizeof info);
    if (rc == PM_OK) rc = pm_device_download(ctx, &n_inl, d_ninl, sizeof n_inl);
    release();
    if (rc != PM_OK) return fail("--align", rc);
    if (info.status != 0) { fprintf(stderr, "pm_cli: --align: no usable %s (warp status %d)\n", model.c_str(), info.status); return 1; }
    long long before = 0, after = 0;
    for (size_t i = 0; i < px; ++i)
        if (valid[i]) {
            before += std::abs(static_cast<int>(im2.px[i]) - static_cast<int>(im1.px[i]));
            after += std::abs(static_cast<int>(dst[i]) - static_cast<int>(im1.px[i]));
        }
    if (!write_pgm(out_path, dst, w, h)) return 1;
    const double nv = info.n_valid > 0 ? static_cast<double>(info.n_valid) : 1.0;
    printf("align: model=%s inliers=%d valid=%d mad_before=%.4f mad_after=%.4f\n", model.c_str(), n_inl, info.n_valid, before / nv, after / nv);
    return 0;
}

// "a,b,c": exactly n finite numbers separated by commas
bool parse_numbers(const char* text, int n, double* out)
{
    const char* p = text;
    for (int i = 0; i < n; ++i) {
        char* end = nullptr;
        out[i] = strtod(p, &end);
        if (end == p || !(out[i] - out[i] == 0.0)) return false;
        if (*end != (i + 1 < n ? ',' : '\0')) return false;
        p = end + 1;
    }
    return true;
}

// --undistort: upload, pm_undistort_dev, download; the PGM and the report
int run_undistort(int device, const std::string& out_path, const std::string& in_path, const pm_camera& K, const pm_lens& lens, const pm_camera* K_new,
                  bool json)
{
    pm_feat::Image im;
    std::string err;
    if (!pm_feat::load_pnm_gray(in_path, im, err)) { fprintf(stderr, "pm_cli: %s\n", err.c_str()); return 1; }
    pm_ctx* ctx = nullptr;
    int rc = pm_ctx_create(device, &ctx);
    if (rc != PM_OK) return fail("pm_ctx_create", rc);
    const int w = im.w, h = im.h;
    const size_t px = static_cast<size_t>(w) * h;
    void *d_src = nullptr, *d_dst = nullptr, *d_info = nullptr;
    rc = pm_device_alloc(ctx, px, &d_src);
    if (rc == PM_OK) rc = pm_device_alloc(ctx, px, &d_dst);
    if (rc == PM_OK) rc = pm_device_alloc(ctx, sizeof(pm_warp_info), &d_info);
    if (rc == PM_OK) rc = pm_device_upload(ctx, d_src, im.px.data(), px);
    pm_warp_params wp;
    wp.flags = 0; wp.border_value = 0; wp.reserved[0] = wp.reserved[1] = 0;
    if (rc == PM_OK)
        rc = pm_undistort_dev(ctx, static_cast<const uint8_t*>(d_src), w, h, w, &K, &lens, nullptr, K_new, &wp, static_cast<uint8_t*>(d_dst), w, h, w,
                              nullptr, static_cast<pm_warp_info*>(d_info));
    std::vector<uint8_t> dst(px);
    pm_warp_info info = {0, 0};
    if (rc == PM_OK) rc = pm_device_download(ctx, dst.data(), d_dst, px);
    if (rc == PM_OK) rc = pm_device_download(ctx, &info, d_info, sizeof info);
    for (void* p : {d_src, d_dst, d_info}) pm_device_free(ctx, p);
    if (rc != PM_OK) { fail("--undistort", rc); pm_ctx_destroy(ctx); return 1; }
    pm_ctx_destroy(ctx);
    if (!write_pgm(out_path, dst, w, h)) return 1;
    if (json) printf("{\"undistort\": {\"width\": %d, \"height\": %d, \"n_valid\": %d}}\n", w, h, info.n_valid);
    else printf("undistort: valid=%d\n", info.n_valid);
    return 0;
}

// --stereo: an already rectified pair through pm_stereo_bm (with --lr-check T16 >= 0 also the FROM_RIGHT pass and the left-right
// check); a 16-bit PGM, most significant byte first: v - 16 * min_disp + 1, 0 where there is no disparity
int run_stereo(int device, const std::string& out_path, const std::string& left_path, const std::string& right_path, const pm_stereo_params& prm,
               const pm_sgm_params* sgm, int lr_check, bool json)
{
    pm_feat::Image im1, im2;
    std::string err;
    if (!pm_feat::load_pnm_gray(left_path, im1, err) || !pm_feat::load_pnm_gray(right_path, im2, err)) { fprintf(stderr, "pm_cli: %s\n", err.c_str()); return 1; }
    if (im1.w != im2.w || im1.h != im2.h) { fprintf(stderr, "pm_cli: --stereo needs two images of one size\n"); return 1; }
    pm_ctx* ctx = nullptr;
    int rc = pm_ctx_create(device, &ctx);
    if (rc != PM_OK) return fail("pm_ctx_create", rc);
    const int w = im1.w, h = im1.h;
    const size_t px = static_cast<size_t>(w) * h;
    std::vector<int16_t> disp(px);
    pm_stereo_info info = {0, 0};
    if (sgm) rc = pm_stereo_sgm(ctx, im1.px.data(), im2.px.data(), w, h, w, w, sgm, lr_check, disp.data(), w, &info);
    else rc = pm_stereo_bm(ctx, im1.px.data(), im2.px.data(), w, h, w, w, &prm, lr_check, disp.data(), w, &info);
    if (rc != PM_OK) { fail("--stereo", rc); pm_ctx_destroy(ctx); return 1; }
    pm_ctx_destroy(ctx);
    std::vector<uint8_t> out(px * 2);
    for (size_t i = 0; i < px; ++i) {
        const int v = disp[i] == PM_STEREO_INVALID ? 0 : disp[i] - 16 * prm.min_disp + 1;
        out[2 * i] = static_cast<uint8_t>(v >> 8);
        out[2 * i + 1] = static_cast<uint8_t>(v & 255);
    }
    FILE* f = fopen(out_path.c_str(), "wb");
    if (!f) { fprintf(stderr, "pm_cli: cannot write %s\n", out_path.c_str()); return 1; }
    fprintf(f, "P5\n%d %d\n65535\n", w, h);
    const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    if (fclose(f) != 0 || !ok) { fprintf(stderr, "pm_cli: cannot write %s\n", out_path.c_str()); return 1; }
    if (json) printf("{\"stereo\": {\"width\": %d, \"height\": %d, \"n_valid\": %d}}\n", w, h, info.n_valid);
    else printf("stereo: valid=%d\n", info.n_valid);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    std::string desc1, desc2, kp1, kp2, filter = "midpoint", fscale = "opencv", method = "7point-lmeds";
    float ratio = 0.8f, thresh = 1.0f, guided_tau = 0.f;
    bool guided = false;
    long iters = 10000;
    unsigned long long seed = 0x5EED;
    int device = 0, gpus = 1, canvas_w = 993, canvas_h = 660;       // canvas default: the size of img01/img02
    std::string epi_ppm, img2_path, matcher = "bf", img1_path, save_prefix, knn_hint, features = "host", descriptor = "grad";
    bool extract_only = false, filter_given = false, descriptor_given = false;
    int lk_radius = 10, lk_levels = 3;
    float lk_fb = 0.f;
    std::string points = "dog", align_pgm, align_model = "homography";
    bool align_model_given = false;
    std::string undistort_pgm, camera_arg, lens_arg, new_camera_arg;
    std::string stereo_pgm;
    pm_stereo_params stereo_prm = {0, 0, 4, 0, 0, {0, 0, 0}};
    int stereo_lr = -1;
    bool stereo_opt_given = false, radius_given = false, paths_given = false, sgm_given = false;
    pm_sgm_params sgm_prm = {0, 0, 0, 0, 8, 0, 0, 0};
    bool points_given = false, corner_opt_given = false;
    float corner_dist = 8.f, corner_quality = 0.01f, corner_min_eig = 1e-4f;
    int max_kp = 4000;
    bool quiet = false, json = false, iters_given = false, print_epi = false, force_mgpu = false;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto val = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "pm_cli: %s needs a value\n", name); exit(2); }
            return argv[++i];
        };
        if (a == "--desc1") desc1 = val("--desc1");
        else if (a == "--desc2") desc2 = val("--desc2");
        else if (a == "--kp1") kp1 = val("--kp1");
        else if (a == "--kp2") kp2 = val("--kp2");
        else if (a == "--filter") { filter = val("--filter"); filter_given = true; }
        else if (a == "--lk-radius") lk_radius = atoi(val("--lk-radius"));
        else if (a == "--lk-levels") lk_levels = atoi(val("--lk-levels"));
        else if (a == "--lk-fb") lk_fb = strtof(val("--lk-fb"), nullptr);
        else if (a == "--points") { points = val("--points"); points_given = true; }
        else if (a == "--align") align_pgm = val("--align");
        else if (a == "--align-model") { align_model = val("--align-model"); align_model_given = true; }
        else if (a == "--undistort") undistort_pgm = val("--undistort");
        else if (a == "--stereo") stereo_pgm = val("--stereo");
        else if (a == "--num-disp") { stereo_prm.num_disp = atoi(val("--num-disp")); stereo_opt_given = true; }
        else if (a == "--min-disp") { stereo_prm.min_disp = atoi(val("--min-disp")); stereo_opt_given = true; }
        else if (a == "--radius") { stereo_prm.radius = atoi(val("--radius")); stereo_opt_given = radius_given = true; }
        else if (a == "--sgm") {
            int used = 0;
            const char* v = val("--sgm");
            if (sscanf(v, "%d,%d%n", &sgm_prm.p1, &sgm_prm.p2, &used) != 2 || v[used] != '\0') {
                fprintf(stderr, "pm_cli: --sgm needs P1,P2 (two integers)\n");
                return 2;
            }
            sgm_given = true;
        }
        else if (a == "--paths") { sgm_prm.paths = atoi(val("--paths")); paths_given = true; }
        else if (a == "--uniqueness") { stereo_prm.uniqueness = atoi(val("--uniqueness")); stereo_opt_given = true; }
        else if (a == "--lr-check") { stereo_lr = atoi(val("--lr-check")); stereo_opt_given = true; }
        else if (a == "--camera") camera_arg = val("--camera");
        else if (a == "--lens") lens_arg = val("--lens");
        else if (a == "--new-camera") new_camera_arg = val("--new-camera");
        else if (a == "--corner-dist") { corner_dist = strtof(val("--corner-dist"), nullptr); corner_opt_given = true; }
        else if (a == "--corner-quality") { corner_quality = strtof(val("--corner-quality"), nullptr); corner_opt_given = true; }
        else if (a == "--corner-min-eig") { corner_min_eig = strtof(val("--corner-min-eig"), nullptr); corner_opt_given = true; }
        else if (a == "--ratio") ratio = strtof(val("--ratio"), nullptr);
        else if (a == "--iters") { iters = strtol(val("--iters"), nullptr, 0); iters_given = true; }
        else if (a == "--guided") { guided_tau = strtof(val("--guided"), nullptr); guided = true; }
        else if (a == "--thresh") thresh = strtof(val("--thresh"), nullptr);
        else if (a == "--seed") seed = strtoull(val("--seed"), nullptr, 0);
        else if (a == "--f-scale") fscale = val("--f-scale");
        else if (a == "--method") method = val("--method");
        else if (a == "--device") device = atoi(val("--device"));
        else if (a == "--gpus") gpus = atoi(val("--gpus"));
        else if (a == "--matcher") matcher = val("--matcher");
        else if (a == "--knn-hint") knn_hint = val("--knn-hint");      // auto | int | u8: what the caller knows about float descriptors
        else if (a == "--mgpu") force_mgpu = true;            // take the pm_mgpu path even with --gpus 1 (tests)
        else if (a == "--print-epilines") print_epi = true;
        else if (a == "--epilines") epi_ppm = val("--epilines");
        else if (a == "--img2") img2_path = val("--img2");
        else if (a == "--img1") img1_path = val("--img1");
        else if (a == "--max-kp") max_kp = atoi(val("--max-kp"));
        else if (a == "--features") features = val("--features");      // host | device | corners: how --img1/--img2 are extracted
        else if (a == "--descriptor") { descriptor = val("--descriptor"); descriptor_given = true; }  // grad | bits: what --img1/--img2 are described with
        else if (a == "--dump-bits-pattern") {                             // the host extractor's 256 tests of S58, one per line; no GPU
            signed char pat[256][4];
            pm_feat::bits_pattern(pat);
            for (int t = 0; t < 256; ++t) printf("%d %d %d %d\n", pat[t][0], pat[t][1], pat[t][2], pat[t][3]);
            return 0;
        }
        else if (a == "--save-features") save_prefix = val("--save-features");   // PREFIX_{desc1,desc2,kp1,kp2}.pmm
        else if (a == "--extract-only") extract_only = true;                     // stop after the feature front-end (no GPU needed)
        else if (a == "--canvas") { canvas_w = atoi(val("--canvas")); canvas_h = atoi(val("--canvas")); }
        else if (a == "--quiet") quiet = true;
        else if (a == "--json") json = true;
        else { fprintf(stderr, "pm_cli: unknown option %s\n", a.c_str()); return 2; }
    }
    if (undistort_pgm.empty() && !(camera_arg.empty() && lens_arg.empty() && new_camera_arg.empty())) {
        fprintf(stderr, "pm_cli: --camera, --lens and --new-camera need --undistort OUT.pgm\n");
        return 2;
    }
    if (stereo_pgm.empty() && stereo_opt_given) {
        fprintf(stderr, "pm_cli: --num-disp, --min-disp, --radius, --uniqueness and --lr-check need --stereo OUT.pgm\n");
        return 2;
    }
    if ((sgm_given && stereo_pgm.empty()) || (paths_given && !sgm_given) || (sgm_given && radius_given)) {
        fprintf(stderr, "pm_cli: --sgm P1,P2 needs --stereo OUT.pgm and takes no --radius; --paths needs --sgm\n");
        return 2;
    }
    if (!stereo_pgm.empty()) {
        // ---- a rectified pair through pm_stereo_bm, then exit (no features, no matcher)
        if (img1_path.empty() || img2_path.empty() || stereo_prm.num_disp < 1 || !undistort_pgm.empty()) {
            fprintf(stderr, "pm_cli: --stereo needs --img1 L.pgm --img2 R.pgm --num-disp N (and no --undistort)\n");
            return 2;
        }
        const bool other_mode = !align_pgm.empty() || align_model_given || guided || !epi_ppm.empty() || print_epi || matcher != "bf" ||
                                features != "host" || filter_given || descriptor_given || points_given || corner_opt_given || extract_only ||
                                !save_prefix.empty() || !knn_hint.empty() || force_mgpu || gpus != 1 || iters_given || !desc1.empty() ||
                                !desc2.empty() || !kp1.empty() || !kp2.empty();
        if (other_mode) {
            fprintf(stderr, "pm_cli: --stereo takes --img1, --img2, its own options, --device and --json only\n");
            return 2;
        }
        sgm_prm.min_disp = stereo_prm.min_disp; sgm_prm.num_disp = stereo_prm.num_disp; sgm_prm.uniqueness = stereo_prm.uniqueness;
        return run_stereo(device, stereo_pgm, img1_path, img2_path, stereo_prm, sgm_given ? &sgm_prm : nullptr, stereo_lr, json);
    }
    if (!undistort_pgm.empty()) {
        // ---- one image through pm_undistort_dev, then exit (no features, no matcher)
        if (img1_path.empty() || camera_arg.empty() || lens_arg.empty()) {
            fprintf(stderr, "pm_cli: --undistort needs --img1 IN.pgm --camera fx,fy,cx,cy --lens k1,k2,p1,p2,k3\n");
            return 2;
        }
        double c[4], l[5], nc[4];
        if (!parse_numbers(camera_arg.c_str(), 4, c)) { fprintf(stderr, "pm_cli: --camera fx,fy,cx,cy (four numbers)\n"); return 2; }
        if (!parse_numbers(lens_arg.c_str(), 5, l)) { fprintf(stderr, "pm_cli: --lens k1,k2,p1,p2,k3 (five numbers)\n"); return 2; }
        if (!new_camera_arg.empty() && !parse_numbers(new_camera_arg.c_str(), 4, nc)) {
            fprintf(stderr, "pm_cli: --new-camera fx,fy,cx,cy (four numbers)\n");
            return 2;
        }
        const pm_camera K = {c[0], c[1], c[2], c[3]}, Kn = {nc[0], nc[1], nc[2], nc[3]};
        const pm_lens lens = {l[0], l[1], l[2], l[3], l[4]};
        return run_undistort(device, undistort_pgm, img1_path, K, lens, new_camera_arg.empty() ? nullptr : &Kn, json);
    }
    Matrix d1, d2, k1, k2;
    const bool from_images = !img1_path.empty();
    const bool corner_feat = features == "corners";
    if (features != "host" && features != "device" && !corner_feat) { fprintf(stderr, "pm_cli: --features host|device|corners\n"); return 2; }
    if (features == "device" && !from_images) { fprintf(stderr, "pm_cli: --features device needs --img1 / --img2\n"); return 2; }
    if (corner_feat && !from_images) { fprintf(stderr, "pm_cli: --features corners needs --img1 / --img2\n"); return 2; }
    if (descriptor != "grad" && descriptor != "bits") { fprintf(stderr, "pm_cli: --descriptor grad|bits\n"); return 2; }
    if (descriptor == "bits" && !from_images) { fprintf(stderr, "pm_cli: --descriptor bits needs --img1 / --img2\n"); return 2; }
    if (corner_feat && descriptor_given && descriptor == "grad") {
        fprintf(stderr, "pm_cli: --features corners describes by bits and takes no --descriptor grad\n");
        return 2;
    }
    if (corner_feat && matcher != "bf") { fprintf(stderr, "pm_cli: --features corners takes --matcher bf only\n"); return 2; }
    if (corner_feat && points_given) { fprintf(stderr, "pm_cli: --features corners takes no --points\n"); return 2; }
    const bool want_bits = descriptor == "bits" || corner_feat;
    const bool track = matcher == "track";
    if (track && (!from_images || features != "device" || want_bits || filter_given || guided || gpus != 1 || force_mgpu)) {
        fprintf(stderr, "pm_cli: --matcher track needs --img1 / --img2 --features device and takes no --descriptor bits, --filter, "
                        "--guided, --gpus N or --mgpu\n");
        return 2;
    }
    if (track && (lk_radius < 2 || lk_radius > 15 || lk_levels < 0 || lk_levels > 7 || !(lk_fb >= 0.f) || !(lk_fb <= 1e6f))) {
        fprintf(stderr, "pm_cli: --lk-radius 2..15, --lk-levels 0..7, --lk-fb >= 0\n");
        return 2;
    }
    const bool corner_points = points == "corners";
    if ((points_given || (corner_opt_given && !corner_feat)) && (!track || (points != "dog" && !corner_points) || (corner_opt_given && !corner_points))) {
        fprintf(stderr, "pm_cli: --points dog|corners needs --matcher track, and the --corner-* options need --points corners\n");
        return 2;
    }
    if ((corner_points || corner_feat) && (!(corner_dist >= 0.f) || !(corner_dist <= 1e6f) || !(corner_quality >= 0.f) || !(corner_quality <= 1.f) ||
                          !(corner_min_eig >= 0.f) || !(corner_min_eig <= 3.0e38f))) {
        fprintf(stderr, "pm_cli: --corner-dist 0..1e6, --corner-quality 0..1, --corner-min-eig >= 0\n");
        return 2;
    }
    const bool align = !align_pgm.empty();
    if (align_model_given && !align) { fprintf(stderr, "pm_cli: --align-model needs --align OUT.pgm\n"); return 2; }
    if (align && align_model != "homography" && align_model != "affine" && align_model != "similarity") {
        fprintf(stderr, "pm_cli: --align-model homography|affine|similarity\n");
        return 2;
    }
    if (align && !from_images) { fprintf(stderr, "pm_cli: --align needs --img1 / --img2\n"); return 2; }
    if (align && (json || guided || print_epi || !epi_ppm.empty() || gpus != 1 || force_mgpu)) {
        fprintf(stderr, "pm_cli: --align takes no --json, --guided, --epilines, --print-epilines, --gpus N or --mgpu\n");
        return 2;
    }
    int img_w[2] = {0, 0}, img_h[2] = {0, 0};
    pm_pyramid* corner_pyr = nullptr;                 // --points corners: the first frame's pyramid, built before the corners are found
    pm_ctx* feat_ctx = nullptr;                       // --features device: the context that extracted, reused by the matcher
    void* dev_img[2] = {nullptr, nullptr};
    void* dev_kp[2] = {nullptr, nullptr};
    void* dev_u8[2] = {nullptr, nullptr};             // n x 128 (bits: n x 32) descriptor bytes, left on the device for the matcher
    void* dev_f32[2] = {nullptr, nullptr};
    void* dev_n[2] = {nullptr, nullptr};
    auto free_device_features = [&]() {               // the device buffers of --features device, then their context
        if (!feat_ctx) return;
        pm_pyramid_destroy(corner_pyr);
        corner_pyr = nullptr;
        for (int i = 0; i < 2; ++i)
            for (void** p : {&dev_img[i], &dev_kp[i], &dev_u8[i], &dev_f32[i], &dev_n[i]}) { pm_device_free(feat_ctx, *p); *p = nullptr; }
        pm_ctx_destroy(feat_ctx);
        feat_ctx = nullptr;
    };
    // what the caller knows about float descriptors (pm.h: a hint is verified on the device, a wrong one only costs time).
    // The build-owned extractor of --img1/--img2 writes u8-valued rows, so that path says so unless told otherwise.
    if (knn_hint.empty()) knn_hint = from_images ? "u8" : "auto";
    if (knn_hint != "auto" && knn_hint != "int" && knn_hint != "u8" && knn_hint != "unit") {
        fprintf(stderr, "pm_cli: --knn-hint auto|int|u8|unit\n");
        return 2;
    }
    const int knn_flags = knn_hint == "u8" ? PM_KNN_HINT_U8 : knn_hint == "int" ? PM_KNN_HINT_INTEGER :
                          knn_hint == "unit" ? PM_KNN_HINT_UNIT_NORM : 0;          // unit: L2-normalised rows (SURF, main.cpp:37-40)
    if (from_images) {
        // ---- imread + detect + compute                                          main.cpp:14-15, :22-26, :36-40
        if (img2_path.empty() || max_kp < 8) { fprintf(stderr, "pm_cli: --img1 needs --img2 (and --max-kp >= 8)\n"); return 2; }
        const std::string* paths[2] = {&img1_path, &img2_path};
        Matrix* dm[2] = {&d1, &d2};
        Matrix* km[2] = {&k1, &k2};
        for (int i = 0; i < 2; ++i) {
            pm_feat::Image im;
            std::string err;
            if (!pm_feat::load_pnm_gray(*paths[i], im, err)) { fprintf(stderr, "pm_cli: %s\n", err.c_str()); return 1; }
            pm_feat::Features ft;
            img_w[i] = im.w;
            img_h[i] = im.h;
            if (track && i == 1) {
                // ---- the second frame is only uploaded: its positions come from tracking, not from a second detection
                if (im.w != img_w[0] || im.h != img_h[0]) { fprintf(stderr, "pm_cli: --matcher track needs two images of one size\n"); return 1; }
                int r = pm_device_alloc(feat_ctx, im.px.size(), &dev_img[i]);
                if (r == PM_OK) r = pm_device_upload(feat_ctx, dev_img[i], im.px.data(), im.px.size());
                if (r != PM_OK) return fail("device buffers", r);
            } else if (track && corner_points) {
                // ---- upload, build the pyramid the tracker will use, find the corners on its level 0; no descriptors
                int r = pm_ctx_create(device, &feat_ctx);
                if (r != PM_OK) return fail("pm_ctx_create", r);
                r = pm_device_alloc(feat_ctx, im.px.size(), &dev_img[i]);
                if (r == PM_OK) r = pm_device_alloc(feat_ctx, static_cast<size_t>(max_kp) * 8, &dev_kp[i]);
                if (r == PM_OK) r = pm_device_alloc(feat_ctx, 4, &dev_n[i]);
                if (r == PM_OK) r = pm_device_upload(feat_ctx, dev_img[i], im.px.data(), im.px.size());
                if (r != PM_OK) return fail("device buffers", r);
                r = pm_pyramid_create(feat_ctx, im.w, im.h, lk_levels, &corner_pyr);
                if (r == PM_OK) r = pm_pyramid_build_dev(feat_ctx, corner_pyr, static_cast<const uint8_t*>(dev_img[i]), im.w);
                if (r != PM_OK) return fail("pyramid of image 1", r);
                pm_corner_params cp;
                cp.block_radius = lk_radius; cp.min_eig = corner_min_eig; cp.quality = corner_quality; cp.min_dist = corner_dist;
                cp.capacity = 0; cp.flags = 0; cp.reserved[0] = cp.reserved[1] = 0;
                int32_t n = -1;
                while (n < 0) {
                    r = pm_corners_dev(feat_ctx, corner_pyr, &cp, nullptr, nullptr, 0, max_kp, static_cast<float*>(dev_kp[i]), nullptr,
                                       static_cast<int32_t*>(dev_n[i]));
                    if (r == PM_OK) r = pm_device_download(feat_ctx, &n, dev_n[i], sizeof n);
                    if (r != PM_OK) return fail("pm_corners_dev", r);
                    if (n < 0) {                              // more candidates than the buffer holds: double it
                        if (cp.capacity == 0) cp.capacity = max_kp > 8192 ? 8 * max_kp : 65536;
                        if (cp.capacity > (1 << 23)) { fprintf(stderr, "pm_cli: too many corner candidates\n"); return 1; }
                        cp.capacity *= 2;
                    }
                }
                ft.n = n;
                ft.kp_xy.resize(2 * static_cast<size_t>(n));
                r = pm_device_download(feat_ctx, ft.kp_xy.data(), dev_kp[i], ft.kp_xy.size() * sizeof(float));
                if (r != PM_OK) return fail("download of the corners", r);
            } else if (corner_feat) {
                // ---- upload, pyramid (level 0), corners, descriptors of the corners at level 0; the rows stay for the matcher
                int r = feat_ctx ? PM_OK : pm_ctx_create(device, &feat_ctx);
                if (r != PM_OK) return fail("pm_ctx_create", r);
                const size_t rows = static_cast<size_t>(max_kp);
                r = pm_device_alloc(feat_ctx, im.px.size(), &dev_img[i]);
                if (r == PM_OK) r = pm_device_alloc(feat_ctx, rows * 8, &dev_kp[i]);
                if (r == PM_OK) r = pm_device_alloc(feat_ctx, rows * 32, &dev_u8[i]);
                if (r == PM_OK) r = pm_device_alloc(feat_ctx, rows * 8 + 16, &dev_f32[i]);     // the corners, then their count
                if (r == PM_OK) r = pm_device_alloc(feat_ctx, 4, &dev_n[i]);
                if (r == PM_OK) r = pm_device_upload(feat_ctx, dev_img[i], im.px.data(), im.px.size());
                if (r != PM_OK) return fail("device buffers", r);
                float* d_corner = static_cast<float*>(dev_f32[i]);
                int32_t* d_ncorner = reinterpret_cast<int32_t*>(static_cast<char*>(dev_f32[i]) + rows * 8);
                pm_pyramid* pyr = nullptr;
                r = pm_pyramid_create(feat_ctx, im.w, im.h, 0, &pyr);
                if (r == PM_OK) r = pm_pyramid_build_dev(feat_ctx, pyr, static_cast<const uint8_t*>(dev_img[i]), im.w);
                pm_corner_params cp;
                cp.block_radius = 10; cp.min_eig = corner_min_eig; cp.quality = corner_quality; cp.min_dist = corner_dist;
                cp.capacity = 0; cp.flags = 0; cp.reserved[0] = cp.reserved[1] = 0;
                pm_describe_params dp;
                dp.level = 0; dp.flags = 0; dp.reserved[0] = dp.reserved[1] = 0;
                int32_t nc = -1, n = 0;
                while (r == PM_OK && nc < 0) {
                    r = pm_corners_dev(feat_ctx, pyr, &cp, nullptr, nullptr, 0, max_kp, d_corner, nullptr, d_ncorner);
                    if (r == PM_OK) r = pm_device_download(feat_ctx, &nc, d_ncorner, sizeof nc);
                    if (r == PM_OK && nc < 0) {               // more candidates than the buffer holds: double it
                        if (cp.capacity == 0) cp.capacity = max_kp > 8192 ? 8 * max_kp : 65536;
                        if (cp.capacity > (1 << 23)) { fprintf(stderr, "pm_cli: too many corner candidates\n"); pm_pyramid_destroy(pyr); return 1; }
                        cp.capacity *= 2;
                    }
                }
                if (r == PM_OK)
                    r = pm_describe_points_gather_dev(feat_ctx, pyr, d_corner, d_ncorner, max_kp, &dp, static_cast<float*>(dev_kp[i]),
                                                      static_cast<uint8_t*>(dev_u8[i]), nullptr, static_cast<int32_t*>(dev_n[i]));
                if (r == PM_OK) r = pm_device_download(feat_ctx, &n, dev_n[i], sizeof n);
                pm_pyramid_destroy(pyr);                      // (the download synchronised: nothing reads it any more)
                if (r != PM_OK) return fail("corners and their descriptors", r);
                ft.n = n;
                ft.kp_xy.resize(2 * static_cast<size_t>(n));
                ft.bits.resize(32 * static_cast<size_t>(n));
                r = pm_device_download(feat_ctx, ft.kp_xy.data(), dev_kp[i], ft.kp_xy.size() * sizeof(float));
                if (r == PM_OK) r = pm_device_download(feat_ctx, ft.bits.data(), dev_u8[i], ft.bits.size());
                if (r != PM_OK) return fail("download of the features", r);
            } else if (features == "device") {
                // ---- upload, extract on the device, bring back keypoints + float rows (match list, --save-features)
                int r = feat_ctx ? PM_OK : pm_ctx_create(device, &feat_ctx);
                if (r != PM_OK) return fail("pm_ctx_create", r);
                const size_t rows = static_cast<size_t>(max_kp);
                r = pm_device_alloc(feat_ctx, im.px.size(), &dev_img[i]);
                if (r == PM_OK) r = pm_device_alloc(feat_ctx, rows * 8, &dev_kp[i]);
                if (r == PM_OK) r = pm_device_alloc(feat_ctx, rows * (want_bits ? 32 : 128), &dev_u8[i]);
                if (r == PM_OK && !want_bits) r = pm_device_alloc(feat_ctx, rows * 512, &dev_f32[i]);
                if (r == PM_OK) r = pm_device_alloc(feat_ctx, 4, &dev_n[i]);
                if (r == PM_OK) r = pm_device_upload(feat_ctx, dev_img[i], im.px.data(), im.px.size());
                if (r != PM_OK) return fail("device buffers", r);
                int32_t n = -1;
                for (int cap = 0; n < 0;) {
                    if (want_bits)
                        r = pm_detect_describe_bits_dev(feat_ctx, static_cast<const uint8_t*>(dev_img[i]), im.w, im.h, im.w, max_kp, 0.03f,
                                                        10.0f, static_cast<float*>(dev_kp[i]), static_cast<uint8_t*>(dev_u8[i]), nullptr,
                                                        static_cast<int32_t*>(dev_n[i]));
                    else
                        r = pm_detect_describe_dev(feat_ctx, static_cast<const uint8_t*>(dev_img[i]), im.w, im.h, im.w, max_kp, 0.03f, 10.0f,
                                                   static_cast<float*>(dev_kp[i]), static_cast<uint8_t*>(dev_u8[i]),
                                                   static_cast<float*>(dev_f32[i]), nullptr, static_cast<int32_t*>(dev_n[i]));
                    if (r == PM_OK) r = pm_device_download(feat_ctx, &n, dev_n[i], sizeof n);
                    if (r != PM_OK) return fail(want_bits ? "pm_detect_describe_bits_dev" : "pm_detect_describe_dev", r);
                    if (n < 0) {                              // more extrema than the candidate buffer holds: double it
                        if (cap == 0) cap = max_kp > 8192 ? 8 * max_kp : 65536;
                        if (cap > (1 << 27)) { fprintf(stderr, "pm_cli: too many extrema\n"); return 1; }
                        cap *= 2;
                        r = pm_ctx_set_option(feat_ctx, PM_OPT_FEAT_CAPACITY, cap);
                        if (r != PM_OK) return fail("pm_ctx_set_option", r);
                    }
                }
                ft.n = n;
                ft.kp_xy.resize(2 * static_cast<size_t>(n));
                if (want_bits) ft.bits.resize(32 * static_cast<size_t>(n));
                else ft.desc.resize(128 * static_cast<size_t>(n));
                r = pm_device_download(feat_ctx, ft.kp_xy.data(), dev_kp[i], ft.kp_xy.size() * sizeof(float));
                if (r == PM_OK && want_bits) r = pm_device_download(feat_ctx, ft.bits.data(), dev_u8[i], ft.bits.size());
                if (r == PM_OK && !want_bits) r = pm_device_download(feat_ctx, ft.desc.data(), dev_f32[i], ft.desc.size() * sizeof(float));
                if (r != PM_OK) return fail("download of the features", r);
            } else
                ft = pm_feat::detect_and_describe(im, max_kp, 0.03f, 10.0f, want_bits ? pm_feat::DESC_BITS : pm_feat::DESC_GRAD);
            if (want_bits) {
                dm[i]->rows = ft.n; dm[i]->cols = 32; dm[i]->dtype = 1;
                dm[i]->data = ft.bits;
            } else {
                dm[i]->rows = ft.n; dm[i]->cols = 128; dm[i]->dtype = 0;
                dm[i]->data.assign(reinterpret_cast<const unsigned char*>(ft.desc.data()),
                                   reinterpret_cast<const unsigned char*>(ft.desc.data()) + ft.desc.size() * sizeof(float));
            }
            km[i]->rows = ft.n; km[i]->cols = 2; km[i]->dtype = 0;
            km[i]->data.assign(reinterpret_cast<const unsigned char*>(ft.kp_xy.data()),
                               reinterpret_cast<const unsigned char*>(ft.kp_xy.data()) + ft.kp_xy.size() * sizeof(float));
            if (!quiet) fprintf(stderr, "pm_cli: %s: %d x %d, %d keypoints\n", paths[i]->c_str(), im.w, im.h, ft.n);
            if (i == 1) { canvas_w = im.w; canvas_h = im.h; }
        }
        if (!save_prefix.empty()) {
            const Matrix* ms[4] = {&d1, &d2, &k1, &k2};
            const char* names[4] = {"_desc1.pmm", "_desc2.pmm", "_kp1.pmm", "_kp2.pmm"};
            for (int i = 0; i < 4; ++i)
                if (!save_matrix(save_prefix + names[i], *ms[i])) return 1;
        }
        if (extract_only) { free_device_features(); return 0; }
        if (d1.rows < 8 || (!track && d2.rows < 8)) { fprintf(stderr, "pm_cli: too few keypoints\n"); free_device_features(); return 1; }
    } else {
    if (desc1.empty() || desc2.empty() || kp1.empty() || kp2.empty()) {
        fprintf(stderr, "usage: pm_cli (--img1 L.pgm --img2 R.pgm | --desc1 A --desc2 B --kp1 KA --kp2 KB) [--filter midpoint|ratio|cross|cross-ratio] "
                        "[--ratio r] [--method 7point-lmeds|ransac8] [--iters n] [--thresh px] [--seed s] [--f-scale opencv|unit] "
                        "[--matcher bf|flann|track [--lk-radius r] [--lk-levels l] [--lk-fb px] [--points dog|corners [--corner-dist px] [--corner-quality q] [--corner-min-eig m]]] [--guided tau_px] [--features host|device|corners] [--descriptor grad|bits] [--knn-hint auto|int|u8|unit] [--align out.pgm [--align-model homography|affine|similarity]] [--undistort out.pgm --camera fx,fy,cx,cy --lens k1,k2,p1,p2,k3 [--new-camera fx,fy,cx,cy]] [--gpus N] [--print-epilines] [--epilines out.ppm] [--json] [--quiet]\n"
                        "  (default matcher bf = exact brute force, main.cpp:43; the reference's active one is --matcher flann, main.cpp:44)\n");
        return 2;
    }
    if (!load_matrix(desc1, d1) || !load_matrix(desc2, d2) || !load_matrix(kp1, k1) || !load_matrix(kp2, k2)) return 1;
    if (d1.cols != d2.cols || d1.dtype != d2.dtype || k1.dtype != 0 || k2.dtype != 0 || k1.cols != 2 ||
        k2.cols != 2 || k1.rows != d1.rows || k2.rows != d2.rows) {
        fprintf(stderr, "pm_cli: inconsistent descriptor / keypoint matrices\n");
        return 1;
    }
    }
    // uint8 descriptors whose column count is no multiple of 4 (AKAZE: 61): both files are zero-padded to the next
    // multiple before every Hamming call (plain, cross, guided) — equal zero bytes on both sides leave every distance as it is
    if (d1.dtype == 1 && d1.cols % 4 != 0) {
        const int padded = (d1.cols + 3) / 4 * 4;
        for (Matrix* m : {&d1, &d2}) {
            std::vector<unsigned char> wide(static_cast<size_t>(m->rows) * padded);
            const int r = pm_pad_rows_u8(m->data.data(), m->rows, m->cols, wide.data(), padded);
            if (r != PM_OK) { fprintf(stderr, "pm_cli: pm_pad_rows_u8 failed: %s\n", pm_last_error()); return 1; }
            m->data.swap(wide);
            m->cols = padded;
        }
    }
    const bool want_ratio = filter == "ratio";
    if (method != "ransac8" && method != "7point-lmeds") { fprintf(stderr, "pm_cli: --method ransac8|7point-lmeds\n"); return 2; }
    const bool want_cross = filter == "cross" || filter == "cross-ratio";
    if (!want_ratio && !want_cross && filter != "midpoint") { fprintf(stderr, "pm_cli: --filter midpoint|ratio|cross|cross-ratio\n"); return 2; }
    if (want_cross && (matcher != "bf" || gpus > 1 || force_mgpu)) {
        fprintf(stderr, "pm_cli: --filter %s needs the brute-force matcher on a single GPU (no --matcher flann, --gpus N, --mgpu)\n", filter.c_str());
        return 2;
    }
    if (method == "ransac8" && !iters_given) iters = 10000;
    if ((gpus > 1 || force_mgpu) && (!want_ratio || method != "ransac8")) {
        fprintf(stderr, "pm_cli: --gpus N needs --filter ratio --method ransac8\n");
        return 2;
    }
    if (guided && (!(guided_tau > 0.f) || gpus > 1 || force_mgpu)) {
        fprintf(stderr, "pm_cli: --guided needs a positive threshold in pixels and a single GPU (no --gpus N, --mgpu)\n");
        return 2;
    }
    if (gpus < 1 || canvas_w < 1 || canvas_h < 1) { fprintf(stderr, "pm_cli: bad --gpus / --canvas\n"); return 2; }
    if (matcher != "bf" && matcher != "flann" && !track) { fprintf(stderr, "pm_cli: --matcher bf|flann|track\n"); return 2; }
    if (matcher == "flann" && (d1.dtype != 0 || gpus > 1 || force_mgpu)) {
        fprintf(stderr, "pm_cli: --matcher flann needs float32 descriptors and a single GPU\n");
        return 2;
    }

    using clk = std::chrono::steady_clock;
    pm_ctx* ctx = nullptr;
    pm_mgpu* mg = nullptr;
    int rc = PM_OK, est_rc = PM_OK;
    std::vector<pm_match> good(static_cast<size_t>(d1.rows) + 1);
    int n_good = 0, n_inl = 0, n_guided = 0, n_guided_inl = 0;
    std::vector<float> xy1, xy2;
    std::vector<uint8_t> mask(static_cast<size_t>(d1.rows) + 1);
    double F[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t key = 0;
    long long lmeds_model = -1;
    pm_ransac_params prm;
    prm.hyp_begin = 0; prm.hyp_end = iters; prm.seed = seed; prm.thresh_px = thresh; prm.error_kind = PM_ERR_SAMPSON;
    auto t0 = clk::now(), t1 = t0, t2 = t0, t3 = t0;
    auto gather_and_list = [&]() -> int {
        // ---- match list + index vectors + KeyPoint::convert                    main.cpp:71-79, 89-91
        std::vector<int32_t> qi(n_good), ti(n_good);
        xy1.assign(2 * static_cast<size_t>(n_good), 0.f);
        xy2.assign(2 * static_cast<size_t>(n_good), 0.f);
        int r = pm_match_indices(good.data(), n_good, qi.data(), ti.data());
        if (r == PM_OK) r = pm_gather_points(k1.f32(), k1.rows, qi.data(), n_good, xy1.data());
        if (r == PM_OK) r = pm_gather_points(k2.f32(), k2.rows, ti.data(), n_good, xy2.data());
        if (r != PM_OK) return r;
        if (!quiet) {
            const long need = pm_format_match_list(good.data(), n_good, nullptr, 0);
            std::string text(static_cast<size_t>(need) + 1, '\0');
            pm_format_match_list(good.data(), n_good, &text[0], text.size());
            fputs(text.c_str(), stdout);
        }
        return PM_OK;
    };
    if (gpus > 1 || force_mgpu) {
        // ---- the sharded form of main.cpp:46 .. :98 (query rows + hypothesis ids over `gpus` devices)
        rc = pm_mgpu_create(gpus, nullptr, &mg);
        if (rc != PM_OK) return fail("pm_mgpu_create", rc);
        t0 = clk::now();
        rc = pm_mgpu_match_ransac(mg, d1.data.data(), d1.rows, d2.data.data(), d2.rows, d1.cols, d1.dtype == 1, k1.f32(), k2.f32(),
                                  ratio, knn_flags, &prm, good.data(), &n_good, F, mask.data(), &n_inl, &key);
        if (rc != PM_OK && rc != PM_E_TOO_FEW && rc != PM_E_NO_MODEL) return fail("pm_mgpu_match_ransac", rc);
        est_rc = rc;
        t1 = t2 = t3 = clk::now();
        good.resize(n_good);
        const int r2 = gather_and_list();
        if (r2 != PM_OK) return fail("gather", r2);
    } else {
    if (feat_ctx) ctx = feat_ctx;
    else rc = pm_ctx_create(device, &ctx);
    if (rc != PM_OK) return fail("pm_ctx_create", rc);
    t0 = clk::now();

    if (track) {
        // ---- tracking in place of matcher + filter + gather: two pyramids, one track launch, one compaction
        pm_lk_params lk;
        lk.win_radius = lk_radius; lk.max_level = lk_levels; lk.max_iters = 30; lk.eps = 0.01f; lk.min_eig = 1e-4f;
        lk.fb_thresh = lk_fb; lk.flags = 0; lk.reserved = 0;
        pm_pyramid *py1 = nullptr, *py2 = nullptr;
        void *d_xy1 = nullptr, *d_xy2 = nullptr, *d_src = nullptr, *d_cnt = nullptr;
        const size_t rows = static_cast<size_t>(max_kp);
        int32_t cnt = 0;
        if (corner_pyr) { py1 = corner_pyr; corner_pyr = nullptr; }   // --points corners built it already
        else rc = pm_pyramid_create(ctx, img_w[0], img_h[0], lk_levels, &py1);
        const bool py1_built = rc == PM_OK && corner_points;
        if (rc == PM_OK) rc = pm_pyramid_create(ctx, img_w[1], img_h[1], lk_levels, &py2);
        if (rc == PM_OK) rc = pm_device_alloc(ctx, rows * 8, &d_xy1);
        if (rc == PM_OK) rc = pm_device_alloc(ctx, rows * 8, &d_xy2);
        if (rc == PM_OK) rc = pm_device_alloc(ctx, rows * 4, &d_src);
        if (rc == PM_OK) rc = pm_device_alloc(ctx, 4, &d_cnt);
        if (rc == PM_OK && !py1_built) rc = pm_pyramid_build_dev(ctx, py1, static_cast<const uint8_t*>(dev_img[0]), img_w[0]);
        if (rc == PM_OK) rc = pm_pyramid_build_dev(ctx, py2, static_cast<const uint8_t*>(dev_img[1]), img_w[1]);
        if (rc == PM_OK)
            rc = pm_track_lk_gather_dev(ctx, py1, py2, static_cast<const float*>(dev_kp[0]), static_cast<const int32_t*>(dev_n[0]), max_kp,
                                        nullptr, &lk, static_cast<float*>(d_xy1), static_cast<float*>(d_xy2), static_cast<int32_t*>(d_src),
                                        static_cast<int32_t*>(d_cnt), nullptr, nullptr);
        if (rc == PM_OK) rc = pm_device_download(ctx, &cnt, d_cnt, sizeof cnt);
        t1 = clk::now();
        std::vector<int32_t> src(static_cast<size_t>(cnt) + 1);
        n_good = cnt;
        xy1.assign(2 * static_cast<size_t>(n_good), 0.f);
        xy2.assign(2 * static_cast<size_t>(n_good), 0.f);
        if (rc == PM_OK) rc = pm_device_download(ctx, xy1.data(), d_xy1, xy1.size() * sizeof(float));
        if (rc == PM_OK) rc = pm_device_download(ctx, xy2.data(), d_xy2, xy2.size() * sizeof(float));
        if (rc == PM_OK) rc = pm_device_download(ctx, src.data(), d_src, static_cast<size_t>(cnt) * sizeof(int32_t));
        for (void* p : {d_xy1, d_xy2, d_src, d_cnt}) pm_device_free(ctx, p);
        pm_pyramid_destroy(py1);
        pm_pyramid_destroy(py2);
        if (rc != PM_OK) return fail("tracking", rc);
        good.resize(n_good);
        for (int i = 0; i < n_good; ++i) { good[i].queryIdx = src[i]; good[i].trainIdx = i; good[i].imgIdx = 0; good[i].distance = 0.f; }
        if (!quiet) {
            const long need = pm_format_match_list(good.data(), n_good, nullptr, 0);
            std::string text(static_cast<size_t>(need) + 1, '\0');
            pm_format_match_list(good.data(), n_good, &text[0], text.size());
            fputs(text.c_str(), stdout);
        }
        t2 = clk::now();
    } else {
    // ---- matcher.match(imageDesc1, imageDesc2, matchePoints, Mat())            main.cpp:42-46
    const int k = want_ratio ? 2 : 1;
    std::vector<pm_match> knn(static_cast<size_t>(d1.rows) * k);
    if (want_cross) {
        // matcher both ways + mutual-nearest-neighbour filter, one call (cv::BFMatcher(norm, crossCheck = true).match)
        const int cross_flags = filter == "cross-ratio" ? PM_CROSS_RATIO_FWD : 0;
        if (d1.dtype == 0)
            rc = pm_bf_match_cross_l2_f32(ctx, d1.f32(), d1.rows, d2.f32(), d2.rows, d1.cols, knn_flags, cross_flags, ratio,
                                          good.data(), &n_good);
        else
            rc = pm_bf_match_cross_hamming_u8(ctx, d1.data.data(), d1.rows, d2.data.data(), d2.rows, d1.cols, cross_flags, ratio,
                                              good.data(), &n_good);
    } else if (matcher == "flann") {
        pm_flann_params fp;
        fp.trees = 4; fp.checks = 32; fp.seed = seed;               // cv::flann defaults behind main.cpp:44
        pm_flann_index* ix = nullptr;
        rc = pm_flann_build(ctx, d2.f32(), d2.rows, d2.cols, &fp, &ix);
        if (rc == PM_OK) rc = pm_flann_knn_l2_f32(ctx, ix, d1.f32(), d1.rows, k, knn.data());
        pm_flann_destroy(ix);
    } else if (dev_u8[0] && dev_u8[1]) {
        // --features device: the descriptor bytes never left the GPU; same records as the float matcher (pm.h)
        void* d_knn = nullptr;
        rc = pm_device_alloc(ctx, knn.size() * sizeof(pm_match), &d_knn);
        if (rc == PM_OK && want_bits)
            rc = pm_bf_knn_hamming_u8_dev(ctx, static_cast<const uint8_t*>(dev_u8[0]), d1.rows, static_cast<const uint8_t*>(dev_u8[1]),
                                          d2.rows, 32, k, static_cast<pm_match*>(d_knn));
        else if (rc == PM_OK)
            rc = pm_bf_knn_l2_u8_dev(ctx, static_cast<const uint8_t*>(dev_u8[0]), d1.rows, static_cast<const uint8_t*>(dev_u8[1]), d2.rows,
                                     128, k, static_cast<pm_match*>(d_knn));
        if (rc == PM_OK) rc = pm_device_download(ctx, knn.data(), d_knn, knn.size() * sizeof(pm_match));
        pm_device_free(ctx, d_knn);
    } else if (d1.dtype == 0)
        rc = pm_bf_knn_l2_f32(ctx, d1.f32(), d1.rows, d2.f32(), d2.rows, d1.cols, k, knn_flags, knn.data());
    else
        rc = pm_bf_knn_hamming_u8(ctx, d1.data.data(), d1.rows, d2.data.data(), d2.rows, d1.cols, k, knn.data());
    if (rc != PM_OK) return fail("matcher", rc);
    t1 = clk::now();

    // ---- selecting strong features                                             main.cpp:48-69
    if (want_cross) {
        // the survivors came out of the one-call form above
    } else if (want_ratio) {
        rc = pm_filter_ratio(knn.data(), d1.rows, k, ratio, good.data(), &n_good);
    } else {
        // OpenCV drops queries without a neighbour (empty train set): keep only matched rows
        std::vector<pm_match> matched;
        for (const pm_match& m : knn) if (m.trainIdx >= 0) matched.push_back(m);
        double lo = 0, hi = 0;
        rc = pm_filter_midpoint(matched.data(), static_cast<int>(matched.size()), &lo, &hi, good.data(), &n_good);
        if (rc == PM_OK && !quiet) {
            // main.cpp:58-59; the full-width colon of the source is not representable in the
            // reference's code page and its binary prints '?' 
            std::cout << "The Best Match is? " << lo << std::endl;
            std::cout << "The Worst Match is? " << hi << std::endl;
        }
    }
    if (rc != PM_OK) return fail("filter", rc);
    good.resize(n_good);
    rc = gather_and_list();
    if (rc != PM_OK) return fail("gather", rc);
    t2 = clk::now();
    }

    if (align) {
        // ---- the 2-D model and the warp in place of the F estimator and its report
        const int arc = run_align(ctx, align_model, align_pgm, img1_path, img2_path, xy1, xy2, n_good, prm);
        if (feat_ctx == ctx) ctx = nullptr;
        free_device_features();
        pm_ctx_destroy(ctx);
        return arc;
    }
    // ---- cv::findFundamentalMat(...)                                           main.cpp:94-98
    if (method == "7point-lmeds") {
        pm_lmeds_params lp;
        lp.hyp_begin = 0; lp.hyp_end = iters_given ? iters : pm_lmeds_default_iters(0.99, 0.45); lp.seed = seed;
        int64_t best_model = -1;
        double median = 0;
        rc = pm_lmeds_fundamental(ctx, xy1.data(), xy2.data(), n_good, &lp, F, mask.data(), &n_inl, &best_model, &median);
        lmeds_model = best_model;
        if (rc != PM_OK && rc != PM_E_TOO_FEW && rc != PM_E_NO_MODEL) return fail("pm_lmeds_fundamental", rc);
    } else {
        rc = pm_ransac_fundamental(ctx, xy1.data(), xy2.data(), n_good, &prm, F, mask.data(), &n_inl, &key);
        if (rc != PM_OK && rc != PM_E_TOO_FEW && rc != PM_E_NO_MODEL) return fail("pm_ransac_fundamental", rc);
    }
    est_rc = rc;                             // the estimator's own status (PM_E_TOO_FEW / PM_E_NO_MODEL are results, not failures)
    t3 = clk::now();

    // ---- guided matching with that F (unit scale, as estimated), then RANSAC-F on its survivors      SPEC S48-S50
    if (guided) {
        std::vector<pm_match> knn2(static_cast<size_t>(d1.rows) * 2), good2(static_cast<size_t>(d1.rows) + 1);
        if (d1.dtype == 0)
            rc = pm_bf_knn_guided_l2_f32(ctx, d1.f32(), d1.rows, d2.f32(), d2.rows, d1.cols, k1.f32(), k2.f32(), PM_GUIDE_F_SAMPSON,
                                         F, guided_tau, 2, knn2.data(), nullptr);
        else
            rc = pm_bf_knn_guided_hamming_u8(ctx, d1.data.data(), d1.rows, d2.data.data(), d2.rows, d1.cols, k1.f32(), k2.f32(),
                                             PM_GUIDE_F_SAMPSON, F, guided_tau, 2, knn2.data(), nullptr);
        if (rc != PM_OK) return fail("guided matcher", rc);
        rc = pm_filter_ratio(knn2.data(), d1.rows, 2, ratio, good2.data(), &n_guided);
        if (rc != PM_OK) return fail("guided filter", rc);
        std::vector<int32_t> qi(n_guided), ti(n_guided);
        std::vector<float> gxy1(2 * static_cast<size_t>(n_guided) + 2), gxy2(2 * static_cast<size_t>(n_guided) + 2);
        rc = pm_match_indices(good2.data(), n_guided, qi.data(), ti.data());
        if (rc == PM_OK) rc = pm_gather_points(k1.f32(), k1.rows, qi.data(), n_guided, gxy1.data());
        if (rc == PM_OK) rc = pm_gather_points(k2.f32(), k2.rows, ti.data(), n_guided, gxy2.data());
        if (rc != PM_OK) return fail("guided gather", rc);
        double F2[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        std::vector<uint8_t> mask2(static_cast<size_t>(n_guided) + 1);
        uint64_t key2 = 0;
        rc = pm_ransac_fundamental(ctx, gxy1.data(), gxy2.data(), n_guided, &prm, F2, mask2.data(), &n_guided_inl, &key2);
        if (rc != PM_OK && rc != PM_E_TOO_FEW && rc != PM_E_NO_MODEL) return fail("pm_ransac_fundamental (guided)", rc);
        if (rc != PM_OK) n_guided_inl = 0;
    }
    }
    // like cv::findFundamentalMat, a failed estimate yields the zero matrix
    if (fscale == "opencv") pm_f_scale_f33(F);

    // ---- residual report, the reference's x1^T F x2 form                       main.cpp:101-123
    std::vector<double> res(static_cast<size_t>(n_good) + 1);
    double mean_abs = 0;
    rc = pm_epipolar_residuals(xy1.data(), xy2.data(), n_good, F, /*transposed=*/1, res.data(), &mean_abs);
    if (rc != PM_OK) return fail("pm_epipolar_residuals", rc);
    if (!quiet) {
        for (int i = 0; i < n_good; ++i) std::cout << "result = " << i << " " << res[i] << std::endl;   // :119
        std::cout << "The average value is  " << mean_abs << std::endl;                                 // :123
    }
    // ---- computeCorrespondEpilines(selPoints1, 1, F, lines1) + the end points of cv::line      main.cpp:127-142
    if (print_epi || !epi_ppm.empty()) {
        int cols = canvas_w, rows_ = canvas_h;
        std::vector<unsigned char> gray;
        if (!img2_path.empty() && !load_pgm(img2_path, gray, cols, rows_)) return 1;
        std::vector<float> lines(3 * static_cast<size_t>(n_good) + 3);
        std::vector<int32_t> ends(4 * static_cast<size_t>(n_good) + 4);
        rc = pm_epilines(xy1.data(), n_good, 1, F, lines.data());
        if (rc == PM_OK) rc = pm_epiline_endpoints(lines.data(), n_good, cols, ends.data());
        if (rc != PM_OK) return fail("pm_epilines", rc);
        if (print_epi)
            for (int i = 0; i < n_good; ++i)
                printf("epiline = %d %g %g %g  (%d, %d) -> (%d, %d)\n", i, lines[3 * i], lines[3 * i + 1], lines[3 * i + 2],
                       ends[4 * i], ends[4 * i + 1], ends[4 * i + 2], ends[4 * i + 3]);
        if (!epi_ppm.empty() && !write_epiline_ppm(epi_ppm, gray, cols, rows_, ends, n_good)) return 1;
    }
    if (guided)
        printf("guided matching: tau = %g px, matches %d -> %d, inliers %d -> %d\n", guided_tau, n_good, n_guided, n_inl,
               n_guided_inl);
    if (json) {
        auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        double mean_fwd = 0;
        pm_epipolar_residuals(xy1.data(), xy2.data(), n_good, F, 0, nullptr, &mean_fwd);
        printf("{\"n1\": %d, \"n2\": %d, \"dim\": %d, \"matches\": %d, \"inliers\": %d, \"best_hyp\": %lld, "
               "\"ransac_status\": %d, \"mean_abs_x1Fx2\": %.17g, \"mean_abs_x2Fx1\": %.17g, "
               "\"ms\": {\"match\": %.3f, \"filter_gather\": %.3f, \"ransac\": %.3f}, "
               "\"F\": [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g, %.17g, %.17g, %.17g]}\n",
               d1.rows, d2.rows, d1.cols, n_good, n_inl,
               method == "7point-lmeds" ? lmeds_model : static_cast<long long>(key ? pm_ransac_key_hyp(key) : 0u), est_rc,
               mean_abs, mean_fwd, ms(t0, t1), ms(t1, t2), ms(t2, t3), F[0], F[1], F[2], F[3], F[4], F[5], F[6],
               F[7], F[8]);
    }
    if (feat_ctx == ctx) ctx = nullptr;                // one context: destroyed with the feature buffers
    free_device_features();
    pm_ctx_destroy(ctx);
    pm_mgpu_destroy(mg);
    return 0;
}
