// features.hip — the device feature front end (docs/SPEC.md S53-S57): difference-of-Gaussian keypoints and 128-D gradient
// descriptors from 8-bit grey pixels.  Slot in the reference: main.cpp:22-26, :36-40.  A port of host/pm_features.cpp, which
// is the specification: every sum below repeats the host's order, the tables come from the host's own expressions, and the
// only calls whose last bit may differ from glibc are atan2f and the fp64 exp of the descriptor weight.
//
// Launches of one call, all on the context's stream:
//   feat_blur      one per Gaussian level: input tile + halo to LDS, y pass, the plane in between rounded to float, x pass
//   feat_decimate  one per octave after the first
//   feat_extrema   one per octave: the three inner DoG levels, survivors appended through an atomic counter
//   feat_rank      rank by counting over the 64-bit keys (~|response| bits, scan position): the first max_kp are kept
//   feat_describe  one workgroup per kept keypoint: orientation histogram, 4x4x8 descriptor, ordered fp64 sums
//   feat_compact   one workgroup: exclusive scan of the row flags, the count (or -1 when the candidate buffer overflowed)
//   feat_gather    rows to their final places
// The binary form (S58-S60, pm_detect_describe_bits*) runs feat_describe_bits and feat_gather_bits in place of feat_describe
// and feat_gather: the same orientation, then 256 pixel comparisons at offsets from a table steered to the orientation bin.
// Every kernel reads the candidate counter itself: nothing of the call depends on a host round trip.
#include <algorithm>
#include <cmath>

#include "pm_common.hpp"
#include "wave_ops.hpp"

namespace {

constexpr int NLEV = 6;            // S + 3 Gaussian levels per octave, S = 3
constexpr int MAXR = 12;           // largest tap radius (4 sigma of the last level increment)
constexpr int NTAP = 2 * MAXR + 1;
constexpr int ORI_N = 393;         // dx^2 + dy^2 <= 2 * 14^2
constexpr int MAX_OCT = 16;
constexpr double PI_ = 3.14159265358979323846;

struct FeatTables {
    double taps[NLEV][NTAP];       // [0]: base blur of octave 0, [1..5]: level increments
    double ori_w[3][ORI_N];        // exp(-(dx^2 + dy^2) / (2 (1.5 sigma)^2)) per inner level
    double cs[36], sn[36], theta[36];
    double sig[3], cell[3];
    int tap_r[NLEV];
    int rad[3], r2[3];
};

struct OctTable {
    unsigned long long off[MAX_OCT];   // first float of the octave's six planes
    int w[MAX_OCT], h[MAX_OCT];
    int n;
};

// Exactly the expressions of host/pm_features.cpp (gaussian(), the scale-space loop, the orientation and descriptor set-up).
void fill_taps(double sigma, double* k, int* r_out)
{
    const int r = static_cast<int>(4.0 * sigma + 0.5);
    double sum = 0;
    for (int i = -r; i <= r; ++i) { k[i + r] = std::exp(-0.5 * i * i / (sigma * sigma)); sum += k[i + r]; }
    for (int i = 0; i < 2 * r + 1; ++i) k[i] /= sum;
    *r_out = r;
}

const FeatTables& tables()
{
    static const FeatTables t = [] {
        FeatTables f;
        memset(&f, 0, sizeof f);
        constexpr int S = 3;
        constexpr double SIGMA0 = 1.6;
        const double kf = std::pow(2.0, 1.0 / S);
        fill_taps(std::sqrt(std::max(SIGMA0 * SIGMA0 - 0.25, 0.01)), f.taps[0], &f.tap_r[0]);
        for (int i = 1; i < S + 3; ++i) {
            const double sp = SIGMA0 * std::pow(kf, i - 1), st = sp * kf;
            fill_taps(std::sqrt(st * st - sp * sp), f.taps[i], &f.tap_r[i]);
        }
        for (int lev = 1; lev <= S; ++lev) {
            const double sig = SIGMA0 * std::pow(kf, lev);
            const int rad = static_cast<int>(std::nearbyint(3 * 1.5 * sig));
            f.sig[lev - 1] = sig;
            f.rad[lev - 1] = rad;
            for (int d2 = 0; d2 <= 2 * rad * rad && d2 < ORI_N; ++d2) f.ori_w[lev - 1][d2] = std::exp(-d2 / (2 * (1.5 * sig) * (1.5 * sig)));
            const double cell = 3.0 * sig;
            f.cell[lev - 1] = cell;
            f.r2[lev - 1] = static_cast<int>(std::ceil(cell * 2.5 * std::sqrt(2.0))) + 1;
        }
        for (int b = 0; b < 36; ++b) {
            const double theta = (b + 0.5) / 36 * 2 * PI_ - PI_;
            f.theta[b] = theta;
            f.cs[b] = std::cos(theta);
            f.sn[b] = std::sin(theta);
        }
        return f;
    }();
    return t;
}

// ---- S58 / S59: the 256 lattice tests and their offsets steered to the 36 bins and scaled to the three inner levels
constexpr int NBITS = 256;
struct BitsTables {
    int8_t base[NBITS][4];             // x1, y1, x2, y2
    int8_t steer[3][36][NBITS][4];     // dx1, dy1, dx2, dy2
};
constexpr size_t STEER_BYTES = sizeof(int8_t) * 3 * 36 * NBITS * 4;
constexpr size_t STEER_OFF = (sizeof(FeatTables) + 255) / 256 * 256;      // behind FeatTables in the feature buffer

const BitsTables& bits_tables()
{
    static const BitsTables t = [] {
        BitsTables b;
        memset(&b, 0, sizeof b);
        // splitmix64; a coordinate is the sum of three draws in -5 .. 5.  host/pm_features.cpp (bits_pattern) holds the second
        // C++ statement of this construction, on purpose: the host extractor is the specification and does not call into this
        // library.  tests/test_features_bits_cpu.py pins both against the numpy statement (this one through
        // pm_detect_bits_table, the host's through the rows of `pm_cli --descriptor bits`).
        unsigned long long state = 0x504D4249545331ULL;
        auto coord = [&]() {
            int v = 0;
            for (int k = 0; k < 3; ++k) {
                state += 0x9E3779B97F4A7C15ULL;
                unsigned long long z = state;
                z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
                z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
                z ^= z >> 31;
                v += static_cast<int>((z >> 33) % 11) - 5;
            }
            return v;
        };
        for (int n = 0; n < NBITS;) {
            const int c[4] = {coord(), coord(), coord(), coord()};          // braces: evaluated left to right
            if (c[0] * c[0] + c[1] * c[1] > 225 || c[2] * c[2] + c[3] * c[3] > 225) continue;
            if (c[0] == c[2] && c[1] == c[3]) continue;
            bool seen = false;
            for (int i = 0; i < n && !seen; ++i) {
                const int8_t* o = b.base[i];
                seen = (o[0] == c[0] && o[1] == c[1] && o[2] == c[2] && o[3] == c[3]) ||
                       (o[0] == c[2] && o[1] == c[3] && o[2] == c[0] && o[3] == c[1]);
            }
            if (seen) continue;
            for (int j = 0; j < 4; ++j) b.base[n][j] = static_cast<int8_t>(c[j]);
            ++n;
        }
        const FeatTables& f = tables();
        for (int l = 0; l < 3; ++l) {
            const double s = f.r2[l] / 15.0;
            for (int k = 0; k < 36; ++k)
                for (int i = 0; i < NBITS; ++i)
                    for (int p = 0; p < 4; p += 2) {
                        const double x = b.base[i][p], y = b.base[i][p + 1];
                        b.steer[l][k][i][p] = static_cast<int8_t>(std::nearbyint(s * (f.cs[k] * x - f.sn[k] * y)));
                        b.steer[l][k][i][p + 1] = static_cast<int8_t>(std::nearbyint(s * (f.sn[k] * x + f.cs[k] * y)));
                    }
        }
        return b;
    }();
    return t;
}

__device__ __forceinline__ int reflect_idx(int i, int n)
{
    while (i < 0 || i >= n) i = i < 0 ? -i - 1 : 2 * n - 1 - i;
    return i;
}

// ---- S53: one Gaussian level.  The input tile with its halo goes to LDS first (reflected at the borders, u8 pixels
// divided by 255 on the way), then the y pass (fp64 sum over ascending taps, rounded to float) into a second tile that
// keeps the x halo, then the x pass from that tile.  A tile column holds the value of the REFLECTED image column, so the x
// pass reads s_tmp[tx + i + r] where the host reads tmp(y, reflect(x + i)).
constexpr int BT_X = 64, BT_Y = 8;
template <bool U8>
__global__ __launch_bounds__(256) void feat_blur(const void* in_, int in_stride, float* out, int w, int h, const FeatTables* tab,
                                                 int which)
{
    __shared__ float s_in[BT_Y + 2 * MAXR][BT_X + 2 * MAXR];
    __shared__ float s_tmp[BT_Y][BT_X + 2 * MAXR];
    __shared__ double s_k[NTAP];
    const int tid = threadIdx.x;
    const int r = tab->tap_r[which];
    if (tid < 2 * r + 1) s_k[tid] = tab->taps[which][tid];
    const int x0 = blockIdx.x * BT_X, y0 = blockIdx.y * BT_Y;
    const int cols = BT_X + 2 * r, rows = BT_Y + 2 * r;
    const unsigned char* in8 = static_cast<const unsigned char*>(in_);
    const float* inf = static_cast<const float*>(in_);
    for (int e = tid; e < rows * cols; e += 256) {
        const int jy = e / cols, jx = e - jy * cols;
        const size_t ys = static_cast<size_t>(reflect_idx(y0 - r + jy, h));
        const int xs = reflect_idx(x0 - r + jx, w);
        s_in[jy][jx] = U8 ? static_cast<float>(in8[ys * in_stride + xs]) / 255.0f : inf[ys * w + xs];
    }
    __syncthreads();
    for (int e = tid; e < BT_Y * cols; e += 256) {
        const int ty = e / cols, j = e - ty * cols;
        float res = 0.f;
        if (y0 + ty < h) {
            double a = 0;
            for (int i = -r; i <= r; ++i) a += s_k[i + r] * s_in[ty + i + r][j];
            res = static_cast<float>(a);
        }
        s_tmp[ty][j] = res;
    }
    __syncthreads();
    for (int e = tid; e < BT_Y * BT_X; e += 256) {
        const int ty = e / BT_X, tx = e % BT_X;
        const int x = x0 + tx, y = y0 + ty;
        if (x < w && y < h) {
            double a = 0;
            for (int i = -r; i <= r; ++i) a += s_k[i + r] * s_tmp[ty][tx + i + r];
            out[static_cast<size_t>(y) * w + x] = static_cast<float>(a);
        }
    }
}

__global__ __launch_bounds__(256) void feat_decimate(const float* src, int sw, float* dst, int dw, int dh)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x < dw && y < dh) dst[static_cast<size_t>(y) * dw + x] = src[static_cast<size_t>(2 * y) * sw + 2 * x];
}

// ---- S54: DoG extrema of one octave, levels 1..3 (blockIdx.z).  Float arithmetic in the host's order.
__global__ __launch_bounds__(256) void feat_extrema(const float* L, int w, int h, int oct, unsigned pos_base, float thr, float edge_r,
                                                    unsigned long long oct_off, unsigned* counter, unsigned cap,
                                                    unsigned long long* keys, int4* info, int4* geom)
{
    const int x = 8 + blockIdx.x * 64 + (threadIdx.x & 63), y = 8 + blockIdx.y * 4 + (threadIdx.x >> 6);
    const int lev = 1 + blockIdx.z;
    if (x >= w - 8 || y >= h - 8) return;
    const size_t plane = static_cast<size_t>(w) * h;
    auto dog = [&](int l, int yy, int xx) {
        const size_t p = static_cast<size_t>(yy) * w + xx;
        return L[(l + 1) * plane + p] - L[l * plane + p];
    };
    const float c = dog(lev, y, x);
    if (!(fabsf(c) > thr)) return;
    bool is_max = true, is_min = true;
    for (int di = -1; di <= 1; ++di)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const float v = dog(lev + di, y + dy, x + dx);
                if (v > c) is_max = false;
                if (v < c) is_min = false;
            }
    if (!is_max && !is_min) return;
    const float dxx = dog(lev, y, x + 1) + dog(lev, y, x - 1) - 2 * c;
    const float dyy = dog(lev, y + 1, x) + dog(lev, y - 1, x) - 2 * c;
    const float dxy = (dog(lev, y + 1, x + 1) - dog(lev, y + 1, x - 1) - dog(lev, y - 1, x + 1) + dog(lev, y - 1, x - 1)) / 4.0f;
    const float tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
    if (det <= 0 || tr * tr * edge_r >= (edge_r + 1) * (edge_r + 1) * det) return;
    const unsigned slot = atomicAdd(counter, 1u);          // keeps counting past the capacity: the host reads the need
    if (slot >= cap) return;
    const unsigned pos = pos_base + static_cast<unsigned>((static_cast<size_t>(lev - 1) * h + y) * w + x);   // the host's scan order
    keys[slot] = (static_cast<unsigned long long>(~__float_as_uint(fabsf(c))) << 32) | pos;
    info[slot] = make_int4(oct, lev, y, x);
    geom[slot] = make_int4(w, h, static_cast<int>(oct_off & 0xFFFFFFFFull), static_cast<int>(oct_off >> 32));   // the octave's planes
}

// ---- S55: selection.  Keys are distinct; ascending key order = |response| descending, then the host's scan order, which is
// what std::stable_sort leaves.  rank = number of smaller keys; the first max_kp ranks are kept.
__global__ __launch_bounds__(256) void feat_rank(const unsigned* counter, unsigned cap, int max_kp, const unsigned long long* keys, int* sel)
{
    __shared__ unsigned long long s_key[256];
    const unsigned cnt = *counter;
    if (cnt > cap) return;
    const unsigned n = cnt;
    if (blockIdx.x * 256u >= n) return;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    const unsigned long long mine = t < n ? keys[t] : 0ull;
    const unsigned rank = pm::rank_below(keys, n, mine, s_key);
    if (t < n && rank < static_cast<unsigned>(max_kp)) sel[rank] = static_cast<int>(t);
}

// The orientation histogram of S56, shared by feat_describe and feat_describe_bits (NT threads): per-pixel records into LDS,
// the lane that owns a bin walks them serially in fp64, lane 0 takes the arg-max of the smoothed histogram.  Leaves theta,
// cos and sin of the dominant bin in s_par[0 .. 2] and its index in *s_bin (where asked for); ends with a barrier.
template <int NT>
__device__ __forceinline__ void feat_orientation(const float* L, int w, int x, int y, int rad, int lev, const FeatTables* tab, int tid,
                                                 double* s_rec, int* s_key, double* s_hist, double* s_par, int* s_bin)
{
    auto at = [&](int yy, int xx) { return L[static_cast<size_t>(yy) * w + xx]; };
    const int side = 2 * rad + 1, npx = side * side;          // <= 841
    const int npx4 = (npx + 3) & ~3;
    for (int p = tid; p < npx4; p += NT) {
        if (p < npx) {
            const int dy = p / side - rad, dx = p % side - rad;
            const float gx = (at(y + dy, x + dx + 1) - at(y + dy, x + dx - 1)) * 0.5f;
            const float gy = (at(y + dy + 1, x + dx) - at(y + dy - 1, x + dx)) * 0.5f;
            const float mag = sqrtf(gx * gx + gy * gy);
            const float ang = atan2f(gy, gx);
            s_rec[p] = tab->ori_w[lev][dx * dx + dy * dy] * mag;
            s_key[p] = static_cast<int>((ang + PI_) / (2 * PI_) * 36) % 36;
        } else {
            s_rec[p] = 0;
            s_key[p] = -1;
        }
    }
    __syncthreads();
    if (tid < 36) {
        double acc = 0;
        const int4* k4 = reinterpret_cast<const int4*>(s_key);
        const double2* m2 = reinterpret_cast<const double2*>(s_rec);
        for (int p4 = 0; p4 < npx4 / 4; ++p4) {
            const int4 k = k4[p4];
            const double2 lo = m2[2 * p4], hi = m2[2 * p4 + 1];
            acc += k.x == tid ? lo.x : 0.0;
            acc += k.y == tid ? lo.y : 0.0;
            acc += k.z == tid ? hi.x : 0.0;
            acc += k.w == tid ? hi.y : 0.0;
        }
        s_hist[tid] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        int best = 0;
        double sm_best = (s_hist[35] + s_hist[0] + s_hist[1]) / 3.0;
        for (int b = 1; b < 36; ++b) {
            const double sm = (s_hist[(b + 35) % 36] + s_hist[b] + s_hist[(b + 1) % 36]) / 3.0;
            if (sm > sm_best) { sm_best = sm; best = b; }
        }
        s_par[0] = tab->theta[best];
        s_par[1] = tab->cs[best];
        s_par[2] = tab->sn[best];
        if (s_bin) *s_bin = best;
    }
    __syncthreads();
}

// ---- S56: orientation and descriptor of one keypoint per workgroup of eight waves.  Every histogram bin and every one of
// the 128 accumulators is an fp64 sum over pixels in (dy, dx) order: the workgroup writes per-pixel records into LDS, then
// the lane that owns a bin walks the records serially and adds what lands in its bin.  No floating-point atomics.
// Descriptor bins: wave k owns the 16 accumulators of row vi = k >> 1, columns ui = 2 (k & 1) and 2 (k & 1) + 1 (lanes
// 0 .. 15).  A chunk of DCH pixels is one pixel per thread; the pixels that touch wave k's cells are compacted, in pixel
// order, into list k (ballot prefix inside a wave, wave totals through LDS), and wave k walks its list only.  A lane adds
// the pixel's product for its bin (the eight products of a pixel are computed by the pixel's thread, in the host's
// operation order) and +0 where the pixel misses the bin: the sums are >= +0, so +0 changes no bit.
constexpr int DCH = 512;           // pixels per LDS chunk = threads (the largest patch has 71 x 71 pixels)
constexpr int DTHREADS = 512;
constexpr int ORI_MAX = 844;       // 29 x 29 orientation pixels, padded to a multiple of 4
__global__ __launch_bounds__(DTHREADS) void feat_describe(const float* pyr, const FeatTables* tab, const unsigned* counter, unsigned cap,
                                                          int max_kp, const unsigned long long* keys, const int4* info, const int4* geom,
                                                          const int* sel, float* kp_tmp, unsigned char* desc_tmp, float* meta_tmp,
                                                          int* valid)
{
    // descriptor: the eight trilinear products of each pixel of the chunk, index a1 * 4 + b1 * 2 + e1 (8 x DCH); orientation:
    // the weights (ORI_MAX)
    __shared__ __attribute__((aligned(16))) double s_rec[8 * DCH];
    __shared__ __attribute__((aligned(16))) int s_key[ORI_MAX];           // orientation: bin, -1 in the padding
    // list k: o0 | (u0 + 1) << 4 | (v0 + 1) << 8 | pixel << 16 of the chunk's pixels that touch wave k, in pixel order
    __shared__ __attribute__((aligned(16))) int s_list[8][DCH];
    __shared__ int s_cnt[8][8];                                           // [list][source wave]
    __shared__ __attribute__((aligned(16))) double s_desc[128], s_sq[128];
    __shared__ double s_hist[36];
    __shared__ double s_norm[2];
    __shared__ double s_par[3];                                           // theta, cos, sin of the dominant bin
    const unsigned cnt = *counter;
    if (cnt > cap) return;
    const int n_sel = min(static_cast<int>(cnt), max_kp);
    const int row = blockIdx.x;
    if (row >= n_sel) return;
    const int tid = threadIdx.x;
    // The keypoint's record is the same for every lane; its index is moved into a vector register on purpose.  Read as a
    // scalar, the record and everything derived from it (geometry, radii, loop bounds) compete with the constants of the fp64
    // exp and fmod of the pixel loop for the scalar registers.  Compiler report of this kernel (hipcc of ROCm 7, build.py's
    // flags): plain `sel[row]` 13 scalar-register spills, 101 VGPRs; the index passed through LDS instead 4 spills, 71 VGPRs;
    // this move 0 spills, 90 VGPRs.  build.py prints this file's report on every compile: a later compiler that spills
    // here again shows up there.
    int ci;
    asm volatile("v_mov_b32 %0, %1" : "=v"(ci) : "s"(sel[row]));
    const int4 c4 = info[ci];
    const int o = c4.x, lev = c4.y - 1, y = c4.z, x = c4.w;
    const int4 g4 = geom[ci];
    const int w = g4.x, h = g4.y;
    const float* L = pyr + ((static_cast<unsigned long long>(static_cast<unsigned>(g4.w)) << 32) | static_cast<unsigned>(g4.z)) +
                     static_cast<size_t>(c4.y) * w * h;
    const int rad = tab->rad[lev], r2 = tab->r2[lev];
    if (y - rad < 1 || x - rad < 1 || y + rad >= h - 1 || x + rad >= w - 1 || y - r2 < 1 || x - r2 < 1 || y + r2 >= h - 1 || x + r2 >= w - 1) {
        if (tid == 0) valid[row] = 0;
        return;
    }
    auto at = [&](int yy, int xx) { return L[static_cast<size_t>(yy) * w + xx]; };

    feat_orientation<DTHREADS>(L, w, x, y, rad, lev, tab, tid, s_rec, s_key, s_hist, s_par, nullptr);
    const double theta = s_par[0], cs = s_par[1], sn = s_par[2], cell = tab->cell[lev];

    // 4 x 4 x 8 descriptor
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int my_v1 = (wave >> 1) + 1, my_u1 = 2 * (wave & 1) + ((lane >> 3) & 1) + 1, my_o = lane & 7;
    const bool owner = lane < 16;
    constexpr int NO_BIN = 15 << 8;                               // v0 + 1 = 15: matches no lane (list padding)
    double acc = 0;
    const int side = 2 * r2 + 1, npx = side * side;
    for (int c0 = 0; c0 < npx; c0 += DCH) {
        __syncthreads();                                          // the walk of the chunk before is over
        int key = 0, waves = 0;
        const int p = c0 + tid;
        if (p < npx) {
            const int dy = p / side - r2, dx = p % side - r2;
            const double u = (cs * dx + sn * dy) / cell + 1.5;
            const double v = (-sn * dx + cs * dy) / cell + 1.5;
            if (u > -1 && u < 4 && v > -1 && v < 4) {
                const float gx = (at(y + dy, x + dx + 1) - at(y + dy, x + dx - 1)) * 0.5f;
                const float gy = (at(y + dy + 1, x + dx) - at(y + dy - 1, x + dx)) * 0.5f;
                const double mag = sqrtf(gx * gx + gy * gy) * exp(-((u - 1.5) * (u - 1.5) + (v - 1.5) * (v - 1.5)) / (2 * 2.0 * 2.0));
                double a = fmod(atan2f(gy, gx) - theta, 2 * PI_);
                if (a < 0) a += 2 * PI_;
                const double ob = a / (2 * PI_) * 8;
                const int u0 = static_cast<int>(floor(u)), v0 = static_cast<int>(floor(v)), o0 = static_cast<int>(floor(ob));
                const double du = u - u0, dv = v - v0, dob = ob - o0;
#pragma unroll
                for (int a1 = 0; a1 < 2; ++a1)
#pragma unroll
                    for (int b1 = 0; b1 < 2; ++b1) {
                        const double t = mag * (a1 ? dv : 1 - dv) * (b1 ? du : 1 - du);       // the host's order: ((mag * v) * u) * o
                        s_rec[tid * 8 + a1 * 4 + b1 * 2] = t * (1 - dob);
                        s_rec[tid * 8 + a1 * 4 + b1 * 2 + 1] = t * dob;
                    }
                for (int vi = max(v0, 0); vi <= min(v0 + 1, 3); ++vi)       // v0, u0 in -1 .. 3, o0 in 0 .. 8
                    for (int ui = max(u0, 0); ui <= min(u0 + 1, 3); ++ui) waves |= 1 << (vi * 2 + (ui >> 1));
                key = o0 | ((u0 + 1) << 4) | ((v0 + 1) << 8) | (tid << 16);
            }
        }
        unsigned long long before = 0;                            // byte t: lower lanes of this wave that go to list t
#pragma unroll 1
        for (int t = 0; t < 8; ++t) {
            const unsigned long long bal = __ballot((waves >> t) & 1);
            before |= static_cast<unsigned long long>(pm::lane_rank(bal, lane)) << (8 * t);
            if (lane == 0) s_cnt[t][wave] = __popcll(bal);
        }
        __syncthreads();
#pragma unroll 1
        for (int t = 0; t < 8; ++t) {
            if (!((waves >> t) & 1)) continue;
            int off = static_cast<int>((before >> (8 * t)) & 255);
            for (int k = 0; k < wave; ++k) off += s_cnt[t][k];
            s_list[t][off] = key;
        }
        int n = 0;
        for (int k = 0; k < 8; ++k) n += s_cnt[wave][k];
        n = __builtin_amdgcn_readfirstlane(n);
        const int n4 = (n + 3) & ~3;
        __syncthreads();                                          // lists and records are complete
        if (lane < n4 - n) s_list[wave][n + lane] = NO_BIN;       // own list, own padding (index < DCH: DCH % 4 == 0)
        const int4* l4 = reinterpret_cast<const int4*>(s_list[wave]);
        for (int i4 = 0; i4 < n4 / 4; ++i4) {
            const int4 e4 = l4[i4];
            const int es[4] = {e4.x, e4.y, e4.z, e4.w};
            double term[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = es[j], q = (e >> 16) & (DCH - 1);
                const int a1 = my_v1 - ((e >> 8) & 15), b1 = my_u1 - ((e >> 4) & 15), e1 = (my_o - (e & 15)) & 7;
                const bool hit = owner && !((a1 | b1 | e1) & ~1);  // each of the three is 0 or 1, or the pixel misses this bin
                const double t = s_rec[q * 8 + (hit ? a1 * 4 + b1 * 2 + e1 : 0)];
                term[j] = hit ? t : 0.0;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += term[j];
        }
    }
    if (owner) s_desc[((my_v1 - 1) * 4 + (my_u1 - 1)) * 8 + my_o] = acc;
    __syncthreads();
    // norm, clip at 0.2, norm again: the squares in parallel, the two sums by one lane in index order
    auto ordered_sum = [&]() {
        double t = 0;
        const double2* s2 = reinterpret_cast<const double2*>(s_sq);
#pragma unroll 8
        for (int i = 0; i < 64; ++i) {
            const double2 v = s2[i];
            t += v.x;
            t += v.y;
        }
        return t;
    };
    const double d = tid < 128 ? s_desc[tid] : 0.0;
    if (tid < 128) s_sq[tid] = d * d;
    __syncthreads();
    if (tid == 0) s_norm[0] = sqrt(ordered_sum());
    __syncthreads();
    const double nrm = s_norm[0];
    if (nrm < 1e-9) {
        if (tid == 0) valid[row] = 0;
        return;
    }
    const double t = d / nrm;
    const double cl = 0.2 < t ? 0.2 : t;
    if (tid < 128) s_sq[tid] = cl * cl;
    __syncthreads();
    if (tid == 0) s_norm[1] = sqrt(ordered_sum());
    __syncthreads();
    const double n2 = s_norm[1];
    if (tid < 128) {
        double qv = nearbyint(cl / n2 * 512);
        qv = qv < 0 ? 0 : (qv > 255 ? 255 : qv);
        desc_tmp[static_cast<size_t>(row) * 128 + tid] = static_cast<unsigned char>(qv);
    }
    if (tid == 0) {
        const float scale = static_cast<float>(1 << o);
        kp_tmp[2 * static_cast<size_t>(row)] = x * scale;
        kp_tmp[2 * static_cast<size_t>(row) + 1] = y * scale;
        float* mt = meta_tmp + 4 * static_cast<size_t>(row);
        mt[0] = static_cast<float>(tab->sig[lev] * scale);
        mt[1] = static_cast<float>(theta);
        mt[2] = __uint_as_float(~static_cast<unsigned>(keys[ci] >> 32));
        mt[3] = static_cast<float>(o);
        valid[row] = 1;
    }
}

// ---- S60: orientation and the 256 steered tests of one keypoint per workgroup of four waves.  The orientation is that of
// feat_describe (one function); thread i then compares the two pixels of test i on the keypoint's level, a wave's ballot is
// eight packed bytes (bit i & 7 of byte i >> 3), and lane 0 of each wave stores them.  The offsets stay within r2, so the
// border rule of feat_describe keeps every read inside the plane; there is no energy rule.
constexpr int BTHREADS = NBITS;
__global__ __launch_bounds__(BTHREADS) void feat_describe_bits(const float* pyr, const FeatTables* tab, const int8_t* steer,
                                                               const unsigned* counter, unsigned cap, int max_kp,
                                                               const unsigned long long* keys, const int4* info, const int4* geom,
                                                               const int* sel, float* kp_tmp, unsigned char* desc_tmp, float* meta_tmp,
                                                               int* valid)
{
    __shared__ __attribute__((aligned(16))) double s_rec[ORI_MAX];
    __shared__ __attribute__((aligned(16))) int s_key[ORI_MAX];
    __shared__ double s_hist[36];
    __shared__ double s_par[3];
    __shared__ int s_bin;
    const unsigned cnt = *counter;
    if (cnt > cap) return;
    const int n_sel = min(static_cast<int>(cnt), max_kp);
    const int row = blockIdx.x;
    if (row >= n_sel) return;
    const int tid = threadIdx.x;
    const int ci = sel[row];
    const int4 c4 = info[ci];
    const int o = c4.x, lev = c4.y - 1, y = c4.z, x = c4.w;
    const int4 g4 = geom[ci];
    const int w = g4.x, h = g4.y;
    const float* L = pyr + ((static_cast<unsigned long long>(static_cast<unsigned>(g4.w)) << 32) | static_cast<unsigned>(g4.z)) +
                     static_cast<size_t>(c4.y) * w * h;
    const int rad = tab->rad[lev], r2 = tab->r2[lev];
    if (y - rad < 1 || x - rad < 1 || y + rad >= h - 1 || x + rad >= w - 1 || y - r2 < 1 || x - r2 < 1 || y + r2 >= h - 1 || x + r2 >= w - 1) {
        if (tid == 0) valid[row] = 0;
        return;
    }
    feat_orientation<BTHREADS>(L, w, x, y, rad, lev, tab, tid, s_rec, s_key, s_hist, s_par, &s_bin);
    const int bin = s_bin;
    const int8_t* t4 = steer + (static_cast<size_t>(lev * 36 + bin) * NBITS + tid) * 4;
    const int dx1 = t4[0], dy1 = t4[1], dx2 = t4[2], dy2 = t4[3];
    const float a = L[static_cast<size_t>(y + dy1) * w + (x + dx1)];
    const float b = L[static_cast<size_t>(y + dy2) * w + (x + dx2)];
    const unsigned long long bal = __ballot(a < b);
    if ((tid & 63) == 0) reinterpret_cast<unsigned long long*>(desc_tmp + static_cast<size_t>(row) * 32)[tid >> 6] = bal;
    if (tid == 0) {
        const float scale = static_cast<float>(1 << o);
        kp_tmp[2 * static_cast<size_t>(row)] = x * scale;
        kp_tmp[2 * static_cast<size_t>(row) + 1] = y * scale;
        float* mt = meta_tmp + 4 * static_cast<size_t>(row);
        mt[0] = static_cast<float>(tab->sig[lev] * scale);
        mt[1] = static_cast<float>(s_par[0]);
        mt[2] = __uint_as_float(~static_cast<unsigned>(keys[ci] >> 32));
        mt[3] = static_cast<float>(o);
        valid[row] = 1;
    }
}

// ---- S57: stable compaction of the rows that survived the border and norm skips.  One workgroup scans the flags in row
// order and publishes the count; on overflow of the candidate buffer the count is -1 and no row is written.
__global__ __launch_bounds__(1024) void feat_compact(const unsigned* counter, unsigned cap, int max_kp, const int* valid, int* pos, int* d_n)
{
    const unsigned cnt = *counter;
    if (cnt > cap) {
        if (threadIdx.x == 0) *d_n = -1;
        return;
    }
    const int n_sel = min(static_cast<int>(cnt), max_kp);
    pm::select_stable_1024(
        n_sel, d_n, [&](int r) { return valid[r] != 0; },
        [&](int r, int dst) {
            if (r < n_sel) pos[r] = dst;
        },
        [](int) {});
}

__global__ __launch_bounds__(128) void feat_gather(const unsigned* counter, unsigned cap, int max_kp, const int* pos, const float* kp_tmp,
                                                   const unsigned char* desc_tmp, const float* meta_tmp, float* kp_xy,
                                                   unsigned char* desc_u8, float* desc_f32, float* meta)
{
    const unsigned cnt = *counter;
    if (cnt > cap) return;
    const int row = blockIdx.x;
    if (row >= min(static_cast<int>(cnt), max_kp)) return;
    const int dst = pos[row];
    if (dst < 0) return;
    const int tid = threadIdx.x;
    const unsigned char d = desc_tmp[static_cast<size_t>(row) * 128 + tid];
    if (desc_u8) desc_u8[static_cast<size_t>(dst) * 128 + tid] = d;
    if (desc_f32) desc_f32[static_cast<size_t>(dst) * 128 + tid] = static_cast<float>(d);
    if (tid < 2) kp_xy[2 * static_cast<size_t>(dst) + tid] = kp_tmp[2 * static_cast<size_t>(row) + tid];
    if (meta && tid < 4) meta[4 * static_cast<size_t>(dst) + tid] = meta_tmp[4 * static_cast<size_t>(row) + tid];
}

// 32-byte rows: eight rows per workgroup, one byte per thread
__global__ __launch_bounds__(256) void feat_gather_bits(const unsigned* counter, unsigned cap, int max_kp, const int* pos, const float* kp_tmp,
                                                        const unsigned char* desc_tmp, const float* meta_tmp, float* kp_xy,
                                                        unsigned char* desc_bits, float* meta)
{
    const unsigned cnt = *counter;
    if (cnt > cap) return;
    const int row = blockIdx.x * 8 + (threadIdx.x >> 5), tid = threadIdx.x & 31;
    if (row >= min(static_cast<int>(cnt), max_kp)) return;
    const int dst = pos[row];
    if (dst < 0) return;
    desc_bits[static_cast<size_t>(dst) * 32 + tid] = desc_tmp[static_cast<size_t>(row) * 32 + tid];
    if (tid < 2) kp_xy[2 * static_cast<size_t>(dst) + tid] = kp_tmp[2 * static_cast<size_t>(row) + tid];
    if (meta && tid < 4) meta[4 * static_cast<size_t>(dst) + tid] = meta_tmp[4 * static_cast<size_t>(row) + tid];
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// The host's octave rule: n_oct from log2 of the shorter side, halving by (w + 1) / 2, stop below 20 pixels.
int plan_octaves(int w, int h, int* ow, int* oh)
{
    const int n_oct = std::max(1, static_cast<int>(std::log2(static_cast<double>(std::min(w, h)))) - 4);
    int n = 0;
    for (int o = 0; o < n_oct && o < MAX_OCT; ++o) {
        ow[o] = w;
        oh[o] = h;
        n = o + 1;
        w = (w + 1) / 2;
        h = (h + 1) / 2;
        if (w < 20 || h < 20) break;
    }
    return n;
}

struct Layout {
    size_t tables, steer, counter, pyr, keys, info, geom, sel, kp, desc, meta, valid, pos, staging, total;
};

// staging: bytes the blocking form asks for behind everything else (its copy of the image and its output block)
Layout plan_layout(const pm_ctx* ctx, size_t cap, size_t rows, size_t staging)
{
    Layout l;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = pm::align_up(off + bytes, 256); return o; };
    l.tables = take(sizeof(FeatTables));
    l.steer = take(STEER_BYTES);                      // == STEER_OFF
    l.counter = take(256);
    size_t px = 0;
    for (int o = 0; o < ctx->feat_noct; ++o) px += static_cast<size_t>(NLEV) * ctx->feat_w[o] * ctx->feat_h[o];
    l.pyr = take(px * sizeof(float));
    l.keys = take(cap * 8);
    l.info = take(cap * 16);
    l.geom = take(cap * 16);
    l.sel = take(rows * 4);
    l.kp = take(rows * 8);
    l.desc = take(rows * 128);
    l.meta = take(rows * 16);
    l.valid = take(rows * 4);
    l.pos = take(rows * 4);
    l.staging = take(staging);
    l.total = off;
    return l;
}

int feat_reserve(pm_ctx* ctx, size_t bytes)
{
    if (bytes <= ctx->feat_cap) return PM_OK;
    PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (ctx->feat) PM_HIP_CHECK(hipFree(ctx->feat));
    ctx->feat = nullptr;
    ctx->feat_cap = 0;
    const size_t cap = pm::align_up(bytes + bytes / 4, size_t(1) << 20);
    if (hipMalloc(reinterpret_cast<void**>(&ctx->feat), cap) != hipSuccess) {
        pm::set_error("hipMalloc(%zu) failed", cap);
        return PM_E_NOMEM;
    }
    ctx->feat_cap = cap;
    // the tables live at the head of the buffer (blocking copy: the stream is idle, and this path runs once per growth)
    PM_HIP_CHECK(hipMemcpy(ctx->feat, &tables(), sizeof(FeatTables), hipMemcpyHostToDevice));
    PM_HIP_CHECK(hipMemcpy(ctx->feat + STEER_OFF, bits_tables().steer, STEER_BYTES, hipMemcpyHostToDevice));
    return PM_OK;
}

size_t default_capacity(const pm_ctx* ctx, int max_kp)
{
    const int opt = ctx->opts[PM_OPT_FEAT_CAPACITY];
    if (opt > 0) return static_cast<size_t>(opt);
    // (the candidate count travels as a 32-bit word: the automatic value stops where the option does, at 2^28)
    return std::min<size_t>(std::max<size_t>(65536, 8 * static_cast<size_t>(max_kp)), size_t(1) << 28);
}

// Octave plan, buffer layout and capacity of a run; the same arguments give the same layout.
int plan_and_reserve(pm_ctx* ctx, int w, int h, int max_kp, size_t cap, size_t staging, Layout* l)
{
    ctx->feat_noct = plan_octaves(w, h, ctx->feat_w, ctx->feat_h);
    *l = plan_layout(ctx, cap, std::min<size_t>(static_cast<size_t>(max_kp), cap), staging);
    return feat_reserve(ctx, l->total);
}

// Everything of S53-S57 on the context's stream.  cap: candidate capacity of this run.  bits: the binary form (S58-S60), whose
// n x 32 bytes go to d_desc_u8.
int detect_enqueue(pm_ctx* ctx, const uint8_t* d_img, int w, int h, int stride, int max_kp, float contrast, float edge_r, size_t cap,
                   size_t staging, bool bits, float* d_kp_xy, uint8_t* d_desc_u8, float* d_desc_f32, float* d_meta, int32_t* d_n)
{
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t rows = std::min<size_t>(static_cast<size_t>(max_kp), cap);
    Layout l;
    int rc = plan_and_reserve(ctx, w, h, max_kp, cap, staging, &l);
    if (rc != PM_OK) return rc;
    char* base = ctx->feat;
    const FeatTables* tab = reinterpret_cast<const FeatTables*>(base + l.tables);
    unsigned* counter = reinterpret_cast<unsigned*>(base + l.counter);
    float* pyr = reinterpret_cast<float*>(base + l.pyr);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base + l.keys);
    int4* info = reinterpret_cast<int4*>(base + l.info);
    int4* geom = reinterpret_cast<int4*>(base + l.geom);
    int* sel = reinterpret_cast<int*>(base + l.sel);
    float* kp_tmp = reinterpret_cast<float*>(base + l.kp);
    unsigned char* desc_tmp = reinterpret_cast<unsigned char*>(base + l.desc);
    float* meta_tmp = reinterpret_cast<float*>(base + l.meta);
    int* valid = reinterpret_cast<int*>(base + l.valid);
    int* pos = reinterpret_cast<int*>(base + l.pos);
    ctx->feat_counter_off = l.counter;
    hipStream_t s = ctx->stream;
    PM_HIP_CHECK(hipMemsetAsync(counter, 0, sizeof(unsigned), s));

    OctTable octs;
    memset(&octs, 0, sizeof octs);
    octs.n = ctx->feat_noct;
    size_t off = 0;
    for (int o = 0; o < octs.n; ++o) {
        octs.off[o] = off;
        octs.w[o] = ctx->feat_w[o];
        octs.h[o] = ctx->feat_h[o];
        ctx->feat_off[o] = l.pyr + off * sizeof(float);
        off += static_cast<size_t>(NLEV) * octs.w[o] * octs.h[o];
    }
    // S53: scale space
    for (int o = 0; o < octs.n; ++o) {
        const int ow = octs.w[o], oh = octs.h[o];
        const size_t plane = static_cast<size_t>(ow) * oh;
        float* L = pyr + octs.off[o];
        const dim3 grid((ow + BT_X - 1) / BT_X, (oh + BT_Y - 1) / BT_Y);
        if (o == 0) {
            pm::ScopedKernelTime timer(ctx, "feat_blur");
            hipLaunchKernelGGL(feat_blur<true>, grid, dim3(256), 0, s, d_img, stride, L, ow, oh, tab, 0);
        } else {
            const int pw = octs.w[o - 1], ph = octs.h[o - 1];
            const float* src = pyr + octs.off[o - 1] + 3 * static_cast<size_t>(pw) * ph;       // level S of the octave before
            pm::ScopedKernelTime timer(ctx, "feat_decimate");
            hipLaunchKernelGGL(feat_decimate, dim3((ow + 63) / 64, (oh + 3) / 4), dim3(256), 0, s, src, pw, L, ow, oh);
        }
        for (int i = 1; i < NLEV; ++i) {
            pm::ScopedKernelTime timer(ctx, "feat_blur");
            hipLaunchKernelGGL(feat_blur<false>, grid, dim3(256), 0, s, L + (i - 1) * plane, 0, L + i * plane, ow, oh, tab, i);
        }
    }
    // S54: extrema
    const float thr = contrast / 3;
    unsigned pos_base = 0;
    for (int o = 0; o < octs.n; ++o) {
        const int ow = octs.w[o], oh = octs.h[o];
        if (ow > 16 && oh > 16) {
            pm::ScopedKernelTime timer(ctx, "feat_extrema");
            hipLaunchKernelGGL(feat_extrema, dim3((ow - 16 + 63) / 64, (oh - 16 + 3) / 4, 3), dim3(256), 0, s, pyr + octs.off[o], ow, oh, o,
                               pos_base, thr, edge_r, octs.off[o], counter, static_cast<unsigned>(cap), keys, info, geom);
        }
        pos_base += 3u * static_cast<unsigned>(ow) * static_cast<unsigned>(oh);
    }
    // S55: selection
    {
        pm::ScopedKernelTime timer(ctx, "feat_rank");
        hipLaunchKernelGGL(feat_rank, dim3(static_cast<unsigned>((cap + 255) / 256)), dim3(256), 0, s, counter, static_cast<unsigned>(cap),
                           max_kp, keys, sel);
    }
    // S56: orientation + descriptor
    if (bits) {
        pm::ScopedKernelTime timer(ctx, "feat_describe_bits");
        hipLaunchKernelGGL(feat_describe_bits, dim3(static_cast<unsigned>(rows)), dim3(BTHREADS), 0, s, pyr, tab,
                           reinterpret_cast<const int8_t*>(base + l.steer), counter, static_cast<unsigned>(cap), max_kp, keys, info, geom,
                           sel, kp_tmp, desc_tmp, meta_tmp, valid);
    } else {
        pm::ScopedKernelTime timer(ctx, "feat_describe");
        hipLaunchKernelGGL(feat_describe, dim3(static_cast<unsigned>(rows)), dim3(DTHREADS), 0, s, pyr, tab, counter,
                           static_cast<unsigned>(cap), max_kp, keys, info, geom, sel, kp_tmp, desc_tmp, meta_tmp, valid);
    }
    // S57: compaction
    {
        pm::ScopedKernelTime timer(ctx, "feat_compact");
        hipLaunchKernelGGL(feat_compact, dim3(1), dim3(1024), 0, s, counter, static_cast<unsigned>(cap), max_kp, valid, pos, d_n);
    }
    if (bits) {
        pm::ScopedKernelTime timer(ctx, "feat_gather_bits");
        hipLaunchKernelGGL(feat_gather_bits, dim3(static_cast<unsigned>((rows + 7) / 8)), dim3(256), 0, s, counter,
                           static_cast<unsigned>(cap), max_kp, pos, kp_tmp, desc_tmp, meta_tmp, d_kp_xy, d_desc_u8, d_meta);
    } else {
        pm::ScopedKernelTime timer(ctx, "feat_gather");
        hipLaunchKernelGGL(feat_gather, dim3(static_cast<unsigned>(rows)), dim3(128), 0, s, counter, static_cast<unsigned>(cap), max_kp, pos,
                           kp_tmp, desc_tmp, meta_tmp, d_kp_xy, d_desc_u8, d_desc_f32, d_meta);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

int check_args(pm_ctx* ctx, const void* img, int w, int h, int stride, int max_kp, float contrast, float edge_r, const void* kp,
               const void* n)
{
    PM_REQUIRE(ctx != nullptr && n != nullptr, PM_E_INVALID, "null context or count pointer");
    PM_REQUIRE(w >= 1 && h >= 1 && stride >= w && max_kp >= 1, PM_E_INVALID, "need w, h >= 1, stride >= w, max_kp >= 1");
    PM_REQUIRE(img != nullptr && kp != nullptr, PM_E_INVALID, "null image or keypoint pointer");
    PM_REQUIRE(contrast == contrast && edge_r == edge_r, PM_E_INVALID, "contrast / edge_r is NaN");
    PM_REQUIRE_PASS(pm_image::pixel_cap(w, h));
    return PM_OK;
}

// The _dev forms: argument checks, the small-image rule, one enqueue.  The entry points check the context and refuse a
// capturing stream themselves, so that those messages carry their names.
int detect_dev(pm_ctx* ctx, const uint8_t* d_img, int w, int h, int stride, int max_kp, float contrast, float edge_r, bool bits,
               float* d_kp_xy, uint8_t* d_desc_u8, float* d_desc_f32, float* d_meta, int32_t* d_n)
{
    const int rc = check_args(ctx, d_img, w, h, stride, max_kp, contrast, edge_r, d_kp_xy, d_n);
    if (rc != PM_OK) return rc;
    if (w < 32 || h < 32) {
        PM_HIP_CHECK(hipSetDevice(ctx->device));
        PM_HIP_CHECK(hipMemsetAsync(d_n, 0, sizeof(int32_t), ctx->stream));
        return PM_OK;
    }
    return detect_enqueue(ctx, d_img, w, h, stride, max_kp, contrast, edge_r, default_capacity(ctx, max_kp), 0, bits, d_kp_xy, d_desc_u8,
                          d_desc_f32, d_meta, d_n);
}

// The blocking forms: device copy of the image, output block, run, grow and run again on overflow, download.
int detect_blocking(pm_ctx* ctx, const char* fn, const uint8_t* img, int w, int h, int stride, int max_kp, float contrast, float edge_r,
                    bool bits, float* kp_xy, uint8_t* desc_u8, float* desc_f32, float* meta, int32_t* n_out)
{
    int rc = check_args(ctx, img, w, h, stride, max_kp, contrast, edge_r, kp_xy, n_out);
    if (rc != PM_OK) return rc;
    *n_out = 0;
    if (w < 32 || h < 32) return PM_OK;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t img_bytes = static_cast<size_t>(h) * stride;
    const size_t row_u8 = bits ? 32 : 128, row_f32 = bits ? 0 : 512;
    pm::StagedBlock image(ctx, fn);                      // lives across the rounds
    const size_t o_img = image.add(img_bytes);
    image.alloc();
    image.upload(o_img, img, img_bytes);
    rc = image.sync();
    size_t cap = default_capacity(ctx, max_kp);
    int32_t n = 0;
    // at most two rounds: the counter of an overflowed run is the exact need of the next (same image, same thresholds)
    for (int round = 0; rc == PM_OK && round < 3; ++round) {
        const size_t rows = std::min<size_t>(static_cast<size_t>(max_kp), cap);
        pm::StagedBlock b(ctx, fn);                      // this round's outputs
        const size_t o_n = b.add(sizeof n), o_kp = b.add(rows * 8), o_u8 = b.add(rows * row_u8), o_f32 = b.add(rows * row_f32);
        const size_t o_meta = b.add(rows * 16);
        b.alloc();
        if (b.rc == PM_OK)
            b.rc = detect_enqueue(ctx, image.at<uint8_t>(o_img), w, h, stride, max_kp, contrast, edge_r, cap, 0, bits, b.at<float>(o_kp),
                                  b.at<uint8_t>(o_u8), bits ? nullptr : b.at<float>(o_f32), b.at<float>(o_meta), b.at<int32_t>(o_n));
        unsigned need = 0;
        b.download(&n, o_n, sizeof n);
        if (b.rc == PM_OK)                               // the candidate counter lives in the context's feature buffer
            b.step(hipMemcpyAsync(&need, ctx->feat + ctx->feat_counter_off, sizeof need, hipMemcpyDeviceToHost, ctx->stream), PM_E_HIP, "D2H copy");
        rc = b.sync();
        if (rc == PM_OK && n >= 0) {
            const size_t m = static_cast<size_t>(n);
            b.download(kp_xy, o_kp, m * 8);
            if (desc_u8) b.download(desc_u8, o_u8, m * row_u8);
            if (desc_f32) b.download(desc_f32, o_f32, m * row_f32);
            if (meta) b.download(meta, o_meta, m * 16);
            rc = b.sync();
            if (rc == PM_OK) *n_out = n;                     // only once every row has arrived
            break;
        }
        if (rc == PM_OK) {
            if (need <= cap) { pm::set_error("%s: overflow reported without a larger need", fn); rc = PM_E_HIP; }
            cap = need;
        }
    }
    if (rc == PM_OK && n < 0) { pm::set_error("%s: the candidate buffer overflowed again after growing", fn); rc = PM_E_HIP; }
    return rc;
}

}  // namespace

extern "C" int pm_detect_describe_dev(pm_ctx* ctx, const uint8_t* d_img, int w, int h, int stride, int max_kp, float contrast,
                                      float edge_r, float* d_kp_xy, uint8_t* d_desc_u8, float* d_desc_f32, float* d_meta,
                                      int32_t* d_n)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    return detect_dev(ctx, d_img, w, h, stride, max_kp, contrast, edge_r, false, d_kp_xy, d_desc_u8, d_desc_f32, d_meta, d_n);
}

extern "C" int pm_detect_describe(pm_ctx* ctx, const uint8_t* img, int w, int h, int stride, int max_kp, float contrast, float edge_r,
                                  float* kp_xy, uint8_t* desc_u8, float* desc_f32, float* meta, int32_t* n_out)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    return detect_blocking(ctx, __func__, img, w, h, stride, max_kp, contrast, edge_r, false, kp_xy, desc_u8, desc_f32, meta, n_out);
}

extern "C" int pm_detect_describe_bits_dev(pm_ctx* ctx, const uint8_t* d_img, int w, int h, int stride, int max_kp, float contrast,
                                           float edge_r, float* d_kp_xy, uint8_t* d_desc_bits, float* d_meta, int32_t* d_n)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(d_desc_bits != nullptr, PM_E_INVALID, "null descriptor pointer");
    return detect_dev(ctx, d_img, w, h, stride, max_kp, contrast, edge_r, true, d_kp_xy, d_desc_bits, nullptr, d_meta, d_n);
}

extern "C" int pm_detect_describe_bits(pm_ctx* ctx, const uint8_t* img, int w, int h, int stride, int max_kp, float contrast,
                                       float edge_r, float* kp_xy, uint8_t* desc_bits, float* meta, int32_t* n_out)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(desc_bits != nullptr, PM_E_INVALID, "null descriptor pointer");
    return detect_blocking(ctx, __func__, img, w, h, stride, max_kp, contrast, edge_r, true, kp_xy, desc_bits, nullptr, meta, n_out);
}

// Test and inspection accessor: Gaussian level `level` of octave `octave` as the LAST detect call on this context left it.
extern "C" int pm_detect_level_get(pm_ctx* ctx, int octave, int level, float* plane, int cap_floats, int* w_out, int* h_out)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REQUIRE(ctx->feat != nullptr && ctx->feat_noct > 0, PM_E_INVALID, "no detect call has run on this context");
    PM_REQUIRE(octave >= 0 && octave < ctx->feat_noct && level >= 0 && level < NLEV, PM_E_INVALID, "no such octave / level");
    const int w = ctx->feat_w[octave], h = ctx->feat_h[octave];
    if (w_out) *w_out = w;
    if (h_out) *h_out = h;
    if (!plane) return PM_OK;
    const size_t n = static_cast<size_t>(w) * h;
    PM_REQUIRE(cap_floats >= 0 && static_cast<size_t>(cap_floats) >= n, PM_E_INVALID, "plane buffer too small");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    PM_HIP_CHECK(hipMemcpy(plane, ctx->feat + ctx->feat_off[octave] + static_cast<size_t>(level) * n * sizeof(float), n * sizeof(float),
                           hipMemcpyDeviceToHost));
    return PM_OK;
}

// The host-computed tables of S53 / S56 (no GPU needed): tap_radius[6], taps[6 * 25] (row i holds 2 r_i + 1 values),
// ori_weight[3 * 393], ori_radius[3], desc_radius[3], cos_sin[72] (36 cosines, then 36 sines).  Any pointer may be NULL.
extern "C" int pm_detect_tables(int32_t* tap_radius, double* taps, double* ori_weight, int32_t* ori_radius, int32_t* desc_radius,
                                double* cos_sin)
{
    const FeatTables& t = tables();
    for (int i = 0; i < NLEV; ++i) {
        if (tap_radius) tap_radius[i] = t.tap_r[i];
        if (taps) memcpy(taps + i * NTAP, t.taps[i], sizeof t.taps[i]);
    }
    for (int l = 0; l < 3; ++l) {
        if (ori_weight) memcpy(ori_weight + l * ORI_N, t.ori_w[l], sizeof t.ori_w[l]);
        if (ori_radius) ori_radius[l] = t.rad[l];
        if (desc_radius) desc_radius[l] = t.r2[l];
    }
    if (cos_sin) {
        memcpy(cos_sin, t.cs, sizeof t.cs);
        memcpy(cos_sin + 36, t.sn, sizeof t.sn);
    }
    return PM_OK;
}

// The tables of S58 / S59 (no GPU needed): base1024 = 256 tests (x1, y1, x2, y2); steered110592 = [3][36][256][4] offsets.
extern "C" int pm_detect_bits_table(int8_t* base1024, int8_t* steered110592)
{
    const BitsTables& t = bits_tables();
    if (base1024) memcpy(base1024, t.base, sizeof t.base);
    if (steered110592) memcpy(steered110592, t.steer, sizeof t.steer);
    return PM_OK;
}
