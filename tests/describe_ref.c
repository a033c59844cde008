/* describe_ref.c — plain-C restatement of docs/SPEC.md S71-S74: oriented 256-bit descriptors of given points on one level of
 * an image pyramid.  Written from the specification alone; it shares no code with the library.  Every quantity is an integer
 * or an exactly specified fp64 / fp32 operation, so the library's rows must equal these byte for byte.
 * Built with -ffp-contract=off by tests/cref.py. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define NT 256

static int8_t g_steer[37][NT][4];      /* S73; row 36 = the S58 pattern */
static int32_t g_q20[72];              /* S72: C[0..35], S[0..35] */
static int g_ready = 0;

static uint64_t g_state;
static int draw_coord(void)
{
    int v = 0;
    for (int k = 0; k < 3; ++k) {
        g_state += 0x9E3779B97F4A7C15ULL;
        uint64_t z = g_state;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        z ^= z >> 31;
        v += (int)((z >> 33) % 11) - 5;
    }
    return v;
}

static void make_tables(void)
{
    if (g_ready) return;
    const double pi = 3.14159265358979323846;
    int8_t (*base)[4] = g_steer[36];
    g_state = 0x504D4249545331ULL;
    for (int n = 0; n < NT;) {
        int c[4];
        for (int j = 0; j < 4; ++j) c[j] = draw_coord();
        if (c[0] * c[0] + c[1] * c[1] > 225 || c[2] * c[2] + c[3] * c[3] > 225) continue;
        if (c[0] == c[2] && c[1] == c[3]) continue;
        int seen = 0;
        for (int i = 0; i < n && !seen; ++i)
            seen = (base[i][0] == c[0] && base[i][1] == c[1] && base[i][2] == c[2] && base[i][3] == c[3]) ||
                   (base[i][0] == c[2] && base[i][1] == c[3] && base[i][2] == c[0] && base[i][3] == c[1]);
        if (seen) continue;
        for (int j = 0; j < 4; ++j) base[n][j] = (int8_t)c[j];
        ++n;
    }
    for (int b = 0; b < 36; ++b) {
        const double theta = (b + 0.5) / 36 * 2 * pi - pi;
        const double cs = cos(theta), sn = sin(theta);
        g_q20[b] = (int32_t)nearbyint(1048576.0 * cs);
        g_q20[36 + b] = (int32_t)nearbyint(1048576.0 * sn);
        for (int i = 0; i < NT; ++i)
            for (int p = 0; p < 4; p += 2) {
                const double x = base[i][p], y = base[i][p + 1];
                g_steer[b][i][p] = (int8_t)nearbyint(cs * x - sn * y);
                g_steer[b][i][p + 1] = (int8_t)nearbyint(sn * x + cs * y);
            }
    }
    g_ready = 1;
}

/* cos_sin_q20[72], steered[37 * 256 * 4]; either may be null */
void describe_tables(int32_t* cos_sin_q20, int8_t* steered)
{
    make_tables();
    if (cos_sin_q20) memcpy(cos_sin_q20, g_q20, sizeof g_q20);
    if (steered) memcpy(steered, g_steer, sizeof g_steer);
}

/* S72: the bin of one moment pair */
int describe_bin(int32_t m10, int32_t m01)
{
    make_tables();
    int best = 0;
    int64_t best_dot = 0;
    for (int b = 0; b < 36; ++b) {
        const int64_t dot = (int64_t)m10 * g_q20[b] + (int64_t)m01 * g_q20[36 + b];
        if (b == 0 || dot > best_dot) {
            best = b;
            best_dot = dot;
        }
    }
    return best;
}

/* S71: 1 and the centre when the point can be described on a w x h level at scale 2^-level */
int describe_position(float x, float y, int level, int w, int h, int* cx, int* cy)
{
    if (!(fabsf(x) <= 1e6f) || !(fabsf(y) <= 1e6f)) return 0;     /* NaN, infinity, beyond 1e6 */
    const float s = 1.0f / (float)(1 << level);
    const int ix = (int)nearbyintf(x * s), iy = (int)nearbyintf(y * s);
    if (ix < 17 || ix > w - 18 || iy < 17 || iy > h - 18) return 0;
    *cx = ix;
    *cy = iy;
    return 1;
}

/* S72: the two moments over the disc of radius 15 */
void describe_moments(const uint8_t* img, int w, int cx, int cy, int32_t* m10, int32_t* m01)
{
    int32_t a = 0, b = 0;
    for (int dy = -15; dy <= 15; ++dy)
        for (int dx = -15; dx <= 15; ++dx) {
            if (dx * dx + dy * dy > 225) continue;
            const int v = img[(size_t)(cy + dy) * w + (cx + dx)];
            a += dx * v;
            b += dy * v;
        }
    *m10 = a;
    *m01 = b;
}

static int box5(const uint8_t* img, int w, int x, int y)
{
    int s = 0;
    for (int j = -2; j <= 2; ++j)
        for (int i = -2; i <= 2; ++i) s += img[(size_t)(y + j) * w + (x + i)];
    return s;
}

/* S71-S74 for n points on one level (a tight w x h plane).  desc: n x 32; valid, bin: n.  Returns the number of valid rows. */
int describe_points(const uint8_t* img, int w, int h, int level, int upright, const float* pts, int n, uint8_t* desc, uint8_t* valid,
                    uint8_t* bin)
{
    make_tables();
    int n_valid = 0;
    for (int k = 0; k < n; ++k) {
        uint8_t* row = desc + (size_t)k * 32;
        memset(row, 0, 32);
        int cx, cy;
        if (!describe_position(pts[2 * k], pts[2 * k + 1], level, w, h, &cx, &cy)) {
            valid[k] = 0;
            bin[k] = 255;
            continue;
        }
        int b = 36;
        if (!upright) {
            int32_t m10, m01;
            describe_moments(img, w, cx, cy, &m10, &m01);
            b = describe_bin(m10, m01);
        }
        for (int i = 0; i < NT; ++i) {
            const int8_t* t = g_steer[b][i];
            if (box5(img, w, cx + t[0], cy + t[1]) < box5(img, w, cx + t[2], cy + t[3])) row[i >> 3] |= (uint8_t)(1u << (i & 7));
        }
        valid[k] = 1;
        bin[k] = (uint8_t)b;
        ++n_valid;
    }
    return n_valid;
}
