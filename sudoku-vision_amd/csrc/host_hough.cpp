// Host side of cv/grid_v2.py's line method: cv2.HoughLinesP (detect_lines, cv/grid_v2.py:135-149), the progressive probabilistic
// Hough transform.  It is sequential by construction -- every accepted line removes its pixels and their votes before the next
// random point is drawn -- so it stays on the host, like the contour search.  cv2 draws its points from a cv::RNG seeded with a
// constant: the transform is deterministic, and so is this restatement of it.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "sv_internal.h"

namespace {

// cv::RNG: multiply-with-carry, the low 32 bits of the state are the output
struct Mwc {
    uint64_t state = ~(uint64_t)0;
    uint32_t next()
    {
        state = (uint64_t)(uint32_t)state * 4164903690u + (state >> 32);
        return (uint32_t)state;
    }
};

// cvRound: round half to even (the default rounding mode)
inline int round_f(float v) { return (int)std::nearbyintf(v); }
inline int round_d(double v) { return (int)std::nearbyint(v); }

struct Point { int x, y; };

}  // namespace

extern "C" int sv_hough_lines_p_u8(const uint8_t *binary, int H, int W, ptrdiff_t pitch, double rho, double theta, int threshold, int min_line_length,
                                   int max_line_gap, int *lines, int cap, int *count)
{
    REQUIRE(binary && count && (lines || cap == 0), "NULL argument");
    REQUIRE(H > 0 && W > 0 && H < 32768 && W < 32768 && pitch >= W && cap >= 0, "bad shape");
    REQUIRE(rho > 0 && theta > 0, "rho and theta must be positive");
    const float frho = (float)rho, ftheta = (float)theta;     // cv2 takes both as float
    const float irho = 1 / frho;
    const int numangle = round_d(3.14159265358979323846 / ftheta);
    const int numrho = round_d(((W + H) * 2 + 1) / frho);
    REQUIRE(numangle > 0 && numrho > 0 && (double)numangle * numrho < 1e9, "accumulator too large");

    std::vector<int> accum((size_t)numangle * numrho, 0);
    std::vector<uint8_t> mask((size_t)H * W);
    std::vector<float> tab((size_t)numangle * 2);
    for (int n = 0; n < numangle; n++) {
        tab[2 * n] = (float)(std::cos((double)n * ftheta) * irho);
        tab[2 * n + 1] = (float)(std::sin((double)n * ftheta) * irho);
    }
    std::vector<Point> nz;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const bool set = binary[(ptrdiff_t)y * pitch + x] != 0;
            mask[(size_t)y * W + x] = set;
            if (set) nz.push_back({x, y});
        }
    const int half = (numrho - 1) / 2, shift = 16;
    // the bin of pixel (j, i) at angle n.  For rho = 1 the row is wide enough for every pixel of the image; the clamp only acts for a
    // rho so coarse that cv2 itself would leave its accumulator
    auto bin = [&](int j, int i, int n) {
        const int r = round_f((float)j * tab[2 * n] + (float)i * tab[2 * n + 1]) + half;
        return r < 0 ? 0 : (r >= numrho ? numrho - 1 : r);
    };

    Mwc rng;
    int found = 0;
    bool overflow = false;
    for (int remaining = (int)nz.size(); remaining > 0; remaining--) {
        const int idx = (int)(rng.next() % (uint32_t)remaining);
        const Point pt = nz[idx];
        nz[idx] = nz[remaining - 1];
        const int i = pt.y, j = pt.x;
        if (!mask[(size_t)i * W + j]) continue;               // already part of an earlier line
        int max_val = threshold - 1, max_n = 0;
        for (int n = 0; n < numangle; n++) {
            const int val = ++accum[(size_t)n * numrho + bin(j, i, n)];
            if (max_val < val) { max_val = val; max_n = n; }
        }
        if (max_val < threshold) continue;

        // walk from the point both ways along the winning line, in 16-bit fixed point on the minor axis
        const float a = -tab[2 * max_n + 1], b = tab[2 * max_n];
        int x0 = j, y0 = i, dx0, dy0;
        bool xflag;
        if (std::fabs(a) > std::fabs(b)) {
            xflag = true;
            dx0 = a > 0 ? 1 : -1;
            dy0 = round_f(b * (1 << shift) / std::fabs(a));
            y0 = (y0 << shift) + (1 << (shift - 1));
        } else {
            xflag = false;
            dy0 = b > 0 ? 1 : -1;
            dx0 = round_f(a * (1 << shift) / std::fabs(b));
            x0 = (x0 << shift) + (1 << (shift - 1));
        }
        Point end[2] = {{j, i}, {j, i}};
        for (int k = 0; k < 2; k++) {
            int gap = 0, x = x0, y = y0;
            const int dx = k ? -dx0 : dx0, dy = k ? -dy0 : dy0;
            for (;; x += dx, y += dy) {
                const int j1 = xflag ? x : x >> shift, i1 = xflag ? y >> shift : y;
                if (j1 < 0 || j1 >= W || i1 < 0 || i1 >= H) break;
                if (mask[(size_t)i1 * W + j1]) {
                    gap = 0;
                    end[k] = {j1, i1};
                } else if (++gap > max_line_gap) {
                    break;
                }
            }
        }
        const bool good = std::abs(end[1].x - end[0].x) >= min_line_length || std::abs(end[1].y - end[0].y) >= min_line_length;
        // second walk: clear the pixels; a good line also takes their votes back
        for (int k = 0; k < 2; k++) {
            int x = x0, y = y0;
            const int dx = k ? -dx0 : dx0, dy = k ? -dy0 : dy0;
            for (;; x += dx, y += dy) {
                const int j1 = xflag ? x : x >> shift, i1 = xflag ? y >> shift : y;
                if (j1 < 0 || j1 >= W || i1 < 0 || i1 >= H) break;     // never taken: the first walk reached end[k] inside the image
                uint8_t &m = mask[(size_t)i1 * W + j1];
                if (m) {
                    if (good)
                        for (int n = 0; n < numangle; n++) accum[(size_t)n * numrho + bin(j1, i1, n)]--;
                    m = 0;
                }
                if (i1 == end[k].y && j1 == end[k].x) break;
            }
        }
        if (good) {
            if (found < cap) {
                int *l = lines + 4 * (size_t)found;
                l[0] = end[0].x; l[1] = end[0].y; l[2] = end[1].x; l[3] = end[1].y;
            } else {
                overflow = true;
            }
            found++;
        }
    }
    *count = found;
    if (overflow) return sv_fail(SV_ERR_BUFFER, "sv_hough_lines_p_u8: %d lines, capacity %d", found, cap);
    return SV_OK;
}
