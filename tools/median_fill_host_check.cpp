// median_fill_host_check.cpp -- the arithmetic of the median fill (lio-slam_amd/csrc/lio_medianfill.h) run on the host: the
// text the kernels run, over accessors that count every read outside the grid or outside the stated halo of the cell that
// reads, against a plain second implementation (iterated 3 x 3 passes, a sorted window).  Stand-alone, needs no GPU:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined tools/median_fill_host_check.cpp -o /tmp/median_fill_host_check && /tmp/median_fill_host_check
//
// Prints one line per case with a checksum (FNV-1a over the filled grid's words, then the fill mask's) and "out-of-range
// accesses: 0, mismatches: 0" at the end; the exit status is their sum (capped).
//   median_fill_host_check case ROWS COLS RES FILL_RADIUS EXISTING_RADIUS FILTER N IN [MASK]
//                                              IN, MASK: rows x cols floats, column-major; prints the checksum of that case
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../lio-slam_amd/csrc/lio_medianfill.h"

static long long g_oob = 0, g_bad = 0;

struct CheckedLine {               // a line of a mask plane: entry k at p[k * stride], read by cell `centre` within R
    const unsigned char* p;
    int stride, n, centre, R;
    unsigned at(int k) const
    {
        if (k < 0 || k >= n || k < centre - R || k > centre + R) { ++g_oob; return 0u; }
        return p[(size_t)k * (size_t)stride];
    }
};

struct CheckedGrid {               // the grid itself, read by cell (r, c) within `halo`
    const float* g;
    int rows, cols, r, c, halo;
    float at(int i, int j) const
    {
        if (i < 0 || i >= rows || j < 0 || j >= cols || i < r - halo || i > r + halo || j < c - halo || j > c + halo) { ++g_oob; return 0.0f; }
        return g[(size_t)i + (size_t)j * (size_t)rows];
    }
};

struct Result {
    std::vector<float> filled, mask, cleaned;
    int counts[5];
};

// the header's text as the kernels apply it: four separable box operations, then one cell after the other
static void run_header(const std::vector<float>& g, const LioMfParams& P, const float* mask_in, Result& R)
{
    const int rows = P.rows, cols = P.cols;
    const size_t n = (size_t)rows * (size_t)cols;
    R.mask.assign(n, 0.0f);
    R.cleaned.assign(n, 0.0f);
    if (mask_in) {
        R.mask.assign(mask_in, mask_in + n);
    } else {
        std::vector<unsigned char> a(n), b(n);
        for (size_t k = 0; k < n; ++k) a[k] = lio_gm_finite(g[k]) ? 1 : 0;
        for (int op = 0; op < LIO_MF_N_OPS; ++op) {
            const int rad = lio_mf_op_radius(P, op);
            const bool erode = lio_mf_op_erodes(op);
            if (rad > 0) {
                for (int j = 0; j < cols; ++j)
                    for (int i = 0; i < rows; ++i) {
                        int lo, hi;
                        lio_gm_clip(i, rad, rows, lo, hi);
                        const CheckedLine line = { a.data() + (size_t)j * (size_t)rows, 1, rows, i, rad };
                        b[(size_t)i + (size_t)j * (size_t)rows] = (unsigned char)lio_mf_line(line, lo, hi, erode);
                    }
                for (int j = 0; j < cols; ++j)
                    for (int i = 0; i < rows; ++i) {
                        int lo, hi;
                        lio_gm_clip(j, rad, cols, lo, hi);
                        const CheckedLine line = { b.data() + (size_t)i, rows, cols, j, rad };
                        a[(size_t)i + (size_t)j * (size_t)rows] = (unsigned char)lio_mf_line(line, lo, hi, erode);
                    }
            }
            if (op == LIO_MF_OP_CLEANED)
                for (size_t k = 0; k < n; ++k) R.cleaned[k] = a[k] ? 1.0f : 0.0f;
        }
        for (size_t k = 0; k < n; ++k) R.mask[k] = a[k] ? 1.0f : 0.0f;
    }
    R.filled.assign(n, 0.0f);
    memset(R.counts, 0, sizeof(R.counts));
    for (int c = 0; c < cols; ++c)
        for (int r = 0; r < rows; ++r) {
            const size_t at = (size_t)r + (size_t)c * (size_t)rows;
            const CheckedGrid G = { g.data(), rows, cols, r, c, P.halo_fill };
            LioMfCell o;
            lio_mf_cell(P, G, R.mask[at], r, c, &o);
            memcpy(&R.filled[at], &o.out, 4);
            R.counts[0] += o.nan_in; R.counts[1] += o.masked; R.counts[2] += o.filled; R.counts[3] += o.filtered; R.counts[4] += o.nan_out;
        }
}

// ---- the second implementation: MedianFillFilter.cpp read literally
static std::vector<unsigned char> morph3(const std::vector<unsigned char>& m, int rows, int cols, bool erode)
{
    std::vector<unsigned char> out(m.size());
    for (int c = 0; c < cols; ++c)
        for (int r = 0; r < rows; ++r) {
            unsigned v = erode ? 1u : 0u;
            for (int j = std::max(c - 1, 0); j <= std::min(c + 1, cols - 1); ++j)
                for (int i = std::max(r - 1, 0); i <= std::min(r + 1, rows - 1); ++i) {
                    const unsigned x = m[(size_t)i + (size_t)j * (size_t)rows];
                    v = erode ? std::min(v, x) : std::max(v, x);
                }
            out[(size_t)r + (size_t)c * (size_t)rows] = (unsigned char)v;
        }
    return out;
}

static float plain_median(const std::vector<float>& g, int rows, int cols, int r, int c, int R)
{
    std::vector<unsigned> keys;
    for (int j = std::max(c - R, 0); j <= std::min(c + R, cols - 1); ++j)
        for (int i = std::max(r - R, 0); i <= std::min(r + R, rows - 1); ++i) {
            const float v = g[(size_t)i + (size_t)j * (size_t)rows];
            if (lio_gm_finite(v)) keys.push_back(lio_f2ord(v));
        }
    if (keys.empty()) return __builtin_bit_cast(float, 0x7fc00000u);
    std::sort(keys.begin(), keys.end());
    return lio_ord2f(keys[keys.size() / 2]);
}

static void run_plain(const std::vector<float>& g, const LioMfParams& P, const float* mask_in, Result& R)
{
    const int rows = P.rows, cols = P.cols;
    const size_t n = (size_t)rows * (size_t)cols;
    std::vector<unsigned char> valid(n), m;
    for (size_t k = 0; k < n; ++k) valid[k] = lio_gm_finite(g[k]) ? 1 : 0;
    m = morph3(morph3(valid, rows, cols, true), rows, cols, false);                     // :220-221
    R.cleaned.assign(n, 0.0f);
    for (size_t k = 0; k < n; ++k) R.cleaned[k] = m[k] ? 1.0f : 0.0f;
    m = morph3(m, rows, cols, false);                                                      // :230
    for (int it = 1; it < P.n_iter; ++it) m = morph3(m, rows, cols, false);
    for (int it = 0; it < P.n_iter; ++it) m = morph3(m, rows, cols, true);
    R.mask.assign(n, 0.0f);
    for (size_t k = 0; k < n; ++k) R.mask[k] = mask_in ? mask_in[k] : (m[k] ? 1.0f : 0.0f);
    R.filled = g;
    memset(R.counts, 0, sizeof(R.counts));
    for (int c = 0; c < cols; ++c)
        for (int r = 0; r < rows; ++r) {
            const size_t at = (size_t)r + (size_t)c * (size_t)rows;
            const bool fin = lio_gm_finite(g[at]), masked = R.mask[at] != 0.0f;
            float out = g[at];
            if (!fin && masked) out = plain_median(g, rows, cols, r, c, P.r_fill);
            else if (P.filter_existing && masked) { out = plain_median(g, rows, cols, r, c, P.r_existing); ++R.counts[3]; }
            memcpy(&R.filled[at], &out, 4);
            R.counts[0] += !fin; R.counts[1] += masked; R.counts[2] += !fin && lio_gm_finite(out); R.counts[4] += !lio_gm_finite(out);
        }
}

static uint64_t checksum(const Result& R)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (const std::vector<float>* a : { &R.filled, &R.mask })
        for (float f : *a) {
            uint32_t w;
            memcpy(&w, &f, 4);
            for (int k = 0; k < 4; ++k) h = (h ^ ((w >> (8 * k)) & 0xffu)) * 0x100000001b3ull;
        }
    return h;
}

static bool plan(LioMfParams& P, int rows, int cols, int r_fill, int r_existing, int filter, int n_iter)
{
    memset(&P, 0, sizeof(P));
    if (n_iter < 0 || n_iter > LIO_MF_MAX_ITERATIONS || r_fill < 0 || r_fill > LIO_TILE_MAX_REACH || r_existing < 0 || r_existing > LIO_TILE_MAX_REACH) return false;
    P.rows = rows; P.cols = cols; P.r_fill = r_fill; P.r_existing = r_existing; P.filter_existing = filter;
    P.n_iter = n_iter; P.n_dilate = n_iter > 1 ? n_iter : 1;
    P.halo_mask = 2 + P.n_dilate + P.n_iter;
    P.halo_fill = (filter && r_existing > r_fill) ? r_existing : r_fill;
    return true;
}

static uint32_t g_seed = 12345u;
static uint32_t lcg() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static std::vector<float> make_grid(int rows, int cols)
{
    std::vector<float> g((size_t)rows * (size_t)cols);
    for (float& v : g) {
        const uint32_t k = lcg();
        v = (k % 10u) < 3u ? __builtin_nanf("") : (float)(k % 4096u) * 0.01f - 20.0f;
        if ((k >> 12) % 97u == 0u) v = (k & 1u) ? -0.0f : 0.0f;
        if ((k >> 12) % 89u == 0u) v = (k & 1u) ? __builtin_huge_valf() : -__builtin_huge_valf();
    }
    if (rows >= 16 && cols >= 12)
        for (int j = 1; j < 10; ++j)
            for (int i = rows - 14; i < rows - 5; ++i) g[(size_t)i + (size_t)j * (size_t)rows] = __builtin_nanf("0x1234");
    return g;
}

static void compare(const char* what, const Result& a, const Result& b, bool with_cleaned)
{
    long long bad = 0;
    bad += memcmp(a.filled.data(), b.filled.data(), 4 * a.filled.size()) != 0;
    bad += memcmp(a.mask.data(), b.mask.data(), 4 * a.mask.size()) != 0;
    if (with_cleaned) bad += memcmp(a.cleaned.data(), b.cleaned.data(), 4 * a.cleaned.size()) != 0;
    bad += memcmp(a.counts, b.counts, sizeof(a.counts)) != 0;
    g_bad += bad;
    printf("%-34s nan_in %5d mask %5d filled %5d filtered %5d nan_out %5d  checksum %016llx%s\n", what, a.counts[0], a.counts[1], a.counts[2],
           a.counts[3], a.counts[4], (unsigned long long)checksum(a), bad ? "  MISMATCH" : "");
}

static bool read_floats(const char* path, std::vector<float>& v, size_t n)
{
    v.assign(n, 0.0f);
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t got = fread(v.data(), 4, n, f);
    fclose(f);
    return got == n;
}

int main(int argc, char** argv)
{
    if (argc >= 10 && !strcmp(argv[1], "case")) {
        const int rows = atoi(argv[2]), cols = atoi(argv[3]);
        const double res = atof(argv[4]);
        LioMfParams P;
        if (rows < 1 || cols < 1 || !(res > 0.0) || !plan(P, rows, cols, (int)(atof(argv[5]) / res), (int)(atof(argv[6]) / res), atoi(argv[7]), atoi(argv[8]))) {
            fprintf(stderr, "bad arguments\n");
            return 2;
        }
        std::vector<float> g, m;
        if (!read_floats(argv[9], g, (size_t)rows * (size_t)cols) || (argc > 10 && !read_floats(argv[10], m, (size_t)rows * (size_t)cols))) {
            fprintf(stderr, "cannot read the grid\n");
            return 2;
        }
        Result R;
        run_header(g, P, argc > 10 ? m.data() : nullptr, R);
        printf("checksum %016llx oob %lld\n", (unsigned long long)checksum(R), g_oob);
        return g_oob ? 1 : 0;
    }
    const int shapes[][2] = { { 1, 1 }, { 1, 40 }, { 40, 1 }, { 2, 2 }, { 32, 8 }, { 33, 9 }, { 69, 19 }, { 80, 70 } };
    const int iters[] = { 0, 1, 4, 15 };
    const int radii[] = { 0, 1, 2, 5, 32 };
    for (const auto& s : shapes) {
        const std::vector<float> g = make_grid(s[0], s[1]);
        for (int n_iter : iters)
            for (int radius : radii) {
                if (radius == 32 && (s[0] != 80 || n_iter != 4)) continue;                 // the widest window on the grid it was meant for
                for (int filter = 0; filter < 2; ++filter) {
                    LioMfParams P;
                    if (!plan(P, s[0], s[1], radius, 2, filter, n_iter)) { ++g_bad; continue; }
                    Result a, b;
                    run_header(g, P, nullptr, a);
                    run_plain(g, P, nullptr, b);
                    char what[64];
                    snprintf(what, sizeof(what), "%dx%d N %d R %d filter %d", s[0], s[1], n_iter, radius, filter);
                    compare(what, a, b, true);
                }
            }
        // the mask of a previous run: every third cell
        std::vector<float> m(g.size());
        for (size_t k = 0; k < m.size(); ++k) m[k] = k % 3 == 0 ? 1.0f : 0.0f;
        LioMfParams P;
        plan(P, s[0], s[1], 2, 1, 1, 4);
        Result a, b;
        run_header(g, P, m.data(), a);
        run_plain(g, P, m.data(), b);
        char what[64];
        snprintf(what, sizeof(what), "%dx%d mask_in", s[0], s[1]);
        compare(what, a, b, false);
    }
    printf("out-of-range accesses: %lld, mismatches: %lld\n", g_oob, g_bad);
    const long long rc = g_oob + g_bad;
    return rc > 100 ? 100 : (int)rc;
}
