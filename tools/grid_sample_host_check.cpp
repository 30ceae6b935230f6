// grid_sample_host_check.cpp -- the arithmetic of the layer sampling (lio-slam_amd/csrc/lio_gridsample.h) run on the host: the
// text the kernel runs, over an accessor that counts every read outside the layer, on the border lattice of the tests (every
// cell centre, edge, corner and quadrant, both map edges and one step beyond them) for all four methods and both border
// modes, on grids with and without holes.  Stand-alone, needs no GPU:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined tools/grid_sample_host_check.cpp -o /tmp/grid_sample_host_check && /tmp/grid_sample_host_check
//
// Prints one line per grid, method and border mode with the counts per method used and a checksum (FNV-1a over the values'
// words, then the method bytes), then the single-thread time per query and method on a 550 x 400 layer, and "out-of-range
// accesses: 0, inconsistencies: 0" at the end; the exit status is their sum (capped).
//   grid_sample_host_check dump ROWS COLS RES POS_X POS_Y METHOD BORDER LAYER POSITIONS N OUT
//       LAYER: rows x cols floats, column-major; POSITIONS: N pairs of doubles; OUT receives N floats, then N method bytes
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <vector>

#include "../lio-slam_amd/csrc/lio_gridsample.h"

static long long g_oob = 0, g_bad = 0;

struct CheckedLayer {
    const float* g;
    int rows, cols;
    float at(int r, int c) const
    {
        if (r < 0 || r >= rows || c < 0 || c >= cols) { ++g_oob; return 0.0f; }
        return g[(size_t)r + (size_t)c * (size_t)rows];
    }
    float at_lin(int k) const
    {
        if (k < 0 || (long long)k >= (long long)rows * cols) { ++g_oob; return 0.0f; }
        return g[k];
    }
};

static void run(const LioGridGeom& G, const std::vector<float>& layer, const std::vector<double>& pos, int method, int border, std::vector<float>& val,
                std::vector<unsigned char>& used)
{
    const size_t n = pos.size() / 2;
    val.assign(n, 0.0f);
    used.assign(n, 0);
    const CheckedLayer in = { layer.data(), G.rows, G.cols };
    for (size_t q = 0; q < n; ++q) {
        LioGsQuery Q;
        lio_gs_query(G, method, border, pos[2 * q], pos[2 * q + 1], &Q);
        float v;
        used[q] = (unsigned char)lio_gs_eval(G, Q, method, in, &v);
        memcpy(&val[q], &v, 4);
    }
}

static uint64_t checksum(const std::vector<float>& val, const std::vector<unsigned char>& used)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (float f : val) {
        uint32_t w;
        memcpy(&w, &f, 4);
        if (f != f) w = 0x7fc00000u;                       // (a NaN out of the arithmetic: its payload is the compiler's)
        for (int k = 0; k < 4; ++k) h = (h ^ ((w >> (8 * k)) & 0xffu)) * 0x100000001b3ull;
    }
    for (unsigned char b : used) h = (h ^ b) * 0x100000001b3ull;
    return h;
}

// the lattice of tests/grid_sample_restate.py border_lattice
static std::vector<double> lattice(const LioGridGeom& G)
{
    std::vector<double> ax[2];
    for (int a = 0; a < 2; ++a) {
        const int n = a == 0 ? G.rows : G.cols;
        const double hi = G.pos[a] + G.half[a], lo = G.pos[a] - G.half[a];
        for (int k = 0; k <= n; ++k) {
            const double edge = hi - k * G.res;
            ax[a].push_back(edge);
            if (k < n) { ax[a].push_back(edge - 0.25 * G.res); ax[a].push_back(edge - 0.5 * G.res); ax[a].push_back(edge - 0.75 * G.res); }
        }
        const double more[] = { hi + 0.3 * G.res, hi + G.res, lo - 0.3 * G.res, lo - G.res, nextafter(hi, 1e300), nextafter(lo, 1e300) };
        for (double v : more) ax[a].push_back(v);
    }
    std::vector<double> p;
    for (double x : ax[0])
        for (double y : ax[1]) { p.push_back(x); p.push_back(y); }
    const double odd[] = { __builtin_nan(""), 0.0, 0.0, __builtin_huge_val(), -__builtin_huge_val(), __builtin_nan("") };
    for (double v : odd) p.push_back(v);
    return p;
}

static bool read_file(const char* path, void* dst, size_t bytes)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t got = fread(dst, 1, bytes, f);
    fclose(f);
    return got == bytes;
}

int main(int argc, char** argv)
{
    if (argc >= 13 && !strcmp(argv[1], "dump")) {
        const int rows = atoi(argv[2]), cols = atoi(argv[3]), method = atoi(argv[7]), border = atoi(argv[8]);
        const double res = atof(argv[4]);
        const size_t n = (size_t)atoll(argv[11]);
        if (rows < 1 || cols < 1 || !(res > 0.0) || method < 0 || method > 3 || border < 0 || border > 1) { fprintf(stderr, "bad arguments\n"); return 2; }
        const LioGridGeom G = lio_gm_geom(rows, cols, res, atof(argv[5]), atof(argv[6]));
        std::vector<float> layer((size_t)rows * (size_t)cols);
        std::vector<double> pos(2 * n);
        if (!read_file(argv[9], layer.data(), 4 * layer.size()) || !read_file(argv[10], pos.data(), 8 * pos.size())) { fprintf(stderr, "cannot read the inputs\n"); return 2; }
        std::vector<float> val;
        std::vector<unsigned char> used;
        run(G, layer, pos, method, border, val, used);
        FILE* f = fopen(argv[12], "wb");
        if (!f) { fprintf(stderr, "cannot write\n"); return 2; }
        fwrite(val.data(), 4, n, f);
        fwrite(used.data(), 1, n, f);
        fclose(f);
        printf("oob %lld\n", g_oob);
        return g_oob ? 1 : 0;
    }
    const int shapes[][2] = { { 1, 1 }, { 2, 2 }, { 1, 7 }, { 5, 4 }, { 4, 5 }, { 12, 9 } };
    const char* names[] = { "nearest", "linear", "cubic convolution", "cubic" };
    for (const auto& s : shapes)
        for (int holes = 0; holes < 2; ++holes) {
            const LioGridGeom G = lio_gm_geom(s[0], s[1], 0.2, holes ? 1e4 : 0.0, holes ? -3e4 : 0.0);
            std::vector<float> layer((size_t)s[0] * (size_t)s[1]);
            for (size_t k = 0; k < layer.size(); ++k) layer[k] = 1.0f + 0.37f * (float)k + 0.01f * (float)(k * k % 7);
            if (holes && layer.size() > 4) {
                layer[1] = __builtin_nanf("");
                layer[layer.size() / 2] = __builtin_huge_valf();
                layer[layer.size() - 2] = -__builtin_huge_valf();
                layer[3] = __builtin_nanf("0x1234");
            }
            const std::vector<double> pos = lattice(G);
            for (int method = 0; method < 4; ++method)
                for (int border = 0; border < 2; ++border) {
                    std::vector<float> val;
                    std::vector<unsigned char> used;
                    run(G, layer, pos, method, border, val, used);
                    long long cnt[5] = { 0, 0, 0, 0, 0 };
                    for (size_t q = 0; q < used.size(); ++q) {
                        const int u = used[q];
                        ++cnt[u == LIO_GRID_OUTSIDE ? 4 : u];
                        // what must hold whatever the values: a method above the one asked for is never used, nearest returns
                        // a cell's bits, the clamped border mode never falls back from linear on a layer without holes
                        if (u != LIO_GRID_OUTSIDE && u > method) ++g_bad;
                        if (u != LIO_GRID_OUTSIDE && u != method && u != LIO_GRID_LINEAR && u != LIO_GRID_NEAREST) ++g_bad;
                        if (border == 1 && method >= 1 && !holes && u != LIO_GRID_OUTSIDE && u != method) ++g_bad;
                    }
                    printf("%2dx%-2d %s %-17s border %d  nearest %5lld linear %5lld conv %5lld cubic %5lld outside %5lld  checksum %016llx\n", s[0], s[1],
                           holes ? "holes" : "plain", names[method], border, cnt[0], cnt[1], cnt[2], cnt[3], cnt[4], (unsigned long long)checksum(val, used));
                }
        }
    {                                                      // the single-thread cost of a query
        const LioGridGeom G = lio_gm_geom(550, 400, 0.2, 0.0, 0.0);
        std::vector<float> layer((size_t)550 * 400);
        for (size_t k = 0; k < layer.size(); ++k) layer[k] = 0.001f * (float)(k % 977);
        uint32_t seed = 12345u;
        std::vector<double> pos(2 * 200000);
        for (size_t q = 0; q < pos.size() / 2; ++q) {
            seed = seed * 1664525u + 1013904223u;
            pos[2 * q] = ((double)(seed >> 8) / 16777216.0 - 0.5) * 0.98 * G.len[0];
            seed = seed * 1664525u + 1013904223u;
            pos[2 * q + 1] = ((double)(seed >> 8) / 16777216.0 - 0.5) * 0.98 * G.len[1];
        }
        for (int method = 0; method < 4; ++method) {
            std::vector<float> val;
            std::vector<unsigned char> used;
            const auto t0 = std::chrono::steady_clock::now();
            run(G, layer, pos, method, 0, val, used);
            const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
            printf("single thread, 550 x 400, %-17s %8.1f ns per query  (checksum %016llx)\n", names[method], ns / (double)(pos.size() / 2),
                   (unsigned long long)checksum(val, used));
        }
    }
    printf("out-of-range accesses: %lld, inconsistencies: %lld\n", g_oob, g_bad);
    const long long rc = g_oob + g_bad;
    return rc > 100 ? 100 : (int)rc;
}
