// sdf_host_check.cpp -- the arithmetic of the signed distance field (lio-slam_amd/csrc/lio_sdf.h) run on the host: the text
// the kernels run, over accessors that count every read or write outside a line, the lower-bound stack, the distance layers
// and the nodes, against the brute-force definition in fp64 at the reference's own 1e-4.  Stand-alone, needs no GPU:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined tools/sdf_host_check.cpp -o /tmp/sdf_host_check && /tmp/sdf_host_check
//
// Prints one line per case and "out-of-range accesses: 0, mismatches: 0" at the end; the exit status is their sum (capped).
//   sdf_host_check time ROWS COLS RES BAND [IN] single-thread build time (IN: the grid of tools/sdf_cost.py --write-grid; else a synthetic terrain)
//   sdf_host_check dump ROWS COLS RES MIN MAX POLICY IN OUT
//                                              IN: rows x cols floats, column-major; OUT: the nodes in data_ order (MIN / MAX: nan = the layer's)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "../lio-slam_amd/csrc/lio_sdf.h"

static long long g_oob = 0, g_bad = 0;

struct CheckedLine {               // n floats, entry q at base[q * pitch]
    const float* base;
    size_t pitch;
    int n;
    float at(int q) const
    {
        if (q < 0 || q >= n) { ++g_oob; return 0.0f; }
        return base[(size_t)q * pitch];
    }
};
struct ElevLine {                  // a column of the elevation layer as the offsets of one (layer, class)
    CheckedLine col;
    float h, inv_res, fill;
    int cls;
    float at(int q) const
    {
        float e = col.at(q);
        if (!lio_gm_finite(e)) e = fill;
        return lio_sdf_init(e, h, inv_res, cls);
    }
};
struct OccLine {
    const int8_t* col;
    int n, occupied_min, cls;
    float at(int q) const
    {
        if (q < 0 || q >= n) { ++g_oob; return 0.0f; }
        return lio_sdf_init_occupancy((int)col[q] >= occupied_min, cls);
    }
};
struct CheckedStack {
    std::vector<int>* bv;
    std::vector<float>* bz;
    bool ok(int k) const { if (k < 0 || k >= (int)bv->size()) { ++g_oob; return false; } return true; }
    int v(int k) const { return ok(k) ? (*bv)[(size_t)k] : 0; }
    float z(int k) const { return ok(k) ? (*bz)[(size_t)k] : LIO_SDF_INF; }
    void set(int k, int v, float z) { if (ok(k)) { (*bv)[(size_t)k] = v; (*bz)[(size_t)k] = z; } }
    void set_z(int k, float z) { if (ok(k)) (*bz)[(size_t)k] = z; }
};
struct CheckedDist {
    const std::vector<float>* d;
    int rows, cols, layers;
    float at(int r, int c, int z) const
    {
        if (r < 0 || r >= rows || c < 0 || c >= cols || z < 0 || z >= layers) { ++g_oob; return 0.0f; }
        return (*d)[((size_t)z * (size_t)cols + (size_t)c) * (size_t)rows + (size_t)r];
    }
};
struct CheckedNodes {
    const std::vector<float4>* n;
    float4 at(size_t i) const
    {
        if (i >= n->size()) { ++g_oob; return make_float4(0, 0, 0, 0); }
        return (*n)[i];
    }
};

// computePixelDistance2dTranspose of one class: `first` gives the column lines, out (rows x cols, column-major) the distances
template <class MakeLine>
static void pixel_distance(int rows, int cols, const MakeLine& column, std::vector<float>& mid, std::vector<float>& out)
{
    std::vector<int> bv((size_t)std::max(rows, cols));
    std::vector<float> bz((size_t)std::max(rows, cols));
    mid.assign((size_t)rows * (size_t)cols, 0.0f);
    out.assign((size_t)rows * (size_t)cols, 0.0f);
    for (int c = 0; c < cols; ++c) {
        const auto line = column(c);
        bv.resize((size_t)rows); bz.resize((size_t)rows);
        CheckedStack st = { &bv, &bz };
        LioSdfCursor<false> cur;
        cur.begin(line, rows, st);
        for (int r = 0; r < rows; ++r) mid[(size_t)c * (size_t)rows + (size_t)r] = cur.at(line, st, r);
    }
    for (int r = 0; r < rows; ++r) {
        const CheckedLine line = { mid.data() + r, (size_t)rows, cols };
        bv.resize((size_t)cols); bz.resize((size_t)cols);
        CheckedStack st = { &bv, &bz };
        LioSdfCursor<true> cur;
        cur.begin(line, cols, st);
        for (int c = 0; c < cols; ++c) out[(size_t)c * (size_t)rows + (size_t)r] = cur.at(line, st, c);
    }
}

struct Field {
    LioSdfLookup L;
    std::vector<float> dist;
    std::vector<float4> nodes;
    std::vector<float> heights;
    float e_min, e_max;
    int n_nan;
};

// SignedDistanceField's constructor; false: no finite cell, or a non-finite one under policy 0
static bool build_field(const std::vector<float>& elev, int rows, int cols, double res, double min_h, double max_h, int policy, Field& F)
{
    float mn = INFINITY, mx = -INFINITY;
    F.n_nan = 0;
    for (float v : elev) {
        if (lio_gm_finite(v)) { mn = fminf(mn, v); mx = fmaxf(mx, v); } else ++F.n_nan;
    }
    if (!(mn <= mx) || (F.n_nan && policy == 0)) return false;
    F.e_min = mn; F.e_max = mx;
    if (std::isnan(min_h)) min_h = mn;
    if (std::isnan(max_h)) max_h = mx;
    F.L.rows = rows; F.L.cols = cols; F.L.layers = (int)lio_sdf_num_layers(min_h, max_h, res); F.L.res = res;
    F.L.origin[0] = 0.5 * rows * res - 0.5 * res; F.L.origin[1] = 0.5 * cols * res - 0.5 * res; F.L.origin[2] = min_h;
    const float resf = (float)res, inv = 1.0f / resf, oz = (float)min_h;
    const size_t cells = (size_t)rows * (size_t)cols;
    F.dist.assign(cells * (size_t)F.L.layers, 0.0f);
    F.heights.clear();
    std::vector<float> mid, d[2];
    for (int z = 0; z < F.L.layers; ++z) {
        const float h = lio_sdf_layer_height(oz, resf, z);
        F.heights.push_back(h);
        const int mode = lio_sdf_layer_mode(h, mn, mx);
        for (int cls = 0; cls < 2; ++cls) {
            if (!lio_sdf_mode_uses(mode, cls)) { d[cls].assign(cells, 0.0f); continue; }
            pixel_distance(rows, cols, [&](int c) { return ElevLine{ { elev.data() + (size_t)c * (size_t)rows, 1, rows }, h, inv, mn, cls }; }, mid, d[cls]);
        }
        for (size_t i = 0; i < cells; ++i) F.dist[(size_t)z * cells + i] = lio_sdf_combine(mode, d[0][i], d[1][i], resf);
    }
    const CheckedDist D = { &F.dist, rows, cols, F.L.layers };
    F.nodes.resize(F.dist.size());
    for (int z = 0; z < F.L.layers; ++z)
        for (int c = 0; c < cols; ++c)
            for (int r = 0; r < rows; ++r) F.nodes[((size_t)z * (size_t)cols + (size_t)c) * (size_t)rows + (size_t)r] = lio_sdf_node(D, r, c, z, rows, cols, F.L.layers, resf);
    return true;
}

// the definition, fp64: cell centre to the border of the nearest cell column of the other class
static double brute(const std::vector<float>& elev, int rows, int cols, double res, double h, int r, int c)
{
    const bool below = (double)elev[(size_t)c * (size_t)rows + (size_t)r] >= h;
    double best = INFINITY;
    for (int j = 0; j < cols; ++j)
        for (int i = 0; i < rows; ++i) {
            const double e = elev[(size_t)j * (size_t)rows + (size_t)i];
            const double dx = res * std::max(std::fabs((double)(i - r)) - 0.5, 0.0), dy = res * std::max(std::fabs((double)(j - c)) - 0.5, 0.0);
            const double dz = below ? std::max(e - h, 0.0) : std::max(h - e, 0.0);
            best = std::min(best, std::sqrt(dx * dx + dy * dy + dz * dz));
        }
    return below ? -best : best;
}

static void check_field(const char* name, const std::vector<float>& elev, int rows, int cols, double res, double min_h, double max_h, int policy = 0, bool n2 = true)
{
    Field F;
    if (!build_field(elev, rows, cols, res, min_h, max_h, policy, F)) { printf("field %-16s %3d x %3d: refused (%d non-finite)\n", name, rows, cols, F.n_nan); return; }
    std::vector<float> clean = elev;
    for (float& v : clean) if (!lio_gm_finite(v)) v = F.e_min;
    double worst = 0.0;
    long long bad = 0;
    for (int z = 0; n2 && z < F.L.layers; ++z)
        for (int c = 0; c < cols; ++c)
            for (int r = 0; r < rows; ++r) {
                const double want = brute(clean, rows, cols, (double)(float)res, (double)F.heights[(size_t)z], r, c);
                const double dev = std::fabs((double)F.nodes[((size_t)z * (size_t)cols + (size_t)c) * (size_t)rows + (size_t)r].x - want);
                worst = std::max(worst, dev);
                if (!(dev < 1e-4)) ++bad;
            }
    // the lookup: every node centre returns the node, and positions far outside stay inside the arrays
    const CheckedNodes N = { &F.nodes };
    for (int k = 0; k < 64; ++k) {
        const double p[3] = { F.L.origin[0] - (k % 9 - 2) * 0.37 * rows * res, F.L.origin[1] - (k % 7 - 2) * 0.41 * cols * res,
                              F.L.origin[2] + (k % 5 - 1) * 0.6 * F.L.layers * res };
        double der[3];
        (void)lio_sdf_value(F.L, N, p, der);
    }
    g_bad += bad;
    if (n2) printf("field %-16s %3d x %3d x %2d res %.3g: worst deviation from the definition %.3g, mismatches %lld\n", name, rows, cols, F.L.layers, res, worst, bad);
    else printf("field %-16s %3d x %3d x %2d res %.3g: accesses only (no N^2 check)\n", name, rows, cols, F.L.layers, res);
}

static void check_occupancy(const char* name, const std::vector<int8_t>& occ, int rows, int cols, float res, int occupied_min)
{
    std::vector<float> mid, d[2];
    for (int cls = 0; cls < 2; ++cls)
        pixel_distance(rows, cols, [&](int c) { return OccLine{ occ.data() + (size_t)c * (size_t)rows, rows, occupied_min, cls }; }, mid, d[cls]);
    long long bad = 0, n_occ = 0;
    for (int8_t v : occ) n_occ += v >= occupied_min ? 1 : 0;
    double worst = 0.0;
    if (n_occ != 0 && n_occ != (long long)occ.size())
        for (int c = 0; c < cols; ++c)
            for (int r = 0; r < rows; ++r) {
                const bool me = occ[(size_t)c * (size_t)rows + (size_t)r] >= occupied_min;
                double best = INFINITY;
                for (int j = 0; j < cols; ++j)
                    for (int i = 0; i < rows; ++i) {
                        if ((occ[(size_t)j * (size_t)rows + (size_t)i] >= occupied_min) == me) continue;
                        const double dx = (double)res * std::max(std::fabs((double)(i - r)) - 0.5, 0.0), dy = (double)res * std::max(std::fabs((double)(j - c)) - 0.5, 0.0);
                        best = std::min(best, std::sqrt(dx * dx + dy * dy));
                    }
                const size_t at = (size_t)c * (size_t)rows + (size_t)r;
                const double dev = std::fabs((double)lio_sdf_combine(LIO_SDF_MIXED, d[0][at], d[1][at], res) - (me ? -best : best));
                worst = std::max(worst, dev);
                if (!(dev < 1e-4)) ++bad;
            }
    g_bad += bad;
    printf("occupancy %-12s %3d x %3d res %.3g: %lld obstacles, worst deviation %.3g, mismatches %lld\n", name, rows, cols, res, n_occ, worst, bad);
}

struct Rng {
    uint64_t s;
    double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
    float range(double lo, double hi) { return (float)(lo + (hi - lo) * uni()); }
};

static std::vector<float> terrain(int rows, int cols, int kind, Rng& rng)
{
    std::vector<float> e((size_t)rows * (size_t)cols);
    for (int c = 0; c < cols; ++c)
        for (int r = 0; r < rows; ++r) {
            float v = 0.0f;
            switch (kind) {
            case 0: v = rng.range(-1, 1); break;                                       // random
            case 1: v = 0.5f; break;                                                   // constant
            case 2: v = 0.4f * (float)((r / 7 + c / 11) % 3); break;                   // plateaus and steps
            case 3: v = (r == rows / 2 && c == cols / 3) ? 1.5f : 0.0f; break;         // a spike
            case 4: v = (r == rows / 3 && c == cols / 2) ? -1.5f : 0.0f; break;        // a pit
            case 5: v = 0.05f * (float)r; break;                                       // a ramp along x
            case 6: v = 0.03f * (float)c; break;                                       // a ramp along y
            default: v = 0.3f * sinf(0.3f * (float)r) * cosf(0.2f * (float)c) + 0.02f * (float)((r * 31 + c * 17) % 13); break;
            }
            e[(size_t)c * (size_t)rows + (size_t)r] = v;
        }
    return e;
}

int main(int argc, char** argv)
{
    Rng rng = { 41 };
    if (argc >= 6 && !strcmp(argv[1], "time")) {
        const int rows = atoi(argv[2]), cols = atoi(argv[3]);
        const double res = atof(argv[4]), band = atof(argv[5]);
        std::vector<float> e = terrain(rows, cols, 7, rng);
        if (argc >= 7) {                                                               // the grid of tools/sdf_cost.py --write-grid
            FILE* f = fopen(argv[6], "rb");
            if (!f || fread(e.data(), sizeof(float), e.size(), f) != e.size()) return 2;
            fclose(f);
        }
        Field F;
        const auto t0 = std::chrono::steady_clock::now();
        const float mn = *std::min_element(e.begin(), e.end());
        if (!build_field(e, rows, cols, res, mn, (double)mn + band, 0, F)) return 2;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("{\"rows\": %d, \"cols\": %d, \"layers\": %d, \"host_single_thread_ms\": %.3f, \"out_of_range\": %lld}\n", rows, cols, F.L.layers, ms, g_oob);
        return g_oob ? 1 : 0;
    }
    if (argc >= 10 && !strcmp(argv[1], "dump")) {
        const int rows = atoi(argv[2]), cols = atoi(argv[3]);
        std::vector<float> e((size_t)rows * (size_t)cols);
        FILE* f = fopen(argv[8], "rb");
        if (!f || fread(e.data(), sizeof(float), e.size(), f) != e.size()) return 2;
        fclose(f);
        Field F;
        if (!build_field(e, rows, cols, atof(argv[4]), atof(argv[5]), atof(argv[6]), atoi(argv[7]), F)) return 3;
        f = fopen(argv[9], "wb");
        if (!f || fwrite(F.nodes.data(), sizeof(float4), F.nodes.size(), f) != F.nodes.size()) return 2;
        fclose(f);
        printf("%d %d %d %lld\n", rows, cols, F.L.layers, g_oob);
        return g_oob ? 1 : 0;
    }
    // the grids of tests/test_gpu_sdf.py: the smallest, odd sizes, a full wave and tile, astride one in both passes, corridors
    const int shapes[][2] = { { 2, 2 }, { 3, 4 }, { 20, 30 }, { 33, 65 }, { 65, 33 }, { 64, 64 } };
    for (const auto& s : shapes)
        for (int kind = 0; kind < 7; ++kind) {
            if (s[0] > 30 && kind != 0 && kind != 2) continue;                         // (the N^2 check of the larger ones takes seconds)
            char name[32];
            snprintf(name, sizeof(name), "kind%d", kind);
            check_field(name, terrain(s[0], s[1], kind, rng), s[0], s[1], s[0] > 30 ? 0.2 : 0.1, NAN, NAN);
        }
    {                                                                                  // 129 x 70 with its two bands (40 layers: two slabs on the device), corridors both ways
        const std::vector<float> e = terrain(129, 70, 0, rng);
        check_field("129x70 band 23", e, 129, 70, 0.1, -1.15, 1.15, 0, false);
        check_field("129x70 band 40", e, 129, 70, 0.1, -2.0, 2.0, 0, false);
        check_field("corridor", terrain(600, 3, 0, rng), 600, 3, 0.1, NAN, NAN, 0, false);
        check_field("corridor", terrain(3, 600, 0, rng), 3, 600, 0.1, NAN, NAN, 0, false);
    }
    {
        const std::vector<float> e = terrain(20, 30, 0, rng);
        check_field("band above", e, 20, 30, 0.1, 1.5, 2.0);
        check_field("band below", e, 20, 30, 0.1, -2.0, -1.5);
        check_field("wide band", e, 20, 30, 0.1, -1.5, 1.5);
        std::vector<float> holes = e;
        holes[7] = NAN; holes[100] = INFINITY; holes[333] = -INFINITY;
        check_field("holes, refused", holes, 20, 30, 0.1, NAN, NAN, 0);
        check_field("holes, filled", holes, 20, 30, 0.1, NAN, NAN, 1);
        std::vector<float> on = terrain(9, 8, 2, rng);                                 // layer heights exactly on an elevation value
        check_field("on a value", on, 9, 8, 0.2, 0.0, 0.8);
    }
    for (const auto& s : shapes) {
        std::vector<int8_t> occ((size_t)s[0] * (size_t)s[1]);
        for (int8_t& v : occ) v = rng.uni() < 0.2 ? 100 : 0;
        check_occupancy("random", occ, s[0], s[1], 1.0f, 100);
        check_occupancy("none", occ, s[0], s[1], 0.1f, 101);
        check_occupancy("all", occ, s[0], s[1], 0.1f, 0);
        std::fill(occ.begin(), occ.end(), (int8_t)0);
        occ[0] = occ[(size_t)s[0] - 1] = occ[occ.size() - 1] = occ[occ.size() - (size_t)s[0]] = 100;          // the four corners
        check_occupancy("corners", occ, s[0], s[1], 0.1f, 100);
        std::fill(occ.begin(), occ.end(), (int8_t)100);
        occ[occ.size() / 2] = 0;
        check_occupancy("one free", occ, s[0], s[1], 0.1f, 100);
    }
    printf("out-of-range accesses: %lld, mismatches: %lld\n", g_oob, g_bad);
    return (int)std::min<long long>(g_oob + g_bad, 100);
}
