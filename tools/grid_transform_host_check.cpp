// grid_transform_host_check.cpp -- the arithmetic of lio_grid_transform and lio_grid_to_occupancy
// (lio-slam_amd/csrc/lio_gridtransform.h) run on the host: the text the kernels run -- the new geometry, the samples, the key of
// the order-independent winner rule folded by a plain maximum, the gather -- over arrays that count every access outside them,
// against a literal transcription of the serial loop of GridMap::getTransformedMap (grid_map_core/src/GridMap.cpp:385-433).
// Stand-alone, needs no GPU:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined tools/grid_transform_host_check.cpp -o /tmp/grid_transform_host_check && /tmp/grid_transform_host_check
//
// Prints one line per case with the new size, the three counts, how many new cells each branch of the rule won and a checksum
// (FNV-1a over every layer's words), and "out-of-range accesses: 0, inconsistencies: 0" at the end; the exit status is their sum
// (capped).  The samples are folded in reverse visit order as well: the maximum does not depend on it.
//   grid_transform_host_check dump ROWS COLS RES POS_X POS_Y N_LAYERS HEIGHT_LAYER RATIO T0 .. T11 LAYERS OUT
//       LAYERS: N_LAYERS x rows x cols floats, each layer column-major.  OUT receives int32 rows, cols; double length[2],
//       position[2]; int64 source cells, samples outside, cells written; N_LAYERS new layers; int32 winning visit per new cell
//   grid_transform_host_check occupancy N DATA_MIN DATA_MAX LAYER OUT
//       LAYER: N floats (column-major); OUT receives N int8 in the message's order
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../lio-slam_amd/csrc/lio_gridtransform.h"

static long long g_oob = 0, g_bad = 0;

static uint32_t word(float f) { uint32_t w; memcpy(&w, &f, 4); return w; }
static float from_word(uint32_t w) { float f; memcpy(&f, &w, 4); return f; }

struct Map {                       // a map on the host: n layers of words, column-major
    LioGridGeom G;
    std::vector<std::vector<uint32_t>> layer;
    long long counts[3] = { 0, 0, 0 };                     // source cells, samples outside, cells written
    std::vector<int32_t> winner;   // per new cell: the visit whose values it holds, -1 none
    long long by_branch[2] = { 0, 0 };
};

static bool new_map(const Map& src, const LioGtXf& T, Map& dst)
{
    double centre[2], new_length[2];
    lio_gt_new_extent(src.G.len, src.G.pos, T, centre, new_length);
    int size[2];
    for (int a = 0; a < 2; ++a) {
        const double n = lio_gm_size(new_length[a], src.G.res);
        if (!(n >= 1.0) || !(n < 16777216.0)) return false;
        size[a] = (int)n;
    }
    dst.G = lio_gm_geom(size[0], size[1], src.G.res, centre[0], centre[1]);
    const size_t cells = (size_t)size[0] * (size_t)size[1];
    dst.layer.assign(src.layer.size(), std::vector<uint32_t>(cells, 0x7fc00000u));
    dst.winner.assign(cells, -1);
    return true;
}

struct KeySink {                   // the scatter kernel's atomicMax, one thread
    std::vector<unsigned long long>* keys;
    void put(size_t at, unsigned long long key)
    {
        if (at >= keys->size()) { ++g_oob; return; }
        if (key == 0ull) ++g_bad;
        if (key > (*keys)[at]) (*keys)[at] = key;
    }
};

// the header's path: keys folded by maximum (source cells ascending or descending), then the gather
static bool by_header(const Map& src, const LioGtXf& T, int height, double ratio, bool reversed, Map& dst)
{
    if (!new_map(src, T, dst)) return false;
    const double sample_length = src.G.res * ratio;
    const int n_samples = ratio > 0.0 ? 5 : 1;
    const int n_src = src.G.rows * src.G.cols;
    std::vector<unsigned long long> keys(dst.winner.size(), 0ull);
    KeySink sink = { &keys };
    for (int k = 0; k < n_src; ++k) {
        const int lin = reversed ? n_src - 1 - k : k;
        const float h = from_word(src.layer[height][lin]);
        if (!lio_gm_finite(h)) continue;
        ++dst.counts[0];
        dst.counts[1] += lio_gt_cell(src.G, dst.G, T, sample_length, n_samples, lin, h, sink);
    }
    for (size_t at = 0; at < keys.size(); ++at) {
        if (keys[at] == 0ull) continue;
        const unsigned visit = lio_gt_key_visit(keys[at]);
        const long long lin = visit / 5u;
        if (lin >= n_src) { ++g_oob; continue; }
        ++dst.counts[2];
        ++dst.by_branch[(keys[at] >> 31) & 1ull];
        dst.winner[at] = (int32_t)visit;
        for (size_t l = 0; l < src.layer.size(); ++l) dst.layer[l][at] = src.layer[l][lin];
        dst.layer[height][at] = word(lio_gt_visit_height(src.G, T, sample_length, visit, from_word(src.layer[height][lin])));
    }
    return true;
}

// GM:385-433 as written: the iterator, getPosition3, the samples, transform * position, getIndex, the float against the
// double, the copy of every layer
static bool as_written(const Map& src, const LioGtXf& T, int height, double sampleRatio, Map& newMap)
{
    if (!new_map(src, T, newMap)) return false;
    const double sampleLength = src.G.res * sampleRatio;
    const int rows = src.G.rows, cols = src.G.cols;
    std::vector<double> positionSamples;
    for (int linear = 0; linear < rows * cols; ++linear) {
        const int row = linear % rows, col = linear / rows;
        const float value = from_word(src.layer[height][(size_t)col * rows + row]);
        if (!std::isfinite(value)) continue;
        ++newMap.counts[0];
        const double center[3] = { lio_gm_centre(src.G, 0, row), lio_gm_centre(src.G, 1, col), (double)value };
        positionSamples.clear();
        if (sampleRatio > 0.0) {
            const double five[5][2] = { { center[0], center[1] }, { center[0] - sampleLength, center[1] }, { center[0] + sampleLength, center[1] },
                                        { center[0], center[1] - sampleLength }, { center[0], center[1] + sampleLength } };
            for (const auto& p : five) { positionSamples.push_back(p[0]); positionSamples.push_back(p[1]); }
        } else {
            positionSamples.push_back(center[0]); positionSamples.push_back(center[1]);
        }
        for (size_t s = 0; s < positionSamples.size() / 2; ++s) {
            const double x = positionSamples[2 * s], y = positionSamples[2 * s + 1], z = center[2];
            double transformedPosition[3];
            for (int i = 0; i < 3; ++i) transformedPosition[i] = ((T.m[4 * i] * x + T.m[4 * i + 1] * y) + T.m[4 * i + 2] * z) + T.m[4 * i + 3];
            int newIndex[2];
            if (!lio_gm_index(newMap.G, transformedPosition[0], transformedPosition[1], &newIndex[0], &newIndex[1])) { ++newMap.counts[1]; continue; }
            const size_t at = (size_t)newIndex[1] * (size_t)newMap.G.rows + (size_t)newIndex[0];
            if (at >= newMap.winner.size()) { ++g_oob; continue; }
            const float newExistingValue = from_word(newMap.layer[height][at]);
            if (!std::isnan(newExistingValue) && newExistingValue > transformedPosition[2]) continue;
            for (size_t l = 0; l < src.layer.size(); ++l) newMap.layer[l][at] = (int)l == height ? word((float)transformedPosition[2]) : src.layer[l][linear];
            newMap.winner[at] = (int32_t)(5 * linear + (int)s);
        }
    }
    for (int32_t w : newMap.winner) newMap.counts[2] += w >= 0;
    return true;
}

static uint64_t checksum(const Map& m)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (const auto& l : m.layer)
        for (uint32_t w : l)
            for (int k = 0; k < 4; ++k) h = (h ^ ((w >> (8 * k)) & 0xffu)) * 0x100000001b3ull;
    return h;
}

static long long differences(const Map& a, const Map& b)
{
    long long d = 0;
    d += a.G.rows != b.G.rows || a.G.cols != b.G.cols || a.layer.size() != b.layer.size();
    if (d) return d;
    for (int k = 0; k < 3; ++k) d += a.counts[k] != b.counts[k];
    for (size_t l = 0; l < a.layer.size(); ++l)
        for (size_t at = 0; at < a.layer[l].size(); ++at) d += a.layer[l][at] != b.layer[l][at];
    for (size_t at = 0; at < a.winner.size(); ++at) d += a.winner[at] != b.winner[at];
    return d;
}

static LioGtXf rotation(double yaw, double pitch, double tx, double ty, double tz)
{
    const double cy = cos(yaw), sy = sin(yaw), cp = cos(pitch), sp = sin(pitch);
    const LioGtXf T = { { cy * cp, -sy, cy * sp, tx, sy * cp, cy, sy * sp, ty, -sp, 0.0, cp, tz } };
    return T;
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
    if (argc == 7 && !strcmp(argv[1], "occupancy")) {
        const size_t n = (size_t)atoll(argv[2]);
        const float lo = (float)atof(argv[3]), hi = (float)atof(argv[4]);
        std::vector<float> layer(n);
        if (!read_file(argv[5], layer.data(), 4 * n)) { fprintf(stderr, "cannot read the layer\n"); return 2; }
        std::vector<int8_t> data(n);
        for (size_t k = 0; k < n; ++k) data[n - 1 - k] = lio_gt_occupancy(layer[k], lo, hi);
        FILE* f = fopen(argv[6], "wb");
        if (!f) { fprintf(stderr, "cannot write\n"); return 2; }
        fwrite(data.data(), 1, n, f);
        fclose(f);
        return 0;
    }
    if (argc == 24 && !strcmp(argv[1], "dump")) {
        const int rows = atoi(argv[2]), cols = atoi(argv[3]), n_layers = atoi(argv[7]), height = atoi(argv[8]);
        const double res = atof(argv[4]), ratio = atof(argv[9]);
        if (rows < 1 || cols < 1 || !(res > 0.0) || n_layers < 1 || n_layers > LIO_GRID_MAX_LAYERS || height < 0 || height >= n_layers) { fprintf(stderr, "bad arguments\n"); return 2; }
        Map src, dst;
        src.G = lio_gm_geom(rows, cols, res, atof(argv[5]), atof(argv[6]));
        LioGtXf T;
        for (int k = 0; k < 12; ++k) T.m[k] = atof(argv[10 + k]);
        const size_t cells = (size_t)rows * (size_t)cols;
        src.layer.assign(n_layers, std::vector<uint32_t>(cells));
        std::vector<uint32_t> all(cells * n_layers);
        if (!read_file(argv[22], all.data(), 4 * all.size())) { fprintf(stderr, "cannot read the layers\n"); return 2; }
        for (int l = 0; l < n_layers; ++l) memcpy(src.layer[l].data(), all.data() + (size_t)l * cells, 4 * cells);
        if (!by_header(src, T, height, ratio, false, dst)) { fprintf(stderr, "no new map\n"); return 3; }
        FILE* f = fopen(argv[23], "wb");
        if (!f) { fprintf(stderr, "cannot write\n"); return 2; }
        const int32_t size[2] = { dst.G.rows, dst.G.cols };
        const double geo[4] = { dst.G.len[0], dst.G.len[1], dst.G.pos[0], dst.G.pos[1] };
        const int64_t counts[3] = { dst.counts[0], dst.counts[1], dst.counts[2] };
        fwrite(size, 4, 2, f); fwrite(geo, 8, 4, f); fwrite(counts, 8, 3, f);
        for (const auto& l : dst.layer) fwrite(l.data(), 4, l.size(), f);
        fwrite(dst.winner.data(), 4, dst.winner.size(), f);
        fclose(f);
        printf("oob %lld\n", g_oob);
        return g_oob ? 1 : 0;
    }
    struct Case { const char* name; int rows, cols; double res, px, py, yaw, pitch, tx, ty, tz, ratio; int kind; };
    const double deg = 3.14159265358979323846 / 180.0;
    const Case cases[] = {
        { "reference literal", 10, 20, 0.1, 0, 0, 90 * deg, 0, 0, 0, 0, 0.25, 0 },
        { "identity", 8, 12, 0.25, 0, 0, 0, 0, 0, 0, 0, 0.0, 1 },
        { "ties, yaw 30", 67, 45, 0.25, 1.5, -2.25, 30 * deg, 0, 3, -1, 0.5, 0.25, 2 },
        { "float class, pitch 1e-9", 33, 21, 0.25, 0, 0, 0, 1e-9, 0, 0, 0, 0.6, 2 },
        { "float class, pitch -3e-8", 33, 21, 0.25, 0, 0, 0.3, -3e-8, 0, 0, 0, 0.6, 2 },
        { "contention, pitch 80", 64, 64, 0.25, 0, 0, 0, 80 * deg, 0, 0, 0, 0.25, 1 },
        { "holes, ratio 0.6", 40, 31, 0.2, 1e3, -3e3, -2.0, 0.05, -7, 2, 1, 0.6, 3 },
        { "1 x 1", 1, 1, 0.5, 0, 0, 1.0, 0, 0, 0, 0, 0.25, 1 },
        { "1 x 300", 1, 300, 0.5, -2, 7, 0.7, 0.1, 0, 0, 0, 0.25, 1 },
        { "zeros of both signs", 9, 9, 0.25, 0, 0, 0.5, 0, 0, 0, 0, 0.6, 4 },
    };
    for (const Case& c : cases) {
        Map src;
        src.G = lio_gm_geom(c.rows, c.cols, c.res, c.px, c.py);
        const size_t cells = (size_t)c.rows * (size_t)c.cols;
        src.layer.assign(3, std::vector<uint32_t>(cells));
        uint32_t seed = 12345u + (uint32_t)cells;
        for (size_t k = 0; k < cells; ++k) {
            seed = seed * 1664525u + 1013904223u;
            const float u = (float)(seed >> 8) / 16777216.0f;
            float h = c.kind == 0 ? (k == 0 ? 1.0f : 0.0f) : c.kind == 2 ? 1.0f : c.kind == 4 ? ((seed >> 7) & 1u ? -0.0f : 0.0f) : 2.0f * u - 1.0f;
            if (c.kind == 3 && (seed >> 3) % 7u == 0u) h = (seed >> 6) & 1u ? __builtin_nanf("") : __builtin_huge_valf();
            src.layer[0][k] = word(h);
            src.layer[1][k] = (seed >> 5) % 11u == 0u ? 0x7fc12345u : word(u);
            src.layer[2][k] = word((float)k);
        }
        const LioGtXf T = rotation(c.yaw, c.pitch, c.tx, c.ty, c.tz);
        Map a, b, w;
        if (!by_header(src, T, 0, c.ratio, false, a) || !by_header(src, T, 0, c.ratio, true, b) || !as_written(src, T, 0, c.ratio, w)) {
            printf("%-26s no new map\n", c.name);
            ++g_bad;
            continue;
        }
        const long long d = differences(a, w) + differences(b, w);
        g_bad += d;
        printf("%-26s %3dx%-3d -> %3dx%-3d  source %5lld outside %5lld written %5lld  last-of-high %5lld first-of-class %5lld  checksum %016llx%s\n", c.name,
               c.rows, c.cols, a.G.rows, a.G.cols, a.counts[0], a.counts[1], a.counts[2], a.by_branch[1], a.by_branch[0], (unsigned long long)checksum(a),
               d ? "  DIFFERS from the serial loop" : "");
    }
    {                                                      // the occupancy cell on its edges
        const float nanf_ = __builtin_nanf(""), inf = __builtin_huge_valf();
        const float v[] = { nanf_, -inf, -1.0f, 0.0f, 0.004f, 0.5f, 0.999f, 1.0f, 7.0f, inf };
        const int want01[] = { -1, 0, 0, 0, 0, 50, 99, 100, 100, 100 }, want11[] = { -1, 0, 0, 0, 0, 0, 0, -1, 100, 100 };
        for (int k = 0; k < 10; ++k) {
            g_bad += lio_gt_occupancy(v[k], 0.0f, 1.0f) != want01[k];
            g_bad += lio_gt_occupancy(v[k], 1.0f, 1.0f) != want11[k];
        }
        for (int k = -1; k <= 100; ++k) g_bad += lio_gt_occupancy(k < 0 ? nanf_ : (float)k, -1.0f, 100.0f) != k;         // roundTrip
    }
    printf("out-of-range accesses: %lld, inconsistencies: %lld\n", g_oob, g_bad);
    const long long rc = g_oob + g_bad;
    return rc > 100 ? 100 : (int)rc;
}
