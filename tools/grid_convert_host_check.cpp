// grid_convert_host_check.cpp -- the arithmetic and the index maps of lio_grid_to_image, lio_grid_add_layer_from_image,
// lio_grid_add_color_layer_from_image, lio_grid_from_occupancy, lio_grid_to_point_cloud, lio_grid_to_grid_cells and
// lio_sdf_to_point_cloud (lio-slam_amd/csrc/lio_gridconvert.h) run on the host: the text the kernels run, with the tile walk of
// k_gc_to_image and k_gc_from_image (tile, lane and wave loops, the runs of whole dwords and single bytes) replayed over heap
// arrays of exactly the layers' and images' sizes, so that AddressSanitizer sees any access outside them.  Stand-alone, needs
// no GPU:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined tools/grid_convert_host_check.cpp -o /tmp/grid_convert_host_check && /tmp/grid_convert_host_check
//
// Without arguments it runs its own cases (every grid shape of tests/test_gpu_grid_convert.py times the nine channel / depth
// pairs out and the accepted ones in) and checks what can be said without a second implementation: the tiled walk against the
// plain per-pixel loop byte for byte, every byte and word written exactly once, the counters against each other and the sizes,
// a round trip through an 8UC4 image.  It prints "inconsistencies: 0" at the end; the exit status is their number (capped).
//   grid_convert_host_check to_image   ROWS COLS CHANNELS DEPTH LOWER UPPER LAYER OUT     (OUT: the image, float lower, upper,
//                                                                                          int64 pixels, low, high, non-finite)
//   grid_convert_host_check from_image ROWS COLS CHANNELS DEPTH COLOR LOWER UPPER ALPHA IMAGE OUT   (OUT: the words, int64 transparent)
//   grid_convert_host_check occupancy  N DATA OUT
//   grid_convert_host_check cloud      ROWS COLS RES PX PY N_LAYERS POINT IDS BASIC_MASK LAYERS OUT  (IDS: a,b,c; OUT: int64 n, records)
//   grid_convert_host_check cells      ROWS COLS RES PX PY LOWER UPPER LAYER OUT                     (OUT: int64 n, pairs of doubles)
//   grid_convert_host_check sdf        ROWS COLS LAYERS OX OY OZ RES DECIMATION LOWER UPPER NODES OUT (OUT: int64 n, float4 records)
// Layers are column-major.  tests/test_grid_convert_cpu.py compares each with the restatement word for word.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../lio-slam_amd/csrc/lio_gridconvert.h"
#include "../lio-slam_amd/csrc/lio_wg.h"

typedef std::vector<unsigned char> Bytes;
static long long g_bad = 0;

static void bad(const char* what, long long a = 0, long long b = 0)
{
    if (g_bad++ < 20) printf("INCONSISTENT: %s (%lld, %lld)\n", what, a, b);
}

struct TileLine {
    const unsigned* p;
    unsigned at(int pixel) const { return p[pixel]; }
};

struct ImageCounts { long long low = 0, high = 0, nonfinite = 0; };

// k_gc_to_image, one workgroup after the other; `written` counts the stores per byte
static void tiled_to_image(const std::vector<float>& layer, int rows, int cols, float lo, float hi, int channels, int depth, Bytes& image,
                           std::vector<unsigned char>& written, ImageCounts& n)
{
    const int tiles_r = (rows + LIO_GC_TILE - 1) / LIO_GC_TILE, tiles_c = (cols + LIO_GC_TILE - 1) / LIO_GC_TILE;
    const int px = channels * lio_gc_elem_bytes(depth);
    for (int block = 0; block < tiles_r * tiles_c; ++block) {
        std::vector<unsigned> tile((size_t)LIO_GC_TILE * LIO_GC_PITCH, 0xdeadbeefu);
        const int r0 = (block % tiles_r) * LIO_GC_TILE, c0 = (block / tiles_r) * LIO_GC_TILE;
        const int nr = rows - r0 < LIO_GC_TILE ? rows - r0 : LIO_GC_TILE, nc = cols - c0 < LIO_GC_TILE ? cols - c0 : LIO_GC_TILE;
        for (int wave = 0; wave < 4; ++wave)
            for (int c = wave; c < LIO_GC_TILE; c += 4)
                for (int lane = 0; lane < 64; ++lane) {
                    int cls = LIO_GC_IN_RANGE;
                    if (lane < nr && c < nc)
                        tile.at((size_t)lane * LIO_GC_PITCH + c) = lio_gc_pixel(layer.at((size_t)(c0 + c) * rows + (r0 + lane)), lo, hi, depth, &cls);
                    n.low += cls == LIO_GC_CLAMPED_LOW; n.high += cls == LIO_GC_CLAMPED_HIGH; n.nonfinite += cls == LIO_GC_NONFINITE;
                }
        for (int wave = 0; wave < 4; ++wave)
            for (int r = wave; r < nr; r += 4) {
                const TileLine line = { tile.data() + (size_t)r * LIO_GC_PITCH };
                const size_t at = ((size_t)(r0 + r) * cols + c0) * px;
                const LioGcRun R = lio_gc_run(at, (size_t)nc * px);
                if (!(at <= R.head_end && R.head_end <= R.tail_begin && R.tail_begin <= R.end && R.d0 <= R.d1 &&
                      (R.d0 == R.d1 || (4 * R.d0 == R.head_end && 4 * R.d1 == R.tail_begin)) && R.head_end - at < 4 && R.end - R.tail_begin < 4))
                    bad("run", (long long)at, (long long)R.end);
                for (int lane = 0; lane < 64; ++lane) {
                    for (size_t b = at + lane; b < R.head_end; b += 64) { image.at(b) = (unsigned char)lio_gc_run_byte(line, b - at, px, channels, depth); ++written.at(b); }
                    for (size_t d = R.d0 + lane; d < R.d1; d += 64) {
                        const unsigned w = lio_gc_run_dword(line, d, at, px, channels, depth);
                        for (int k = 0; k < 4; ++k) { image.at(4 * d + k) = (unsigned char)(w >> (8 * k)); ++written.at(4 * d + k); }
                    }
                    for (size_t b = R.tail_begin + lane; b < R.end; b += 64) { image.at(b) = (unsigned char)lio_gc_run_byte(line, b - at, px, channels, depth); ++written.at(b); }
                }
            }
    }
}

// k_gc_to_image_direct
static void direct_to_image(const std::vector<float>& layer, int rows, int cols, float lo, float hi, int channels, int depth, Bytes& image, ImageCounts& n)
{
    const int px = channels * lio_gc_elem_bytes(depth);
    for (long long q = 0; q < (long long)rows * cols; ++q) {
        int cls;
        const unsigned w = lio_gc_pixel(layer.at((size_t)(q % cols) * rows + (size_t)(q / cols)), lo, hi, depth, &cls);
        for (int b = 0; b < px; ++b) image.at((size_t)q * px + b) = (unsigned char)lio_gc_pixel_byte(w, b, channels, depth);
        n.low += cls == LIO_GC_CLAMPED_LOW; n.high += cls == LIO_GC_CLAMPED_HIGH; n.nonfinite += cls == LIO_GC_NONFINITE;
    }
}

// k_gc_from_image
static long long tiled_from_image(const LioGcIngest& I, const Bytes& image, std::vector<unsigned>& layer, std::vector<unsigned char>& written)
{
    const int tiles_r = (I.rows + LIO_GC_TILE - 1) / LIO_GC_TILE, tiles_c = (I.cols + LIO_GC_TILE - 1) / LIO_GC_TILE;
    const int px = I.channels * lio_gc_elem_bytes(I.depth);
    long long n_transparent = 0;
    // (the element reads of a pixel must stay inside the image: a copy of exactly the pixel's bytes is what they see)
    for (int block = 0; block < tiles_r * tiles_c; ++block) {
        std::vector<unsigned> tile((size_t)LIO_GC_TILE * LIO_GC_PITCH, 0xdeadbeefu);
        const int r0 = (block % tiles_r) * LIO_GC_TILE, c0 = (block / tiles_r) * LIO_GC_TILE;
        const int nr = I.rows - r0 < LIO_GC_TILE ? I.rows - r0 : LIO_GC_TILE, nc = I.cols - c0 < LIO_GC_TILE ? I.cols - c0 : LIO_GC_TILE;
        for (int wave = 0; wave < 4; ++wave)
            for (int r = wave; r < LIO_GC_TILE; r += 4)
                for (int lane = 0; lane < 64; ++lane) {
                    bool transparent = false;
                    if (r < nr && lane < nc) {
                        const size_t at = ((size_t)(r0 + r) * I.cols + (c0 + lane)) * px;
                        const Bytes pixel(image.begin() + at, image.begin() + at + px);
                        tile.at((size_t)lane * LIO_GC_PITCH + r) = lio_gc_word_from_pixel(I, pixel.data(), &transparent);
                    }
                    n_transparent += transparent;
                }
        for (int wave = 0; wave < 4; ++wave)
            for (int c = wave; c < nc; c += 4)
                for (int lane = 0; lane < 64; ++lane)
                    if (lane < nr) {
                        const size_t at = (size_t)(c0 + c) * I.rows + (r0 + lane);
                        layer.at(at) = tile.at((size_t)c * LIO_GC_PITCH + lane);
                        ++written.at(at);
                    }
    }
    return n_transparent;
}

static long long direct_from_image(const LioGcIngest& I, const Bytes& image, std::vector<unsigned>& layer)
{
    const int px = I.channels * lio_gc_elem_bytes(I.depth);
    long long n_transparent = 0;
    for (long long i = 0; i < (long long)I.rows * I.cols; ++i) {
        bool transparent;
        const size_t at = ((size_t)(i % I.rows) * I.cols + (size_t)(i / I.rows)) * px;
        const Bytes pixel(image.begin() + at, image.begin() + at + px);
        layer.at(i) = lio_gc_word_from_pixel(I, pixel.data(), &transparent);
        n_transparent += transparent;
    }
    return n_transparent;
}

// minCoeffOfFinites / maxCoeffOfFinites as k_gc_extremes leaves them: ordered words; false without a finite cell
static bool extremes(const std::vector<float>& layer, float* lo, float* hi)
{
    unsigned mn = LIO_ORD_NO_MIN, mx = LIO_ORD_NO_MAX;
    for (float v : layer)
        if (lio_gm_finite(v)) { const unsigned o = lio_f2ord(v); mn = o < mn ? o : mn; mx = o > mx ? o : mx; }
    *lo = lio_ord2f(mn); *hi = lio_ord2f(mx);
    return !(mn == LIO_ORD_NO_MIN && mx == LIO_ORD_NO_MAX);
}

template <class T>
static std::vector<T> read_file(const char* path, size_t n)
{
    std::vector<T> v(n);
    FILE* f = fopen(path, "rb");
    if (!f || fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "cannot read %zu items of %s\n", n, path); exit(2); }
    fclose(f);
    return v;
}

struct Out {
    FILE* f;
    explicit Out(const char* path) : f(fopen(path, "wb")) { if (!f) { fprintf(stderr, "cannot write %s\n", path); exit(2); } }
    ~Out() { fclose(f); }
    void put(const void* p, size_t bytes) { if (bytes && fwrite(p, 1, bytes, f) != bytes) exit(2); }
};

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static std::vector<float> test_layer(int rows, int cols, uint32_t seed)
{
    std::vector<float> v((size_t)rows * cols);
    for (float& x : v) {
        const uint32_t k = lcg(seed) % 64;
        x = k == 0 ? NAN : k == 1 ? INFINITY : k == 2 ? -INFINITY : k == 3 ? -1.0f : k == 4 ? 1.0f : k == 5 ? 1.5f : k == 6 ? -1.5f
            : (float)(lcg(seed) % 20001) * 1e-4f - 1.0f;
    }
    return v;
}

static int self_check()
{
    const int shapes[][2] = { { 1, 1 }, { 1, 70 }, { 70, 1 }, { 33, 65 }, { 64, 64 }, { 67, 45 }, { 9, 7 }, { 5, 3 }, { 130, 3 } };
    const int chans[] = { 1, 3, 4 }, depths[] = { LIO_IMAGE_8U, LIO_IMAGE_16U, LIO_IMAGE_32F };
    for (const auto& sh : shapes) {
        const int rows = sh[0], cols = sh[1];
        const std::vector<float> layer = test_layer(rows, cols, 17u * rows + cols);
        for (int ch : chans)
            for (int depth : depths) {
                const size_t bytes = (size_t)rows * cols * ch * lio_gc_elem_bytes(depth);
                Bytes a(bytes, 0xa5), b(bytes, 0x5a);
                std::vector<unsigned char> written(bytes, 0);
                ImageCounts na, nb;
                tiled_to_image(layer, rows, cols, -1.0f, 1.0f, ch, depth, a, written, na);
                direct_to_image(layer, rows, cols, -1.0f, 1.0f, ch, depth, b, nb);
                if (a != b) bad("tiled image differs from the direct one", rows, cols);
                for (size_t k = 0; k < bytes; ++k)
                    if (written[k] != 1) { bad("a byte written other than once", (long long)k, written[k]); break; }
                if (na.low != nb.low || na.high != nb.high || na.nonfinite != nb.nonfinite) bad("image counts", rows, cols);
                if (depth == LIO_IMAGE_32F && ch != 1) continue;
                // the image back in: grey, and colour for 8U with 3 or 4 channels
                for (int color = 0; color < 2; ++color) {
                    if (color && (depth != LIO_IMAGE_8U || ch == 1)) continue;
                    LioGcIngest I;
                    memset(&I, 0, sizeof(I));
                    I.rows = rows; I.cols = cols; I.channels = ch; I.depth = depth; I.color = color;
                    I.lower = -1.0f; I.upper = 1.0f;
                    I.alpha_min = depth == LIO_IMAGE_32F ? 0u : lio_gc_alpha_min(0.5, depth);
                    std::vector<unsigned> la((size_t)rows * cols, 0x11111111u), lb((size_t)rows * cols, 0x22222222u);
                    std::vector<unsigned char> wl((size_t)rows * cols, 0);
                    const long long ta = tiled_from_image(I, a, la, wl), tb = direct_from_image(I, a, lb);
                    if (la != lb || ta != tb) bad("tiled ingest differs from the direct one", rows, cols);
                    for (size_t k = 0; k < wl.size(); ++k)
                        if (wl[k] != 1) { bad("a cell written other than once", (long long)k, wl[k]); break; }
                    if (!color && ch == 4 && depth == LIO_IMAGE_8U) {           // GridMapCvTest's round trip: NaN back as NaN, the rest within 2 / 255
                        if (ta != na.nonfinite) bad("transparent cells are not the non-finite ones", ta, na.nonfinite);
                        for (size_t k = 0; k < la.size(); ++k) {
                            const float x = layer[(size_t)k], y = __builtin_bit_cast(float, la[k]);
                            const float want = lio_gc_clamp(x, -1.0f, 1.0f);
                            if (lio_gm_finite(want) ? !(fabsf(y - want) <= 2.0f / 255.0f) : y == y) { bad("round trip", (long long)k); break; }
                        }
                    }
                }
            }
    }
    for (size_t at = 0; at < 9; ++at)                        // runs shorter than, equal to and longer than a dword at every phase
        for (size_t n = 1; n < 14; ++n) {
            const LioGcRun R = lio_gc_run(at, n);
            size_t covered = (R.head_end - at) + 4 * (R.d1 - R.d0) + (R.end - R.tail_begin);
            if (covered != n || R.end != at + n) bad("run cover", (long long)at, (long long)n);
        }
    printf("inconsistencies: %lld\n", g_bad);
    return g_bad > 100 ? 100 : (int)g_bad;
}

int main(int argc, char** argv)
{
    if (argc < 2) return self_check();
    const std::string mode = argv[1];
    if (mode == "to_image" && argc == 10) {
        const int rows = atoi(argv[2]), cols = atoi(argv[3]), ch = atoi(argv[4]), depth = atoi(argv[5]);
        float lo = strtof(argv[6], nullptr), hi = strtof(argv[7], nullptr);
        const std::vector<float> layer = read_file<float>(argv[8], (size_t)rows * cols);
        if (lo != lo && hi != hi && !extremes(layer, &lo, &hi)) return 3;
        if (!(hi > lo) || !lio_gm_finite(hi - lo)) return 3;
        const size_t bytes = (size_t)rows * cols * ch * lio_gc_elem_bytes(depth);
        Bytes img(bytes, 0xa5);
        std::vector<unsigned char> written(bytes, 0);
        ImageCounts n;
        tiled_to_image(layer, rows, cols, lo, hi, ch, depth, img, written, n);
        const int64_t counts[4] = { (int64_t)rows * cols - n.nonfinite, n.low, n.high, n.nonfinite };
        Out out(argv[9]);
        out.put(img.data(), bytes); out.put(&lo, 4); out.put(&hi, 4); out.put(counts, sizeof(counts));
        return 0;
    }
    if (mode == "from_image" && argc == 12) {
        LioGcIngest I;
        memset(&I, 0, sizeof(I));
        I.rows = atoi(argv[2]); I.cols = atoi(argv[3]); I.channels = atoi(argv[4]); I.depth = atoi(argv[5]); I.color = atoi(argv[6]);
        I.lower = strtof(argv[7], nullptr); I.upper = strtof(argv[8], nullptr);
        I.alpha_min = I.depth == LIO_IMAGE_32F ? 0u : lio_gc_alpha_min(strtod(argv[9], nullptr), I.depth);
        const size_t cells = (size_t)I.rows * I.cols;
        const Bytes img = read_file<unsigned char>(argv[10], cells * I.channels * lio_gc_elem_bytes(I.depth));
        std::vector<unsigned> layer(cells, 0x11111111u);
        std::vector<unsigned char> written(cells, 0);
        const int64_t t = tiled_from_image(I, img, layer, written);
        Out out(argv[11]);
        out.put(layer.data(), 4 * cells); out.put(&t, 8);
        return 0;
    }
    if (mode == "occupancy" && argc == 5) {
        const size_t n = strtoull(argv[2], nullptr, 10);
        const std::vector<int8_t> data = read_file<int8_t>(argv[3], n);
        std::vector<unsigned> layer(n);
        for (size_t i = 0; i < n; ++i) layer.at(i) = lio_gc_occupancy_word(data.at(n - 1 - i));
        Out out(argv[4]);
        out.put(layer.data(), 4 * n);
        return 0;
    }
    if ((mode == "cloud" && argc == 13) || (mode == "cells" && argc == 11)) {
        const int rows = atoi(argv[2]), cols = atoi(argv[3]);
        const LioGridGeom G = lio_gm_geom(rows, cols, strtod(argv[4], nullptr), strtod(argv[5], nullptr), strtod(argv[6], nullptr));
        const size_t cells = (size_t)rows * cols;
        if (mode == "cells") {
            const float lo = strtof(argv[7], nullptr), hi = strtof(argv[8], nullptr);
            const std::vector<float> layer = read_file<float>(argv[9], cells);
            std::vector<double> rec;
            for (size_t i = 0; i < cells; ++i)
                if (lio_gc_cell_kept(layer.at(i), lo, hi)) { rec.push_back(lio_gm_centre(G, 0, (int)(i % rows))); rec.push_back(lio_gm_centre(G, 1, (int)(i / rows))); }
            const int64_t n = (int64_t)rec.size() / 2;
            Out out(argv[10]);
            out.put(&n, 8); out.put(rec.data(), 8 * rec.size());
            return 0;
        }
        const int n_layers = atoi(argv[7]), point = atoi(argv[8]);
        const unsigned basic = (unsigned)strtoul(argv[10], nullptr, 0);
        const std::vector<unsigned> all = read_file<unsigned>(argv[11], cells * n_layers);
        LioGcCloud C;
        memset(&C, 0, sizeof(C));
        C.point = all.data() + cells * point;
        C.point_at = -1;
        for (char* tok = strtok(argv[9], ","); tok; tok = strtok(nullptr, ",")) {
            const int id = atoi(tok);
            C.layer[C.n_layers] = all.data() + cells * id;
            if (id == point) C.point_at = C.n_layers;
            C.n_fields += id == point ? 3 : 1;
            ++C.n_layers;
        }
        for (int k = 0; k < n_layers; ++k)
            if ((basic >> k) & 1u) C.basic[C.n_basic++] = all.data() + cells * k;
        std::vector<unsigned> rec;
        int64_t n = 0;
        for (size_t i = 0; i < cells; ++i)
            if (lio_gc_cloud_kept(C, (int)i)) {
                rec.resize(rec.size() + C.n_fields);
                lio_gc_cloud_record(C, G, (int)i, rec.data() + rec.size() - C.n_fields);
                ++n;
            }
        Out out(argv[12]);
        out.put(&n, 8); out.put(rec.data(), 4 * rec.size());
        return 0;
    }
    if (mode == "sdf" && argc == 14) {
        LioSdfLookup L;
        L.rows = atoi(argv[2]); L.cols = atoi(argv[3]); L.layers = atoi(argv[4]);
        for (int a = 0; a < 3; ++a) L.origin[a] = strtod(argv[5 + a], nullptr);
        L.res = strtod(argv[8], nullptr);
        const int decimation = atoi(argv[9]);
        const float lo = strtof(argv[10], nullptr), hi = strtof(argv[11], nullptr);
        const std::vector<float> nodes = read_file<float>(argv[12], 4 * (size_t)L.rows * L.cols * L.layers);
        const LioGcSdfVisit V = lio_gc_sdf_visit(L, decimation);
        std::vector<float> rec;
        for (int i = 0; i < V.nx * V.ny * V.nz; ++i) {
            int idx[3];
            lio_gc_sdf_node(V, i, idx);
            const float d = nodes.at(4 * lio_sdf_linear_index(L, idx));
            if (!lio_gc_sdf_kept(d, lo, hi)) continue;
            const float4 q = lio_gc_sdf_point(L, idx, d);
            rec.insert(rec.end(), { q.x, q.y, q.z, q.w });
        }
        const int64_t n = (int64_t)rec.size() / 4;
        Out out(argv[13]);
        out.put(&n, 8); out.put(rec.data(), 4 * rec.size());
        return 0;
    }
    fprintf(stderr, "usage: see the head of tools/grid_convert_host_check.cpp\n");
    return 2;
}
