// grid_filter_host_check.cpp -- the arithmetic of lio_grid_filter_radius, lio_grid_filter_window, lio_grid_filter_curvature and
// lio_grid_filter_threshold (lio-slam_amd/csrc/lio_gridfilter.h) run on the host: the text the kernels run, one cell after the
// other, through an accessor that counts every read outside the grid or further from the cell than the halo the kernel
// stages around its tile (floor(radius / resolution + 0.5) + 1 cells, the half-window, 1 cell).  Stand-alone, needs no GPU:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined tools/grid_filter_host_check.cpp -o /tmp/grid_filter_host_check && /tmp/grid_filter_host_check
//
// Without arguments it runs its own cases -- radii of 0, 0.5, 1, 2, 3, 3.3, 7.5, 16 and 32 cells, windows of 1, 3, 5, 9, 33 and
// 65 and the derived sizes, every op and edge mode, at positions (0, 0) and (1e4, -3e4), on grids from 1 x 1 to 69 x 19 with
// holes and infinities -- and checks what can be said without a second implementation: no read outside the grid or the halo,
// the counts against each other and against the sizes, a radius of 0 and a window of 1 against the layer itself, the number
// of finites against a plain count.  It prints a checksum per case (FNV-1a over the layer's words) and "inconsistencies: 0"
// at the end; the exit status is their number (capped).  Before that line it runs the terrain layers' cell (lio_terrain.h, both
// normal methods) on a 33 x 9 grid with holes, the smooth radius below the normal radius, and prints how many cells it compared
// and in how many `smooth` is not the MEAN filter's word or `edges` not STDDEV / CROP's on the same slope layer: 0.
//   grid_filter_host_check filter KIND ROWS COLS RES PX PY OP EDGE SIZE P1 P2 IN OUT
//       KIND 0 radius (P1 the radius), 1 window (P1 the length), 2 curvature, 3 threshold (OP = upper, P1 the threshold, P2
//       set_to).  IN: the layer, column-major floats; for the threshold the layer to set follows; for LIO_GW_WEIGHTED_SUM the
//       weights follow.  OUT receives int32 refused, window size; int64 visited, written, changed, bad reads; then the layer.
//   grid_filter_host_check batch LIST
//       LIST holds one such argument list a line (without the word `filter`): the same runs in one process.
//       tests/test_grid_filter_cpu.py compares them with the restatement word for word.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../lio-slam_amd/csrc/lio_gridfilter.h"
#include "../lio-slam_amd/csrc/lio_terrain.h"

static long long g_bad = 0, g_outside = 0;

struct Checked {                   // the layer, with the cell that reads and the halo it may read within
    const float* p;
    int rows, cols, r, c, halo;
    float at(int i, int j) const
    {
        const int di = i > r ? i - r : r - i, dj = j > c ? j - c : c - j;
        if (i < 0 || i >= rows || j < 0 || j >= cols || di > halo || dj > halo) { ++g_outside; return 0.0f; }
        return p[(size_t)i + (size_t)j * (size_t)rows];
    }
};

struct Result {
    int refused = 0, size = 0;
    long long visited = 0, written = 0, changed = 0;
    std::vector<float> out;
};

static void store(Result& R, const LioGfCell& o, size_t at)
{
    R.out[at] = o.written ? o.value : LIO_QNAN;
    R.visited += o.visited; R.written += o.written;
}

static void run_radius(const std::vector<float>& z, int rows, int cols, double res, double px, double py, int op, double radius, Result& R)
{
    LioGfRadius P;
    R.out.assign(z.size(), 0.0f);
    if (lio_gf_radius_plan(lio_gm_geom(rows, cols, res, px, py), radius, &P)) { R.refused = 1; return; }
    for (int c = 0; c < cols; ++c)
        for (int r = 0; r < rows; ++r) {
            const Checked in = { z.data(), rows, cols, r, c, P.halo };
            store(R, op == LIO_GF_MIN ? lio_gf_radius_cell<LIO_GF_MIN>(P, in, r, c) : lio_gf_radius_cell<LIO_GF_MEAN>(P, in, r, c), (size_t)r + (size_t)c * rows);
        }
}

template <int OP, int EDGE>
static void window_cells(const LioGfWindow& P, const std::vector<float>& z, const float* K, Result& R)
{
    for (int c = 0; c < P.cols; ++c)
        for (int r = 0; r < P.rows; ++r) {
            const Checked in = { z.data(), P.rows, P.cols, r, c, P.margin };
            store(R, lio_gf_window_cell<OP, EDGE>(P, in, K, r, c), (size_t)r + (size_t)c * P.rows);
        }
}

template <int OP>
static void window_edges(int edge, const LioGfWindow& P, const std::vector<float>& z, const float* K, Result& R)
{
    if (edge == LIO_GW_INSIDE) window_cells<OP, LIO_GW_INSIDE>(P, z, K, R);
    else if (edge == LIO_GW_CROP) window_cells<OP, LIO_GW_CROP>(P, z, K, R);
    else if (edge == LIO_GW_EMPTY) window_cells<OP, LIO_GW_EMPTY>(P, z, K, R);
    else window_cells<OP, LIO_GW_EDGE_MEAN>(P, z, K, R);
}

static void run_window(const std::vector<float>& z, int rows, int cols, double res, int op, int edge, int size, double length, const float* K, Result& R)
{
    LioGfWindow P;
    R.out.assign(z.size(), 0.0f);
    if ((size != 0 && size % 2 == 0) || size < 0 || lio_gf_window_plan(rows, cols, res, edge, size, length, &P)) { R.refused = 1; return; }
    if (op == LIO_GW_WEIGHTED_SUM && edge == LIO_GW_CROP && P.size > 1) { R.refused = 1; return; }
    R.size = P.size;
    switch (op) {
    case LIO_GW_SUM: window_edges<LIO_GW_SUM>(edge, P, z, K, R); break;
    case LIO_GW_MEAN_OF_FINITES: window_edges<LIO_GW_MEAN_OF_FINITES>(edge, P, z, K, R); break;
    case LIO_GW_MIN_OF_FINITES: window_edges<LIO_GW_MIN_OF_FINITES>(edge, P, z, K, R); break;
    case LIO_GW_MAX_OF_FINITES: window_edges<LIO_GW_MAX_OF_FINITES>(edge, P, z, K, R); break;
    case LIO_GW_NUMBER_OF_FINITES: window_edges<LIO_GW_NUMBER_OF_FINITES>(edge, P, z, K, R); break;
    case LIO_GW_STDDEV: window_edges<LIO_GW_STDDEV>(edge, P, z, K, R); break;
    default: window_edges<LIO_GW_WEIGHTED_SUM>(edge, P, z, K, R); break;
    }
}

static void run_curvature(const std::vector<float>& z, int rows, int cols, double res, Result& R)
{
    R.out.assign(z.size(), 0.0f);
    const float L2 = (float)(res * res);
    for (int c = 0; c < cols; ++c)
        for (int r = 0; r < rows; ++r) {
            const Checked in = { z.data(), rows, cols, r, c, 1 };
            store(R, lio_gf_curvature_cell(rows, cols, L2, in, r, c), (size_t)r + (size_t)c * rows);
        }
}

static void run_threshold(const std::vector<float>& cond, const std::vector<float>& data, int upper, double threshold, double set_to, Result& R)
{
    R.out = data;
    const float v = (float)set_to;
    for (size_t k = 0; k < cond.size(); ++k) {
        ++R.visited;
        if (lio_gf_threshold_sets(cond[k], upper, threshold)) { memcpy(&R.out[k], &v, 4); ++R.changed; ++R.written; }
    }
}

// ---- the self-run
static uint32_t word(float v) { uint32_t w; memcpy(&w, &v, 4); return w; }

static uint32_t checksum(const std::vector<float>& a)
{
    uint32_t h = 2166136261u;
    for (float v : a) {
        uint32_t w = word(v);
        if (v != v) w = LIO_QNAN_BITS;                       // one word for every NaN
        for (int b = 0; b < 4; ++b) { h ^= (w >> (8 * b)) & 0xffu; h *= 16777619u; }
    }
    return h;
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static double uniform() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (double)(g_rng >> 11) / 9007199254740992.0; }

static std::vector<float> scene(int rows, int cols)
{
    std::vector<float> z((size_t)rows * cols);
    for (int c = 0; c < cols; ++c)
        for (int r = 0; r < rows; ++r) {
            const double u = uniform();
            float v = (float)(0.08 * r - 0.05 * c + 0.02 * (uniform() - 0.5));
            if (u < 0.08) v = LIO_QNAN;
            else if (u < 0.10) v = INFINITY;
            else if (u < 0.12) v = -INFINITY;
            z[(size_t)r + (size_t)c * rows] = v;
        }
    return z;
}

static void expect(bool ok, const char* what, const char* tag)
{
    if (!ok) { ++g_bad; printf("INCONSISTENT %s: %s\n", tag, what); }
}

static bool finite(float v) { return v - v == 0.0f; }

// lio_terr_cell under the tile's halo against the filter under its own; the edge cell over the terrain plan's window against
// the filter's plan.  Every read goes through the checked accessor.
static void terrain_identity()
{
    const int rows = 33, cols = 9;
    const double res = 0.25;
    const std::vector<float> z = scene(rows, cols);
    for (int method = 0; method < 2; ++method) {
        LioTerrParams P;
        memset(&P, 0, sizeof(P));
        P.G = lio_gm_geom(rows, cols, res, 1e4, -3e4);
        P.r_smooth = 1.5 * res; P.r_normal = 3.0 * res;
        P.method = method; P.axis = 2;
        P.halo = lio_gf_halo(method == 0 ? 3.0 : 1.5);
        P.margin = 2;
        P.s_crit = 0.6f; P.r_crit = 0.1f; P.w_s = 0.5f; P.w_r = 0.5f;
        LioGfRadius S;
        LioGfWindow W;
        if (lio_gf_radius_plan(P.G, P.r_smooth, &S) || lio_gf_window_plan(rows, cols, res, LIO_GW_CROP, 2 * P.margin + 1, 0.0, &W)) { expect(false, "plans", "terrain"); return; }
        std::vector<float> smooth(z.size()), slope(z.size());
        long long compared = 0, differ = 0;
        for (int c = 0; c < cols; ++c)
            for (int r = 0; r < rows; ++r) {
                const size_t at = (size_t)r + (size_t)c * rows;
                const Checked tile = { z.data(), rows, cols, r, c, P.halo }, own = { z.data(), rows, cols, r, c, S.halo };
                LioTerrCell o;
                lio_terr_cell(P, tile, r, c, &o);
                smooth[at] = o.smooth; slope[at] = o.slope;
                const LioGfCell m = lio_gf_radius_cell<LIO_GF_MEAN>(S, own, r, c);
                differ += word(o.smooth) != word(m.written ? m.value : LIO_QNAN);
            }
        for (int c = 0; c < cols; ++c)
            for (int r = 0; r < rows; ++r) {
                const Checked in = { slope.data(), rows, cols, r, c, P.margin };
                const LioGfCell e = lio_gf_window_cell<LIO_GW_STDDEV, LIO_GW_CROP>(lio_terr_edge_window(P), in, nullptr, r, c);
                const LioGfCell f = lio_gf_window_cell<LIO_GW_STDDEV, LIO_GW_CROP>(W, in, nullptr, r, c);
                differ += word(e.value) != word(f.written ? f.value : LIO_QNAN);
                ++compared;
            }
        expect(compared == (long long)rows * cols && differ == 0, "smooth is MEAN in the radius, edges is STDDEV over CROP", "terrain");
        printf("terrain %dx%d method %d: smooth %08x slope %08x; cells compared %lld, words that differ %lld\n", rows, cols, method, checksum(smooth),
               checksum(slope), compared, differ);
    }
}

static int self_run()
{
    const int shapes[][2] = { { 1, 1 }, { 1, 300 }, { 2, 2 }, { 8, 5 }, { 33, 9 }, { 69, 19 }, { 40, 9 } };
    const double positions[][2] = { { 0.0, 0.0 }, { 1e4, -3e4 } };
    const double radii[] = { 0.0, 0.5, 1.0, 2.0, 3.0, 3.3, 7.5, 16.0, 32.0 };
    const int sizes[] = { 1, 3, 5, 9, 33, 65 };
    const double lengths[] = { 0.0, 0.1, 0.2, 0.25, 0.7 };
    char tag[160];
    for (const auto& sh : shapes) {
        const int rows = sh[0], cols = sh[1];
        const size_t cells = (size_t)rows * cols;
        const std::vector<float> z = scene(rows, cols);
        long long n_finite = 0;
        for (float v : z) n_finite += finite(v);
        for (const auto& pos : positions) {
            for (const double res : { 0.1, 0.25 }) {
                for (double cells_r : radii) {
                    if (cells_r > 8.0 && cells > 400) continue;          // (the long circles on the small grids only)
                    for (int op = 0; op < LIO_GF_N_RADIUS_OPS; ++op) {
                        Result R;
                        const double radius = cells_r * res;
                        run_radius(z, rows, cols, res, pos[0], pos[1], op, radius, R);
                        snprintf(tag, sizeof(tag), "radius %dx%d pos %g res %g r %g cells op %d", rows, cols, pos[0], res, cells_r, op);
                        if (R.refused) { expect(radius / res > 32.0, "refused within 32 cells", tag); continue; }
                        expect(R.visited == (op == LIO_GF_MIN ? n_finite : (long long)cells), "visited", tag);
                        expect(op == LIO_GF_MIN ? R.written == R.visited : R.written >= n_finite, "written", tag);
                        if (cells_r == 0.0)
                            for (size_t k = 0; k < cells; ++k)
                                if (finite(z[k]) ? word(R.out[k]) != word(z[k]) : word(R.out[k]) != LIO_QNAN_BITS) { expect(false, "radius 0 is the cell alone", tag); break; }
                        printf("%s: %08x visited %lld written %lld\n", tag, checksum(R.out), R.visited, R.written);
                    }
                }
                Result C;
                run_curvature(z, rows, cols, res, C);
                snprintf(tag, sizeof(tag), "curvature %dx%d res %g", rows, cols, res);
                expect(C.visited == (long long)cells && C.written == n_finite, "counts", tag);
                if (pos[0] == 0.0) printf("%s: %08x\n", tag, checksum(C.out));
            }
        }
        std::vector<float> K((size_t)65 * 65);
        for (float& k : K) k = (float)(4.0 * uniform() - 2.0);
        K[0] = INFINITY; K[1] = LIO_QNAN; K[2] = -0.0f;
        for (int edge = 0; edge < LIO_GW_N_EDGES; ++edge)
            for (int op = 0; op < LIO_GW_N_OPS; ++op) {
                for (int derived = 0; derived < 2; ++derived)
                    for (int k = 0; k < (derived ? 5 : 6); ++k) {
                        const int size = derived ? 0 : sizes[k];
                        if (size > 9 && cells > 400 && !(op == LIO_GW_STDDEV || op == LIO_GW_SUM)) continue;
                        Result R;
                        run_window(z, rows, cols, 0.1, op, edge, size, derived ? lengths[k] : 0.0, op == LIO_GW_WEIGHTED_SUM ? K.data() : nullptr, R);
                        snprintf(tag, sizeof(tag), "window %dx%d op %d edge %d size %d length %g", rows, cols, op, edge, size, derived ? lengths[k] : 0.0);
                        if (R.refused) { expect(op == LIO_GW_WEIGHTED_SUM && edge == LIO_GW_CROP, "refused", tag); continue; }
                        const int m = (R.size - 1) / 2;
                        long long fits = (rows > 2 * m && cols > 2 * m) ? (long long)(rows - 2 * m) * (cols - 2 * m) : 0;
                        if (derived && edge == LIO_GW_INSIDE && R.size == 1) fits = (rows >= 3 && cols >= 3) ? (long long)cells - rows - 1 : 0;
                        expect(R.visited == (edge == LIO_GW_INSIDE ? fits : (long long)cells) && R.written == R.visited, "visited", tag);
                        if (R.size == 1 && op == LIO_GW_SUM && edge != LIO_GW_INSIDE)
                            for (size_t q = 0; q < cells; ++q)
                                if (z[q] == z[q] && word(R.out[q]) != word(z[q])) { expect(false, "a window of 1 is the cell", tag); break; }
                        if (op == LIO_GW_NUMBER_OF_FINITES && edge == LIO_GW_CROP && R.size == 65 && rows <= 33 && cols <= 33) {
                            long long n = 0;
                            for (float v : z) n += v == v;
                            expect(R.out[0] == (float)n, "the window that covers the map counts its x == x", tag);
                        }
                        printf("%s: %08x visited %lld\n", tag, checksum(R.out), R.visited);
                    }
            }
    }
    terrain_identity();
    expect(g_outside == 0, "reads outside the grid or the halo", "all");
    printf("reads outside the grid or the halo: %lld\ninconsistencies: %lld\n", g_outside, g_bad);
    return (int)(g_bad > 100 ? 100 : g_bad);
}

static bool read_floats(FILE* f, std::vector<float>& v, size_t n)
{
    v.resize(n);
    return fread(v.data(), sizeof(float), n, f) == n;
}

// one `filter` run: a[0 .. 12] = KIND ROWS COLS RES PX PY OP EDGE SIZE P1 P2 IN OUT
static int filter(char** a)
{
    const int kind = atoi(a[0]), rows = atoi(a[1]), cols = atoi(a[2]);
    const double res = atof(a[3]), px = atof(a[4]), py = atof(a[5]);
    const int op = atoi(a[6]), edge = atoi(a[7]), size = atoi(a[8]);
    const double p1 = strtod(a[9], nullptr), p2 = strtod(a[10], nullptr);
    if (rows < 1 || cols < 1 || !(res > 0.0) || kind < 0 || kind > 3) { fprintf(stderr, "bad arguments\n"); return 2; }
    const size_t cells = (size_t)rows * cols;
    FILE* f = fopen(a[11], "rb");
    std::vector<float> z, data, K;
    if (!f || !read_floats(f, z, cells)) { fprintf(stderr, "cannot read the layer\n"); return 2; }
    if (kind == 3 && !read_floats(f, data, cells)) { fprintf(stderr, "cannot read the layer to set\n"); return 2; }
    const long long outside_before = g_outside;
    Result R;
    if (kind == 0) {
        if (op < 0 || op >= LIO_GF_N_RADIUS_OPS) return 2;
        run_radius(z, rows, cols, res, px, py, op, p1, R);
    } else if (kind == 1) {
        if (op < 0 || op >= LIO_GW_N_OPS || edge < 0 || edge >= LIO_GW_N_EDGES) return 2;
        if (op == LIO_GW_WEIGHTED_SUM) {
            LioGfWindow P;
            if (size < 0 || (size != 0 && size % 2 == 0) || lio_gf_window_plan(rows, cols, res, edge, size, p1, &P)) R.refused = 1;
            else if (!read_floats(f, K, (size_t)P.size * P.size)) { fprintf(stderr, "cannot read the weights\n"); return 2; }
        }
        if (!R.refused) run_window(z, rows, cols, res, op, edge, size, p1, K.empty() ? nullptr : K.data(), R);
        else R.out.assign(cells, 0.0f);
    } else if (kind == 2) {
        run_curvature(z, rows, cols, res, R);
    } else {
        run_threshold(z, data, op, p1, p2, R);
    }
    fclose(f);
    FILE* o = fopen(a[12], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", a[12]); return 2; }
    const int32_t head[2] = { R.refused, R.size };
    const int64_t cnt[4] = { R.visited, R.written, R.changed, g_outside - outside_before };
    fwrite(head, sizeof(head), 1, o);
    fwrite(cnt, sizeof(cnt), 1, o);
    fwrite(R.out.data(), sizeof(float), R.out.size(), o);
    fclose(o);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 1) return self_run();
    if (argc == 15 && strcmp(argv[1], "filter") == 0) return filter(argv + 2);
    if (argc == 3 && strcmp(argv[1], "batch") == 0) {        // LIST: one `filter` argument list a line
        FILE* l = fopen(argv[2], "r");
        if (!l) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
        char line[4096];
        while (fgets(line, sizeof(line), l)) {
            char* a[13];
            int n = 0;
            for (char* t = strtok(line, " \n"); t && n < 13; t = strtok(nullptr, " \n")) a[n++] = t;
            if (n == 0) continue;
            if (n != 13) { fprintf(stderr, "a line of %d fields\n", n); return 2; }
            const int rc = filter(a);
            if (rc != 0) return rc;
        }
        fclose(l);
        return 0;
    }
    fprintf(stderr, "usage: see the head of tools/grid_filter_host_check.cpp\n");
    return 2;
}
