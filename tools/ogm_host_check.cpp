// ogm_host_check.cpp -- the index arithmetic of the occupancy grid (lio-slam_amd/csrc/lio_ogm.h) run on the host: the text
// the kernels run, over accessors that count every read outside cell_start / the sorted cloud and every grid index outside
// width x height, against a brute-force count and the draft's literal raster.  Stand-alone, needs no GPU:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined tools/ogm_host_check.cpp -o /tmp/ogm_host_check && /tmp/ogm_host_check
//
// Prints one line per case and "out-of-range reads: 0, mismatches: 0" at the end; the exit status is their sum (capped).
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>

#include "../lio-slam_amd/csrc/lio_ogm.h"

static long long g_oob = 0, g_bad = 0;

struct CheckedInts {
    const std::vector<int>* v;
    int at(int i) const
    {
        if (i < 0 || i >= (int)v->size()) { ++g_oob; return 0; }
        return (*v)[(size_t)i];
    }
};
struct CheckedPts {
    const std::vector<float4>* v;
    int n_valid;                   // cell_start[n_cells]: entries beyond it were never written
    float4 at(int i) const
    {
        if (i < 0 || i >= n_valid) { ++g_oob; return make_float4(0, 0, 0, 0); }
        return (*v)[(size_t)i];
    }
};

struct Rng {
    uint64_t s;
    double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
    float range(double lo, double hi) { return (float)(lo + (hi - lo) * uni()); }
};

typedef std::vector<float4> Cloud;

// the cell of a point as lio_map_cell bins it (-1: takes no part)
static int bin_of(const LioGrid& g, const float4& p)
{
    if (!lio_ogm_takes_part(p.x, p.y, p.z)) return -1;
    const int cx = lio_ogm_cell_coord(p.x, g.ox, g.inv_cell, g.nx), cy = lio_ogm_cell_coord(p.y, g.oy, g.inv_cell, g.ny),
              cz = lio_ogm_cell_coord(p.z, g.oz, g.inv_cell, g.nz);
    if (cx < 0 || cx >= g.nx || cy < 0 || cy >= g.ny || cz < 0 || cz >= g.nz) return -1;
    return (cz * g.ny + cy) * g.nx + cx;
}

static void check_filter(const char* name, const Cloud& pts, float radius, int min_nb)
{
    const int n = (int)pts.size();
    // box of the coordinates within the bound, per axis, as k_map_bbox takes it
    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (const float4& p : pts) {
        const float v[3] = { p.x, p.y, p.z };
        for (int a = 0; a < 3; ++a)
            if (fabsf(v[a]) <= LIO_OGM_MAX_COORD) { mn[a] = fminf(mn[a], v[a]); mx[a] = fmaxf(mx[a], v[a]); }
    }
    if (!(mn[0] <= mx[0] && mn[1] <= mx[1] && mn[2] <= mx[2])) { for (int a = 0; a < 3; ++a) mn[a] = mx[a] = 0.0f; }
    LioGrid g;
    const float edge = lio_ogm_choose_grid(mn, mx, radius, &g);
    // counting sort by cell
    std::vector<int> cell_of((size_t)n), start((size_t)g.n_cells + 1, 0), fill((size_t)g.n_cells, 0);
    int n_part = 0, n_unbinned = 0;
    for (int i = 0; i < n; ++i) {
        cell_of[(size_t)i] = bin_of(g, pts[(size_t)i]);
        if (cell_of[(size_t)i] >= 0) { ++start[(size_t)cell_of[(size_t)i] + 1]; ++n_part; }
        else if (lio_ogm_takes_part(pts[(size_t)i].x, pts[(size_t)i].y, pts[(size_t)i].z)) ++n_unbinned;
    }
    for (int c = 0; c < g.n_cells; ++c) start[(size_t)c + 1] += start[(size_t)c];
    Cloud sorted((size_t)(n > 0 ? n : 1));
    for (int i = 0; i < n; ++i) {
        const int c = cell_of[(size_t)i];
        if (c < 0) continue;
        float4 p = pts[(size_t)i];
        p.w = __builtin_bit_cast(float, i);
        sorted[(size_t)(start[(size_t)c] + fill[(size_t)c]++)] = p;
    }
    const CheckedInts cs = { &start };
    const CheckedPts sp = { &sorted, n_part };
    const float r2 = (float)((double)radius * (double)radius);
    std::vector<int> exact((size_t)n, -1), early((size_t)n, -1);
    for (int s = 0; s < n_part; ++s) {
        const float4 q = sp.at(s);
        const int i = __builtin_bit_cast(int, q.w);
        exact[(size_t)i] = lio_ogm_count(g, cs, sp, q.x, q.y, q.z, r2, INT_MAX);
        early[(size_t)i] = lio_ogm_count(g, cs, sp, q.x, q.y, q.z, r2, min_nb);
    }
    // brute force over the points that take part
    long long bad = n_unbinned;                         // a point that takes part must be binned
    int kept = 0;
    for (int i = 0; i < n; ++i) {
        const float4& q = pts[(size_t)i];
        int k = -1;
        if (lio_ogm_takes_part(q.x, q.y, q.z)) {
            k = 0;
            for (int j = 0; j < n; ++j) {
                const float4& m = pts[(size_t)j];
                if (!lio_ogm_takes_part(m.x, m.y, m.z)) continue;
                const float dx = q.x - m.x, dy = q.y - m.y, dz = q.z - m.z;
                const float d2 = ((dx * dx) + dy * dy) + dz * dz;
                k += d2 < r2 ? 1 : 0;
            }
        }
        if (k != exact[(size_t)i]) ++bad;
        if ((k > min_nb) != (early[(size_t)i] > min_nb)) ++bad;
        kept += k > min_nb ? 1 : 0;
    }
    g_bad += bad;
    printf("filter %-22s n %5d r %.3g min %2d: grid %d x %d x %d edge %.6g, part %d, kept %d, mismatches %lld\n", name, n, radius, min_nb,
           g.nx, g.ny, g.nz, edge, n_part, kept, bad);
}

static void check_raster(const char* name, const Cloud& pts, double res, int whole_box)
{
    const int n = (int)pts.size();
    if (n == 0) return;
    const int m = (whole_box || n == 1) ? n : n - 1;
    double x_min = pts[0].x, x_max = pts[0].x, y_min = pts[0].y, y_max = pts[0].y;
    for (int i = 0; i < m; ++i) {
        const double x = pts[(size_t)i].x, y = pts[(size_t)i].y;
        if (x < x_min) x_min = x;
        if (x > x_max) x_max = x;
        if (y < y_min) y_min = y;
        if (y > y_max) y_max = y;
    }
    LioOgmRaster R;
    R.x_min = x_min; R.y_min = y_min; R.res = res;
    if (!lio_ogm_dims(x_min, x_max, y_min, y_max, res, &R.width, &R.height)) { printf("raster %-22s: too many cells\n", name); return; }
    R.j_end = whole_box ? R.height : R.height - 1;
    const long long cells = (long long)R.width * R.height;
    std::vector<signed char> a((size_t)cells, 0), b((size_t)cells, 0);
    long long bad = 0;
    int binned = 0;
    for (int k = 0; k < n; ++k) {
        const long long c = lio_ogm_raster_cell(R, pts[(size_t)k].x, pts[(size_t)k].y);
        if (c >= cells) { ++g_oob; continue; }
        if (c >= 0) { a[(size_t)c] = 100; ++binned; }
        // the draft's lines, with the conversion guarded (a quotient that does not fit an int is outside the grid)
        const double di = ((double)pts[(size_t)k].x - x_min) / res, dj = ((double)pts[(size_t)k].y - y_min) / res;
        if (!(fabs(di) < 2.0e9) || !(fabs(dj) < 2.0e9)) { if (c >= 0) ++bad; continue; }
        const int i = (int)di, j = (int)dj;
        const bool skip = i < 0 || i >= R.width || j < 0 || j >= R.j_end;
        if (skip != (c < 0)) ++bad;
        if (!skip) b[(size_t)(i + (long long)j * R.width)] = 100;
    }
    if (a != b) ++bad;
    g_bad += bad;
    printf("raster %-22s n %5d res %.3g whole_box %d: %d x %d, binned %d, mismatches %lld\n", name, n, res, whole_box, R.width, R.height,
           binned, bad);
}

static Cloud shifted(const Cloud& c, float ox, float oy, float oz)
{
    Cloud o = c;
    for (float4& p : o) { p.x += ox; p.y += oy; p.z += oz; }
    return o;
}

int main()
{
    Rng rng = { 31 };
    const float params[3][2] = { { 1.0f, 3 }, { 1.5f, 10 }, { 0.5f, 1 } };
    const float offs[4][3] = { { 0, 0, 0 }, { 100.0f, -250.0f, 3.0f }, { 1.0e4f, -1.0e4f, 50.0f }, { -9999.5f, 1.0e4f, -1.0e3f } };
    for (int n : { 257, 513 }) {
        Cloud c;
        for (int i = 0; i < n; ++i) c.push_back(make_float4(rng.range(-6, 6), rng.range(-6, 6), rng.range(-1.2, 1.2), (float)i));
        for (const auto& o : offs)
            for (const auto& p : params) {
                const Cloud s = shifted(c, o[0], o[1], o[2]);
                check_filter(n == 257 ? "uniform257" : "uniform513", s, p[0], (int)p[1]);
            }
        for (const auto& o : offs)
            for (int wb = 0; wb < 2; ++wb) check_raster("uniform", shifted(c, o[0], o[1], o[2]), 0.25, wb);
        Cloud d = c;
        d.insert(d.end(), c.begin(), c.end());
        check_filter("duplicated", d, 1.0f, 3);
    }
    {
        Cloud c;
        for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) for (int k = 0; k < 2; ++k) c.push_back(make_float4(0.5f * i, 0.5f * j, 0.5f * k, 0));
        for (const auto& o : offs) { check_filter("lattice", shifted(c, o[0], o[1], o[2]), 0.5f, 0); check_filter("lattice", shifted(c, o[0], o[1], o[2]), 0.5f, 1); }
    }
    {
        Cloud c;
        for (int i = 0; i < 3000; ++i) c.push_back(make_float4(rng.range(-10, 10), rng.range(-10, 10), rng.range(0, 0.5), 0));
        for (int i = 0; i < 20; ++i) {
            const double r = 100.0 + 45.0 * i, a = 0.7 * i;
            c.push_back(make_float4((float)(r * cos(a)), (float)(r * sin(a)), rng.range(-50, 50), 0));
        }
        for (const auto& o : offs) check_filter("isolated", shifted(c, o[0], o[1], o[2]), 0.5f, 10);
        check_raster("isolated", c, 0.05, 0);
        check_raster("isolated", c, 0.05, 1);
    }
    for (float radius : { 0.5f, 0.3f }) {               // points at multiples of the cell edge from the origin, pairs astride borders
        const float e = radius * 1.001f + 1.0e-5f * 8.0f;
        Cloud c;
        c.push_back(make_float4(0, 0, 0, 0));
        c.push_back(make_float4(8.0f, 8.0f, 8.0f, 0));
        for (int i = 1; i < 12; ++i) {
            const float b = e * (float)i;
            c.push_back(make_float4(b, b, 0.0f, 0));
            c.push_back(make_float4(nextafterf(b, 0.0f), b, 0.0f, 0));
            c.push_back(make_float4(b - 0.4f * radius, 1.0f, 1.0f, 0));
            c.push_back(make_float4(b + 0.4f * radius, 1.0f, 1.0f, 0));
            c.push_back(make_float4(2.0f, b - 0.45f * radius, b + 0.45f * radius, 0));
            c.push_back(make_float4(2.0f, b + 0.45f * radius, b - 0.45f * radius, 0));
        }
        for (const auto& o : offs) check_filter("cell_border", shifted(c, o[0], o[1], o[2]), radius, 1);
    }
    {
        Cloud c;
        for (int i = 0; i < 5; ++i) c.push_back(make_float4(0.01f * i, 0, 0, 0));
        check_filter("below_min", c, 0.5f, 5);
        check_filter("below_min", c, 0.5f, 10);
        check_filter("empty", Cloud(), 0.5f, 1);
        check_filter("one", Cloud(1, make_float4(1, 2, 3, 0)), 0.5f, 0);
        check_raster("one", Cloud(1, make_float4(1, 2, 3, 0)), 0.25, 0);
    }
    {
        Cloud c;
        for (int i = 0; i < 300; ++i) c.push_back(make_float4(rng.range(-3, 3), rng.range(-3, 3), rng.range(0, 1), 0));
        c[7].x = NAN; c[100].y = INFINITY; c[200].z = -INFINITY; c[250].x = 2.0e15f; c[299].z = -1.5e15f;
        check_filter("nonfinite", c, 0.5f, 2);
    }
    {                                                    // the raster's quirks: the last point as the extreme, no extent along x
        Cloud c = { make_float4(0, 0, 0, 0), make_float4(1.0f, 0.75f, 0, 0), make_float4(0.3f, 0.3f, 0, 0), make_float4(0.6f, 0.55f, 0, 0),
                    make_float4(2, 2, 0, 0) };
        for (int wb = 0; wb < 2; ++wb) for (const auto& o : offs) check_raster("by_hand", shifted(c, o[0], o[1], 0), 0.25, wb);
        c.back() = make_float4(-0.2f, -0.1f, 0, 0);
        for (int wb = 0; wb < 2; ++wb) check_raster("last_below_min", c, 0.25, wb);
        c.back() = make_float4(-3.0e9f, 4.0e9f, 0, 0);
        check_raster("last_far", c, 1.0e-3, 0);
        Cloud x = { make_float4(1, 0, 0, 0), make_float4(1, 2, 0, 0), make_float4(1, 1, 0, 0) };
        for (int wb = 0; wb < 2; ++wb) check_raster("no_extent_x", x, 0.25, wb);
    }
    printf("out-of-range reads: %lld, mismatches: %lld\n", g_oob, g_bad);
    return (int)std::min<long long>(g_oob + g_bad, 100);
}
