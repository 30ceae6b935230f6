// grid_geom_host_check.cpp -- the arithmetic of lio_grid_submap, lio_grid_move, lio_grid_extend_to_include and
// lio_grid_add_data_from (lio-slam_amd/csrc/lio_gridgeom.h) run on the host: the text the kernels run -- the geometry each
// call decides, the integer-offset cell and the fp64 position cell -- one cell after the other over heap arrays of exactly
// the layers' sizes, so that AddressSanitizer sees any access outside them.  Stand-alone, needs no GPU:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined tools/grid_geom_host_check.cpp -o /tmp/grid_geom_host_check && /tmp/grid_geom_host_check
//
// Without arguments it runs its own cases (every shape of tests/test_gpu_grid_geom.py, shifts around 0 and the size, windows
// over every edge, `other` inside, across each side and disjoint at several resolutions) and checks what can be said without
// a second implementation: a moved layer against a plain shifted copy, a submap against the source block, the counters
// against each other and against the sizes, every word of a new layer written.  It prints a checksum per shape (FNV-1a over
// every layer's words) and "inconsistencies: 0" at the end; the exit status is their number (capped).
//   grid_geom_host_check submap G QX QY LX LY LAYERS OUT
//   grid_geom_host_check move   G QX QY LAYERS OUT
//   grid_geom_host_check add    G O EXTEND ADD OVERWRITE LISTED_MASK BASIC_MASK LAYERS LAYERS_OTHER OUT
//       G, O: ROWS COLS RES POS_X POS_Y LAYER_MASK.  LAYERS: the layers of the mask, ascending, each column-major.  OUT
//       receives int32 flag (success / moved / resized), rows, cols, layer mask, a[2] (top left / index shift), b[2]
//       (requested index); double length[2], position[2]; int64 cleared, kept, skipped, outside, index outside, copied; then
//       the layers of the mask afterwards.  tests/test_grid_geom_cpu.py compares it with the restatement word for word.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../lio-slam_amd/csrc/lio_gridgeom.h"

static long long g_bad = 0;

struct Map {                       // a map on the host: the layers of `mask` as words, column-major
    LioGridGeom G;
    unsigned mask = 0;
    std::vector<uint32_t> layer[LIO_GRID_MAX_LAYERS];
    size_t cells() const { return (size_t)G.rows * (size_t)G.cols; }
};

struct Result {
    int flag = 0, a[2] = { 0, 0 }, b[2] = { 0, 0 };
    long long cleared = 0, kept = 0, skipped = 0, outside = 0, index_outside = 0, copied = 0;
};

static void make(Map& m, int rows, int cols, double res, double px, double py, unsigned mask)
{
    m.G = lio_gm_geom(rows, cols, res, px, py);
    m.mask = mask;
    for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k) m.layer[k].assign(((mask >> k) & 1u) ? m.cells() : 0, LIO_QNAN_BITS);
}

static bool submap(const Map& src, const double q[2], const double len[2], Map& dst, Result& R)
{
    LioGgSubmap S;
    lio_gg_submap_information(src.G, q, len, &S);
    R.flag = S.ok;
    if (!S.ok) { make(dst, 0, 0, src.G.res, 0.0, 0.0, 0u); return false; }
    make(dst, S.size[0], S.size[1], src.G.res, S.position[0], S.position[1], src.mask);
    for (int a = 0; a < 2; ++a) { R.a[a] = S.top_left[a]; R.b[a] = S.requested[a]; }
    LioGgTable T;
    memset(&T, 0, sizeof(T));
    for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k)
        if ((src.mask >> k) & 1u) { T.self[T.n] = src.layer[k].data(); T.dst[T.n] = dst.layer[k].data(); ++T.n; }
    for (int c = 0; c < dst.G.cols; ++c)
        for (int r = 0; r < dst.G.rows; ++r) R.cleared += lio_gg_offset_cell(T, dst.G.rows, src.G.rows, src.G.cols, S.top_left[0], S.top_left[1], r, c) ? 1 : 0;
    return true;
}

static bool move(Map& m, const double q[2], Result& R)
{
    int shift[2];
    double to[2];
    for (int a = 0; a < 2; ++a) {
        if (!lio_gg_index_shift(q[a] - m.G.pos[a], m.G.res, &shift[a])) return false;
        to[a] = m.G.pos[a] + lio_gg_position_shift(shift[a], m.G.res);
        R.a[a] = shift[a];
    }
    R.flag = (shift[0] != 0 || shift[1] != 0) ? 1 : 0;
    if (R.flag) {
        Map old = m;
        LioGgTable T;
        memset(&T, 0, sizeof(T));
        for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k)
            if ((m.mask >> k) & 1u) { T.self[T.n] = old.layer[k].data(); T.dst[T.n] = m.layer[k].data(); ++T.n; }
        for (int c = 0; c < m.G.cols; ++c)
            for (int r = 0; r < m.G.rows; ++r) R.cleared += lio_gg_offset_cell(T, m.G.rows, m.G.rows, m.G.cols, shift[0], shift[1], r, c) ? 1 : 0;
    }
    m.G = lio_gm_geom(m.G.rows, m.G.cols, m.G.res, to[0], to[1]);
    return true;
}

// extendToInclude (add = false) and addDataFrom, as lio_gridgeom.hip's gg_extend_add decides them
static bool extend_add(Map& g, const Map& other, bool extend, bool add, bool overwrite, unsigned listed, unsigned basic, Result& R)
{
    const LioGridGeom O = g.G, X = other.G;
    LioGridGeom N = O;
    bool resized = false;
    if (extend) {
        double position[2], length[2];
        int size[2];
        for (int a = 0; a < 2; ++a) {
            position[a] = O.pos[a]; length[a] = O.len[a];
            if (lio_gg_extend_axis(X.pos[a], X.len[a], &position[a], &length[a])) resized = true;
        }
        if (resized) {
            for (int a = 0; a < 2; ++a) {
                const double n = lio_gm_size(length[a], O.res);
                if (!(n >= 1.0) || !(n < 16777216.0)) return false;
                size[a] = (int)n;
            }
            for (int a = 0; a < 2; ++a) position[a] = lio_gg_align_axis(position[a], O.pos[a], O.res, size[a], a == 0 ? O.rows : O.cols);
            N = lio_gm_geom(size[0], size[1], O.res, position[0], position[1]);
        }
    }
    R.flag = resized ? 1 : 0;
    if (!resized && !add) return true;
    const unsigned final_mask = g.mask | (add ? listed : 0u);
    const unsigned in_table = resized ? final_mask : ((listed | basic) & final_mask);
    Map old = g;
    if (resized) make(g, N.rows, N.cols, N.res, N.pos[0], N.pos[1], final_mask);
    LioGgTable T;
    memset(&T, 0, sizeof(T));
    for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k) {
        if (!((in_table >> k) & 1u)) continue;
        const bool held = (old.mask >> k) & 1u;
        if (!resized && !held) g.layer[k].assign(g.cells(), 0xdeadbeefu);          // a new slot holds anything before the kernel
        T.dst[T.n] = g.layer[k].data();
        T.self[T.n] = held ? (resized ? old.layer[k].data() : g.layer[k].data()) : nullptr;
        T.other[T.n] = (add && ((listed >> k) & 1u)) ? other.layer[k].data() : nullptr;
        if ((basic >> k) & 1u) T.basic |= 1u << T.n;
        ++T.n;
    }
    g.mask = final_mask;
    const int flags = (resized ? LIO_GG_RESIZE : 0) | (add ? LIO_GG_ADD : 0) | (overwrite ? LIO_GG_OVERWRITE : 0);
    for (int c = 0; c < N.cols; ++c)
        for (int r = 0; r < N.rows; ++r) {
            LioGgCellCount n;
            lio_gg_position_cell(T, N, O, X, flags, r, c, &n);
            R.kept += n.kept; R.skipped += n.skipped_valid; R.outside += n.outside_other;
            R.index_outside += (n.index_outside_self ? 1 : 0) + (n.index_outside_other ? 1 : 0);
            R.copied += n.copied;
        }
    return true;
}

// ---- the dump modes
static bool read_map(char** v, Map& m)
{
    make(m, atoi(v[0]), atoi(v[1]), atof(v[2]), atof(v[3]), atof(v[4]), (unsigned)strtoul(v[5], nullptr, 0));
    return m.G.rows >= 1 && m.G.cols >= 1;
}

static bool read_layers(const char* path, Map& m)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    bool ok = true;
    for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k)
        if ((m.mask >> k) & 1u) ok = ok && fread(m.layer[k].data(), 4, m.cells(), f) == m.cells();
    fclose(f);
    return ok;
}

static bool write_out(const char* path, const Map& m, const Result& R)
{
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const int32_t head[8] = { R.flag, m.G.rows, m.G.cols, (int32_t)m.mask, R.a[0], R.a[1], R.b[0], R.b[1] };
    const double geo[4] = { m.G.len[0], m.G.len[1], m.G.pos[0], m.G.pos[1] };
    const int64_t cnt[6] = { R.cleared, R.kept, R.skipped, R.outside, R.index_outside, R.copied };
    fwrite(head, sizeof(head), 1, f); fwrite(geo, sizeof(geo), 1, f); fwrite(cnt, sizeof(cnt), 1, f);
    for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k)
        if ((m.mask >> k) & 1u) fwrite(m.layer[k].data(), 4, m.cells(), f);
    return fclose(f) == 0;
}

static int dump(int argc, char** argv)
{
    const char* mode = argv[1];
    Map g, other, out;
    Result R;
    if (!strcmp(mode, "submap") && argc == 14) {
        if (!read_map(argv + 2, g) || !read_layers(argv[12], g)) return 2;
        const double q[2] = { atof(argv[8]), atof(argv[9]) }, len[2] = { atof(argv[10]), atof(argv[11]) };
        submap(g, q, len, out, R);
        return write_out(argv[13], out, R) ? 0 : 2;
    }
    if (!strcmp(mode, "move") && argc == 12) {
        if (!read_map(argv + 2, g) || !read_layers(argv[10], g)) return 2;
        const double q[2] = { atof(argv[8]), atof(argv[9]) };
        if (!move(g, q, R)) return 3;
        return write_out(argv[11], g, R) ? 0 : 2;
    }
    if (!strcmp(mode, "add") && argc == 22) {
        if (!read_map(argv + 2, g) || !read_map(argv + 8, other) || !read_layers(argv[19], g) || !read_layers(argv[20], other)) return 2;
        if (!extend_add(g, other, atoi(argv[14]) != 0, atoi(argv[15]) != 0, atoi(argv[16]) != 0, (unsigned)strtoul(argv[17], nullptr, 0),
                        (unsigned)strtoul(argv[18], nullptr, 0), R))
            return 3;
        return write_out(argv[21], g, R) ? 0 : 2;
    }
    fprintf(stderr, "usage: see the head of tools/grid_geom_host_check.cpp\n");
    return 2;
}

// ---- the program's own cases
static uint32_t g_seed = 12345u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static void fill(Map& m)
{
    static const uint32_t special[6] = { 0x7fc12345u, 0xffc54321u, 0x7f800000u, 0xff800000u, 0x80000000u, 0x7f812345u };
    for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k)
        for (uint32_t& w : m.layer[k]) {
            const uint32_t r = rnd();
            float f = (float)(r & 0xffff) / 65536.0f - 0.5f;
            memcpy(&w, &f, 4);
            if ((r >> 16) % 5 == 0) w = special[(r >> 19) % 6];
        }
}

static uint64_t checksum(const Map& m)
{
    uint64_t h = 1469598103934665603ull;
    for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k)
        for (uint32_t w : m.layer[k])
            for (int b = 0; b < 4; ++b) { h ^= (w >> (8 * b)) & 0xffu; h *= 1099511628211ull; }
    return h;
}

static void expect(bool ok, const char* what, int a, int b)
{
    if (!ok) { ++g_bad; printf("  INCONSISTENT %s (%d, %d)\n", what, a, b); }
}

static int own_cases()
{
    static const int rows_of[6] = { 1, 2, 63, 64, 65, 257 }, cols_of[3] = { 1, 2, 5 }, n_layers_of[3] = { 1, 10, 16 };
    int n_case = 0;
    for (int ri = 0; ri < 6; ++ri)
        for (int ci = 0; ci < 3; ++ci) {
            const int rows = rows_of[ri], cols = cols_of[ci], nl = n_layers_of[(ri + ci) % 3];
            const unsigned mask = nl == 16 ? 0xffffu : ((1u << nl) - 1u);
            const double res = (ri & 1) ? 0.1 : 0.25;
            Map g;
            make(g, rows, cols, res, 1.5, -2.25, mask);
            fill(g);
            // move: shifts of 0, +-1, size - 1, size, size + 1 per axis and both
            const int s0[8] = { 0, 1, -1, rows - 1, rows, rows + 1, -(rows - 1), -rows }, s1[6] = { 0, 1, -1, cols - 1, cols, -(cols + 1) };
            for (int i = 0; i < 8; ++i)
                for (int j = 0; j < 6; ++j) {
                    Map m = g;
                    Result R;
                    const double q[2] = { g.G.pos[0] - (double)s0[i] * res, g.G.pos[1] - (double)s1[j] * res };
                    expect(move(m, q, R), "move refused", i, j);
                    expect(R.a[0] == s0[i] && R.a[1] == s1[j], "index shift", R.a[0], R.a[1]);
                    long long cleared = 0;
                    for (int k = 0; k < LIO_GRID_MAX_LAYERS && ((mask >> k) & 1u); ++k)
                        for (int c = 0; c < cols; ++c)
                            for (int r = 0; r < rows; ++r) {
                                const int sr = r + s0[i], sc = c + s1[j];
                                const bool in = sr >= 0 && sr < rows && sc >= 0 && sc < cols;
                                const uint32_t want = in ? g.layer[k][(size_t)sc * rows + sr] : LIO_QNAN_BITS;
                                if (m.layer[k][(size_t)c * rows + r] != want) { expect(false, "moved word", r, c); r = rows; c = cols; }
                                if (k == 0 && !in) ++cleared;
                            }
                    expect(R.cleared == (R.flag ? cleared : 0), "cleared", (int)R.cleared, (int)cleared);
                }
            // submap: windows inside, over each edge and corner, zero length, larger than the map, a centre outside
            const double L0 = g.G.len[0], L1 = g.G.len[1];
            const double win[9][4] = { { 0, 0, 0.3, 0.3 }, { 0.5, 0, 0.4, 0.2 }, { -0.5, 0, 0.4, 0.2 }, { 0, 0.5, 0.2, 0.4 }, { 0, -0.5, 0.2, 0.4 },
                                       { 0.45, 0.45, 0.3, 0.3 }, { -0.45, -0.45, 0.3, 0.3 }, { 0.1, -0.2, 0.0, 0.0 }, { 0, 0, 3.0, 3.0 } };
            for (int w = 0; w < 10; ++w) {
                Map sub;
                Result R;
                double q[2], len[2];
                if (w < 9) { q[0] = g.G.pos[0] + win[w][0] * L0; q[1] = g.G.pos[1] + win[w][1] * L1; len[0] = win[w][2] * L0; len[1] = win[w][3] * L1; }
                else { q[0] = g.G.pos[0] + 0.75 * L0; q[1] = g.G.pos[1]; len[0] = L0; len[1] = L1; }
                const bool ok = submap(g, q, len, sub, R);
                if (w == 9) { expect(!ok, "a centre outside the map succeeded", w, 0); continue; }
                if (!ok) continue;                             // (a centre on the low edge may fail, as in the reference)
                expect(R.cleared == 0, "submap cell outside its source", (int)R.cleared, w);
                expect(R.a[0] >= 0 && R.a[0] + sub.G.rows <= rows && R.a[1] >= 0 && R.a[1] + sub.G.cols <= cols, "submap block", R.a[0], R.a[1]);
                for (int k = 0; k < LIO_GRID_MAX_LAYERS && ((mask >> k) & 1u); ++k)
                    for (int c = 0; c < sub.G.cols; ++c)
                        for (int r = 0; r < sub.G.rows; ++r)
                            if (sub.layer[k][(size_t)c * sub.G.rows + r] != g.layer[k][(size_t)(c + R.a[1]) * rows + (r + R.a[0])]) {
                                expect(false, "submap word", r, c);
                                r = sub.G.rows; c = sub.G.cols;
                            }
            }
            // extend and add: other inside, across each side, disjoint; offsets of 0, 0.2, 0.5 cells; four resolutions
            const double at[6][2] = { { 0, 0 }, { 0.6, 0 }, { -0.6, 0 }, { 0, 0.6 }, { 0, -0.6 }, { 2.0, -2.0 } };
            const double off[3] = { 0.0, 0.2, 0.5 }, scale[4] = { 0.5, 1.0, 2.0, 3.0 };
            for (int p = 0; p < 6; ++p)
                for (int o = 0; o < 3; ++o) {
                    const double ores = res * scale[(p + o) % 4];
                    Map other;
                    make(other, 7, 4, ores, g.G.pos[0] + at[p][0] * L0 + off[o] * res, g.G.pos[1] + at[p][1] * L1 - off[o] * res, 0x8005u & (mask | 0x8000u));
                    fill(other);
                    for (int variant = 0; variant < 4; ++variant) {
                        Map m = g;
                        Result R;
                        const bool add = variant != 0, extend = variant != 3, overwrite = variant == 2;
                        const unsigned basic = variant == 1 ? 1u : (variant == 2 ? mask : 0u);
                        expect(extend_add(m, other, extend, add, overwrite, other.mask, basic, R), "extend_add refused", p, o);
                        const long long cells = (long long)m.cells();
                        if (add) expect(R.skipped + R.outside <= cells && R.copied <= 16 * (cells - R.skipped - R.outside), "counters", p, o);
                        if (R.flag) expect(R.kept <= (long long)g.cells() && cells > (long long)g.cells(), "kept", (int)R.kept, (int)g.cells());
                        if (!R.flag && !add) expect(checksum(m) == checksum(g), "untouched", p, o);
                        for (int k = 0; k < LIO_GRID_MAX_LAYERS; ++k)
                            for (uint32_t w : m.layer[k])
                                if (w == 0xdeadbeefu) { expect(false, "a word of a new layer was never written", k, variant); break; }
                        if (variant == 1 && p == 1 && o == 1)
                            printf("case %3d  %3d x %d, %2d layers -> %3d x %d  kept %lld skipped %lld outside %lld index %lld copied %lld  %016llx\n", n_case, rows,
                                   cols, nl, m.G.rows, m.G.cols, R.kept, R.skipped, R.outside, R.index_outside, R.copied, (unsigned long long)checksum(m));
                    }
                }
            ++n_case;
        }
    printf("inconsistencies: %lld\n", g_bad);
    return g_bad > 100 ? 100 : (int)g_bad;
}

int main(int argc, char** argv)
{
    if (argc > 1) return dump(argc, argv);
    return own_cases();
}
