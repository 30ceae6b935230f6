// grid_expression_host_check.cpp -- the compiler and the interpreter of lio_grid_filter_expression
// (lio-slam_amd/csrc/lio_gridexpr.h) run on the host: the text the kernels run, one cell after the other, with a stack that
// counts every access outside the compiled depth.  Stand-alone, needs no GPU:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined tools/grid_expression_host_check.cpp -o /tmp/grid_expression_host_check && /tmp/grid_expression_host_check
//
// It runs its own cases and checks what can be said without a second implementation of the parser:
//   - every accepted expression compiles, within the limits, and its program is well formed: a pass never pops an empty stack,
//     ends with one word, reads only slots of earlier passes, and the depth the compiler reports is the depth a walk finds;
//   - every refused expression is refused with its code and a message that names the construct;
//   - the host evaluation of the exact operations equals a plain loop written here, word for word where the value is not a NaN,
//     on grids from 1 x 1 to 37 x 59 with NaN, infinities, signed zeros and denormals; no stack access leaves the compiled depth;
//   - the single-thread time of the traversability expression on a 550 x 400 grid.
// It prints a checksum per evaluated case (FNV-1a over the layer's words, NaNs as one word) and "inconsistencies: 0" at the end;
// the exit status is their number (capped).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <functional>
#include <string>
#include <vector>

#include "../lio-slam_amd/csrc/lio_gridexpr.h"

static int g_bad = 0;
static void bad(const char* what, const std::string& e)
{
    ++g_bad;
    printf("INCONSISTENT %s: '%s'\n", what, e.size() > 80 ? (e.substr(0, 77) + "...").c_str() : e.c_str());
}

static const char* const NAMES[] = { "a", "b", "c" };
static const int32_t IDS[] = { 0, 1, 2 };

static std::string chain(int n)
{
    std::string s;
    for (int k = 0; k < n - 1; ++k) s += "a + (";
    s += "a";
    for (int k = 0; k < n - 1; ++k) s += ")";
    return s;
}
static std::string repeat(const std::string& head, const std::string& part, int n)
{
    std::string s = head;
    for (int k = 0; k < n; ++k) s += part;
    return s;
}

// the program's own consistency: what a kernel relies on
static void check_program(const LioGxProgram& P, const std::string& e)
{
    if (P.n_passes < 1 || P.n_passes > LIO_GX_MAX_REDUCE + 1 || P.n_ops < 1 || P.n_ops > LIO_GX_MAX_OPS || P.end[P.n_passes - 1] != P.n_ops) { bad("limits", e); return; }
    if (P.kind[P.n_passes - 1] != LIO_GX_STORE) bad("last pass does not store", e);
    int deepest = 0;
    for (int p = 0; p < P.n_passes; ++p) {
        if (p + 1 < P.n_passes && (P.kind[p] < LIO_GX_SUM || P.kind[p] > LIO_GX_COUNT)) bad("sink", e);
        int sp = 0;
        for (int k = p == 0 ? 0 : P.end[p - 1]; k < P.end[p]; ++k) {
            const LioGxOp o = P.ops[k];
            if (o.code >= LIO_GX_N_CODES) { bad("op code", e); return; }
            if (o.code >= LIO_GX_FIRST_BINARY) { if (sp < 2) { bad("binary op on fewer than two words", e); return; } --sp; }
            else if (o.code > LIO_GX_PUSH_SLOT) { if (sp < 1) { bad("unary op on an empty stack", e); return; } }
            else {
                ++sp;
                if (o.code == LIO_GX_PUSH_LAYER && (o.arg >= LIO_GRID_MAX_LAYERS || !(P.layers_read >> o.arg & 1u))) bad("layer id", e);
                if (o.code == LIO_GX_PUSH_SLOT && (int)o.arg >= p) bad("slot of a later pass", e);
            }
            if (sp > deepest) deepest = sp;
        }
        if (sp != 1) bad("a pass does not end with one word", e);
    }
    if (deepest != P.stack_depth || deepest > LIO_GX_MAX_STACK) bad("stack depth", e);
}

static std::vector<float> make_layer(int cells, unsigned seed)
{
    static const float special[] = { NAN, INFINITY, -INFINITY, 0.0f, -0.0f, 1e-40f, -1e-42f, 1.0f, -1.0f, 3.0e38f, 1.1754944e-38f };
    std::vector<float> z((size_t)cells);
    unsigned s = seed * 2654435761u + 12345u;
    for (int k = 0; k < cells; ++k) {
        s = s * 1664525u + 1013904223u;
        const unsigned r = s >> 8;
        z[(size_t)k] = r % 10 < 3 ? special[(r / 16) % 11] : ((float)(r % 40001) - 20000.0f) / 10000.0f;
    }
    return z;
}

static uint32_t word(float v) { return v != v ? LIO_QNAN_BITS : __builtin_bit_cast(uint32_t, v); }

typedef std::function<void(const float*, const float*, const float*, size_t, float*)> Loop;

struct Case {
    const char* e;
    Loop loop;
};

// Eigen's serial redux, written plainly
static float sum_finites(const std::vector<float>& v)
{
    float acc = v[0];
    for (size_t k = 1; k < v.size(); ++k) acc = lio_gf_sum_of_finites(acc, v[k]);
    return acc;
}
static float count_numbers(const std::vector<float>& v)
{
    long long n = 0;
    for (float x : v) n += x == x;
    return (float)n;
}

#define CELL(expr) [](const float* a, const float* b, const float* c, size_t n, float* o) { (void)b; (void)c; for (size_t k = 0; k < n; ++k) o[k] = (expr); }

int main()
{
    // ---- the compiler on what it accepts
    const std::string accepted[] = {
        "a + b", "a - 3", "3 - a", "a .* b", "3 ./ a", "-a^2", "a.^b.^c", "a^2^3", "2^-1 * a", "a - -b", "a - b + c", "1e-3 * a", "a*1.5e+1-b", "abs (a)", " a  +  b ",
        "cwiseMin(a, b)", "cwiseMax(cwiseMin(a, 1), -1)", "acos(a)", "abs(a - b)", "0.5 * (1.0 - (a / 0.6)) + 0.5 * (1.0 - (b / 0.1))", "exp(a) + log(b) + log10(c) + sin(a)",
        "cos(a) + tan(b) + asin(c)", "a - meanOfFinites(a)", "0 * a + sqrt(sumOfFinites(square(a - meanOfFinites(a))) ./ numberOfFinites(a))",
        "numberOfFinites(2) * a", "meanOfFinites(maxOfFinites(a)) + b", "a - meanOfFinites(a - meanOfFinites(a))", "(a - minOfFinites(a)) / (maxOfFinites(a) - minOfFinites(a))",
        chain(16), repeat("a", " + a", 63), repeat("a", " - meanOfFinites(a)", 8), repeat("a", " ", 1023) };
    for (const std::string& e : accepted) {
        LioGxProgram P;
        std::string why;
        if (lio_gx_compile(e.c_str(), NAMES, IDS, 3, &P, &why) != LIO_OK) { bad(("accepted case refused: " + why).c_str(), e); continue; }
        check_program(P, e);
    }
    // ---- and on what it refuses
    const struct { std::string e; int code; const char* part; } refused[] = {
        { "[1, 2; 3, 4] .* a", LIO_ERR_ARG, "matrix literal" }, { "a + 1:3", LIO_ERR_ARG, "range" }, { "a(1, 2)", LIO_ERR_ARG, "index group" },
        { "a = b", LIO_ERR_ARG, "assignment" }, { "a * b", LIO_ERR_ARG, "between two matrices" }, { "a / b", LIO_ERR_ARG, "between two matrices" },
        { "a ^ b", LIO_ERR_ARG, "between two matrices" }, { "trace(a)", LIO_ERR_ARG, "'trace'" }, { "transpose(a)", LIO_ERR_ARG, "'transpose'" },
        { "sum(a) + a", LIO_ERR_ARG, "'sum'" }, { "min(a, 0)", LIO_ERR_ARG, "'min'" }, { "sumOfFinites(a, 0) + a", LIO_ERR_ARG, "dimension" },
        { "cwiseMin(a)", LIO_ERR_ARG, "two arguments" }, { "a + d", LIO_ERR_ARG, "unknown name 'd'" }, { "a b", LIO_ERR_ARG, "unknown name 'a b'" },
        { "sqrt", LIO_ERR_ARG, "without '('" }, { "(a + b", LIO_ERR_ARG, "missing closing bracket" }, { "", LIO_ERR_ARG, "empty expression" },
        { "abs()", LIO_ERR_ARG, "empty expression" }, { "+a", LIO_ERR_ARG, "does not reduce" }, { "--a", LIO_ERR_ARG, "does not reduce" },
        { "a * * b", LIO_ERR_ARG, "lacks an operand" }, { "(a) b", LIO_ERR_ARG, "without an operator" }, { "meanOfFinites(a)", LIO_ERR_ARG, "yields a scalar" },
        { repeat("a", " ", 1024), LIO_ERR_CAPACITY, "1024 bytes" }, { repeat("a", " + a", 64), LIO_ERR_CAPACITY, "128 ops" },
        { chain(17), LIO_ERR_CAPACITY, "deeper than 16" }, { repeat("a", " - meanOfFinites(a)", 9), LIO_ERR_CAPACITY, "8 map-wide reductions" } };
    for (const auto& r : refused) {
        LioGxProgram P;
        std::string why;
        const int rc = lio_gx_compile(r.e.c_str(), NAMES, IDS, 3, &P, &why);
        if (rc != r.code || why.find(r.part) == std::string::npos) bad(("refusal: " + why).c_str(), r.e);
        if (P.n_ops != 0 || P.n_passes != 0) bad("a refused program is not cleared", r.e);
    }
    // ---- the host evaluation of the exact operations against plain loops
    const Case cases[] = {
        { "a + b", CELL(a[k] + b[k]) }, { "3 - a", CELL(3.0f - a[k]) }, { "a .* b ./ c", CELL(a[k] * b[k] / c[k]) }, { "0.5 / a", CELL(0.5f / a[k]) },
        { "-a - -b", CELL(a[k] * -1.0f - b[k] * -1.0f) }, { "a - b + c", CELL(a[k] - b[k] + c[k]) }, { "a / 2 * 3", CELL(a[k] / 2.0f * 3.0f) },
        { "sqrt(abs(a))", CELL(sqrtf(fabsf(a[k]))) }, { "square(a - b)", CELL((a[k] - b[k]) * (a[k] - b[k])) },
        { "cwiseMax(cwiseMin(a, 1), -1)", CELL((1.0f < a[k] ? 1.0f : a[k]) < -1.0f ? -1.0f : (1.0f < a[k] ? 1.0f : a[k])) },
        { "cwiseMin(a, b)", CELL(b[k] < a[k] ? b[k] : a[k]) },
        { "0.5 * (1.0 - (a / 0.6)) + 0.5 * (1.0 - (b / 0.1))", CELL(0.5f * (1.0f - a[k] / 0.6f) + 0.5f * (1.0f - b[k] / 0.1f)) },
        { "a - meanOfFinites(a)", [](const float* a, const float*, const float*, size_t n, float* o) {
             const std::vector<float> v(a, a + n);
             const float mean = sum_finites(v) / count_numbers(v);
             for (size_t k = 0; k < n; ++k) o[k] = a[k] - mean;
         } },
        { "0 * a + sqrt(sumOfFinites(square(a - meanOfFinites(a))) ./ numberOfFinites(a))", [](const float* a, const float*, const float*, size_t n, float* o) {
             const std::vector<float> v(a, a + n);
             const float mean = sum_finites(v) / count_numbers(v);
             std::vector<float> d(n);
             for (size_t k = 0; k < n; ++k) d[k] = (a[k] - mean) * (a[k] - mean);
             const float sd = sqrtf(sum_finites(d) / count_numbers(v));
             for (size_t k = 0; k < n; ++k) o[k] = 0.0f * a[k] + sd;
         } },
        { "", nullptr } };                                    // chain(16), the deepest stack: the plain loop is below
    const std::string deep = chain(16);
    const int shapes[][2] = { { 1, 1 }, { 1, 7 }, { 7, 1 }, { 33, 9 }, { 37, 59 } };
    for (const auto& sh : shapes) {
        const size_t n = (size_t)sh[0] * (size_t)sh[1];
        const std::vector<float> a = make_layer((int)n, 1), b = make_layer((int)n, 2), c = make_layer((int)n, 3);
        const float* layer[LIO_GX_MAX_NAMES] = { a.data(), b.data(), c.data() };
        for (const Case& K : cases) {
            const std::string e = K.loop ? K.e : deep;
            LioGxProgram P;
            std::string why;
            if (lio_gx_compile(e.c_str(), NAMES, IDS, 3, &P, &why) != LIO_OK) { bad("refused", e); continue; }
            std::vector<float> got(n), want(n);
            long long outside = 0;
            const long long n_finite = lio_gx_host_run(P, layer, n, got.data(), &outside);
            if (outside) bad("stack access outside the compiled depth", e);
            if (K.loop) K.loop(a.data(), b.data(), c.data(), n, want.data());
            else
                for (size_t k = 0; k < n; ++k) {                // a + (a + (... + a)): the innermost sum first
                    float s = a[k];
                    for (int j = 1; j < 16; ++j) s = a[k] + s;
                    want[k] = s;
                }
            uint32_t h = 2166136261u;
            long long finite = 0;
            for (size_t k = 0; k < n; ++k) {
                if (word(got[k]) != word(want[k])) { bad("differs from the plain loop", e); break; }
                h = (h ^ word(got[k])) * 16777619u;
                finite += lio_gm_finite(got[k]);
            }
            if (finite != n_finite) bad("finite count", e);
            printf("%2d x %2d  %08x  %s\n", sh[0], sh[1], h, e.size() > 60 ? (e.substr(0, 57) + "...").c_str() : e.c_str());
        }
    }
    // ---- the single-thread time of the host route
    {
        const size_t n = 550 * 400;
        const std::vector<float> a = make_layer((int)n, 4), b = make_layer((int)n, 5);
        const float* layer[LIO_GX_MAX_NAMES] = { a.data(), b.data() };
        std::vector<float> out(n);
        LioGxProgram P;
        std::string why;
        for (const char* e : { "0.5 * (1.0 - (a / 0.6)) + 0.5 * (1.0 - (b / 0.1))", "a - meanOfFinites(a)" }) {
            if (lio_gx_compile(e, NAMES, IDS, 3, &P, &why) != LIO_OK) { bad("refused", e); continue; }
            const auto t0 = std::chrono::steady_clock::now();
            lio_gx_host_run(P, layer, n, out.data(), nullptr);
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            printf("550 x 400, one thread: %.2f ms  %s\n", ms, e);
        }
    }
    printf("inconsistencies: %d\n", g_bad);
    return g_bad > 100 ? 100 : g_bad;
}
