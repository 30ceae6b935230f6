// lio_gridexpr.h -- grid_map_filters' MathExpressionFilter on the layers of a resident object (lio_gridexpr.hip): an EigenLab
// expression (EigenLab.h, Parser<Eigen::MatrixXf>) compiled on the host into a small postfix program, and the program's
// arithmetic as __host__ __device__ functions, so that the kernels (an LDS stack) and a host program (a checked array) run the
// same text.  The compiler is a port of the parser's chunk passes in their order and with their loops --
// splitEquationIntoChunks (:316-492), evalNegations (:1139), evalPowers (:1181), evalMultiplication (:1248), evalAddition
// (:1339), evalFunction (:805) -- where a chunk's value is a node of an expression tree instead of a matrix: the parser's
// quirks (negation before powers, left to right within a pass, fields that run to the next operator) carry over by
// construction.  A value is a full layer ("matrix") or 1 x 1 ("scalar"); the shapes exist only here, on the device a scalar is
// a value that is the same in every lane.  DESIGN.md section 4q lists the conventions and the labelled deviations (parity
// unpinned).  Everything here relies on -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <errno.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/liogpu.h"
#include "lio_gridfilter.h"

#define LIO_GX_MAX_EXPR 1024       // bytes of the expression
#define LIO_GX_MAX_OPS 128         // instructions over all passes
#define LIO_GX_MAX_STACK 16
#define LIO_GX_MAX_REDUCE 8        // map-wide reductions, one pass each
#define LIO_GX_MAX_NAMES 16
#define LIO_GX_LANES 256           // k_gx_eval's block and k_gx_reduce's evaluating lanes
#define LIO_GX_CHUNK 1024          // cells the reduction walker evaluates between two folds
#define LIO_GX_INV_LN10 ((float)(1.0 / 2.302585092994046))      // EigenLab.h:831, (1.0 / log(10)) narrowed by the float product

enum {                             // instructions
    LIO_GX_PUSH_LAYER = 0,         // arg: the layer id
    LIO_GX_PUSH_CONST,             // arg: the float's word
    LIO_GX_PUSH_SLOT,              // arg: the pass whose reduction it is
    LIO_GX_NEG, LIO_GX_ABS, LIO_GX_SQRT, LIO_GX_SQUARE, LIO_GX_EXP, LIO_GX_LOG, LIO_GX_LOG10, LIO_GX_SIN, LIO_GX_COS, LIO_GX_TAN,
    LIO_GX_ASIN, LIO_GX_ACOS,
    LIO_GX_ISNUM,                  // numberOfFinites of a scalar: x == x ? 1 : 0
    LIO_GX_MEAN1,                  // meanOfFinites of a scalar: x / (x == x ? 1 : 0)
    LIO_GX_ADD, LIO_GX_SUB, LIO_GX_MUL, LIO_GX_DIV, LIO_GX_POW, LIO_GX_CWMIN, LIO_GX_CWMAX,
    LIO_GX_N_CODES
};
#define LIO_GX_FIRST_BINARY LIO_GX_ADD

enum { LIO_GX_SUM = 0, LIO_GX_MEAN, LIO_GX_MIN, LIO_GX_MAX, LIO_GX_COUNT, LIO_GX_STORE };     // a pass's sink

struct LioGxOp {
    uint32_t code, arg;
};

// Pass p is ops [p == 0 ? 0 : end[p - 1], end[p]); passes 0 .. n_passes - 2 reduce into scalar slot p, the last one stores.  A
// kernel argument by value: the layout is part of the kernels' code.
struct LioGxProgram {
    LioGxOp ops[LIO_GX_MAX_OPS];
    int32_t end[LIO_GX_MAX_REDUCE + 1];
    int32_t kind[LIO_GX_MAX_REDUCE + 1];
    int32_t n_ops, n_passes, stack_depth;
    uint32_t layers_read;
};

// ---- the arithmetic (EigenLab.h:809-853, :1202-1222, :1269-1304, :1360-1395, :766-793) ------------------------------------
// acos is the call lio_terr_cell makes; every other transcendental and pow is the fp64 function on the widened argument,
// narrowed once (Eigen's packet functions depend on its version and SIMD width: a labelled deviation).
LIO_HD float lio_gx_unary(uint32_t code, float x)
{
    switch (code) {
    case LIO_GX_NEG: return x * -1.0f;                       // :1151, array() *= -1
    case LIO_GX_ABS: return fabsf(x);
    case LIO_GX_SQRT: return sqrtf(x);
    case LIO_GX_SQUARE: return x * x;
    case LIO_GX_EXP: return (float)exp((double)x);
    case LIO_GX_LOG: return (float)log((double)x);
    case LIO_GX_LOG10: return (float)log((double)x) * LIO_GX_INV_LN10;
    case LIO_GX_SIN: return (float)sin((double)x);
    case LIO_GX_COS: return (float)cos((double)x);
    case LIO_GX_TAN: return (float)tan((double)x);
    case LIO_GX_ASIN: return (float)asin((double)x);
    case LIO_GX_ACOS: return acosf(x);
    case LIO_GX_ISNUM: return x == x ? 1.0f : 0.0f;
    default: return x / (x == x ? 1.0f : 0.0f);              // LIO_GX_MEAN1
    }
}

// a is the left operand.  cwiseMin / cwiseMax are Eigen's scalar path numext::mini / maxi, also on a NaN (a labelled
// deviation from a vectorised build's packet min / max), the convention of lio_gf_min_of_finites.
LIO_HD float lio_gx_binary(uint32_t code, float a, float b)
{
    switch (code) {
    case LIO_GX_ADD: return a + b;
    case LIO_GX_SUB: return a - b;
    case LIO_GX_MUL: return a * b;
    case LIO_GX_DIV: return a / b;
    case LIO_GX_POW: return (float)pow((double)a, (double)b);
    case LIO_GX_CWMIN: return b < a ? b : a;
    default: return a < b ? b : a;                           // LIO_GX_CWMAX
    }
}

// One pass on one cell.  The top of the stack is a register; S::put(slot, v) / S::get(slot) hold the words below it, slot <
// stack_depth - 1.  C::layer(id) is the cell's word of a layer, C::slot(p) the scalar of an earlier pass.  Every branch here
// depends on the program alone.
template <class S, class C>
LIO_HD float lio_gx_run_pass(const LioGxProgram& P, int pass, S& stack, const C& cell)
{
    float top = 0.0f;
    int sp = 0;                                              // words on the stack, the top included
    for (int k = pass == 0 ? 0 : P.end[pass - 1]; k < P.end[pass]; ++k) {
        const uint32_t code = P.ops[k].code, arg = P.ops[k].arg;
        if (code >= LIO_GX_FIRST_BINARY) {
            top = lio_gx_binary(code, stack.get(sp - 2), top);
            --sp;
        } else if (code > LIO_GX_PUSH_SLOT) {
            top = lio_gx_unary(code, top);
        } else {
            if (sp > 0) stack.put(sp - 1, top);
            ++sp;
            if (code == LIO_GX_PUSH_LAYER) top = cell.layer((int)arg);
            else if (code == LIO_GX_PUSH_CONST) top = __builtin_bit_cast(float, arg);
            else top = cell.slot((int)arg);
        }
    }
    return top;
}

// Eigen's default-traversal redux with a functor without packet access, one coefficient further: serial in memory order, the
// first coefficient initialises (DenseBasePlugin.hpp:3-30 over FunctorsPlugin.hpp).
struct LioGxFold {
    float acc;
    long long cnt;
    bool first;
};
LIO_HD void lio_gx_fold_begin(LioGxFold& F) { F.acc = 0.0f; F.cnt = 0; F.first = true; }
LIO_HD void lio_gx_fold(LioGxFold& F, int kind, float v)
{
    if (kind == LIO_GX_MIN) F.acc = F.first ? v : lio_gf_min_of_finites(F.acc, v);
    else if (kind == LIO_GX_MAX) F.acc = F.first ? v : lio_gf_max_of_finites(F.acc, v);
    else if (kind != LIO_GX_COUNT) F.acc = F.first ? v : lio_gf_sum_of_finites(F.acc, v);
    F.first = false;
    F.cnt += v == v ? 1 : 0;                                 // numberOfFinites counts x == x: an infinity counts
}
LIO_HD float lio_gx_fold_end(const LioGxFold& F, int kind)
{
    if (kind == LIO_GX_COUNT) return (float)F.cnt;
    if (kind == LIO_GX_MEAN) return F.acc / (float)F.cnt;
    return F.acc;
}

// ---- the compiler (host) ---------------------------------------------------------------------------------------------------
struct LioGxRefusal {
    int code;
    std::string why;
};

namespace lio_gx {

enum { VALUE = 0, VARIABLE, OPERATOR, FUNCTION };            // EigenLab's ChunkType
enum { N_REDUCE = 100 };                                     // a tree node's code: an instruction, or N_REDUCE + the sink's kind

struct Node {
    int code, a, b;
    uint32_t arg;
    bool matrix;
};

struct Chunk {
    std::string field;
    int type, node;
};

inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }
inline bool is_digit(char c) { return c >= '0' && c <= '9'; }
inline bool is_op1(char c) { return c != '\0' && strchr("+-*/^()[]=", c) != nullptr; }
inline bool is_op2(const std::string& s, size_t at)
{
    return at + 1 < s.size() && s[at] == '.' && (s[at + 1] == '+' || s[at + 1] == '-' || s[at + 1] == '*' || s[at + 1] == '/' || s[at + 1] == '^');
}

inline std::string trim(const std::string& s)              // :1538-1546 (a string of spaces alone keeps one)
{
    if (s.empty()) return s;
    size_t first = 0, last = s.size() - 1;
    while (first < last && is_space(s[first])) ++first;
    while (first < last && is_space(s[last])) --last;
    return s.substr(first, last + 1 - first);
}

// isNumber<double> (:1565-1575): what operator>>(double) consumes to the end of the field -- an optional sign, digits with an
// optional point, an optional exponent -- and represents (an overflow fails the stream)
inline bool is_number(const std::string& s, double* num)
{
    size_t i = 0, digits = 0;
    if (i < s.size() && (s[i] == '+' || s[i] == '-')) ++i;
    while (i < s.size() && is_digit(s[i])) { ++i; ++digits; }
    if (i < s.size() && s[i] == '.') {
        ++i;
        while (i < s.size() && is_digit(s[i])) { ++i; ++digits; }
    }
    if (!digits) return false;
    if (i < s.size() && (s[i] == 'e' || s[i] == 'E')) {
        ++i;
        if (i < s.size() && (s[i] == '+' || s[i] == '-')) ++i;
        const size_t e0 = i;
        while (i < s.size() && is_digit(s[i])) ++i;
        if (i == e0) return false;
    }
    if (i != s.size()) return false;
    errno = 0;
    const double v = strtod(s.c_str(), nullptr);
    if (errno == ERANGE && (v == HUGE_VAL || v == -HUGE_VAL)) return false;
    *num = v;
    return true;
}

const char* const FUNCTIONS[] = { "abs", "sqrt", "square", "exp", "log", "log10", "sin", "cos", "tan", "asin", "acos", "trace", "norm", "size", "min",
                                  "minOfFinites", "max", "maxOfFinites", "absmax", "cwiseMin", "cwiseMax", "mean", "meanOfFinites", "sum", "sumOfFinites", "prod",
                                  "numberOfFinites", "transpose", "conjugate", "adjoint", "zeros", "ones", "eye" };

struct Compiler {
    std::vector<std::string> names;
    std::vector<int> ids;
    std::vector<Node> nodes;

    [[noreturn]] static void refuse(const std::string& why) { throw LioGxRefusal{ LIO_ERR_ARG, why }; }

    bool is_function(const std::string& s) const
    {
        for (const char* f : FUNCTIONS)
            if (s == f) return true;
        return false;
    }
    int variable(const std::string& s) const
    {
        for (size_t k = 0; k < names.size(); ++k)
            if (names[k] == s) return (int)k;
        return -1;
    }
    int add(int code, int a, int b, uint32_t arg, bool matrix)
    {
        nodes.push_back(Node{ code, a, b, arg, matrix });
        return (int)nodes.size() - 1;
    }
    // the value of an operand chunk: a VARIABLE resolves when an operation first reads it (:1153, :1193, ...)
    int value_of(Chunk& c, const std::string& op)
    {
        if (c.type == VARIABLE) {
            const int k = variable(c.field);
            if (k < 0) refuse("unknown name '" + c.field + "'");
            c.node = add(LIO_GX_PUSH_LAYER, -1, -1, (uint32_t)ids[(size_t)k], true);
            c.type = VALUE;
        }
        if (c.type != VALUE) refuse("operator '" + op + "' lacks an operand");
        return c.node;
    }

    static size_t closing(const std::string& s, size_t open, char close)      // :495-505; s.size(): none
    {
        int depth = 1;
        for (size_t i = open + 1; i < s.size(); ++i) {
            if (s[i] == s[open]) ++depth;
            else if (s[i] == close) --depth;
            if (depth == 0) return i;
        }
        return s.size();
    }

    static std::vector<std::string> split_arguments(const std::string& s)     // :508-522 with ','
    {
        std::vector<std::string> args;
        size_t i0 = 0;
        for (size_t i = 0; i < s.size(); ++i) {
            if (s[i] == '(' || s[i] == '[') {
                i = closing(s, i, s[i] == '(' ? ')' : ']');
                if (i == s.size()) refuse("missing closing bracket in '" + s + "'");
            } else if (s[i] == ',') {
                args.push_back(trim(s.substr(i0, i - i0)));
                i0 = i + 1;
            }
        }
        args.push_back(s.substr(i0));
        return args;
    }

    int reduction(int kind, int arg)
    {
        if (nodes[(size_t)arg].matrix) return add(N_REDUCE + kind, arg, -1, 0, false);
        if (kind == LIO_GX_COUNT) return add(LIO_GX_ISNUM, arg, -1, 0, false);
        if (kind == LIO_GX_MEAN) return add(LIO_GX_MEAN1, arg, -1, 0, false);
        return arg;                                          // the redux of one coefficient is the coefficient
    }

    int eval_function(const std::string& name, const std::vector<std::string>& args)      // :805-1027
    {
        static const char* const refused[] = { "trace", "norm", "size", "transpose", "conjugate", "adjoint", "zeros", "ones", "eye", "prod" };
        static const char* const packet[] = { "sum", "mean", "min", "max", "absmax" };
        for (const char* f : refused)
            if (name == f) refuse("function '" + name + "' is a matrix operation and not supported");
        for (const char* f : packet)
            if (name == f) refuse("function '" + name + "' reduces in the order of the Eigen build (use " + name + "OfFinites)");
        static const struct { const char* name; int code; } unary[] = {
            { "abs", LIO_GX_ABS }, { "sqrt", LIO_GX_SQRT }, { "square", LIO_GX_SQUARE }, { "exp", LIO_GX_EXP }, { "log", LIO_GX_LOG }, { "log10", LIO_GX_LOG10 },
            { "sin", LIO_GX_SIN }, { "cos", LIO_GX_COS }, { "tan", LIO_GX_TAN }, { "asin", LIO_GX_ASIN }, { "acos", LIO_GX_ACOS } };
        static const struct { const char* name; int kind; } reduce[] = {
            { "sumOfFinites", LIO_GX_SUM }, { "meanOfFinites", LIO_GX_MEAN }, { "minOfFinites", LIO_GX_MIN }, { "maxOfFinites", LIO_GX_MAX },
            { "numberOfFinites", LIO_GX_COUNT } };
        const bool cw = name == "cwiseMin" || name == "cwiseMax";
        if (args.size() == 1) {
            if (cw) refuse("function '" + name + "' takes two arguments");
            const int arg = eval(args[0]);
            for (const auto& u : unary)
                if (name == u.name) return add(u.code, arg, -1, 0, nodes[(size_t)arg].matrix);
            for (const auto& r : reduce)
                if (name == r.name) return reduction(r.kind, arg);
        } else if (args.size() == 2) {
            if (!cw) refuse("function '" + name + "' with a second (dimension) argument is not supported");
            const int a = eval(args[0]), b = eval(args[1]);
            if (!nodes[(size_t)a].matrix && nodes[(size_t)b].matrix) refuse("function '" + name + "': a scalar against a matrix has no dimensions in common");
            return add(name == "cwiseMin" ? LIO_GX_CWMIN : LIO_GX_CWMAX, a, b, 0, nodes[(size_t)a].matrix);
        }
        refuse("function '" + name + "' does not take " + std::to_string(args.size()) + " arguments");
    }

    std::vector<Chunk> split(const std::string& e)          // :316-492
    {
        std::vector<Chunk> chunks;
        for (size_t it = 0; it < e.size();) {
            const int prev = chunks.empty() ? -1 : chunks.back().type;
            const char ci = e[it];
            if (is_space(ci)) {
                ++it;
            } else if (ci == '(' && (prev == VALUE || prev == VARIABLE)) {
                refuse("index group '" + chunks.back().field + "(...)' is not supported");
            } else if (ci == '(') {
                const size_t jt = closing(e, it, ')');
                if (jt == e.size()) refuse("missing closing bracket for '" + e.substr(it) + "'");
                const std::string field = e.substr(it + 1, jt - it - 1);
                if (prev == FUNCTION) {
                    chunks.back().node = eval_function(chunks.back().field, split_arguments(field));
                    chunks.back().field += "(" + field + ")";
                    chunks.back().type = VALUE;
                } else {
                    chunks.push_back(Chunk{ field, VALUE, eval(field) });
                }
                it = jt + 1;
            } else if (ci == '[') {
                refuse("matrix literal '[...]' is not supported");
            } else if (is_op2(e, it)) {
                chunks.push_back(Chunk{ e.substr(it, 2), OPERATOR, -1 });
                it += 2;
            } else if (is_op1(ci)) {
                chunks.push_back(Chunk{ std::string(1, ci), OPERATOR, -1 });
                it += 1;
            } else {
                size_t jt = it + 1;
                unsigned char state = 1;                     // accept fp-strings: the exponent's sign is no operator (:428-451)
                static const unsigned char nextstate[9][5] = { { 0, 0, 0, 0, 0 }, { 1, 2, 3, 4, 0 }, { 0, 0, 3, 4, 0 }, { 0, 0, 3, 5, 6 }, { 0, 0, 5, 0, 0 },
                                                               { 0, 0, 5, 0, 6 }, { 0, 7, 8, 0, 0 }, { 0, 0, 8, 0, 0 }, { 0, 0, 8, 0, 0 } };
                for (size_t kt = it; state && kt < e.size(); ++kt) {
                    int token;
                    if (e[kt] == ' ') token = 0;
                    else if (e[kt] == '+' || e[kt] == '-') token = 1;
                    else if (is_digit(e[kt])) token = 2;
                    else if (e[kt] == '.') token = 3;
                    else if (e[kt] == 'e' || e[kt] == 'E') token = 4;
                    else break;
                    state = nextstate[state][token];
                    if (state == 8) jt = kt;
                }
                for (; jt < e.size(); ++jt)
                    if (is_op1(e[jt]) || is_op2(e, jt)) break;
                const std::string field = trim(e.substr(it, jt - it));
                if (prev == VALUE || prev == VARIABLE) refuse("'" + chunks.back().field + "' and '" + field + "' follow each other without an operator");
                double num;
                if (field.find(':') != std::string::npos) refuse("range '" + field + "' with ':' is not supported");
                if (is_number(field, &num)) chunks.push_back(Chunk{ field, VALUE, add(LIO_GX_PUSH_CONST, -1, -1, __builtin_bit_cast(uint32_t, (float)num), false) });
                else if (variable(field) >= 0) chunks.push_back(Chunk{ field, VARIABLE, -1 });
                else if (is_function(field)) chunks.push_back(Chunk{ field, FUNCTION, -1 });
                else chunks.push_back(Chunk{ field, VARIABLE, -1 });          // "new undefined variable": refused where it is read
                it = jt;
            }
        }
        for (const Chunk& c : chunks)
            if (c.type == FUNCTION) refuse("function '" + c.field + "' without '('");
        return chunks;
    }

    void eval_negations(std::vector<Chunk>& C)              // :1139-1178
    {
        if (C.size() < 2) return;
        size_t lhs = 0, op = 0, rhs = 1;
        while (lhs < C.size() && op < C.size() && rhs < C.size()) {
            if (C[op].type == OPERATOR && C[op].field == "-" && (op == 0 || (C[lhs].type != VALUE && C[lhs].type != VARIABLE)) &&
                (C[rhs].type == VALUE || C[rhs].type == VARIABLE)) {
                const int v = value_of(C[rhs], "-");
                C[rhs].node = add(LIO_GX_NEG, v, -1, 0, nodes[(size_t)v].matrix);
                C.erase(C.begin() + (long)op);
                lhs = op;
                op = lhs < C.size() ? lhs + 1 : lhs;
                rhs = op < C.size() ? op + 1 : op;
            } else {
                lhs = op;
                op = rhs;
                ++rhs;
            }
        }
    }

    // evalPowers (:1181), evalMultiplication (:1248) and evalAddition (:1339) are one loop over three operator sets
    void eval_binary(std::vector<Chunk>& C, int level)
    {
        if (C.size() < 3) return;
        size_t lhs = 0, op = 1, rhs = 2;
        while (lhs < C.size() && op < C.size() && rhs < C.size()) {
            const std::string& f = C[op].field;
            const bool mine = C[op].type == OPERATOR && (level == 0 ? (f == "^" || f == ".^") : level == 1 ? (f == "*" || f == "/" || f == ".*" || f == "./")
                                                                                                          : (f == "+" || f == "-" || f == ".+" || f == ".-"));
            if (mine) {
                const int a = value_of(C[lhs], f), b = value_of(C[rhs], f);
                const bool ma = nodes[(size_t)a].matrix, mb = nodes[(size_t)b].matrix, dotted = f[0] == '.';
                const char sign = f[f.size() - 1];
                if (ma && mb && !dotted && level == 0) refuse("'^' between two matrices is not supported (use '.^')");
                if (ma && mb && !dotted && level == 1) refuse("'" + f + "' between two matrices is not supported (use '." + f + "')");
                const int code = sign == '^' ? LIO_GX_POW : sign == '*' ? LIO_GX_MUL : sign == '/' ? LIO_GX_DIV : sign == '+' ? LIO_GX_ADD : LIO_GX_SUB;
                C[lhs].node = add(code, a, b, 0, ma || mb);
                C[lhs].type = VALUE;
                C.erase(C.begin() + (long)op, C.begin() + (long)rhs + 1);
                op = lhs + 1;
                rhs = op < C.size() ? op + 1 : op;
            } else {
                lhs = op;
                op = rhs;
                ++rhs;
            }
        }
    }

    int eval(const std::string& expression)                 // :283-313
    {
        const std::string e = trim(expression);
        std::vector<Chunk> chunks = split(e);
        eval_negations(chunks);
        eval_binary(chunks, 0);
        eval_binary(chunks, 1);
        eval_binary(chunks, 2);
        for (const Chunk& c : chunks)
            if (c.type == OPERATOR && c.field == "=") refuse("assignment '=' is not supported");
        if (chunks.empty()) refuse("empty expression");
        if (chunks.size() != 1) refuse("'" + e + "' does not reduce to a single value");
        return value_of(chunks[0], chunks[0].field);
    }

    // ---- the tree into passes, operands in the order written
    struct Pass {
        std::vector<LioGxOp> ops;
        int kind;
    };
    std::vector<Pass> passes;

    void lower(int n, std::vector<LioGxOp>& code)
    {
        const Node& N = nodes[(size_t)n];
        if (N.code >= N_REDUCE) {
            std::vector<LioGxOp> sub;
            lower(N.a, sub);
            if (passes.size() >= LIO_GX_MAX_REDUCE) throw LioGxRefusal{ LIO_ERR_CAPACITY, "more than 8 map-wide reductions" };
            passes.push_back(Pass{ sub, N.code - N_REDUCE });
            code.push_back(LioGxOp{ LIO_GX_PUSH_SLOT, (uint32_t)passes.size() - 1 });
            return;
        }
        if (N.a >= 0) lower(N.a, code);
        if (N.b >= 0) lower(N.b, code);
        code.push_back(LioGxOp{ (uint32_t)N.code, N.arg });
    }
};

inline bool name_ok(const char* s)
{
    if (!s || !*s || is_digit(*s)) return false;
    for (; *s; ++s)
        if (!(is_digit(*s) || (*s >= 'a' && *s <= 'z') || (*s >= 'A' && *s <= 'Z') || *s == '_')) return false;
    return true;
}

}  // namespace lio_gx

// LIO_OK and *P, or the refusal's code and *why.  Reads no grid and no device.
inline int lio_gx_compile(const char* expression, const char* const* names, const int32_t* layer_ids, int n_names, LioGxProgram* P, std::string* why)
try {
    using namespace lio_gx;
    memset(P, 0, sizeof(*P));
    if (!expression) Compiler::refuse("null argument");
    if (n_names < 0 || n_names > LIO_GX_MAX_NAMES) Compiler::refuse("n_names must be in [0, 16]");
    if (n_names > 0 && (!names || !layer_ids)) Compiler::refuse("null argument");
    Compiler K;
    for (int k = 0; k < n_names; ++k) {
        if (!name_ok(names[k])) Compiler::refuse("a name must be of [A-Za-z0-9_], not empty and not start with a digit");
        if (K.variable(names[k]) >= 0) Compiler::refuse(std::string("name '") + names[k] + "' is listed twice");
        if (layer_ids[k] < 0 || layer_ids[k] >= LIO_GRID_MAX_LAYERS) Compiler::refuse("a layer id is outside 0 .. 15");
        K.names.push_back(names[k]);
        K.ids.push_back(layer_ids[k]);
    }
    if (strnlen(expression, LIO_GX_MAX_EXPR + 1) > LIO_GX_MAX_EXPR) throw LioGxRefusal{ LIO_ERR_CAPACITY, "the expression is longer than 1024 bytes" };
    const int root = K.eval(expression);
    if (!K.nodes[(size_t)root].matrix) Compiler::refuse("the expression yields a scalar, not a layer");
    std::vector<LioGxOp> last;
    K.lower(root, last);
    K.passes.push_back(Compiler::Pass{ last, LIO_GX_STORE });
    int n = 0, deepest = 0;
    for (size_t p = 0; p < K.passes.size(); ++p) {
        int sp = 0;
        for (const LioGxOp& o : K.passes[p].ops) {
            if (n >= LIO_GX_MAX_OPS) throw LioGxRefusal{ LIO_ERR_CAPACITY, "the expression compiles to more than 128 ops" };
            P->ops[n++] = o;
            if (o.code >= LIO_GX_FIRST_BINARY) --sp;
            else if (o.code <= LIO_GX_PUSH_SLOT) ++sp;
            if (sp > deepest) deepest = sp;
            if (o.code == LIO_GX_PUSH_LAYER) P->layers_read |= 1u << o.arg;
        }
        P->end[p] = n;
        P->kind[p] = K.passes[p].kind;
    }
    if (deepest > LIO_GX_MAX_STACK) throw LioGxRefusal{ LIO_ERR_CAPACITY, "the expression needs a stack deeper than 16" };
    P->n_ops = n;
    P->n_passes = (int)K.passes.size();
    P->stack_depth = deepest;
    return LIO_OK;
} catch (const LioGxRefusal& r) {
    memset(P, 0, sizeof(*P));
    if (why) *why = "expression: " + r.why;
    return r.code;
}

// ---- the program on the host, serially: the text the kernels run.  layer[id]: column-major cells, for every id the program
// reads.  bad (may be null) counts the stack accesses outside the compiled depth.
struct LioGxHostStack {
    float v[LIO_GX_MAX_STACK];
    int depth;
    long long* bad;
    void put(int slot, float x) { if (slot < 0 || slot >= depth - 1) { if (bad) ++*bad; return; } v[slot] = x; }
    float get(int slot) const { if (slot < 0 || slot >= depth - 1) { if (bad) ++*bad; return 0.0f; } return v[slot]; }
};
struct LioGxHostCell {
    const float* const* layers;
    const float* slots;
    size_t lin;
    float layer(int id) const { return layers[id][lin]; }
    float slot(int p) const { return slots[p]; }
};
inline long long lio_gx_host_run(const LioGxProgram& P, const float* const* layer, size_t cells, float* out, long long* bad)
{
    float slots[LIO_GX_MAX_REDUCE] = {};
    LioGxHostStack S;
    S.depth = P.stack_depth; S.bad = bad;
    long long n_finite = 0;
    std::vector<float> result(cells);                        // out may be a layer the program reads
    for (int p = 0; p < P.n_passes; ++p) {
        LioGxFold F;
        lio_gx_fold_begin(F);
        for (size_t lin = 0; lin < cells; ++lin) {
            const LioGxHostCell cell = { layer, slots, lin };
            const float v = lio_gx_run_pass(P, p, S, cell);
            if (P.kind[p] == LIO_GX_STORE) { result[lin] = v; n_finite += lio_gm_finite(v) ? 1 : 0; }
            else lio_gx_fold(F, P.kind[p], v);
        }
        if (P.kind[p] != LIO_GX_STORE) slots[p] = lio_gx_fold_end(F, P.kind[p]);
    }
    if (cells) memcpy(out, result.data(), sizeof(float) * cells);
    return n_finite;
}
