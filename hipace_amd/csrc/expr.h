// expr.h -- expression programs (include/hpslice.h: hps_expr): the validator and the ONE evaluation routine that
// the host (hps_expr_eval_host) and every kernel (k_expr_eval, k_beam_push<ORDER, true>) run.
//
// A program is postfix.  The routine keeps the top of the stack in a register and the levels below it behind a Stack
// policy: a plain array on the host; on the device LDS laid out [level][lane], so that the level index -- the same for
// every lane of a wave -- selects a row and consecutive lanes hit consecutive 8-byte slots (ds_read_b64 / ds_write_b64
// without bank conflicts), and nothing is a runtime-indexed private array (which would live in scratch).  The variables
// come through a Vars policy for the same reason.  Instructions and constants are read with wave-uniform indices from
// read-only memory and dispatched by a switch on the uniform opcode: scalar loads, scalar branches, no divergence.
#ifndef HPS_EXPR_H_
#define HPS_EXPR_H_

#include "common.h"
#include <cmath>

namespace hps {

// values popped by an opcode (every opcode pushes one)
__host__ __device__ inline int expr_npop (int op)
{
    if (op == HPS_EX_CONST || op == HPS_EX_VAR) return 0;
    if (op == HPS_EX_SELECT) return 3;
    switch (op) {
    case HPS_EX_ADD: case HPS_EX_SUB: case HPS_EX_MUL: case HPS_EX_DIV: case HPS_EX_POW: case HPS_EX_LT: case HPS_EX_LE:
    case HPS_EX_GT: case HPS_EX_GE: case HPS_EX_EQ: case HPS_EX_NE: case HPS_EX_AND: case HPS_EX_OR: case HPS_EX_ATAN2:
    case HPS_EX_FMOD: case HPS_EX_MIN: case HPS_EX_MAX: case HPS_EX_HEAVISIDE:
        return 2;
    default:
        return 1;
    }
}

// hps_expr_check: HPS_OK, or HPS_ERR_ARG with the reason in *why (a static string) and the instruction in *at (-1: none)
inline int expr_validate (const hps_expr* p, int n_vars, int* depth, const char** why, int* at)
{
    *at = -1;
    if (!p) { *why = "null program"; return HPS_ERR_ARG; }
    if (n_vars < 0 || n_vars > HPS_EXPR_MAX_VARS) { *why = "exceeds the limits: more than HPS_EXPR_MAX_VARS variables"; return HPS_ERR_ARG; }
    if (p->n_ins > HPS_EXPR_MAX_INS) { *why = "exceeds the limits: more than HPS_EXPR_MAX_INS instructions"; return HPS_ERR_ARG; }
    if (p->n_const < 0 || p->n_const > HPS_EXPR_MAX_CONST) { *why = "exceeds the limits: more than HPS_EXPR_MAX_CONST constants"; return HPS_ERR_ARG; }
    if (p->n_ins <= 0 || !p->ins) { *why = "empty program"; return HPS_ERR_ARG; }
    if (p->n_const > 0 && !p->consts) { *why = "null constant pool"; return HPS_ERR_ARG; }
    int sp = 0, deepest = 0;
    for (int i = 0; i < p->n_ins; ++i) {
        const int op = p->ins[i].op, arg = p->ins[i].arg;
        *at = i;
        if (op < 0 || op >= HPS_EX_NOPS) { *why = "bad opcode"; return HPS_ERR_ARG; }
        if (op == HPS_EX_CONST && (arg < 0 || arg >= p->n_const)) { *why = "operand out of range: constant index outside the pool"; return HPS_ERR_ARG; }
        if (op == HPS_EX_VAR && (arg < 0 || arg >= n_vars)) { *why = "operand out of range: variable index beyond n_vars"; return HPS_ERR_ARG; }
        if (op == HPS_EX_POWI && (arg < -HPS_EXPR_MAX_POWI || arg > HPS_EXPR_MAX_POWI)) { *why = "operand out of range: integer power beyond HPS_EXPR_MAX_POWI"; return HPS_ERR_ARG; }
        const int npop = expr_npop(op);
        if (sp < npop) { *why = "stack underflow"; return HPS_ERR_ARG; }
        sp += 1 - npop;
        if (sp > HPS_EXPR_MAX_DEPTH) { *why = "stack overflow: deeper than HPS_EXPR_MAX_DEPTH"; return HPS_ERR_ARG; }
        deepest = sp > deepest ? sp : deepest;
    }
    *at = -1;
    if (sp != 1) { *why = "the program does not end with exactly one value"; return HPS_ERR_ARG; }
    if (depth) *depth = deepest;
    return HPS_OK;
}

// host stack: the levels below the top
struct ExprHostStack {
    double v[HPS_EXPR_MAX_DEPTH];
    __host__ __device__ void put (int level, double x) { v[level] = x; }
    __host__ __device__ double get (int level) const { return v[level]; }
};
// variables as arrays: vars[k][i] (the host's arrays, or a device table of device arrays)
struct ExprArrayVars {
    const double* const* p; long i;
    __host__ __device__ double get (int k) const { return p[k][i]; }
};
// dynamic LDS of a workgroup of `threads` lanes running programs of at most `depth` levels: the levels below the top (ExprLdsStack)
inline size_t expr_lds_bytes (int depth, int threads) { return (size_t)(depth > 1 ? depth - 1 : 0)*threads*sizeof(double); }
#ifdef __HIPCC__
// device stack: base = this lane's slot of level 0, stride = lanes of the workgroup
struct ExprLdsStack {
    double* base; int stride;
    __device__ __forceinline__ void put (int level, double x) { base[level*stride] = x; }
    __device__ __forceinline__ double get (int level) const { return base[level*stride]; }
};
// the four variables of a particle, in registers: the index is wave-uniform, the chain of selects costs three v_cndmask pairs
struct ExprXyzt {
    double x, y, z, t;
    __device__ __forceinline__ double get (int k) const { return k == 0 ? x : k == 1 ? y : k == 2 ? z : t; }
};
// the three variables of a density program, density(x, y, z), likewise; on the host too (adaptive.hip)
struct ExprXyz {
    double x, y, z;
    __host__ __device__ __forceinline__ double get (int k) const { return k == 0 ? x : k == 1 ? y : z; }
};
#endif

// The routine.  ins / consts: a checked program (expr_validate); the caller's Stack holds depth - 1 levels.
// Every operation rounds once: no contraction to fused multiply-adds in here, whatever the translation unit's default is.
template <class Vars, class Stack>
__host__ __device__ __forceinline__ double expr_run (const hps_expr_ins* __restrict__ ins, int n_ins, const double* __restrict__ consts,
                                                     const Vars& vars, Stack& st)
{
#pragma clang fp contract(off)
    double top = 0.0;
    int below = -1;      // levels in st: 0 .. below - 1 once the first value has been pushed (below = -1: nothing yet)
    for (int pc = 0; pc < n_ins; ++pc) {
        const int op = ins[pc].op, arg = ins[pc].arg;
        if (op == HPS_EX_CONST || op == HPS_EX_VAR) {
            if (below >= 0) st.put(below, top);
            ++below;
            top = (op == HPS_EX_CONST) ? consts[arg] : vars.get(arg);
            continue;
        }
        const int npop = expr_npop(op);
        double a = top, b = 0.0, c = 0.0;      // one argument: a; two: a op b; select: c ? a : b
        if (npop == 2) { b = top; a = st.get(below - 1); below -= 1; }
        if (npop == 3) { b = top; a = st.get(below - 1); c = st.get(below - 2); below -= 2; }
        switch (op) {
        case HPS_EX_ADD: top = a + b; break;
        case HPS_EX_SUB: top = a - b; break;
        case HPS_EX_MUL: top = a*b; break;
        case HPS_EX_DIV: top = a/b; break;
        case HPS_EX_NEG: top = -a; break;
        case HPS_EX_POW: top = pow(a, b); break;
        case HPS_EX_POWI: {
            const int n = arg < 0 ? -arg : arg;
            double r = n == 0 ? 1.0 : a;
            for (int q = 1; q < n; ++q) r = r*a;
            top = arg < 0 ? 1.0/r : r;
        } break;
        case HPS_EX_LT: top = a < b ? 1.0 : 0.0; break;
        case HPS_EX_LE: top = a <= b ? 1.0 : 0.0; break;
        case HPS_EX_GT: top = a > b ? 1.0 : 0.0; break;
        case HPS_EX_GE: top = a >= b ? 1.0 : 0.0; break;
        case HPS_EX_EQ: top = a == b ? 1.0 : 0.0; break;
        case HPS_EX_NE: top = a != b ? 1.0 : 0.0; break;
        case HPS_EX_AND: top = (a != 0.0 && b != 0.0) ? 1.0 : 0.0; break;
        case HPS_EX_OR: top = (a != 0.0 || b != 0.0) ? 1.0 : 0.0; break;
        case HPS_EX_NOT: top = a == 0.0 ? 1.0 : 0.0; break;
        case HPS_EX_SELECT: top = c != 0.0 ? a : b; break;
        case HPS_EX_SQRT: top = sqrt(a); break;
        case HPS_EX_EXP: top = exp(a); break;
        case HPS_EX_LOG: top = log(a); break;
        case HPS_EX_LOG10: top = log10(a); break;
        case HPS_EX_SIN: top = sin(a); break;
        case HPS_EX_COS: top = cos(a); break;
        case HPS_EX_TAN: top = tan(a); break;
        case HPS_EX_ASIN: top = asin(a); break;
        case HPS_EX_ACOS: top = acos(a); break;
        case HPS_EX_ATAN: top = atan(a); break;
        case HPS_EX_ATAN2: top = atan2(a, b); break;
        case HPS_EX_SINH: top = sinh(a); break;
        case HPS_EX_COSH: top = cosh(a); break;
        case HPS_EX_TANH: top = tanh(a); break;
        case HPS_EX_ABS: top = fabs(a); break;
        case HPS_EX_FLOOR: top = floor(a); break;
        case HPS_EX_CEIL: top = ceil(a); break;
        case HPS_EX_FMOD: top = fmod(a, b); break;
        case HPS_EX_MIN: top = a < b ? a : b; break;
        case HPS_EX_MAX: top = a > b ? a : b; break;
        case HPS_EX_HEAVISIDE: top = a < 0.0 ? 0.0 : (a == 0.0 ? b : 1.0); break;
        case HPS_EX_ERF: top = erf(a); break;
        default: break;      // (unreachable behind expr_validate)
        }
    }
    return top;
}

} // namespace hps
#endif
