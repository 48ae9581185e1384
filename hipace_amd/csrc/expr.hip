// expr.hip -- the C entry points of the expression programs (include/hpslice.h): the check, the host evaluation,
// the stand-alone device operator, and ExprImage: the packing of several programs into one image and its upload.
#include "engine.h"

namespace hps {

// one lane per element, grid-stride; dynamic LDS: (depth - 1) levels of blockDim.x doubles
__global__ __launch_bounds__(256)
void k_expr_eval (const hps_expr_ins* __restrict__ ins, int n_ins, const double* __restrict__ consts,
                  const double* const* __restrict__ vars, double* __restrict__ out, long n)
{
    extern __shared__ double s_expr_stack[];
    ExprLdsStack st{s_expr_stack + threadIdx.x, (int)blockDim.x};
    for (long i = (long)blockIdx.x*blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x*blockDim.x) {
        const ExprArrayVars v{vars, i};
        out[i] = expr_run(ins, n_ins, consts, v, st);
    }
}

int expr_check_named (const char* fn, const char* what, const hps_expr* p, int n_vars, int* depth)
{
    const char* why = ""; int at = -1;
    if (int e = expr_validate(p, n_vars, depth, &why, &at)) {
        set_error(std::string(fn) + ": " + what + why + (at >= 0 ? " (instruction " + std::to_string(at) + ")" : std::string()));
        return e;
    }
    return HPS_OK;
}

bool expr_is_zero (const hps_expr& p)
{
    return p.n_ins == 0 || (p.n_ins == 1 && p.ins && p.ins[0].op == HPS_EX_CONST && p.consts && p.ins[0].arg >= 0 &&
                            p.ins[0].arg < p.n_const && p.consts[p.ins[0].arg] == 0.0);
}

// its constants behind the pool's, its instructions (constant indices rebased) behind the stream's
int ExprImage::add (const hps_expr& p)
{
    const int off = (int)h_ins.size(), base = (int)h_consts.size();
    h_consts.insert(h_consts.end(), p.consts, p.consts + p.n_const);
    for (int i = 0; i < p.n_ins; ++i) {
        hps_expr_ins q = p.ins[i];
        if (q.op == HPS_EX_CONST) q.arg += base;
        h_ins.push_back(q);
    }
    return off;
}

// (neither device array is ever empty: a program without constants still gets a pool to point at)
int ExprImage::upload ()
{
    if (int e = d_ins.alloc(std::max<size_t>(h_ins.size(), 1))) return e;
    if (int e = d_consts.alloc(std::max<size_t>(h_consts.size(), 1))) return e;
    if (!h_ins.empty()) HPS_HIP_CHECK(hipMemcpy(d_ins.get(), h_ins.data(), h_ins.size()*sizeof(hps_expr_ins), hipMemcpyHostToDevice));
    if (!h_consts.empty()) HPS_HIP_CHECK(hipMemcpy(d_consts.get(), h_consts.data(), h_consts.size()*sizeof(double), hipMemcpyHostToDevice));
    return HPS_OK;
}

} // namespace hps

using namespace hps;

extern "C" int hps_expr_check (const hps_expr* prog, int n_vars, int* depth_host)
{
    return expr_check_named("hps_expr_check", "", prog, n_vars, depth_host);
}

extern "C" int hps_expr_eval_host (const hps_expr* prog, int n_vars, long n, const double* const* vars_host, double* out_host)
{
    if (int e = expr_check_named("hps_expr_eval_host", "", prog, n_vars, nullptr)) return e;
    if (n <= 0) return HPS_OK;
    HPS_REQUIRE(out_host && (n_vars == 0 || vars_host), "hps_expr_eval_host: null argument");
    for (int k = 0; k < n_vars; ++k) HPS_REQUIRE(vars_host[k], "hps_expr_eval_host: null variable array");
    ExprHostStack st;
    for (long i = 0; i < n; ++i) {
        const ExprArrayVars v{vars_host, i};
        out_host[i] = expr_run(prog->ins, prog->n_ins, prog->consts, v, st);
    }
    return HPS_OK;
}

extern "C" int hps_expr_eval (const hps_expr* prog, int n_vars, long n, const double* const* vars_dev, double* out_dev, hps_stream stream)
{
    int depth = 0;
    if (int e = expr_check_named("hps_expr_eval", "", prog, n_vars, &depth)) return e;
    if (n <= 0) return HPS_OK;
    HPS_REQUIRE(out_dev && (n_vars == 0 || vars_dev), "hps_expr_eval: null argument");
    const double* ptrs[HPS_EXPR_MAX_VARS] = {};
    for (int k = 0; k < n_vars; ++k) { HPS_REQUIRE(vars_dev[k], "hps_expr_eval: null variable array"); ptrs[k] = vars_dev[k]; }
    hipStream_t st = (hipStream_t)stream;
    const size_t ins_bytes = (size_t)prog->n_ins*sizeof(hps_expr_ins), const_bytes = (size_t)std::max(prog->n_const, 1)*sizeof(double);
    // the image: constants | instructions | the table of variable pointers (read with the wave-uniform variable index)
    char* image = nullptr;
    HPS_HIP_CHECK(hipMalloc(&image, const_bytes + ins_bytes + sizeof(ptrs)));
    hipError_t err = hipSuccess;
    if (prog->n_const > 0) err = hipMemcpy(image, prog->consts, (size_t)prog->n_const*sizeof(double), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(image + const_bytes, prog->ins, ins_bytes, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(image + const_bytes + ins_bytes, ptrs, sizeof(ptrs), hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        const unsigned blocks = (unsigned)std::min<long>(ceil_div(n, 256), 2048);
        const size_t lds = expr_lds_bytes(depth, 256);
        hipLaunchKernelGGL(k_expr_eval, dim3(blocks), dim3(256), lds, st, (const hps_expr_ins*)(image + const_bytes), prog->n_ins,
                           (const double*)image, (const double* const*)(image + const_bytes + ins_bytes), out_dev, n);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    (void)hipFree(image);
    HPS_HIP_CHECK(err);
    return HPS_OK;
}
