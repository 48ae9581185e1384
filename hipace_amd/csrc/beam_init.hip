// beam_init.hip -- the beams the device generates: fixed_ppc, fixed_weight (8o) and fixed_weight_pdf (8p).
//
// Every setter checks all its arguments, fills the argument struct of its kernels, and then goes through the same three steps:
//     begin_device_beam     the stream drained, the old beam released, beam_off and n_left_out zeroed
//     (the generator)       its programs in one ExprImage, its scratch in DevBufs -> the slices' blocks [7][count_p], beam_off
//     finish_device_beam    k_beam_extent and the box of the particles, install_beam_device (the blocks become the engine's)
// A generator that fails leaves the engine without a beam (drop_device_beam).  Every random draw is a function of (seed, tag, the
// point's or the draw's index, component), never of a lane or of the packed index: a generator computes a point twice -- to count
// or to sort, then to fill -- from the same numbers, and the beam does not depend on the launch.  No atomics.  A program's stack
// is the lane's column of the workgroup's dynamic LDS ([level][lane], expr.h).
//
// fixed_ppc (InitBeamFixedPPC3D / InitBeamFixedPPCSlice, particles/beam/BeamParticleContainerInit.cpp:119-346;
// get_position_unit_cell, particles/particles_utils/ParticleUtil.H:30-64): a lattice point is (cell i, j, k; i_part < ppc_x ppc_y
// ppc_z), the order Engine::init_beam's and the reference's exclusive scan: slices head first (k descending), inside a slice j,
// then i, then i_part.  One workgroup owns one row (k, j) of the window that zmin, zmax and the radius leave, and walks the row's
// points (i, i_part) in that order, 256 at a time:
//     k_beam_fixed_ppc<false>   counts the row's particles                    -> count[row j][slice k]
//     k_beam_row_offsets        running sums along j, one lane per slice      -> the row's first index in its slice, slice totals
//     (host)                    running sum of the nz slice totals            -> beam_off[nz + 1]
//     k_beam_fixed_ppc<true>    the same walk; a ballot ranks the particles of a chunk, the row's running index carries over
//                               the chunks, and every particle goes straight into the engine's block of its slice
//
// fixed_weight and fixed_weight_pdf (InitBeamFixedWeight3D / ..Slice, :348-475; InitBeamFixedWeightPDF3D / ..Slice, :477-695):
// nothing but a key and the index i is ever stored per draw, and the two beams share one stage (fw_generate):
//     k_fw_keys | k_fwp_keys   one lane per draw: z, x, y, validity -> key = slice from the head | nz (invalid) | nz + 1 (outside
//                              the box), i
//     (sort.hip)               stable radix sort of (key, i): slices head first, ascending i inside a slice -- the reference's box sort
//     k_fw_starts              first sorted position of every key -> the slices' counts and the two left-out counts
//     k_fw_fill | k_fwp_fill   one lane per kept position o: i = perm[o], the draws of i again, the means at z, the particle (or its
//                              four mirror copies at 4o + q) straight into the block of its slice
// The z draw is a stage of its own (fw_draw_z, fwp_draw_z) behind which everything else only reads z.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace hps {

constexpr int BI_THREADS = 256;
constexpr unsigned long long BI_TAG_POSITION = 0, BI_TAG_MOMENTUM = 1;      // second link of the draws' key

struct BeamInit {
    int nx, ny, nz, ppc[3], nppc;
    int i_lo, ni, j_lo, nj, k_lo, nk;             // the window of cells that can hold a particle
    double lo[3], h[3];
    double x_mean, y_mean, zmin, zmax, radius_sq, min_density, scale_fac, c;
    double u_mean[3], u_std[3];
    int rnd[3];                                   // random_ppc
    unsigned long long key_pos, key_mom;          // hash(seed, tag)
    const hps_expr_ins* ins; int n_ins; const double* consts;
};

struct BeamPoint { double x, y, z, density; bool keep; unsigned long long slot; };

// the three momentum deviates of particle i (a lattice slot, a draw) of every generated beam -- the pair n[0], n[1] and n[2] each
// only if wanted (a Box-Muller pair nobody reads is not drawn); u_mean + u_std n is the caller's
__device__ __forceinline__ void beam_deviates (unsigned long long key_mom, unsigned long long i, bool want_xy, bool want_z, double n[3])
{
    const unsigned long long zk = coll_hash(key_mom, i);
    n[0] = n[1] = n[2] = 0.0;
    if (want_xy) normal_pair(zk, 0u, n[0], n[1]);
    if (want_z) { double unused; normal_pair(zk, 2u, n[2], unused); }
}

// point q = (i - i_lo) nppc + i_part of row (k, j): position, selection and density.  Every operation rounds once (no
// contraction), in the order of Engine::init_beam, so that numpy reproduces the positions bit for bit.
__device__ __forceinline__ BeamPoint beam_point (const BeamInit& a, int k, int j, int q, ExprLdsStack& st)
{
#pragma clang fp contract(off)
    const int ci = q/a.nppc, ip = q - ci*a.nppc, i = a.i_lo + ci;
    const int nyz = a.ppc[1]*a.ppc[2];
    const int ixp = ip/nyz, iyp = (ip % nyz) % a.ppc[1], izp = (ip % nyz)/a.ppc[1];      // get_position_unit_cell
    BeamPoint p;
    p.slot = (((unsigned long long)k*a.ny + j)*a.nx + i)*a.nppc + ip;
    double r[3] = {(0.5 + ixp)/a.ppc[0], (0.5 + iyp)/a.ppc[1], (0.5 + izp)/a.ppc[2]};
    const bool random = (a.rnd[0] | a.rnd[1] | a.rnd[2]) != 0;
    if (random) {
        const unsigned long long zk = coll_hash(a.key_pos, p.slot);
#pragma unroll
        for (int d = 0; d < 3; ++d) if (a.rnd[d]) r[d] = coll_unit(coll_hash(zk, (unsigned long long)d));
    }
    p.x = a.lo[0] + (i + r[0])*a.h[0];
    p.y = a.lo[1] + (j + r[1])*a.h[1];
    p.z = a.lo[2] + (k + r[2])*a.h[2];
    // evenly spaced: the point itself is tested; randomly placed: the lower corner of its cell (:166-183)
    const double tx = random ? a.lo[0] + i*a.h[0] : p.x, ty = random ? a.lo[1] + j*a.h[1] : p.y, tz = random ? a.lo[2] + k*a.h[2] : p.z;
    const double rx = tx - a.x_mean, ry = ty - a.y_mean;
    const bool out = tz >= a.zmax || tz < a.zmin || (rx*rx + ry*ry) > a.radius_sq;
    const ExprXyz v{p.x, p.y, p.z};
    p.density = expr_run(a.ins, a.n_ins, a.consts, v, st);
    p.keep = !out && !(p.density <= a.min_density);
    return p;
}

// FILL = false: count[jj*nk + kk] = particles of row (k_lo + kk, j_lo + jj).
// FILL = true: the particles, into block p = nz - 1 - k of `blocks` ([7][count_p] at 7 off[p]) from index first[jj*nk + kk] on.
template <bool FILL>
__global__ __launch_bounds__(BI_THREADS)
void k_beam_fixed_ppc (BeamInit a, int* __restrict__ count, const long* __restrict__ first, const long* __restrict__ off,
                       double* __restrict__ blocks)
{
    extern __shared__ double s_beam_stack[];
    __shared__ int s_wave[BI_THREADS/64];
    const int jj = blockIdx.x, kk = blockIdx.y, j = a.j_lo + jj, k = a.k_lo + kk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ExprLdsStack st{s_beam_stack + threadIdx.x, BI_THREADS};
    const int nitems = a.ni*a.nppc;
    long run = 0, cnt_p = 0;
    double* blk = nullptr;
    if constexpr (FILL) {
        const int p = a.nz - 1 - k;
        cnt_p = off[p + 1] - off[p];
        blk = blocks + 7*off[p];
        run = first[(long)jj*a.nk + kk];
    }
    for (int base = 0; base < nitems; base += BI_THREADS) {
        const int q = base + (int)threadIdx.x;
        const bool valid = q < nitems;
        const BeamPoint pt = beam_point(a, k, j, valid ? q : nitems - 1, st);      // (every lane runs the program: uniform opcodes)
        const bool keep = valid && pt.keep;
        const unsigned long long mask = __ballot(keep);
        if constexpr (!FILL) {
            run += __popcll(mask);                // per wave
        } else {
            if (lane == 0) s_wave[wave] = __popcll(mask);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < BI_THREADS/64; ++w) { const int n = s_wave[w]; before += w < wave ? n : 0; total += n; }
            __syncthreads();
            if (keep) {
                const long o = run + before + __popcll(mask & ((1ULL << lane) - 1ULL));
                double u[3] = {a.u_mean[0], a.u_mean[1], a.u_mean[2]};
                if (a.u_std[0] != 0.0 || a.u_std[1] != 0.0 || a.u_std[2] != 0.0) {
                    double n[3];
                    beam_deviates(a.key_mom, pt.slot, a.u_std[0] != 0.0 || a.u_std[1] != 0.0, a.u_std[2] != 0.0, n);
#pragma unroll
                    for (int q = 0; q < 3; ++q) if (a.u_std[q] != 0.0) u[q] += a.u_std[q]*n[q];
                }
                blk[o] = pt.x; blk[cnt_p + o] = pt.y; blk[2*cnt_p + o] = pt.z;
                blk[3*cnt_p + o] = u[0]*a.c; blk[4*cnt_p + o] = u[1]*a.c; blk[5*cnt_p + o] = u[2]*a.c;
                blk[6*cnt_p + o] = fabs(pt.density*a.scale_fac);
            }
            run += total;
        }
    }
    if constexpr (!FILL) {
        if (lane == 0) s_wave[wave] = (int)run;
        __syncthreads();
        if (threadIdx.x == 0) {
            int n = 0;
#pragma unroll
            for (int w = 0; w < BI_THREADS/64; ++w) n += s_wave[w];
            count[(long)jj*a.nk + kk] = n;
        }
    }
}

// one lane per slice of the window: the running sum of its rows' counts (consecutive lanes read consecutive words)
__global__ __launch_bounds__(BI_THREADS)
void k_beam_row_offsets (const int* __restrict__ count, long* __restrict__ first, long* __restrict__ total, int nj, int nk)
{
    const int kk = blockIdx.x*blockDim.x + threadIdx.x;
    if (kk >= nk) return;
    long run = 0;
    for (int jj = 0; jj < nj; ++jj) {
        first[(long)jj*nk + kk] = run;
        run += count[(long)jj*nk + kk];
    }
    total[kk] = run;
}

// min and max of x and y of slice p's block: mm[p] = {xlo, xhi, ylo, yhi} (an empty block: +inf, -inf)
__global__ __launch_bounds__(BI_THREADS)
void k_beam_extent (const double* __restrict__ blocks, const long* __restrict__ off, double* __restrict__ mm)
{
    __shared__ double s[4][BI_THREADS];
    const int p = blockIdx.x;
    const long cnt = off[p + 1] - off[p];
    const double* x = blocks + 7*off[p];
    const double* y = x + cnt;
    const double inf = __longlong_as_double(0x7FF0000000000000LL);
    double v[4] = {inf, -inf, inf, -inf};
    for (long i = threadIdx.x; i < cnt; i += BI_THREADS) {
        v[0] = fmin(v[0], x[i]); v[1] = fmax(v[1], x[i]); v[2] = fmin(v[2], y[i]); v[3] = fmax(v[3], y[i]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q][threadIdx.x] = v[q];
    __syncthreads();
    for (int n = BI_THREADS/2; n > 0; n >>= 1) {
        if ((int)threadIdx.x < n) {
            s[0][threadIdx.x] = fmin(s[0][threadIdx.x], s[0][threadIdx.x + n]); s[1][threadIdx.x] = fmax(s[1][threadIdx.x], s[1][threadIdx.x + n]);
            s[2][threadIdx.x] = fmin(s[2][threadIdx.x], s[2][threadIdx.x + n]); s[3][threadIdx.x] = fmax(s[3][threadIdx.x], s[3][threadIdx.x + n]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) mm[4*p + threadIdx.x] = s[threadIdx.x][0];
}

// the moving beam's global SoA (row k at soa + k nb, particles head slice first) from the slice-major blocks
__global__ __launch_bounds__(BI_THREADS)
void k_beam_blocks_to_soa (const double* __restrict__ blocks, const long* __restrict__ off, double* __restrict__ soa, long nb)
{
    const int p = blockIdx.x, k = blockIdx.y;
    const long first = off[p], cnt = off[p + 1] - first;
    const double* src = blocks + 7*first + k*cnt;
    double* dst = soa + k*nb + first;
    for (long i = threadIdx.x; i < cnt; i += BI_THREADS) dst[i] = src[i];
}

// beam_off[nz + 1] for the kernels above
static int beam_off_to_device (Engine& E, DevBuf<long>& off)
{
    const size_t n = (size_t)E.d.nz + 1;
    if (int e = off.alloc(n)) return e;
    HPS_HIP_CHECK(hipMemcpyAsync(off.get(), E.beam_off.data(), n*sizeof(long), hipMemcpyHostToDevice, E.st));
    return HPS_OK;
}

int beam_blocks_to_soa (Engine& E, const double* blocks, double* soa, long nb)
{
    DevBuf<long> off;
    if (int e = beam_off_to_device(E, off)) return e;
    hipLaunchKernelGGL(k_beam_blocks_to_soa, dim3(E.d.nz, 7), dim3(BI_THREADS), 0, E.st, blocks, off.get(), soa, nb);
    HPS_HIP_CHECK(hipGetLastError());
    HPS_HIP_CHECK(hipStreamSynchronize(E.st));
    return HPS_OK;
}

// box = {xlo, xhi, ylo, yhi} of the particles of `blocks` (beam_off filled in, at least one particle)
static int beam_extent (Engine& E, const double* blocks, double box[4])
{
    const int nz = E.d.nz;
    DevBuf<long> off; DevBuf<double> d_mm;
    if (int e = beam_off_to_device(E, off)) return e;
    if (int e = d_mm.alloc((size_t)4*nz)) return e;
    hipLaunchKernelGGL(k_beam_extent, dim3(nz), dim3(BI_THREADS), 0, E.st, blocks, off.get(), d_mm.get());
    HPS_HIP_CHECK(hipGetLastError());
    std::vector<double> mm((size_t)4*nz);
    HPS_HIP_CHECK(hipMemcpyAsync(mm.data(), d_mm.get(), mm.size()*sizeof(double), hipMemcpyDeviceToHost, E.st));
    HPS_HIP_CHECK(hipStreamSynchronize(E.st));
    box[0] = box[2] = std::numeric_limits<double>::infinity(); box[1] = box[3] = -std::numeric_limits<double>::infinity();
    for (int p = 0; p < nz; ++p) {
        box[0] = std::min(box[0], mm[(size_t)4*p]);     box[1] = std::max(box[1], mm[(size_t)4*p + 1]);
        box[2] = std::min(box[2], mm[(size_t)4*p + 2]); box[3] = std::max(box[3], mm[(size_t)4*p + 3]);
    }
    return HPS_OK;
}

int Engine::begin_device_beam (long* n_left_out)
{
    HPS_HIP_CHECK(hipStreamSynchronize(st));
    release_beam();
    host_beam = true;
    beam_off.assign(d.nz + 1, 0);
    if (n_left_out) n_left_out[0] = n_left_out[1] = 0;
    return HPS_OK;
}

int Engine::drop_device_beam (int e, long* n_left_out)
{
    const double box[4] = {0.0, 0.0, 0.0, 0.0};
    beam_off.assign(d.nz + 1, 0);
    if (n_left_out) n_left_out[0] = n_left_out[1] = 0;
    (void)install_beam_device(nullptr, 0, box);
    return e;
}

int Engine::finish_device_beam (DevBuf<double>& blocks, long n, long* n_left_out)
{
    double box[4] = {0.0, 0.0, 0.0, 0.0};
    if (int e = n > 0 ? beam_extent(*this, blocks.get(), box) : HPS_OK) return drop_device_beam(e, n_left_out);
    return install_beam_device(blocks.release(), n, box);
}

// first and last cell index (clamped to 0 .. n - 1; an empty range has first > last) a coordinate range [a, b] can touch,
// one cell of margin for the rounding of the positions; NaN or infinite ends open the range
static void cell_window (double a, double b, double lo, double h, int n, int* first, int* count)
{
    const double fa = std::floor((a - lo)/h) - 1.0, fb = std::floor((b - lo)/h) + 1.0;
    const int ia = fa > 0.0 ? (int)std::min<double>(fa, n) : 0;
    const int ib = fb < n - 1 ? (int)std::max<double>(fb, -1.0) : n - 1;
    *first = ia; *count = std::max(ib - ia + 1, 0);
}

// the two walks over the rows of a's window: beam_off, and the n > 0 particles in `blocks`
static int fixed_ppc_generate (Engine& E, BeamInit a, const hps_expr& density, size_t lds, DevBuf<double>& blocks, long& n)
{
    const int nz = E.d.nz;
    ExprImage image;
    image.add(density);
    if (int e = image.upload()) return e;
    a.ins = image.ins(); a.consts = image.consts();
    const size_t rows = (size_t)a.nj*a.nk;
    DevBuf<int> count; DevBuf<long> first, total, off;
    if (int e = count.alloc(rows)) return e;
    if (int e = first.alloc(rows)) return e;
    if (int e = total.alloc((size_t)a.nk)) return e;
    const dim3 grid(a.nj, a.nk), block(BI_THREADS);
    hipLaunchKernelGGL(k_beam_fixed_ppc<false>, grid, block, lds, E.st, a, count.get(), nullptr, nullptr, nullptr);
    HPS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_beam_row_offsets, dim3(ceil_div(a.nk, BI_THREADS)), block, 0, E.st, count.get(), first.get(), total.get(), a.nj, a.nk);
    HPS_HIP_CHECK(hipGetLastError());
    std::vector<long> h_total((size_t)a.nk);
    HPS_HIP_CHECK(hipMemcpyAsync(h_total.data(), total.get(), h_total.size()*sizeof(long), hipMemcpyDeviceToHost, E.st));
    HPS_HIP_CHECK(hipStreamSynchronize(E.st));
    for (int p = 0; p < nz; ++p) {              // head slice first
        const int kk = nz - 1 - p - a.k_lo;
        E.beam_off[p + 1] = E.beam_off[p] + ((kk >= 0 && kk < a.nk) ? h_total[(size_t)kk] : 0);
    }
    n = E.beam_off[nz];
    if (n == 0) return HPS_OK;
    if (int e = beam_off_to_device(E, off)) return e;
    if (int e = blocks.alloc((size_t)7*n)) return e;
    hipLaunchKernelGGL(k_beam_fixed_ppc<true>, grid, block, lds, E.st, a, nullptr, first.get(), off.get(), blocks.get());
    HPS_HIP_CHECK(hipGetLastError());
    HPS_HIP_CHECK(hipStreamSynchronize(E.st));      // (the image and the scratch go out of scope)
    return HPS_OK;
}

// hps_engine_set_beam_fixed_ppc: everything is checked before anything of the engine changes
int Engine::set_beam_fixed_ppc (const hps_expr* density, double min_density, const double* u_std, const int* random_ppc, unsigned long long seed)
{
    static const char* const fn = "hps_engine_set_beam_fixed_ppc";
    HPS_REQUIRE(density, std::string(fn) + ": null program");
    HPS_REQUIRE(steps_begun == 0 && step_index < 0, std::string(fn) + ": call before the first hps_engine_begin_step");
    HPS_REQUIRE(d.beam_ppc[0] >= 1 && d.beam_ppc[1] >= 1 && d.beam_ppc[2] >= 1, std::string(fn) + ": every entry of beam_ppc must be at least 1");
    HPS_REQUIRE(!std::isnan(min_density) && min_density != std::numeric_limits<double>::infinity(), std::string(fn) + ": min_density must be a number below +infinity");
    for (int q = 0; u_std && q < 3; ++q)
        HPS_REQUIRE(std::isfinite(u_std[q]) && u_std[q] >= 0.0, std::string(fn) + ": u_std must be finite and must not be negative");
    int depth = 0;
    if (int e = expr_check_named(fn, "density: ", density, 3, &depth)) return e;
    const long nppc = (long)d.beam_ppc[0]*d.beam_ppc[1]*d.beam_ppc[2];
    HPS_REQUIRE(nppc*d.nx < (1L << 30), std::string(fn) + ": beam_ppc is too large (more than 2^30 lattice points in a row of cells)");

    BeamInit a{};
    a.nx = d.nx; a.ny = d.ny; a.nz = d.nz; a.nppc = (int)nppc;
    for (int q = 0; q < 3; ++q) {
        a.ppc[q] = d.beam_ppc[q]; a.lo[q] = d.lo[q];
        a.u_mean[q] = d.beam_umean[q]; a.u_std[q] = u_std ? u_std[q] : 0.0; a.rnd[q] = random_ppc ? (random_ppc[q] != 0) : 0;
    }
    a.h[0] = gm.dx; a.h[1] = gm.dy; a.h[2] = gm.dz;
    a.x_mean = d.beam_pos_mean[0]; a.y_mean = d.beam_pos_mean[1]; a.zmin = d.beam_zmin; a.zmax = d.beam_zmax;
    a.radius_sq = d.beam_radius*d.beam_radius; a.min_density = min_density; a.c = gm.c;
    a.scale_fac = d.si_units ? gm.dx*gm.dy*gm.dz/(int)nppc : 1.0/(int)nppc;      // BeamParticleContainerInit.cpp:215-216, as Engine::init_beam
    a.key_pos = coll_hash(seed, BI_TAG_POSITION); a.key_mom = coll_hash(seed, BI_TAG_MOMENTUM);
    a.n_ins = density->n_ins;
    const double R = std::fabs(d.beam_radius);
    cell_window(a.x_mean - R, a.x_mean + R, d.lo[0], gm.dx, d.nx, &a.i_lo, &a.ni);
    cell_window(a.y_mean - R, a.y_mean + R, d.lo[1], gm.dy, d.ny, &a.j_lo, &a.nj);
    cell_window(a.zmin, a.zmax, d.lo[2], gm.dz, d.nz, &a.k_lo, &a.nk);
    const bool window = a.ni > 0 && a.nj > 0 && a.nk > 0;
    HPS_REQUIRE(a.nk <= 65535, std::string(fn) + ": more than 65535 slices");

    if (int e = begin_device_beam()) return e;
    DevBuf<double> blocks; long n = 0;
    if (window)
        if (int e = fixed_ppc_generate(*this, a, *density, expr_lds_bytes(depth, BI_THREADS), blocks, n)) return drop_device_beam(e, nullptr);
    return finish_device_beam(blocks, n);
}

// ---- the fixed_weight beam ----
constexpr unsigned long long BI_TAG_FW_Z = 2, BI_TAG_FW_XY = 3;      // beside BI_TAG_POSITION / BI_TAG_MOMENTUM

struct BeamFixedWeight {
    long nd; int can, sym, nz;
    double lo_z, inv_dz, pos_mean_z, z_mean, std[3], u_mean[3], u_std[3], zmin, zmax, radius_sq, z_foc, duz, c, weight;
    unsigned long long key_z, key_xy, key_mom;        // hash(seed, tag)
    const hps_expr_ins *ins_x, *ins_y; int n_ins_x, n_ins_y; const double *consts_x, *consts_y;
};

struct ExprZ {      // the one variable of position_mean[0], position_mean[1]
    double z;
    __device__ __forceinline__ double get (int) const { return z; }
};

struct FwDraw { double z, x, y; bool valid; };

// stage 1: z of draw i
__device__ __forceinline__ double fw_draw_z (const BeamFixedWeight& a, unsigned long long i)
{
#pragma clang fp contract(off)
    const unsigned long long zk = coll_hash(a.key_z, i);
    if (a.can) return coll_unit(coll_hash(zk, 0ULL))*(a.zmax - a.zmin) + a.zmin;
    double n, unused;
    normal_pair(zk, 0u, n, unused);
    return a.pos_mean_z + a.std[2]*n;
}

// z, the transverse offsets about the mean and the validity of draw i (:433-443); every operation rounds once
__device__ __forceinline__ FwDraw fw_draw (const BeamFixedWeight& a, unsigned long long i)
{
#pragma clang fp contract(off)
    FwDraw d;
    d.z = fw_draw_z(a, i);
    double n0, n1;
    normal_pair(coll_hash(a.key_xy, i), 0u, n0, n1);
    d.x = a.std[0]*n0; d.y = a.std[1]*n1;
    d.valid = !(d.z < a.zmin || d.z > a.zmax || d.x*d.x + d.y*d.y > a.radius_sq);
    return d;
}

// Engine::set_beam_particles' rule: slice from the head, -1 outside the box (Args: BeamFixedWeight, BeamFwPdf)
template <class Args>
__device__ __forceinline__ int fw_slice (const Args& a, double z)
{
#pragma clang fp contract(off)
    const double t = (z - a.lo_z)*a.inv_dz;
    const int q = (t > -1.0e9 && t < 1.0e9) ? static_cast<int>(t) : -1;
    return (q < 0 || q >= a.nz) ? -1 : a.nz - 1 - q;
}

// the sort key of a draw: its slice from the head | nz (invalid) | nz + 1 (valid, outside the box)
template <class Args>
__device__ __forceinline__ unsigned int fw_key (const Args& a, bool valid, double z)
{
    const int p = fw_slice(a, z);
    return (unsigned int)(!valid ? a.nz : p < 0 ? a.nz + 1 : p);
}

// the particle at (X + x, Y + y, z) with momentum u, or its m = 4 mirror copies about (X, Y): (+,+), (-,+), (+,-), (-,-)
// (:459-470, :676-690), into rows of cnt slots from blk on
__device__ __forceinline__ void fw_store_copies (double* blk, long cnt, int m, double X, double x, double Y, double y, double z,
                                                 const double u[3], double c, double weight)
{
#pragma clang fp contract(off)
    for (int q = 0; q < m; ++q) {
        const bool nx = (q & 1) != 0, ny = (q & 2) != 0;
        blk[q] = nx ? X - x : X + x; blk[cnt + q] = ny ? Y - y : Y + y; blk[2*cnt + q] = z;
        blk[3*cnt + q] = (nx ? -u[0] : u[0])*c; blk[4*cnt + q] = (ny ? -u[1] : u[1])*c; blk[5*cnt + q] = u[2]*c;
        blk[6*cnt + q] = weight;
    }
}

__global__ __launch_bounds__(BI_THREADS)
void k_fw_keys (BeamFixedWeight a, unsigned int* __restrict__ keys, unsigned int* __restrict__ idx)
{
    const long i = (long)blockIdx.x*BI_THREADS + threadIdx.x;
    if (i >= a.nd) return;
    const FwDraw d = fw_draw(a, (unsigned long long)i);
    keys[i] = fw_key(a, d.valid, d.z);
    idx[i] = (unsigned int)i;
}

// first[k] = first sorted position with key >= k, k = 0 .. nkeys (keys ascending, < nkeys)
__global__ __launch_bounds__(BI_THREADS)
void k_fw_starts (const unsigned int* __restrict__ keys, long n, int nkeys, long* __restrict__ first)
{
    const long p = (long)blockIdx.x*BI_THREADS + threadIdx.x;
    if (p > n) return;
    const int prev = (p == 0) ? -1 : (int)keys[p - 1];
    const int cur = (p == n) ? nkeys : (int)keys[p];
    for (int k = prev + 1; k <= cur; ++k) first[k] = p;
}

// kept position o (sorted order, o < nkept = first[nz]) -> block keys[o] of `blocks`: [7][count_p] at 7 m first[p], m = 4 copies or 1
__global__ __launch_bounds__(BI_THREADS)
void k_fw_fill (BeamFixedWeight a, const unsigned int* __restrict__ keys, const unsigned int* __restrict__ perm,
                const long* __restrict__ first, long nkept, double* __restrict__ blocks)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double s_fw_stack[];
    const long o = (long)blockIdx.x*BI_THREADS + threadIdx.x;
    const bool live = o < nkept;
    const long oo = live ? o : nkept - 1;             // (every lane runs the programs: uniform opcodes)
    const unsigned long long i = perm[oo];
    const int p = (int)keys[oo];
    const FwDraw d = fw_draw(a, i);
    double u[3] = {a.u_mean[0], a.u_mean[1], a.u_mean[2]};
    if (a.u_std[0] != 0.0 || a.u_std[1] != 0.0 || a.u_std[2] != 0.0) {
        double n[3];
        beam_deviates(a.key_mom, i, a.u_std[0] != 0.0 || a.u_std[1] != 0.0, a.u_std[2] != 0.0, n);
#pragma unroll
        for (int q = 0; q < 3; ++q) if (a.u_std[q] != 0.0) u[q] = a.u_mean[q] + a.u_std[q]*n[q];
    }
    u[2] = u[2] + (d.z - a.z_mean)*a.duz*a.u_mean[2];      // GetInitialMomentum.H:47
    double x = d.x, y = d.y;
    if (a.z_foc != 0.0) { x = x - a.z_foc*u[0]/u[2]; y = y - a.z_foc*u[1]/u[2]; }      // (:446-447)
    ExprLdsStack st{s_fw_stack + threadIdx.x, BI_THREADS};
    const ExprZ v{d.z};
    const double X = expr_run(a.ins_x, a.n_ins_x, a.consts_x, v, st);
    const double Y = expr_run(a.ins_y, a.n_ins_y, a.consts_y, v, st);
    if (!live) return;
    const int m = a.sym ? 4 : 1;
    const long f = first[p], cnt = m*(first[p + 1] - f);
    fw_store_copies(blocks + 7*m*f + m*(o - f), cnt, m, X, x, Y, y, d.z, u, a.c, a.weight);
}

// The stage both fixed-weight beams share (Args: BeamFixedWeight, BeamFwPdf, filled in, their programs on the device): the keys of
// the nd draws, the sort, the first position of every key -> beam_off, n_left_out and the n = m nkept particles (m = 4 mirror
// copies or 1 per draw) that `fill` writes into `blocks`
template <class Args>
static int fw_generate (Engine& E, const Args& a, long nd, int m, void (*keys) (Args, unsigned int*, unsigned int*), size_t lds_keys,
                        void (*fill) (Args, const unsigned int*, const unsigned int*, const long*, long, double*), size_t lds_fill,
                        long* n_left_out, DevBuf<double>& blocks, long& n)
{
    const int nz = E.d.nz, nkeys = nz + 2;
    int bits = 1; while ((1L << bits) < (long)nkeys) ++bits;
    DevBuf<unsigned int> pairs; DevBuf<long> d_first;
    if (int e = pairs.alloc((size_t)4*nd)) return e;      // keys, indices; sorted keys, sorted indices
    unsigned int *ka = pairs.get(), *ia = ka + nd, *kb = ia + nd, *ib = kb + nd;
    if (int e = d_first.alloc((size_t)nkeys + 1)) return e;
    const dim3 block(BI_THREADS);
    hipLaunchKernelGGL(keys, dim3(ceil_div(nd, BI_THREADS)), block, lds_keys, E.st, a, ka, ia);
    HPS_HIP_CHECK(hipGetLastError());
    if (int e = sort_pairs_u32(ka, kb, ia, ib, nd, bits, E.st)) return e;
    hipLaunchKernelGGL(k_fw_starts, dim3(ceil_div(nd + 1, BI_THREADS)), block, 0, E.st, kb, nd, nkeys, d_first.get());
    HPS_HIP_CHECK(hipGetLastError());
    std::vector<long> first((size_t)nkeys + 1);
    HPS_HIP_CHECK(hipMemcpyAsync(first.data(), d_first.get(), first.size()*sizeof(long), hipMemcpyDeviceToHost, E.st));
    HPS_HIP_CHECK(hipStreamSynchronize(E.st));
    for (int p = 0; p <= nz; ++p) E.beam_off[p] = m*first[(size_t)p];
    if (n_left_out) { n_left_out[0] = m*(first[(size_t)nz + 1] - first[(size_t)nz]); n_left_out[1] = m*(nd - first[(size_t)nz + 1]); }
    const long nkept = first[(size_t)nz];
    n = m*nkept;
    if (n == 0) return HPS_OK;
    if (int e = blocks.alloc((size_t)7*n)) return e;
    hipLaunchKernelGGL(fill, dim3(ceil_div(nkept, BI_THREADS)), block, lds_fill, E.st, a, kb, ib, d_first.get(), nkept, blocks.get());
    HPS_HIP_CHECK(hipGetLastError());
    HPS_HIP_CHECK(hipStreamSynchronize(E.st));      // (the scratch goes out of scope)
    return HPS_OK;
}

// ... and the beam becomes the engine's
template <class Args, class Keys, class Fill>
static int fixed_weight_beam (Engine& E, const Args& a, long nd, int m, Keys keys, size_t lds_keys, Fill fill, size_t lds_fill, long* n_left_out)
{
    DevBuf<double> blocks; long n = 0;
    if (int e = fw_generate<Args>(E, a, nd, m, keys, lds_keys, fill, lds_fill, n_left_out, blocks, n)) return E.drop_device_beam(e, n_left_out);
    return E.finish_device_beam(blocks, n, n_left_out);
}

// hps_engine_set_beam_fixed_weight: everything is checked before anything of the engine changes
int Engine::set_beam_fixed_weight (const hps_beam_fixed_weight* s, const hps_expr* mean_x, const hps_expr* mean_y, unsigned long long seed,
                                   long* n_left_out)
{
    static const char* const name = "hps_engine_set_beam_fixed_weight";
    const std::string fn = std::string(name) + ": ";
    HPS_REQUIRE(s && mean_x && mean_y, fn + "null argument");
    HPS_REQUIRE(steps_begun == 0 && step_index < 0, fn + "call before the first hps_engine_begin_step");
    HPS_REQUIRE(s->num_particles > 0, fn + "num_particles must be positive");
    HPS_REQUIRE(!s->do_symmetrize || s->num_particles % 4 == 0, fn + "num_particles must be divisible by 4 with do_symmetrize");
    const long nd = s->do_symmetrize ? s->num_particles/4 : s->num_particles;
    HPS_REQUIRE(nd < (1L << 32), fn + "num_particles: 2^32 draws or more");
    HPS_REQUIRE(s->profile == 0 || s->profile == 1, fn + "profile must be 0 (gaussian) or 1 (can)");
    HPS_REQUIRE(std::isfinite(s->pos_mean_z), fn + "pos_mean_z must be finite");
    for (int q = 0; q < 3; ++q) {
        HPS_REQUIRE(std::isfinite(s->pos_std[q]) && s->pos_std[q] > 0.0, fn + "pos_std must be positive and finite");
        HPS_REQUIRE(std::isfinite(s->u_std[q]) && s->u_std[q] >= 0.0, fn + "u_std must be finite and must not be negative");
        HPS_REQUIRE(std::isfinite(s->u_mean[q]), fn + "u_mean must be finite");
    }
    HPS_REQUIRE(!std::isnan(s->zmin) && !std::isnan(s->zmax) && !std::isnan(s->radius), fn + "zmin, zmax and radius must be numbers");
    HPS_REQUIRE(s->profile != 1 || (std::isfinite(s->zmin) && std::isfinite(s->zmax) && s->zmin < s->zmax),
                fn + "the can profile needs finite zmin < zmax");
    HPS_REQUIRE(!s->charge_is_specified || d.si_units, fn + "total_charge is only valid in SI units: give the density (BeamParticleContainer.cpp:169)");
    HPS_REQUIRE(std::isfinite(s->charge_is_specified ? s->total_charge : s->density), fn + (s->charge_is_specified ? "total_charge" : "density") + " must be finite");
    HPS_REQUIRE(std::isfinite(s->z_foc) && std::isfinite(s->duz_per_uz0_dzeta), fn + "z_foc and duz_per_uz0_dzeta must be finite");
    HPS_REQUIRE(s->z_foc == 0.0 || s->u_mean[2] != 0.0, fn + "z_foc needs u_mean[2] != 0");
    HPS_REQUIRE(d.beam_charge != 0.0, fn + "the deck's beam_charge must not be 0");
    HPS_REQUIRE(!(d.beam_do_salame && s->profile == 0 && (std::isinf(s->zmin) || std::isinf(s->zmax))),
                fn + "a beam_do_salame deck needs the can profile, or zmin and zmax with the gaussian profile (BeamParticleContainer.cpp:149)");
    HPS_REQUIRE(!(sel_species > 0 && sel_species < (int)bsp.size() && bsp[(size_t)sel_species].s.do_salame && s->profile == 0 && (std::isinf(s->zmin) || std::isinf(s->zmax))),
                fn + "a do_salame beam species needs the can profile, or zmin and zmax with the gaussian profile (BeamParticleContainer.cpp:149)");
    int depth_x = 0, depth_y = 0;
    if (int e = expr_check_named(name, "position_mean[0]: ", mean_x, 1, &depth_x)) return e;
    if (int e = expr_check_named(name, "position_mean[1]: ", mean_y, 1, &depth_y)) return e;

    BeamFixedWeight a{};
    a.nd = nd; a.can = s->profile == 1; a.sym = s->do_symmetrize != 0; a.nz = d.nz;
    a.lo_z = d.lo[2]; a.inv_dz = 1.0/gm.dz; a.pos_mean_z = s->pos_mean_z;
    a.z_mean = a.can ? 0.5*(s->zmin + s->zmax) : s->pos_mean_z;      // (:419)
    for (int q = 0; q < 3; ++q) { a.std[q] = s->pos_std[q]; a.u_mean[q] = s->u_mean[q]; a.u_std[q] = s->u_std[q]; }
    a.zmin = s->zmin; a.zmax = s->zmax; a.radius_sq = s->radius*s->radius; a.z_foc = s->z_foc; a.duz = s->duz_per_uz0_dzeta; a.c = gm.c;
    {   // BeamParticleContainer.cpp:179-190, BeamParticleContainerInit.cpp:425; tests/beam_fixed_weight_reference.weight follows this chain
        double total_charge = s->total_charge;
        if (!s->charge_is_specified) {
            total_charge = s->density*d.beam_charge;
            for (int q = 0; q < 3; ++q) total_charge *= s->pos_std[q]*std::sqrt(2.0*M_PI);
        }
        if (!d.si_units) total_charge *= (1.0/gm.dx)*(1.0/gm.dy)*(1.0/gm.dz);
        a.weight = std::fabs(total_charge/((double)s->num_particles*d.beam_charge));
    }
    a.key_z = coll_hash(seed, BI_TAG_FW_Z); a.key_xy = coll_hash(seed, BI_TAG_FW_XY); a.key_mom = coll_hash(seed, BI_TAG_MOMENTUM);
    a.n_ins_x = mean_x->n_ins; a.n_ins_y = mean_y->n_ins;

    if (int e = begin_device_beam(n_left_out)) return e;
    ExprImage image;
    const int off_x = image.add(*mean_x), off_y = image.add(*mean_y);
    if (int e = image.upload()) return drop_device_beam(e, n_left_out);
    a.ins_x = image.ins() + off_x; a.ins_y = image.ins() + off_y; a.consts_x = a.consts_y = image.consts();
    return fixed_weight_beam(*this, a, nd, a.sym ? 4 : 1, k_fw_keys, 0, k_fw_fill, expr_lds_bytes(std::max(depth_x, depth_y), BI_THREADS), n_left_out);
}

// ---- the fixed_weight_pdf beam: a table-driven z draw, every mean and width a program over z ----
//     (host)         pe[s] = pdf(edge s), lw, integral, max_density, the u_z moments, cum[] -- once, in the reference's order
//     k_fwp_keys     the draw: s by binary search in cum, z, std_x(z), std_y(z), the rejection loop
//     k_fwp_fill     the draw of i again, all ten programs at z
// cum and pe (at most 2 x 8193 doubles for 2048 slices of 4 sub-slices) are read through L2: every lane's search starts on the same
// few lines, and an image in LDS would cost a workgroup of 256 draws 128 KiB of loads and the CU all but one workgroup.
constexpr unsigned long long BI_TAG_FW_PDF_Z = 4;
constexpr int FWP_MAX_ATTEMPTS = 4096;              // of the (x, y) pair of a total_charge beam inside the radius (:662-666)
constexpr int FWP_MEAN_X = 0, FWP_MEAN_Y = 1, FWP_STD_X = 2, FWP_STD_Y = 3, FWP_U_MEAN = 4, FWP_U_STD = 7, FWP_NPROG = 10;

struct BeamFwPdf {
    long nd; int sym, nz, ns, last, retry;          // last: the last sub-slice with lw > 0; retry: total_charge was given
    double lo_z, inv_dz, zs, radius_sq, z_foc, c, weight;
    unsigned long long key_z, key_xy, key_mom;      // hash(seed, tag)
    const double *cum, *pe;                         // [ns + 1] each
    const hps_expr_ins* ins; const double* consts; int off[FWP_NPROG + 1];      // the ten programs in one image
};

struct FwpDraw { double z, x, y; int s, attempt; bool valid; };

template <class Stack>
__device__ __forceinline__ double fwp_prog (const BeamFwPdf& a, int k, const ExprZ& v, Stack& st)
{
    return expr_run(a.ins + a.off[k], a.off[k + 1] - a.off[k], a.consts, v, st);
}

// stage 1: sub-slice and z of draw i (:631-652); every operation rounds once
__device__ __forceinline__ double fwp_draw_z (const BeamFwPdf& a, unsigned long long i, int& s)
{
#pragma clang fp contract(off)
    const unsigned long long zk = coll_hash(a.key_z, i);
    const double t = coll_unit(coll_hash(zk, 0ULL))*a.cum[a.ns];
    int lo = 0, hi = a.last;                        // the last index with cum[.] <= t, at most `last` (cum[0] = 0 <= t)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.cum[mid] <= t) lo = mid; else hi = mid - 1;
    }
    s = lo;
    const double w = coll_unit(coll_hash(zk, 1ULL));
    const double lo_w = a.pe[lo], hi_w = a.pe[lo + 1];
    const bool taylor = fmin(lo_w, hi_w)*1.1 > fmax(lo_w, hi_w);
    double f;
    if (taylor) {
        const double inv = 1.0/(hi_w + lo_w);
        f = w - w*(w - 1.0)*(hi_w - lo_w)*inv;
    } else {
        const double inv = 1.0/(hi_w - lo_w);
        f = (sqrt(lo_w*lo_w + w*(hi_w*hi_w - lo_w*lo_w)) - lo_w)*inv;
    }
    return (a.lo_z + lo*a.zs) + a.zs*f;
}

// z, the widths at z, the transverse offsets and the validity of draw i (:654-666)
template <class Stack>
__device__ __forceinline__ FwpDraw fwp_draw (const BeamFwPdf& a, unsigned long long i, Stack& st)
{
#pragma clang fp contract(off)
    FwpDraw d;
    d.z = fwp_draw_z(a, i, d.s);
    const ExprZ v{d.z};
    const double sx = fwp_prog(a, FWP_STD_X, v, st), sy = fwp_prog(a, FWP_STD_Y, v, st);
    const unsigned long long xk = coll_hash(a.key_xy, i);
    const int cap = a.retry ? FWP_MAX_ATTEMPTS : 1;
    d.valid = false; d.attempt = 0; d.x = 0.0; d.y = 0.0;
    for (int k = 0; k < cap; ++k) {
        double n0, n1;
        normal_pair(xk, 2u*(unsigned)k, n0, n1);
        d.x = sx*n0; d.y = sy*n1; d.attempt = k;
        if (d.x*d.x + d.y*d.y <= a.radius_sq) { d.valid = true; break; }
    }
    return d;
}

__global__ __launch_bounds__(BI_THREADS)
void k_fwp_keys (BeamFwPdf a, unsigned int* __restrict__ keys, unsigned int* __restrict__ idx)
{
    extern __shared__ __attribute__((aligned(16))) double s_fwp_key_stack[];
    const long i = (long)blockIdx.x*BI_THREADS + threadIdx.x;
    const bool live = i < a.nd;
    ExprLdsStack st{s_fwp_key_stack + threadIdx.x, BI_THREADS};
    const FwpDraw d = fwp_draw(a, (unsigned long long)(live ? i : a.nd - 1), st);      // (every lane runs the programs: uniform opcodes)
    if (!live) return;
    keys[i] = fw_key(a, d.valid, d.z);
    idx[i] = (unsigned int)i;
}

// kept position o (sorted order, o < nkept = first[nz]) -> block keys[o] of `blocks`, as k_fw_fill
__global__ __launch_bounds__(BI_THREADS)
void k_fwp_fill (BeamFwPdf a, const unsigned int* __restrict__ keys, const unsigned int* __restrict__ perm,
                 const long* __restrict__ first, long nkept, double* __restrict__ blocks)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double s_fwp_stack[];
    const long o = (long)blockIdx.x*BI_THREADS + threadIdx.x;
    const bool live = o < nkept;
    const long oo = live ? o : nkept - 1;             // (every lane runs the programs: uniform opcodes)
    const unsigned long long i = perm[oo];
    const int p = (int)keys[oo];
    ExprLdsStack st{s_fwp_stack + threadIdx.x, BI_THREADS};
    const FwpDraw d = fwp_draw(a, i, st);
    const ExprZ v{d.z};
    const double X = fwp_prog(a, FWP_MEAN_X, v, st), Y = fwp_prog(a, FWP_MEAN_Y, v, st);
    double m[3], u[3];
    beam_deviates(a.key_mom, i, true, true, m);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double um = fwp_prog(a, FWP_U_MEAN + q, v, st), us = fwp_prog(a, FWP_U_STD + q, v, st);
        u[q] = um + us*m[q];
    }
    double x = d.x, y = d.y;
    if (a.z_foc != 0.0) { x = x - a.z_foc*u[0]/u[2]; y = y - a.z_foc*u[1]/u[2]; }      // (:673-674)
    if (!live) return;
    const int n = a.sym ? 4 : 1;
    const long f = first[p], cnt = n*(first[p + 1] - f);
    fw_store_copies(blocks + 7*n*f + n*(o - f), cnt, n, X, x, Y, y, d.z, u, a.c, a.weight);
}

// the ten programs and the table cum | pe on the device
static int fwp_upload (ExprImage& image, const std::vector<double>& tab, DevBuf<double>& d_tab)
{
    if (int e = image.upload()) return e;
    if (int e = d_tab.alloc(tab.size())) return e;
    HPS_HIP_CHECK(hipMemcpy(d_tab.get(), tab.data(), tab.size()*sizeof(double), hipMemcpyHostToDevice));
    return HPS_OK;
}

// hps_engine_set_beam_fixed_weight_pdf: everything is checked before anything of the engine changes
int Engine::set_beam_fixed_weight_pdf (const hps_beam_fixed_weight_pdf* s, const hps_expr* pdf, const hps_expr* progs, unsigned long long seed,
                                       long* n_left_out, double* uz_moments)
{
    static const char* const name = "hps_engine_set_beam_fixed_weight_pdf";
    static const char* const prog_name[FWP_NPROG] = {"position_mean[0]: ", "position_mean[1]: ", "position_std[0]: ", "position_std[1]: ",
                                                     "u_mean[0]: ", "u_mean[1]: ", "u_mean[2]: ", "u_std[0]: ", "u_std[1]: ", "u_std[2]: "};
    const std::string fn = std::string(name) + ": ";
    HPS_REQUIRE(s && pdf && progs, fn + "null argument");
    HPS_REQUIRE(steps_begun == 0 && step_index < 0, fn + "call before the first hps_engine_begin_step");
    HPS_REQUIRE(s->num_particles > 0, fn + "num_particles must be positive");
    HPS_REQUIRE(!s->do_symmetrize || s->num_particles % 4 == 0, fn + "num_particles must be divisible by 4 with do_symmetrize");
    const long nd = s->do_symmetrize ? s->num_particles/4 : s->num_particles;
    HPS_REQUIRE(nd < (1L << 32), fn + "num_particles: 2^32 draws or more");
    HPS_REQUIRE(s->pdf_ref_ratio >= 1, fn + "pdf_ref_ratio must be at least 1");
    HPS_REQUIRE((long)d.nz*s->pdf_ref_ratio < (long)std::numeric_limits<int>::max(), fn + "pdf_ref_ratio: nz pdf_ref_ratio overflows an int");
    int depth_pdf = 0, depth[FWP_NPROG] = {};
    if (int e = expr_check_named(name, "pdf: ", pdf, 1, &depth_pdf)) return e;
    for (int k = 0; k < FWP_NPROG; ++k)
        if (int e = expr_check_named(name, prog_name[k], &progs[k], 1, &depth[k])) return e;
    HPS_REQUIRE(!s->charge_is_specified || d.si_units, fn + "total_charge is only valid in SI units: give the density (BeamParticleContainer.cpp:242)");
    HPS_REQUIRE(std::isfinite(s->charge_is_specified ? s->total_charge : s->density), fn + (s->charge_is_specified ? "total_charge" : "density") + " must be finite");
    HPS_REQUIRE(d.beam_charge != 0.0, fn + "the deck's beam_charge must not be 0");
    HPS_REQUIRE(s->radius > 0.0, fn + "radius must be positive");
    HPS_REQUIRE(std::isfinite(s->z_foc), fn + "z_foc must be finite");

    // the host part (:489-542), with the routine of hps_expr_eval_host
    const int ns = d.nz*s->pdf_ref_ratio;
    const double lo_z = d.lo[2], zs = gm.dz/s->pdf_ref_ratio;
    auto value = [] (const hps_expr& p, double z) {
        ExprHostStack hs;
        const double* const vp[1] = {&z};
        const ExprArrayVars v{vp, 0};
        return expr_run(p.ins, p.n_ins, p.consts, v, hs);
    };
    std::vector<double> tab((size_t)2*(ns + 1));      // cum[ns + 1], pe[ns + 1]
    double* const cum = tab.data(); double* const pe = cum + (ns + 1);
    for (int q = 0; q <= ns; ++q) {
        pe[q] = value(*pdf, lo_z + q*zs);
        HPS_REQUIRE(std::isfinite(pe[q]) && pe[q] >= 0.0, fn + "pdf: PDF must be >= 0 everywhere (and finite), at z = " + std::to_string(lo_z + q*zs));
    }
    double integral = 0.0, max_density = 0.0, avg_uz = 0.0, avg_uz_sq = 0.0, weight = 0.0, uz_mean = 0.0, uz_std = 0.0;
    int last = -1;
    {
#pragma clang fp contract(off)
        for (int q = ns - 1; q >= 0; --q) {
            const double zmin = lo_z + q*zs, zmax = lo_z + (q + 1)*zs, zmid = 0.5*(zmin + zmax);
            const double lw = 0.5*(pe[q] + pe[q + 1]);
            if (lw > 0.0) {
                if (last < 0) last = q;
                const double sx = value(progs[FWP_STD_X], zmid), sy = value(progs[FWP_STD_Y], zmid);
                HPS_REQUIRE(std::isfinite(sx) && sx > 0.0 && std::isfinite(sy) && sy > 0.0,
                            fn + "position_std must be positive and finite wherever the pdf is positive, at z = " + std::to_string(zmid));
                if (!s->charge_is_specified) max_density = std::max(max_density, lw/(zs*sx*sy*2.0*M_PI));
            }
            const double um = value(progs[FWP_U_MEAN + 2], zmid), us = value(progs[FWP_U_STD + 2], zmid);
            avg_uz += lw*um;
            avg_uz_sq += lw*(um*um + us*us);
            integral += lw;
        }
        HPS_REQUIRE(integral > 0.0 && std::isfinite(integral), fn + "pdf: the integral over the box must be positive and finite");
        double total_weight = s->charge_is_specified ? s->total_charge/d.beam_charge : s->density*integral/max_density;
        if (!d.si_units) total_weight *= (1.0/gm.dx)*(1.0/gm.dy)*(1.0/gm.dz);
        weight = std::fabs(total_weight/(double)s->num_particles);
        uz_mean = avg_uz/integral;
        uz_std = std::sqrt(std::max(avg_uz_sq/integral - (avg_uz/integral)*(avg_uz/integral), 0.0));      // (a rounding below 0 is 0)
        cum[0] = 0.0;
        for (int q = 0; q < ns; ++q) cum[q + 1] = cum[q] + 0.5*(pe[q] + pe[q + 1]);
    }
    HPS_REQUIRE(std::isfinite(weight), fn + "the weight density integral / (max_density num_particles) is not finite");

    BeamFwPdf a{};
    a.nd = nd; a.sym = s->do_symmetrize != 0; a.nz = d.nz; a.ns = ns; a.last = last; a.retry = s->charge_is_specified != 0;
    a.lo_z = lo_z; a.inv_dz = 1.0/gm.dz; a.zs = zs; a.radius_sq = s->radius*s->radius; a.z_foc = s->z_foc; a.c = gm.c; a.weight = weight;
    a.key_z = coll_hash(seed, BI_TAG_FW_PDF_Z); a.key_xy = coll_hash(seed, BI_TAG_FW_XY); a.key_mom = coll_hash(seed, BI_TAG_MOMENTUM);
    ExprImage image;
    for (int k = 0; k < FWP_NPROG; ++k) a.off[k] = image.add(progs[k]);
    a.off[FWP_NPROG] = image.n_ins();
    const int depth_keys = std::max(depth[FWP_STD_X], depth[FWP_STD_Y]), depth_fill = *std::max_element(depth, depth + FWP_NPROG);

    if (int e = begin_device_beam(n_left_out)) return e;
    if (uz_moments) { uz_moments[0] = uz_mean; uz_moments[1] = uz_std; }
    DevBuf<double> d_tab;
    if (int e = fwp_upload(image, tab, d_tab)) return drop_device_beam(e, n_left_out);
    a.ins = image.ins(); a.consts = image.consts(); a.cum = d_tab.get(); a.pe = d_tab.get() + (ns + 1);
    return fixed_weight_beam(*this, a, nd, a.sym ? 4 : 1, k_fwp_keys, expr_lds_bytes(depth_keys, BI_THREADS), k_fwp_fill,
                             expr_lds_bytes(depth_fill, BI_THREADS), n_left_out);
}

} // namespace hps

extern "C" int hps_engine_set_beam_fixed_weight_pdf (void* h, const hps_beam_fixed_weight_pdf* spec, const hps_expr* pdf, const hps_expr progs[10],
                                                     unsigned long long seed, long n_left_out[2], double uz_moments[2])
{
    HPS_REQUIRE(h, "hps_engine_set_beam_fixed_weight_pdf: null engine");
    hps::Engine* E = static_cast<hps::Engine*>(h);
    return E->fill_selected_species("hps_engine_set_beam_fixed_weight_pdf", [&] { return E->set_beam_fixed_weight_pdf(spec, pdf, progs, seed, n_left_out, uz_moments); });
}

extern "C" int hps_engine_set_beam_fixed_weight (void* h, const hps_beam_fixed_weight* spec, const hps_expr* mean_x_of_z,
                                                 const hps_expr* mean_y_of_z, unsigned long long seed, long n_left_out[2])
{
    HPS_REQUIRE(h, "hps_engine_set_beam_fixed_weight: null engine");
    hps::Engine* E = static_cast<hps::Engine*>(h);
    return E->fill_selected_species("hps_engine_set_beam_fixed_weight", [&] { return E->set_beam_fixed_weight(spec, mean_x_of_z, mean_y_of_z, seed, n_left_out); });
}

extern "C" int hps_engine_set_beam_fixed_ppc (void* h, const hps_expr* density, double min_density, const double u_std[3], const int random_ppc[3],
                                              unsigned long long seed)
{
    HPS_REQUIRE(h, "hps_engine_set_beam_fixed_ppc: null engine");
    hps::Engine* E = static_cast<hps::Engine*>(h);
    return E->fill_selected_species("hps_engine_set_beam_fixed_ppc", [&] { return E->set_beam_fixed_ppc(density, min_density, u_std, random_ppc, seed); });
}
