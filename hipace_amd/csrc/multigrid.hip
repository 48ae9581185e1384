// multigrid.hip -- geometric multigrid for  -a*phi + Lap(phi) = rhs  (2 right-hand sides sharing
// one coefficient a: the explicit Bx/By solve), homogeneous Dirichlet walls, on gfx950.
//
// Numerically a restatement of hpmg::MultiGrid system type 1 (mg_solver/HpMultiGrid.cpp):
// V-cycle with 4 red-black Gauss-Seidel sweeps per level (colour (i+j+s)%2, s = 0..3), residual
// behind the sweeps, cell-centred 4-average / nodal full-weighting restriction, piecewise
// constant / bilinear prolongation, 16 sweeps on the coarsest level, cell-centred wall stencil
// with the 4/3-2 coefficients (HpMultiGrid.cpp:162-182,265-292), stop rule of solve_doit
// (:1307-1427).  Because Bx/By are only converged to tol_rel = 1e-4 from the previous slice's
// field, parity of the slice engine requires this exact per-cell arithmetic.
//
// MI355X mapping (one HBM read + one HBM write of each plane per smoothing step):
//  * k_smooth: one LDS-tiled kernel per level and direction.  A 256-thread workgroup sweeps a
//    64x32-cell tile 4 times in LDS (phi in LDS; rhs, coefficient and 1/diagonal in registers),
//    and fuses what the reference does in separate passes: the prolongation of the coarse
//    correction into the tile load (up-leg), the residual, its max-norm and -- cell-centred --
//    its restriction to the next level (down-leg: the fine residual never touches HBM).
//  * k_lower_v: every level with <= 32x32 unknowns runs inside ONE 1024-thread workgroup with all
//    its arrays in LDS (whole lower V incl. the 16 bottom sweeps), replacing ~4 launches per level.
#include "common.h"
#include <type_traits>
#include "mg_gate.h"
#include "slab_ops.h"

#include <vector>
#include <algorithm>
#include <cmath>
#include <cstring>

namespace hps {

// 2-D multi-component view in level index space: (i,j,n) -> p[(i+oi) + (j+oj)*js + n*ns]
// (the element's byte offset in 32-bit arithmetic from the view's base -- global_load / global_store with the
//  base in SGPRs and one offset VGPR instead of a 64-bit address per access: the level-0 passes spend more instructions on
//  index arithmetic than on fp64; the solver's planes hold at most 2^28 doubles, checked in mg_create)
// Block rows (BR in smooth_tile): a thread's GPAIRS cell pairs sit in GPAIRS consecutive rows of the tile (a 2 x GPAIRS block of cells) instead
// of rows NT/PR apart, and the values it has written last stay in registers: of the four neighbours of a cell it updates, the
// partner in its pair and the cells above / below inside its block come from registers, not from LDS -- 5 instead of 12 LDS reads
// per half-sweep and component for GPAIRS = 3.  (The sweeps of the fused level-0 pass ran at 1900 cycles per half-sweep, which is
// what the LDS pipe carries for two workgroups of 123 KB each.)
// Measured (round 4): the kernels with GPAIRS = 2 (64 x 32 tiles: the initial level-0 pass 24.4 -> 22.0 us, the level-1 passes
// 9.1 -> 8.2) gain; the fused 8-sweep level-0 pass (GPAIRS = 3, 128 registers for two workgroups per CU) does not have the 24
// registers for the values and takes 39.2 instead of 32.2 us: block rows up to two pairs per thread only,
// and for any number of pairs in the tiles that touch no wall (their path has no wall multipliers and masks in registers).
struct FView {
    double* p; long js, ns; int oi, oj;
    __device__ __forceinline__ double& operator() (int i, int j, int n) const {
        const unsigned o = (unsigned)((i + oi) + (j + oj)*(int)js + n*(int)ns)*8u;
        return *reinterpret_cast<double*>(reinterpret_cast<char*>(p) + o);
    }
};

struct LevBox { int lox, loy, hix, hiy;      // index bounds of the level box (walls for nodal)
                int vlx, vly, vhx, vhy; };   // unknowns (valid_domain_box)

enum { SRC_ZERO = 0, SRC_DIRECT = 1, SRC_PROLONG = 2 };

// A value that must be in its register here: keeps the compiler from sinking a load below the gate that follows it.
#define HPS_KEEP(x) asm volatile("" :: "v"(x))

// optional shader-clock stamps of workgroup 0 (set through hps_mg_debug_stamps)
// -- only in the diagnostic build (make stamps: -DHPS_STAMPS): the read of the pointer is one more dependent trip to
// memory at the head of every kernel, ~1 us behind a kernel boundary
#ifdef HPS_STAMPS
__device__ long long* g_mg_dbg = nullptr;
#define MG_STAMP(i) do { if (g_mg_dbg && blockIdx.x == 0 && threadIdx.x == 0) g_mg_dbg[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define MG_STAMP(i) do { } while (0)
#endif

// Smoother tile shapes: TX x TY cells swept by NT threads (TX*TY/2/NT cell pairs per thread).  A
// workgroup streams its tile through one CU (~10 B/clk from memory, one instruction stream per
// SIMD), so the levels with few cells get small tiles -- more workgroups on more CUs -- and the
// fine levels large ones (less rim re-computation: the 4 sweeps need a rim of 3..4 cells).
template <int TX_, int TY_, int NT_>
struct TileShape {
    static constexpr int TX = TX_, TY = TY_, NT = NT_;
    static constexpr int AX = TX + 2, AY = TY + 2;          // LDS array with ring
    static constexpr int PR = TX/2;                          // cell pairs per row
    static constexpr int GPAIRS = TX*TY/2/NT;                // cell pairs per thread
    static_assert(TX*TY/2 % NT == 0 && NT % 64 == 0 && (PR == 16 || PR == 32), "tile shape");
};
using TileBig = TileShape<64, 32, 512>;
using TileMid = TileShape<32, 32, 256>;
// (64 x 64 tiles with 512 or 1024 threads and 64 x 32 were measured for this pass: multigrid 0.293 / 0.282 / 0.290 against
// 0.278 ms per slice; 64 x 96: profiles/r04_mg_level0_tile.txt)
using TileHuge = TileShape<64, 48, 512>;      // the fused 8-sweep pass of level 0 (rim 8: 48 x 32 of 64 x 48 final)
// ... of the node-centred hierarchy (2^K - 1 cells per side): on 64 x 48 tiles that pass spills 37 registers under its cap
// (no fused restriction: the residual planes are stored, the prolongation is bilinear) -- 64 x 32 tiles (two pairs per thread)
// do not: Bx/By solve at 1023^2 413 -> 391 us per slice (profiles/r05_nodal_multigrid.txt); the cell-centred pass keeps 64 x 48
using TileHugeNodal = TileShape<64, 32, 512>;
template <bool CC> struct HugeTileOf { using type = TileHuge; };
template <> struct HugeTileOf<false> { using type = TileHugeNodal; };
using TileSmall = TileShape<32, 16, 256>;
// k_lower_v3's [acf | 1/diag] image of the levels below its top one is at most this long (32^2 .. 2^2 with their rings)
constexpr int COEF_GUEST_MAX_IMG = 2*(34*34 + 18*18 + 10*10 + 6*6 + 4*4);

// diagonal of the operator at (i,j): -(a + 2(fx+fy)) with the wall modification (gs1 :265-292)
template <bool CC>
__device__ __forceinline__ double diag_c0 (int i, int j, const LevBox& b, double acf, double facx, double facy)
{
    double c0 = -(acf + 2.0*(facx + facy));
    if (CC && (i == b.lox || i == b.hix)) c0 -= 2.0*facx;
    if (CC && (j == b.loy || j == b.hiy)) c0 -= 2.0*facy;
    return c0;
}

// Off-diagonal part of the stencil at (i,j); `c` points at the cell, `sy` is the row stride.
// Branch-free: all four neighbours are read unconditionally (the arrays carry a ring / walls), the
// cell-centred wall variants (gs1 :265-292: facx*(4/3)*phi instead of facx*(phi_w+phi_e)) are picked
// with selects, so the result is bit-identical to the branching form while the loads of several
// cells can be in flight together.  INTERIOR = no cell of the tile touches a wall.
template <bool CC, bool INTERIOR = false, class P>
__device__ __forceinline__ double offdiag (P c, int sy, int i, int j, const LevBox& b, double facx, double facy)
{
    const double w = c[-1], e = c[1], s = c[-sy], n = c[sy];
    double lx = facx*(w + e), ly = facy*(s + n);
    if (CC && !INTERIOR) {
        const double fx43 = facx*(4./3.), fy43 = facy*(4./3.);
        lx = (i == b.lox) ? fx43*e : ((i == b.hix) ? fx43*w : lx);
        ly = (j == b.loy) ? fy43*n : ((j == b.hiy) ? fy43*s : ly);
    }
    return lx + ly;
}

// The same with per-cell multipliers, for arrays whose cells outside the unknowns' box hold 0:
// fxm = facx*(4/3) on a cell-centred wall column, facx elsewhere (fym alike), so that
// fxm*(w + e) is facx*(4/3)*e at the low wall (w = 0 and 0 + e == e), facx*(4/3)*w at the high wall
// and facx*(w + e) inside -- the values of gs1 :265-292 without a select or a branch per neighbour.
template <class P>
__device__ __forceinline__ double offdiag_m (P c, int sy, double fxm, double fym)
{
    return fxm*(c[-1] + c[1]) + fym*(c[-sy] + c[sy]);
}
template <bool CC>
__device__ __forceinline__ double wall_mult (int i, int lo, int hi, double fac)
{
    return (CC && (i == lo || i == hi)) ? fac*(4./3.) : fac;
}

// residual rhs - L(phi) at (i,j) (laplacian :162-182, residual1 :184-190), branch-free as above
template <bool INTERIOR = false>
__device__ __forceinline__ double residual_v (double p0, double w, double e, double s, double n, int i, int j, const LevBox& b,
                                              double rhs, double acf, double facx, double facy);

template <bool INTERIOR = false, class P>
__device__ __forceinline__ double residual_at (P c, int sy, int i, int j, const LevBox& b,
                                               double rhs, double acf, double facx, double facy)
{
    return residual_v<INTERIOR>(c[0], c[-1], c[1], c[-sy], c[sy], i, j, b, rhs, acf, facx, facy);
}

template <bool INTERIOR>
__device__ __forceinline__ double residual_v (double p0, double w, double e, double s, double n, int i, int j, const LevBox& b,
                                              double rhs, double acf, double facx, double facy)
{
    double lap = -2.0*(facx + facy)*p0;
    double tx = facx*(w + e), ty = facy*(s + n);
    if (!INTERIOR) {
        tx = (i == b.lox) ? facx*((4./3.)*e - 2.0*p0) : ((i == b.hix) ? facx*((4./3.)*w - 2.0*p0) : tx);
        ty = (j == b.loy) ? facy*((4./3.)*n - 2.0*p0) : ((j == b.hiy) ? facy*((4./3.)*s - 2.0*p0) : ty);
    }
    lap += tx;
    lap += ty;
    return rhs + acf*p0 - lap;
}

// P(coarse) at fine point (i,j): piecewise constant (cell-centred) or bilinear (nodal)
template <bool CC>
__device__ __forceinline__ double prolong_at (const FView& crse, int i, int j, int n)
{
    const int ic = i >> 1, jc = j >> 1;      // indices are >= 0
    if (CC) return crse(ic, jc, n);
    const bool io = (i & 1), jo = (j & 1);
    if (io && jo)  return (crse(ic, jc, n) + crse(ic+1, jc, n) + crse(ic, jc+1, n) + crse(ic+1, jc+1, n))*0.25;
    if (io)        return (crse(ic, jc, n) + crse(ic+1, jc, n))*0.5;
    if (jo)        return (crse(ic, jc, n) + crse(ic, jc+1, n))*0.5;
    return crse(ic, jc, n);
}

// Device-side stopping rule (solve_doit :1352-1398).  norms[0] = initial residual norm, norms[1] =
// rhs norm, norms[2+k] = residual norm after V-cycle k (all zeroed before a solve).  V-cycles are
// enqueued speculatively; every kernel of V-cycle k evaluates the rule itself and returns at once
// if V-cycle k-1 already met the target (an inactive V-cycle leaves its slot at 0, which switches
// off all later ones).  k < 0: unconditional.
constexpr int MG_MAX_VCYCLES = 1024;
// max-norm accumulation: one fire-and-forget atomic per workgroup into one of the slot's words
template <int NT>
__device__ __forceinline__ void block_max_to (unsigned long long* slot, double v, double* s_red)
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = 0.0;
        for (int w = 0; w < NT/64; ++w) m = fmax(m, s_red[w]);
        if (m > 0.0) atomicMax(slot + (blockIdx.x & (MG_NSUB - 1)), (unsigned long long)__double_as_longlong(m));
    }
    __syncthreads();
}

// One Gauss-Seidel cell update with the multipliers of offdiag_m (`we` = west + east; `s`, `n`: south, north).  Its one fused
// multiply-add is spelled out and nothing else in it may be contracted.  Left to the compiler, `fxm*we + fym*(s + n)` came out
// as fma(fxm, we, fym*(s + n)) in the tiles that touch no wall and as fma(fym, s + n, fxm*we) for some components and pairs of
// the tiles that do, differently in every instance of k_smooth; and where a thread keeps the value it wrote last in a register
// (block rows), the closing `*ci` was fused into the next half-sweep's west + east in some sweeps of some instances, so that
// the neighbour in the register and the one in LDS were not the same number.  A cell's last bit depended on which tile of which
// launch swept it.  This is the form every interior path had for the stencil; smooth_tile and k_up_fused both go through it,
// so that a level gives the same bits whichever of them sweeps it and however it is tiled.
__device__ __forceinline__ double gs_cell (double rhs, double fxm, double we, double fym, double s, double n, double ci)
{
#pragma clang fp contract(off)
    const double t = fym*(s + n);
    return (rhs - __builtin_fma(fxm, we, t))*ci;
}

// row (within the tile) and pair index of a thread's m-th cell pair (BR: block rows, see the note above FView)
#define MG_ROWPK(m) const int jj = BR ? (tid / PR)*GPAIRS + (m) : (tid + MG_NT*(m)) / PR, pk = BR ? (tid & (PR - 1)) : (tid + MG_NT*(m)) - jj*PR
// phi_out = GSRB^4(start), start = 0 | phi_in | phi_in + P(crse);
// DO_RES: residual r = rhs - L(phi_out), max|r| (and max|rhs|) -> norms;
//         FUSE_R (cell-centred): cres = R(r) written straight to the next level; else r -> res_out.
// INTERIOR tiles (no swept cell on a wall / outside the box) take a path without masks.
template <bool CC> __device__ __forceinline__ double restrict_at (const FView& fine, int i, int j, int n);
// RPULL (node-centred down-leg): the tile's right-hand side IS the restriction of the finer level's residual -- `crse` then
// is that residual (level above, twice the index), formed while the tile loads (9 reads per cell) and written to `rhs` for
// the up-leg by the tile that finalises the cell: no k_restrict launch between two levels' smoothers
template <class TS, bool CC, int SRC, bool DO_RES, bool FUSE_R, bool INTERIOR, int NSW, bool GATE_IN = (NSW == 4), bool RPULL = false>
__device__ __forceinline__ void smooth_tile (double (&s_phi)[2][TS::AY*TS::AX], double* s_red, double* s_crs, const LevBox& b, const FView& phi_out,
                                             const FView& phi_out2, const FView& rhs, const FView& acf, const FView& phi_in, const FView& crse,
                                             const FView& res_out, const FView& cres_out, double facx, double facy,
                                             int gi0, int gj0, unsigned long long* resnorm, unsigned long long* rhsnorm, const StopRule& sr)
{
    constexpr int E = DO_RES ? NSW : NSW - 1;         // rim of the swept tile that is not final
    constexpr int GT_X = TS::TX, GT_Y = TS::TY, GA_X = TS::AX, GA_Y = TS::AY, MG_NT = TS::NT, GPAIRS = TS::GPAIRS, PR = TS::PR;
    constexpr int AXH = GA_X/2, CH = GA_Y*AXH;        // entries per row / per plane of one colour
    constexpr bool BR = GPAIRS <= 2 || INTERIOR;
    const int tid = threadIdx.x;
    const int cpar = (gi0 + gj0) & 1;                 // colour of ringed cell (0, 0) is (gi0 - 1 + gj0 - 1) & 1
    MG_STAMP(0);
    // per-thread cell pairs: rhs, coefficient and inverse diagonal stay in registers.  Index p is the
    // sweep parity in which the cell is updated (p = 0: sweeps 0 and 2, p = 1: sweeps 1 and 3), so
    // that every register array below is indexed by compile-time constants only.
    double r0[GPAIRS][2], r1[GPAIRS][2], ac[GPAIRS][2], ci[GPAIRS][2];
    bool in[GPAIRS][2];
    int hx[GPAIRS];                                   // x offset (0/1) within the pair of the p = 0 cell
    double fxm[GPAIRS][2], fym[GPAIRS];               // wall multipliers (boundary tiles only)
    double rmax = 0.0;
#pragma unroll
    for (int m = 0; m < GPAIRS; ++m) {
        MG_ROWPK(m);
        const int j = gj0 + jj;
        hx[m] = (gi0 + 2*pk + j) & 1;                 // colour 0 cell: (i + j) even
        fym[m] = INTERIOR ? facy : wall_mult<CC>(j, b.loy, b.hiy, facy);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int i = gi0 + 2*pk + (hx[m] ^ p);
            fxm[m][p] = INTERIOR ? facx : wall_mult<CC>(i, b.lox, b.hix, facx);
            const int ic = INTERIOR ? i : min(max(i, b.vlx), b.vhx), jc = INTERIOR ? j : min(max(j, b.vly), b.vhy);
            const bool ok = INTERIOR || (ic == i && jc == j);
            in[m][p] = ok;
            double a0, a1;
            if constexpr (RPULL) { a0 = restrict_at<CC>(crse, ic, jc, 0); a1 = restrict_at<CC>(crse, ic, jc, 1); }
            else { a0 = rhs(ic, jc, 0); a1 = rhs(ic, jc, 1); }
            const double a2 = acf(ic, jc, 0);
            r0[m][p] = ok ? a0 : 0.0;
            r1[m][p] = ok ? a1 : 0.0;
            ac[m][p] = ok ? a2 : 0.0;
            ci[m][p] = 1.0/diag_c0<CC>(i, j, b, ac[m][p], facx, facy);
            if (rhsnorm) rmax = fmax(rmax, fmax(fabs(r0[m][p]), fabs(r1[m][p])));
        }
    }
    MG_STAMP(1);
    // fill LDS (ring included): start value inside the unknowns' box, 0 elsewhere.  Loads are
    // unconditional (clamped address + select) and all issued before the first LDS store.
    {
        constexpr int NF = (GA_X*GA_Y + MG_NT - 1)/MG_NT;
        double v0[NF], v1[NF];
        // Node-centred prolongation (bilinear: up to four coarse values per fine cell) THROUGH LDS: asked for from global memory
        // inside the loop below, the 7 cells of a thread had up to 70 loads in flight -- the fused 8-sweep pass of level 0 spilled
        // 39 registers under its 128-register cap (58 us against 32 for the cell-centred pass, n = 1023).  The coarse cells under
        // the ringed tile go to LDS once (one load per coarse cell instead of one per fine neighbour), the interpolation reads them there.
        constexpr bool PLDS = !CC && SRC == SRC_PROLONG;
        constexpr int CXN = GA_X/2 + 2, CYN = GA_Y/2 + 2;
        const int cx0 = (INTERIOR ? gi0 - 1 : min(max(gi0 - 1, b.vlx), b.vhx)) >> 1, cy0 = (INTERIOR ? gj0 - 1 : min(max(gj0 - 1, b.vly), b.vhy)) >> 1;
        if constexpr (PLDS) {
            const int cxl = b.vlx >> 1, cxh = (b.vhx >> 1) + 1, cyl = b.vly >> 1, cyh = (b.vhy >> 1) + 1;      // the coarse level's box, walls included
            constexpr int NC = (CXN*CYN + MG_NT - 1)/MG_NT;
            double c0[NC], c1[NC];
#pragma unroll
            for (int m = 0; m < NC; ++m) {
                const int q = min(tid + MG_NT*m, CXN*CYN - 1);
                const int ly = q / CXN, lx = q - ly*CXN;
                const int X = min(max(cx0 + lx, cxl), cxh), Y = min(max(cy0 + ly, cyl), cyh);
                c0[m] = crse(X, Y, 0); c1[m] = crse(X, Y, 1);
            }
#pragma unroll
            for (int m = 0; m < NC; ++m) {
                const int q = tid + MG_NT*m;
                if (q < CXN*CYN) { s_crs[q] = c0[m]; s_crs[CXN*CYN + q] = c1[m]; }
            }
        }
#pragma unroll
        for (int m = 0; m < NF; ++m) {
            const int s = min(tid + MG_NT*m, GA_X*GA_Y - 1);
            const int lj = s / GA_X, li = s - lj*GA_X;
            const int i = gi0 - 1 + li, j = gj0 - 1 + lj;
            v0[m] = 0.0; v1[m] = 0.0;
            if (SRC != SRC_ZERO) {
                const int ic = INTERIOR ? i : min(max(i, b.vlx), b.vhx), jc = INTERIOR ? j : min(max(j, b.vly), b.vhy);
                double a0 = phi_in(ic, jc, 0), a1 = phi_in(ic, jc, 1);
                if (SRC == SRC_PROLONG && !PLDS) { a0 += prolong_at<CC>(crse, ic, jc, 0); a1 += prolong_at<CC>(crse, ic, jc, 1); }
                const bool inside = INTERIOR || (ic == i && jc == j);
                v0[m] = inside ? a0 : 0.0; v1[m] = inside ? a1 : 0.0;
            }
        }
        if constexpr (PLDS) {
            __syncthreads();
#pragma unroll
            for (int m = 0; m < NF; ++m) {
                const int s = min(tid + MG_NT*m, GA_X*GA_Y - 1);
                const int lj = s / GA_X, li = s - lj*GA_X;
                const int i = gi0 - 1 + li, j = gj0 - 1 + lj;
                const int ic = INTERIOR ? i : min(max(i, b.vlx), b.vhx), jc = INTERIOR ? j : min(max(j, b.vly), b.vhy);
                const bool inside = INTERIOR || (ic == i && jc == j);
                // prolong_at<false>'s four cases with its order of additions, on the LDS copy
                const int o = ((jc >> 1) - cy0)*CXN + (ic >> 1) - cx0;
                const bool io = (ic & 1), jo = (jc & 1);
                double p0, p1;
                const double* q0 = s_crs + o; const double* q1 = s_crs + CXN*CYN + o;
                if (io && jo)  { p0 = (q0[0] + q0[1] + q0[CXN] + q0[CXN + 1])*0.25; p1 = (q1[0] + q1[1] + q1[CXN] + q1[CXN + 1])*0.25; }
                else if (io)   { p0 = (q0[0] + q0[1])*0.5; p1 = (q1[0] + q1[1])*0.5; }
                else if (jo)   { p0 = (q0[0] + q0[CXN])*0.5; p1 = (q1[0] + q1[CXN])*0.5; }
                else           { p0 = q0[0]; p1 = q1[0]; }
                if (inside) { v0[m] += p0; v1[m] += p1; }
            }
        }
        {   // The gate of a speculative V-cycle, read while ALL the tile's loads are in flight (a kernel's first dependent
            // read of global memory costs ~1.5 us behind a kernel boundary; read first, the gate was one such trip ahead
            // of the loads).  HPS_KEEP: the loads must not sink below the branch.
            // Only the 4-sweep kernels of the coarser levels do this (a handful of workgroups, each a chain of latencies);
            // the 8-sweep pass of level 0 is bound by bandwidth and registers (all its operands live at once would cost
            // it a workgroup per CU) and reads its gate first.
            if (GATE_IN) {
                const bool active = vcycle_active(sr);
#pragma unroll
                for (int m = 0; m < GPAIRS; ++m) { HPS_KEEP(r0[m][0]); HPS_KEEP(r0[m][1]); HPS_KEEP(r1[m][0]); HPS_KEEP(r1[m][1]); HPS_KEEP(ac[m][0]); HPS_KEEP(ac[m][1]); }
#pragma unroll
                for (int m = 0; m < NF; ++m) { HPS_KEEP(v0[m]); HPS_KEEP(v1[m]); }
                if (!active) return;
            }
        }
        // LDS layout: the two colours of the red-black ordering in separate planes (cell (li, lj) of the
        // ringed tile -> plane (i + j) & 1, row lj, entry li >> 1): a half-sweep then reads and writes
        // consecutive doubles per lane instead of every other one (which is a 2-way bank conflict).
#pragma unroll
        for (int m = 0; m < NF; ++m) {
            const int s = tid + MG_NT*m;
            if (s < GA_X*GA_Y) {
                const int lj = s / GA_X, li = s - lj*GA_X;
                const int o = ((cpar + li + lj) & 1)*CH + lj*AXH + (li >> 1);
                s_phi[0][o] = v0[m]; s_phi[1][o] = v1[m];
            }
        }
    }
    __syncthreads();
    MG_STAMP(2);

    double l0[GPAIRS][2], l1[GPAIRS][2];              // BR: the thread's own cells, as it wrote them last (pair, sweep parity of the cell)
    if constexpr (BR) {
        // the thread's own cells, as it wrote them last (index: pair, sweep parity of the cell)
#pragma unroll
        for (int m = 0; m < GPAIRS; ++m) {
            MG_ROWPK(m);
            const int row = (jj + 1)*AXH + pk;
#pragma unroll
            for (int p = 0; p < 2; ++p) { const int h = hx[m] ^ p; l0[m][p] = s_phi[0][p*CH + row + h]; l1[m][p] = s_phi[1][p*CH + row + h]; }
        }
#pragma unroll
        for (int icolor = 0; icolor < NSW; ++icolor) {
            const int p = icolor & 1;                     // compile-time after unrolling
#pragma unroll
            for (int m = 0; m < GPAIRS; ++m) {
                MG_ROWPK(m);
                const int h = hx[m] ^ p;
                // self: plane p, entry pk + h.  West / east: the partner (register) and entry pk + h of plane 1-p (the pair's other side);
                // south / north: the block's own rows (registers) or entry pk + h of the rows below / above it
                const int row = (jj + 1)*AXH + pk;
                const double* nb0 = &s_phi[0][(1 - p)*CH + row];
                const double* nb1 = &s_phi[1][(1 - p)*CH + row];
                const double we0 = nb0[h] + l0[m][1 - p], we1 = nb1[h] + l1[m][1 - p];      // (west + east: a + b = b + a to the bit)
                const double s0 = (m > 0) ? l0[m > 0 ? m - 1 : 0][1 - p] : nb0[h - AXH], s1 = (m > 0) ? l1[m > 0 ? m - 1 : 0][1 - p] : nb1[h - AXH];
                const double t0 = (m + 1 < GPAIRS) ? l0[m + 1 < GPAIRS ? m + 1 : m][1 - p] : nb0[h + AXH], t1 = (m + 1 < GPAIRS) ? l1[m + 1 < GPAIRS ? m + 1 : m][1 - p] : nb1[h + AXH];
                const double n0 = gs_cell(r0[m][p], fxm[m][p], we0, fym[m], s0, t0, ci[m][p]);
                const double n1 = gs_cell(r1[m][p], fxm[m][p], we1, fym[m], s1, t1, ci[m][p]);
                if (INTERIOR || in[m][p]) { s_phi[0][p*CH + row + h] = n0; s_phi[1][p*CH + row + h] = n1; l0[m][p] = n0; l1[m][p] = n1; }
            }
            __syncthreads();
        }
    } else {
#pragma unroll
        for (int icolor = 0; icolor < NSW; ++icolor) {
            constexpr int dummy = 0; (void)dummy;
            const int p = icolor & 1;                     // compile-time after unrolling
#pragma unroll
            for (int m = 0; m < GPAIRS; ++m) {
                MG_ROWPK(m);
                const int h = hx[m] ^ p;
                // self: plane p, entry pk + h; west / east: plane 1-p, entries pk, pk + 1; south / north: pk + h
                const int row = (jj + 1)*AXH + pk;
                const double* nb0 = &s_phi[0][(1 - p)*CH + row];
                const double* nb1 = &s_phi[1][(1 - p)*CH + row];
                const double n0 = gs_cell(r0[m][p], fxm[m][p], nb0[0] + nb0[1], fym[m], nb0[h - AXH], nb0[h + AXH], ci[m][p]);
                const double n1 = gs_cell(r1[m][p], fxm[m][p], nb1[0] + nb1[1], fym[m], nb1[h - AXH], nb1[h + AXH], ci[m][p]);
                if (INTERIOR || in[m][p]) { s_phi[0][p*CH + row + h] = n0; s_phi[1][p*CH + row + h] = n1; }
            }
            __syncthreads();
        }
    }
    MG_STAMP(3);

    double resmax = 0.0;
    if constexpr (BR) {
        double la0[GPAIRS], ra0[GPAIRS], la1[GPAIRS], ra1[GPAIRS];      // FUSE_R: residual of the left / right cell of a pair, per component
        bool finr[GPAIRS];
#pragma unroll
        for (int m = 0; m < GPAIRS; ++m) {
            MG_ROWPK(m);
            const int j = gj0 + jj;
            const bool rowok = (jj >= E && jj < GT_Y - E);
            double q0[2], q1[2];                          // by sweep parity p
            bool fin[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int h = hx[m] ^ p;
                const int ii = 2*pk + h;
                fin[p] = rowok && ii >= E && ii < GT_X - E && in[m][p];
                const int i = gi0 + ii;
                const int row = (jj + 1)*AXH + pk;
                const double f0 = l0[m][p], f1 = l1[m][p];
                q0[p] = 0.0; q1[p] = 0.0;
                if (DO_RES) {
                    const double* nb0 = &s_phi[0][(1 - p)*CH + row];
                    const double* nb1 = &s_phi[1][(1 - p)*CH + row];
                    const double o0 = nb0[h], o1 = nb1[h];                      // the pair's other side; the partner is in a register
                    const double w0 = h ? l0[m][1 - p] : o0, e0 = h ? o0 : l0[m][1 - p];
                    const double w1 = h ? l1[m][1 - p] : o1, e1 = h ? o1 : l1[m][1 - p];
                    const double s0 = (m > 0) ? l0[m > 0 ? m - 1 : 0][1 - p] : nb0[h - AXH], s1 = (m > 0) ? l1[m > 0 ? m - 1 : 0][1 - p] : nb1[h - AXH];
                    const double n0 = (m + 1 < GPAIRS) ? l0[m + 1 < GPAIRS ? m + 1 : m][1 - p] : nb0[h + AXH], n1 = (m + 1 < GPAIRS) ? l1[m + 1 < GPAIRS ? m + 1 : m][1 - p] : nb1[h + AXH];
                    const double t0 = residual_v<INTERIOR>(f0, w0, e0, s0, n0, i, j, b, r0[m][p], ac[m][p], facx, facy);
                    const double t1 = residual_v<INTERIOR>(f1, w1, e1, s1, n1, i, j, b, r1[m][p], ac[m][p], facx, facy);
                    q0[p] = fin[p] ? t0 : 0.0; q1[p] = fin[p] ? t1 : 0.0;
                    resmax = fmax(resmax, fmax(fabs(q0[p]), fabs(q1[p])));
                }
                if (fin[p]) {
                    if constexpr (RPULL) { rhs(i, j, 0) = r0[m][p]; rhs(i, j, 1) = r1[m][p]; }
                    if (DO_RES && !FUSE_R) { res_out(i, j, 0) = q0[p]; res_out(i, j, 1) = q1[p]; }
                    phi_out(i, j, 0) = f0;
                    phi_out(i, j, 1) = f1;
                    if (phi_out2.p) { phi_out2(i, j, 0) = f0; phi_out2(i, j, 1) = f1; }
                }
            }
            const bool sw = (hx[m] != 0);             // the p = 0 cell is the right one
            la0[m] = sw ? q0[1] : q0[0]; ra0[m] = sw ? q0[0] : q0[1];
            la1[m] = sw ? q1[1] : q1[0]; ra1[m] = sw ? q1[0] : q1[1];
            finr[m] = fin[0];
        }
        if (FUSE_R) {
            // restrict_cc (:29-37): 0.25*(((a+b)+c)+d), a,b = left,right cell of an even row, c,d the row above.  Tile origins are
            // even, so a pair is one coarse cell's x-extent; the row above an even row is the thread's next pair, or -- for the last
            // row of its block -- the first pair of the thread PR lanes on (a wave holds 64/PR consecutive blocks, an even number of
            // rows from an even row on: the pairs that straddle two blocks never straddle two waves)
            const double c0 = __shfl_down(la0[0], PR), d0 = __shfl_down(ra0[0], PR);
            const double c1 = __shfl_down(la1[0], PR), d1 = __shfl_down(ra1[0], PR);
#pragma unroll
            for (int m = 0; m < GPAIRS; ++m) {
                MG_ROWPK(m);
                if (finr[m] && ((jj & 1) == 0)) {
                    const bool own = (m + 1 < GPAIRS);
                    const int mu = own ? m + 1 : m;
                    const double ua0 = own ? la0[mu] : c0, ub0 = own ? ra0[mu] : d0, ua1 = own ? la1[mu] : c1, ub1 = own ? ra1[mu] : d1;
                    const int ic = (gi0 + 2*pk) >> 1, jc = (gj0 + jj) >> 1;
                    cres_out(ic, jc, 0) = 0.25*(la0[m] + ra0[m] + ua0 + ub0);
                    cres_out(ic, jc, 1) = 0.25*(la1[m] + ra1[m] + ua1 + ub1);
                }
            }
        }
    } else {
#pragma unroll
        for (int m = 0; m < GPAIRS; ++m) {
            MG_ROWPK(m);
            const int j = gj0 + jj;
            const bool rowok = (jj >= E && jj < GT_Y - E);
            double q0[2], q1[2];                          // by sweep parity p
            bool fin[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int h = hx[m] ^ p;
                const int ii = 2*pk + h;
                fin[p] = rowok && ii >= E && ii < GT_X - E && in[m][p];
                const int i = gi0 + ii;
                const int row = (jj + 1)*AXH + pk;
                const double f0 = s_phi[0][p*CH + row + h], f1 = s_phi[1][p*CH + row + h];
                q0[p] = 0.0; q1[p] = 0.0;
                if (DO_RES) {
                    const double* nb0 = &s_phi[0][(1 - p)*CH + row];
                    const double* nb1 = &s_phi[1][(1 - p)*CH + row];
                    const double t0 = residual_v<INTERIOR>(f0, nb0[0], nb0[1], nb0[h - AXH], nb0[h + AXH], i, j, b, r0[m][p], ac[m][p], facx, facy);
                    const double t1 = residual_v<INTERIOR>(f1, nb1[0], nb1[1], nb1[h - AXH], nb1[h + AXH], i, j, b, r1[m][p], ac[m][p], facx, facy);
                    q0[p] = fin[p] ? t0 : 0.0; q1[p] = fin[p] ? t1 : 0.0;
                    resmax = fmax(resmax, fmax(fabs(q0[p]), fabs(q1[p])));
                }
                if (fin[p]) {
                    if constexpr (RPULL) { rhs(i, j, 0) = r0[m][p]; rhs(i, j, 1) = r1[m][p]; }
                    if (DO_RES && !FUSE_R) { res_out(i, j, 0) = q0[p]; res_out(i, j, 1) = q1[p]; }
                    phi_out(i, j, 0) = f0;
                    phi_out(i, j, 1) = f1;
                    if (phi_out2.p) { phi_out2(i, j, 0) = f0; phi_out2(i, j, 1) = f1; }
                }
            }
            if (FUSE_R) {
                // restrict_cc (:29-37): 0.25*(((a+b)+c)+d), a,b = left,right cell of this row (even j),
                // c,d the row above.  Tile origins are even, so a pair is one coarse cell's x-extent and
                // lanes l / l+32 of a wave hold rows jj / jj+1.
                const bool sw = (hx[m] != 0);             // the p = 0 cell is the right one
                const double la0 = sw ? q0[1] : q0[0], ra0 = sw ? q0[0] : q0[1];
                const double la1 = sw ? q1[1] : q1[0], ra1 = sw ? q1[0] : q1[1];
                const double c0 = __shfl_down(la0, PR), d0 = __shfl_down(ra0, PR);
                const double c1 = __shfl_down(la1, PR), d1 = __shfl_down(ra1, PR);
                if (fin[0] && ((tid & PR) == 0)) {
                    const int ic = (gi0 + 2*pk) >> 1, jc = j >> 1;
                    cres_out(ic, jc, 0) = 0.25*(la0 + ra0 + c0 + d0);
                    cres_out(ic, jc, 1) = 0.25*(la1 + ra1 + c1 + d1);
                }
            }
        }
    }
    MG_STAMP(4);
    if (DO_RES && resnorm) block_max_to<MG_NT>(resnorm, resmax, s_red);
    if (rhsnorm) block_max_to<MG_NT>(rhsnorm, rmax, s_red);
    MG_STAMP(5);
}

// NSW red-black half-sweeps per launch: 4 (one GSRB^4 of the reference) or 8 (the two consecutive
// GSRB^4 that end a V-cycle on level 0, fused: one pass over HBM instead of two)
// GUEST (none, or one CoefGuest: the instance that makes a solve's initial level-0 pass where the lower V is k_lower_v3):
// workgroup 0 of that launch is no tile but derives the lower V's coefficient image (coef_guest_derive) in the tile's static
// LDS: it starts with the first round of tiles and is done long before the pass is; the tiles are workgroups 1 .. .  Instances
// without a guest have the same arguments and the same code as before the guest existed.
struct CoefGuest;
__device__ void coef_guest_derive (double* s_img, const CoefGuest& g, int nt);

template <class TS, bool CC, int SRC, bool DO_RES, bool FUSE_R, int NSW = 4, bool RPULL = false, class... GUEST>
__global__ __launch_bounds__(TS::NT, (RPULL && TS::GPAIRS > 1) ? 2 : 4)      // at most 128 VGPRs: two 512-thread workgroups per CU (several variants sit at 113-130); the pulling smoother with two pairs per thread (36 + 36 loads in flight) gets 256
void k_smooth (LevBox b, FView phi_out, FView phi_out2, FView rhs, FView acf, FView phi_in, FView crse, FView res_out,
               FView cres_out, double facx, double facy, int ntx, unsigned long long* resnorm,
               unsigned long long* rhsnorm, StopRule sr, GUEST... guest)
{
    static_assert(!FUSE_R || (CC && DO_RES), "fused restriction is cell-centred only");
    constexpr int HOST = (int)sizeof...(GUEST);       // workgroups ahead of the tiles
    static_assert(HOST <= 1 && (HOST == 0 || (CC && NSW == 4)), "the guest rides in the cell-centred initial pass");
    // (the 4-sweep kernels read the gate behind their loads, see smooth_tile; the 8-sweep pass first: with the gate behind its
    //  loads all of the tile's operands are live across it, 61 registers spilled under its 128-register cap, round 4)
    if (NSW != 4 && !vcycle_active(sr)) return;
    constexpr int GT_X = TS::TX, GT_Y = TS::TY;
    __shared__ double s_phi[2][TS::AY*TS::AX];
    __shared__ double s_red[TS::NT/64];
    if constexpr (HOST > 0) {
        static_assert(2*TS::AY*TS::AX >= COEF_GUEST_MAX_IMG, "the image is staged in the tile's static LDS");
        if (blockIdx.x == 0) { coef_guest_derive(&s_phi[0][0], guest..., TS::NT); return; }
    }
    // node-centred prolongation goes through LDS (smooth_tile): the coarse cells under the ringed tile, two components
    constexpr bool PLDS = !CC && SRC == SRC_PROLONG;
    __shared__ double s_crs[PLDS ? 2*(TS::AX/2 + 2)*(TS::AY/2 + 2) : 1];
    constexpr int E = DO_RES ? NSW : NSW - 1;
    constexpr int FX = GT_X - 2*E, FY = GT_Y - 2*E;   // cells a tile finalises (even numbers)
    // workgroups go round-robin to the 8 XCDs: give each XCD a contiguous run of tiles, so that the
    // rims shared by neighbouring tiles hit in that XCD's L2
    // (behind a guest the runs belong to XCD (xcd + 1) & 7: contiguous all the same)
    const unsigned wg = blockIdx.x - HOST;
    const int nb = gridDim.x - HOST, q8 = nb >> 3, r8 = nb & 7, xcd = wg & 7;
    const int tile = xcd*q8 + min(xcd, r8) + (wg >> 3);
    const int bx = tile % ntx, by = tile / ntx;
    const int gi0 = b.vlx + bx*FX - E;                // global index of swept cell (0,0)
    const int gj0 = b.vly + by*FY - E;
    // every swept cell and its ring strictly inside the unknowns' box and off the walls
    const bool interior = (gi0 - 1 >= b.vlx) && (gi0 + GT_X <= b.vhx) && (gj0 - 1 >= b.vly) && (gj0 + GT_Y <= b.vhy)
                       && (gi0 > b.lox) && (gi0 + GT_X - 1 < b.hix) && (gj0 > b.loy) && (gj0 + GT_Y - 1 < b.hiy);
    constexpr bool GATE_IN = (NSW == 4);
    if (interior) smooth_tile<TS, CC, SRC, DO_RES, FUSE_R, true, NSW, GATE_IN, RPULL>(s_phi, s_red, s_crs, b, phi_out, phi_out2, rhs, acf, phi_in, crse, res_out, cres_out,
                                                             facx, facy, gi0, gj0, resnorm, rhsnorm, sr);
    else          smooth_tile<TS, CC, SRC, DO_RES, FUSE_R, false, NSW, GATE_IN, RPULL>(s_phi, s_red, s_crs, b, phi_out, phi_out2, rhs, acf, phi_in, crse, res_out, cres_out,
                                                              facx, facy, gi0, gj0, resnorm, rhsnorm, sr);
}

// ---- the up-leg of the mid levels 1 .. NL in one launch (cell-centred) ---------------------------
// Per V-cycle the up-leg of levels 3, 2, 1 was three dependent launches of ~5, 5 and 8 us, each a launch floor + a first read
// + four barrier phases + a store.  The cell-centred prolongation is piecewise constant and an up-leg smoother needs neither
// residual nor norm, so the smoothed correction a level-1 tile reads from level 2 is a function of a small region of level 2,
// and that of a smaller one of level 3: a workgroup that owns a level-1 tile first smooths the level-3 cells under it in LDS,
// then the level-2 cells, then its own tile.  The redundant sweeps fall on the cheap levels; rescor[2], rescor[3] (read by the
// next up-leg level only) stay in LDS.  All three levels' inputs exist when the launch starts: every load is issued up front.
//
// Geometry.  A level with SX x SY swept cells (ringed: + 2) reads the coarser level under its ringed region clipped to its
// box: at most (SX + 2)/2 + 1 coarse cells in x for any parity of the origin.  Those must be final, i.e. 3 cells inside the
// coarse swept region or behind the box's edge: the coarse level sweeps (SX + 2)/2 + 7 cells from 3 below the first one.
// 64 x 32 on level 1 -> 40 x 24 on level 2 -> 28 x 20 on level 3; 32 x 16 -> 24 x 16 -> 20 x 16.
//
// UpLev: one level's share of a thread -- GP cell pairs in GP consecutive rows (the block rows of smooth_tile: the values
// it wrote last stay in registers), right-hand side, multipliers and inverse diagonal in registers, and its share of the
// ringed region's start values.  The arithmetic per cell is smooth_tile's (gs_cell, wall_mult, diag_c0, the same masks).
struct UpLevArg { LevBox b; FView rhs, acf, cor; double facx, facy; };
struct UpArgs { UpLevArg l[3]; FView crse, out; int ntx; };      // l[k]: level 1 + k; crse: below the coarsest fused level; out: rescor[1]

template <int SX_, int SY_, int NT_, bool INTERIOR, bool GCRSE>
struct UpLev {
    static constexpr int SX = SX_, SY = SY_, NT = NT_, AX = SX + 2, AY = SY + 2, AXH = AX/2, CH = AY*AXH, PR = SX/2;
    static constexpr int GP = (PR*SY + NT - 1)/NT;         // cell pairs per thread
    static constexpr int NF = (AX*AY + NT - 1)/NT;         // ringed cells per thread
    static constexpr int NBLK = SY/GP;                     // row blocks of PR threads each
    static_assert(SX % 2 == 0 && SY % GP == 0 && PR*NBLK <= NT, "level shape");
    int gi0, gj0, cpar, pk, blk;
    double r0[GP][2], r1[GP][2], ac[GP][2], ci[GP][2], fxm[GP][2], fym[GP];
    bool in[GP][2];
    int hx[GP];
    double v0[NF], v1[NF], c0[GCRSE ? NF : 1], c1[GCRSE ? NF : 1];
    double l0[GP][2], l1[GP][2];

    // every read of global memory this level makes: clamped addresses, nothing depends on a loaded value
    __device__ __forceinline__ void issue (const UpLevArg& a, const FView& crse, int gi0_, int gj0_)
    {
        const LevBox& b = a.b;
        const int tid = threadIdx.x;
        gi0 = gi0_; gj0 = gj0_; cpar = (gi0 + gj0) & 1;
        const bool live = tid < PR*NBLK;                   // (the coarse levels have fewer pairs than the workgroup has threads)
        blk = live ? tid / PR : 0; pk = tid % PR;
#pragma unroll
        for (int m = 0; m < GP; ++m) {
            const int j = gj0 + blk*GP + m;
            hx[m] = (gi0 + 2*pk + j) & 1;                  // colour 0 cell: (i + j) even
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int i = gi0 + 2*pk + (hx[m] ^ p);
                const int ic = INTERIOR ? i : min(max(i, b.vlx), b.vhx), jc = INTERIOR ? j : min(max(j, b.vly), b.vhy);
                in[m][p] = live && (INTERIOR || (ic == i && jc == j));
                r0[m][p] = a.rhs(ic, jc, 0); r1[m][p] = a.rhs(ic, jc, 1); ac[m][p] = a.acf(ic, jc, 0);
            }
        }
#pragma unroll
        for (int m = 0; m < NF; ++m) {
            const int s = min(tid + NT*m, AX*AY - 1);
            const int lj = s / AX, li = s - lj*AX;
            const int i = gi0 - 1 + li, j = gj0 - 1 + lj;
            const int ic = INTERIOR ? i : min(max(i, b.vlx), b.vhx), jc = INTERIOR ? j : min(max(j, b.vly), b.vhy);
            v0[m] = a.cor(ic, jc, 0); v1[m] = a.cor(ic, jc, 1);
            if constexpr (GCRSE) { c0[m] = crse(ic >> 1, jc >> 1, 0); c1[m] = crse(ic >> 1, jc >> 1, 1); }
        }
    }
    __device__ __forceinline__ void keep () const
    {
#pragma unroll
        for (int m = 0; m < GP; ++m) { HPS_KEEP(r0[m][0]); HPS_KEEP(r0[m][1]); HPS_KEEP(r1[m][0]); HPS_KEEP(r1[m][1]); HPS_KEEP(ac[m][0]); HPS_KEEP(ac[m][1]); }
#pragma unroll
        for (int m = 0; m < NF; ++m) { HPS_KEEP(v0[m]); HPS_KEEP(v1[m]); if constexpr (GCRSE) { HPS_KEEP(c0[m]); HPS_KEEP(c1[m]); } }
    }
    // masks, multipliers, inverse diagonals (smooth_tile's expressions)
    __device__ __forceinline__ void coefficients (const UpLevArg& a)
    {
        const LevBox& b = a.b;
#pragma unroll
        for (int m = 0; m < GP; ++m) {
            const int j = gj0 + blk*GP + m;
            fym[m] = INTERIOR ? a.facy : wall_mult<true>(j, b.loy, b.hiy, a.facy);
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int i = gi0 + 2*pk + (hx[m] ^ p);
                fxm[m][p] = INTERIOR ? a.facx : wall_mult<true>(i, b.lox, b.hix, a.facx);
                const bool ok = in[m][p];
                r0[m][p] = ok ? r0[m][p] : 0.0;
                r1[m][p] = ok ? r1[m][p] : 0.0;
                ac[m][p] = ok ? ac[m][p] : 0.0;
                ci[m][p] = 1.0/diag_c0<true>(i, j, b, ac[m][p], a.facx, a.facy);
            }
        }
    }
    // start = cor + P(coarser result) inside the unknowns' box, 0 elsewhere, ring included; the two colours in separate
    // planes as in smooth_tile.  CL: the coarser level, whose result is in sc (its two component planes); none for GCRSE.
    template <class CL>
    __device__ __forceinline__ void fill (double* s, const UpLevArg& a, const CL* cl, const double* sc)
    {
        const LevBox& b = a.b;
        const int tid = threadIdx.x;
#pragma unroll
        for (int m = 0; m < NF; ++m) {
            const int q = tid + NT*m;
            if (q < AX*AY) {
                const int lj = q / AX, li = q - lj*AX;
                const int i = gi0 - 1 + li, j = gj0 - 1 + lj;
                const int ic = INTERIOR ? i : min(max(i, b.vlx), b.vhx), jc = INTERIOR ? j : min(max(j, b.vly), b.vhy);
                double a0 = v0[m], a1 = v1[m];
                if constexpr (GCRSE) { a0 += c0[m]; a1 += c1[m]; }
                else {
                    const int cli = (ic >> 1) - (cl->gi0 - 1), clj = (jc >> 1) - (cl->gj0 - 1);
                    const int oc = ((cl->cpar + cli + clj) & 1)*CL::CH + clj*CL::AXH + (cli >> 1);
                    a0 += sc[oc]; a1 += sc[2*CL::CH + oc];
                }
                const bool inside = INTERIOR || (ic == i && jc == j);
                const int o = ((cpar + li + lj) & 1)*CH + lj*AXH + (li >> 1);
                s[o] = inside ? a0 : 0.0; s[2*CH + o] = inside ? a1 : 0.0;
            }
        }
    }
    // four red-black half-sweeps in LDS, colour 0 first (the block-row path of smooth_tile)
    __device__ __forceinline__ void sweeps (double* s)
    {
        double* s0p = s; double* s1p = s + 2*CH;
#pragma unroll
        for (int m = 0; m < GP; ++m) {
            const int row = (blk*GP + m + 1)*AXH + pk;
#pragma unroll
            for (int p = 0; p < 2; ++p) { const int h = hx[m] ^ p; l0[m][p] = s0p[p*CH + row + h]; l1[m][p] = s1p[p*CH + row + h]; }
        }
#pragma unroll
        for (int icolor = 0; icolor < 4; ++icolor) {
            const int p = icolor & 1;
#pragma unroll
            for (int m = 0; m < GP; ++m) {
                const int h = hx[m] ^ p;
                const int row = (blk*GP + m + 1)*AXH + pk;
                const double* nb0 = &s0p[(1 - p)*CH + row];
                const double* nb1 = &s1p[(1 - p)*CH + row];
                const double we0 = nb0[h] + l0[m][1 - p], we1 = nb1[h] + l1[m][1 - p];
                const double b0 = (m > 0) ? l0[m > 0 ? m - 1 : 0][1 - p] : nb0[h - AXH], b1 = (m > 0) ? l1[m > 0 ? m - 1 : 0][1 - p] : nb1[h - AXH];
                const double t0 = (m + 1 < GP) ? l0[m + 1 < GP ? m + 1 : m][1 - p] : nb0[h + AXH], t1 = (m + 1 < GP) ? l1[m + 1 < GP ? m + 1 : m][1 - p] : nb1[h + AXH];
                const double n0 = gs_cell(r0[m][p], fxm[m][p], we0, fym[m], b0, t0, ci[m][p]);
                const double n1 = gs_cell(r1[m][p], fxm[m][p], we1, fym[m], b1, t1, ci[m][p]);
                if (INTERIOR || in[m][p]) { s0p[p*CH + row + h] = n0; s1p[p*CH + row + h] = n1; l0[m][p] = n0; l1[m][p] = n1; }
            }
            __syncthreads();
        }
    }
    // the cells at least 3 inside the swept tile are final
    __device__ __forceinline__ void store (const FView& out) const
    {
#pragma unroll
        for (int m = 0; m < GP; ++m) {
            const int jj = blk*GP + m;
            const bool rowok = (jj >= 3 && jj < SY - 3);
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int ii = 2*pk + (hx[m] ^ p);
                if (rowok && ii >= 3 && ii < SX - 3 && in[m][p]) { out(gi0 + ii, gj0 + jj, 0) = l0[m][p]; out(gi0 + ii, gj0 + jj, 1) = l1[m][p]; }
            }
        }
    }
};

// swept origin of the coarser level under a level whose swept region starts at g (see "Geometry" above)
__device__ __forceinline__ int up_coarse_origin (int g, int vl, int vh) { return (min(max(g - 1, vl), vh) >> 1) - 3; }

template <class TS, int NL, bool INTERIOR>
__device__ __forceinline__ void up_fused_tile (double* s1, double* s2, double* s3, const UpArgs& A, int gi0, int gj0, const StopRule& sr)
{
    constexpr int X2 = (TS::TX + 2)/2 + 7, Y2 = (TS::TY + 2)/2 + 7, X3 = (X2 + 2)/2 + 7, Y3 = (Y2 + 2)/2 + 7;
    UpLev<TS::TX, TS::TY, TS::NT, INTERIOR, false> L1;
    UpLev<X2, Y2, TS::NT, false, NL == 2> L2;
    UpLev<X3, Y3, TS::NT, false, true> L3;
    const int g2i = up_coarse_origin(gi0, A.l[0].b.vlx, A.l[0].b.vhx), g2j = up_coarse_origin(gj0, A.l[0].b.vly, A.l[0].b.vhy);
    L1.issue(A.l[0], A.crse, gi0, gj0);
    L2.issue(A.l[1], A.crse, g2i, g2j);
    if constexpr (NL == 3)
        L3.issue(A.l[2], A.crse, up_coarse_origin(g2i, A.l[1].b.vlx, A.l[1].b.vhx), up_coarse_origin(g2j, A.l[1].b.vly, A.l[1].b.vhy));
    {   // the gate of a speculative V-cycle behind the issued loads, as in smooth_tile
        const bool active = vcycle_active(sr);
        L1.keep(); L2.keep();
        if constexpr (NL == 3) L3.keep();
        if (!active) return;
    }
    if constexpr (NL == 3) {
        L3.coefficients(A.l[2]);
        L3.fill(s3, A.l[2], &L3, s3);
        __syncthreads();
        L3.sweeps(s3);
    }
    L2.coefficients(A.l[1]);
    L2.fill(s2, A.l[1], &L3, s3);
    __syncthreads();
    L2.sweeps(s2);
    L1.coefficients(A.l[0]);
    L1.fill(s1, A.l[0], &L2, s2);
    __syncthreads();
    L1.sweeps(s1);
    L1.store(A.out);
}

template <class TS, int NL>
__global__ __launch_bounds__(TS::NT, 1)      // one workgroup per CU (the grid has about as many workgroups as the chip has CUs): no register cap
void k_up_fused (UpArgs A, StopRule sr)
{
    static_assert(NL == 2 || NL == 3, "two or three mid levels");
    constexpr int X2 = (TS::TX + 2)/2 + 7, Y2 = (TS::TY + 2)/2 + 7, X3 = (X2 + 2)/2 + 7, Y3 = (Y2 + 2)/2 + 7;
    __shared__ double s1[2*TS::AX*TS::AY];
    __shared__ double s2[2*(X2 + 2)*(Y2 + 2)];
    __shared__ double s3[NL == 3 ? 2*(X3 + 2)*(Y3 + 2) : 1];
    constexpr int E = 3, FX = TS::TX - 2*E, FY = TS::TY - 2*E;
    const LevBox& b = A.l[0].b;
    // k_smooth's tiling and its XCD-contiguous tile mapping
    const unsigned wg = blockIdx.x;
    const int nb = gridDim.x, q8 = nb >> 3, r8 = nb & 7, xcd = wg & 7;
    const int tile = xcd*q8 + min(xcd, r8) + (wg >> 3);
    const int bx = tile % A.ntx, by = tile / A.ntx;
    const int gi0 = b.vlx + bx*FX - E, gj0 = b.vly + by*FY - E;
    const bool interior = (gi0 - 1 >= b.vlx) && (gi0 + TS::TX <= b.vhx) && (gj0 - 1 >= b.vly) && (gj0 + TS::TY <= b.vhy)
                       && (gi0 > b.lox) && (gi0 + TS::TX - 1 < b.hix) && (gj0 > b.loy) && (gj0 + TS::TY - 1 < b.hiy);
    if (interior) up_fused_tile<TS, NL, true>(s1, s2, s3, A, gi0, gj0, sr);
    else          up_fused_tile<TS, NL, false>(s1, s2, s3, A, gi0, gj0, sr);
}

// coarse = R(fine): 4-average (cell-centred) or 9-point full weighting (nodal)
template <bool CC>
__device__ __forceinline__ double restrict_at (const FView& fine, int i, int j, int n)
{
    if (CC) return 0.25*(fine(2*i, 2*j, n) + fine(2*i+1, 2*j, n) + fine(2*i, 2*j+1, n) + fine(2*i+1, 2*j+1, n));
    return (1./16.)*(fine(2*i-1, 2*j-1, n) + 2.*fine(2*i, 2*j-1, n) + fine(2*i+1, 2*j-1, n)
                   + 2.*fine(2*i-1, 2*j, n) + 4.*fine(2*i, 2*j, n) + 2.*fine(2*i+1, 2*j, n)
                   + fine(2*i-1, 2*j+1, n) + 2.*fine(2*i, 2*j+1, n) + fine(2*i+1, 2*j+1, n));
}

template <bool CC>
__global__ __launch_bounds__(256)
void k_restrict (LevBox cb, FView crse, FView fine, int ncomp, StopRule sr)
{
    if (!vcycle_active(sr)) return;
    const int i = cb.vlx + blockIdx.x*blockDim.x + threadIdx.x;
    const int j = cb.vly + blockIdx.y;
    if (i > cb.vhx || j > cb.vhy) return;
    for (int n = 0; n < ncomp; ++n) crse(i, j, n) = restrict_at<CC>(fine, i, j, n);
}

// ---- all small levels in one workgroup, LDS resident --------------------------------------------
typedef __attribute__((address_space(3))) double lds_double;

// per small level: box, row length, points, offset (in doubles) of its 8-plane block in LDS:
// [acf | res0 res1 | cor0 cor1 | rescor0 rescor1 | 1/diagonal]
struct LowLev { LevBox b; int nxb; int cells; int off; };

struct LView {      // one component plane of a small level in LDS, level index space
    lds_double* p; int nxb; int lox, loy;
    __device__ __forceinline__ lds_double& operator() (int i, int j) const { return p[(i - lox) + (j - loy)*nxb]; }
};
__device__ __forceinline__ LView lplane (lds_double* base, const LowLev& l, int plane)
{
    return LView{base + l.off + plane*l.cells, l.nxb, l.b.lox, l.b.loy};
}

template <bool CC>
__device__ __forceinline__ double lrestrict (const LView& f, int i, int j)
{
    if (CC) return 0.25*(f(2*i, 2*j) + f(2*i+1, 2*j) + f(2*i, 2*j+1) + f(2*i+1, 2*j+1));
    return (1./16.)*(f(2*i-1, 2*j-1) + 2.*f(2*i, 2*j-1) + f(2*i+1, 2*j-1)
                   + 2.*f(2*i-1, 2*j) + 4.*f(2*i, 2*j) + 2.*f(2*i+1, 2*j)
                   + f(2*i-1, 2*j+1) + 2.*f(2*i, 2*j+1) + f(2*i+1, 2*j+1));
}

template <bool CC>
__device__ __forceinline__ double lprolong (const LView& c, int i, int j)
{
    const int ic = i >> 1, jc = j >> 1;
    if (CC) return c(ic, jc);
    const bool io = (i & 1), jo = (j & 1);
    if (io && jo)  return (c(ic, jc) + c(ic+1, jc) + c(ic, jc+1) + c(ic+1, jc+1))*0.25;
    if (io)        return (c(ic, jc) + c(ic+1, jc))*0.5;
    if (jo)        return (c(ic, jc) + c(ic, jc+1))*0.5;
    return c(ic, jc);
}

// Every level is worked by the whole workgroup: its threads as a 32-wide patch swept over the level (no integer divisions in the
// loops), phases separated by __syncthreads.  (Round 6 measured the levels of at most 17^2 points on wave 0 alone, phases separated
// by a fence only: slower, 396.3 against 371.8 us per slice at 1023^2, and 336 against 331 with batched phases -- a phase is bound
// by its instruction stream, not by the barrier: DESIGN section 4 "tried", profiles/r06_lowv_wave_ab.txt.)
#define HPS_LOW_FOR_VALID(l, i, j)                                                          \
    for (int j = (l).b.vly + (int)(threadIdx.x >> 5); j <= (l).b.vhy; j += (int)(blockDim.x >> 5))   \
        for (int i = (l).b.vlx + (int)(threadIdx.x & 31); i <= (l).b.vhx; i += 32)

__device__ __forceinline__ double low_fac (double f0, int l) { for (int k = 0; k < l; ++k) f0 *= 0.25; return f0; }      // (exact: powers of two)

template <bool CC>
__device__ void low_sweeps (lds_double* base, const LowLev& l, double facx, double facy, int nsweeps, int n0 = 0, int n1 = 2)
{
    // A half-sweep touches the points of one colour only: the threads are mapped onto THOSE -- a patch 16 half-columns wide,
    // so a 31^2 level is one trip of 496 threads (8 waves: two per SIMD) instead of 961 threads of which every other one sits
    // out (16 waves: four per SIMD, all of them issuing the loop's ~150 instructions)
    const int ti = (int)(threadIdx.x & 15), tj = (int)(threadIdx.x >> 4);
    const int si = 16, sj = (int)(blockDim.x >> 4);
    const LView cinv = lplane(base, l, 7);
    if (!CC && l.b.vhy - l.b.vly < sj && l.b.vhx - l.b.vlx < 2*si) {
        // One trip per thread (every level the node-centred lower V holds): the thread's row is fixed and its point alternates
        // between two columns with the colour -- both points' offsets, coefficients and right-hand sides are set up ONCE, ahead
        // of the half-sweeps, whose bodies are then four neighbour reads, six fp64 operations and a store.  (The stamps had
        // shown the phases bound by their instruction streams: the generic views' index arithmetic and the loops' exec-mask
        // control were most of a phase's 130-250 instructions.)  No wall variants on node-centred levels: walls hold zeros.
        const int j = l.b.vly + tj;
        const bool rowok = j <= l.b.vhy;
        const int jc = rowok ? j : l.b.vly;
        int off[2]; bool ok[2]; double ci[2], r0[2], r1[2];
        const bool two = (n1 - n0) == 2;
        lds_double* ph0 = base + l.off + (3 + n0)*l.cells;
        lds_double* ph1 = base + l.off + (2 + n1)*l.cells;
#pragma unroll
        for (int par = 0; par < 2; ++par) {            // par = is & 1
            const int i = l.b.vlx + ((l.b.vlx + jc + par) & 1) + 2*ti;
            ok[par] = rowok && i <= l.b.vhx;
            const int ic = ok[par] ? i : l.b.vlx;
            off[par] = (ic - l.b.lox) + (jc - l.b.loy)*l.nxb;
            ci[par] = cinv(ic, jc);
            r0[par] = base[l.off + (1 + n0)*l.cells + off[par]];
            r1[par] = base[l.off + n1*l.cells + off[par]];
        }
        const int sy = l.nxb;
        for (int is = 0; is < nsweeps; ++is) {
            const int par = is & 1;
            const int o = par ? off[1] : off[0];
            const bool k = par ? ok[1] : ok[0];
            const double c = par ? ci[1] : ci[0], ra = par ? r0[1] : r0[0], rb = par ? r1[1] : r1[0];
            if (k) {
                {   const lds_double* q = ph0 + o;
                    const double w = q[-1], e = q[1], so = q[-sy], no = q[sy];
                    ph0[o] = (ra - (facx*(w + e) + facy*(so + no)))*c; }
                if (two) {
                    const lds_double* q = ph1 + o;
                    const double w = q[-1], e = q[1], so = q[-sy], no = q[sy];
                    ph1[o] = (rb - (facx*(w + e) + facy*(so + no)))*c; }
            }
            __syncthreads();
        }
        return;
    }
    for (int is = 0; is < nsweeps; ++is) {
        for (int j = l.b.vly + tj; j <= l.b.vhy; j += sj) {
            for (int i = l.b.vlx + ((l.b.vlx + j + is) & 1) + 2*ti; i <= l.b.vhx; i += 2*si) {      // (i + j + is) even
                const double ci = cinv(i, j);
                for (int n = n0; n < n1; ++n) {
                    const LView rhs = lplane(base, l, 1 + n), phi = lplane(base, l, 3 + n);
                    phi(i, j) = (rhs(i, j) - offdiag<CC, false>((const lds_double*)&phi(i, j), l.nxb, i, j, l.b, facx, facy))*ci;
                }
            }
        }
        __syncthreads();
    }
}

// coefficient of level c from level f (average_down_acoef) and the inverse diagonals of a level
template <bool CC>
__device__ void low_hier_level (lds_double* base, const LowLev& f, const LowLev& c)
{
    const LView fine = lplane(base, f, 0), crse = lplane(base, c, 0);
    // (the walls of every plane hold the zeros the kernel starts from: only unknowns are ever written)
    HPS_LOW_FOR_VALID(c, i, j) crse(i, j) = lrestrict<CC>(fine, i, j);
    __syncthreads();
}
template <bool CC>
__device__ void low_cinv_level (lds_double* base, const LowLev& l, double fx, double fy)
{
    const LView acf = lplane(base, l, 0), cinv = lplane(base, l, 7);
    HPS_LOW_FOR_VALID(l, i, j) cinv(i, j) = 1.0/diag_c0<CC>(i, j, l.b, acf(i, j), fx, fy);
}

// down-leg of level l: cor = 0, four half-sweeps, residual, its restriction = right-hand side of level c
template <bool CC>
__device__ void low_down_level (lds_double* base, const LowLev& l, const LowLev& c, double facx, double facy, int n0, int n1)
{
    // cor = 0 and the walls of rescor = 0 (the nodal restriction reads them): both still hold the zeros the kernel starts from --
    // a level is visited once per launch -- so neither costs a phase of its own (round 6: 13 of the ~105 barrier-separated
    // phases of a V-cycle at 1023^2)
    low_sweeps<CC>(base, l, facx, facy, 4, n0, n1);
    {   // residual -> rescor
        const LView acf = lplane(base, l, 0);
        HPS_LOW_FOR_VALID(l, i, j) {
            const double a = acf(i, j);
            for (int n = n0; n < n1; ++n) {
                const LView rhs = lplane(base, l, 1 + n), phi = lplane(base, l, 3 + n), rc = lplane(base, l, 5 + n);
                rc(i, j) = residual_at<false>((const lds_double*)&phi(i, j), l.nxb, i, j, l.b, rhs(i, j), a, facx, facy);
            }
        }
        __syncthreads();
    }
    {   // restriction -> res of the next level
        HPS_LOW_FOR_VALID(c, i, j) {
            for (int n = n0; n < n1; ++n) lplane(base, c, 1 + n)(i, j) = lrestrict<CC>(lplane(base, l, 5 + n), i, j);
        }
        __syncthreads();
    }
}
// up-leg of level l: cor += P(cor of level c), four half-sweeps
template <bool CC>
__device__ void low_up_level (lds_double* base, const LowLev& l, const LowLev& c, double facx, double facy, int n0, int n1)
{
    HPS_LOW_FOR_VALID(l, i, j) {
        for (int n = n0; n < n1; ++n) {
            const LView fine = lplane(base, l, 3 + n);
            fine(i, j) = fine(i, j) + lprolong<CC>(lplane(base, c, 3 + n), i, j);
        }
    }
    __syncthreads();
    low_sweeps<CC>(base, l, facx, facy, 4, n0, n1);
}

// The bottom level of a 2^K - 1 grid holds 3 x 3 unknowns and takes 16+ half-sweeps (HpMultiGrid.cpp:854-1033): as phases of the
// whole workgroup that was 16 x ~1100 clocks, a quarter of the kernel, for nine numbers.  One lane per component does them in
// registers instead: the same expression per point ((rhs - offdiag) * 1/diag, offdiag<CC, false>'s), the same colour order; points
// of one colour do not read one another, so doing them one after the other changes nothing.
template <bool CC, int P0>          // P0 = (vlx + vly) & 1: the colour of the level's first unknown, so that every point's colour is a constant
__device__ __forceinline__ void low_bottom_regs_p (lds_double* base, const LowLev& l, double facx, double facy, int nsweeps, int n0, int n1)
{
    const int nvx = l.b.vhx - l.b.vlx + 1, nvy = l.b.vhy - l.b.vly + 1;      // <= 3 each (caller)
    for (int n = n0 + (int)threadIdx.x; n < n1; n += (int)blockDim.x) {       // (thread 0: component n0; thread 1: the other one without the split)
        const LView rhs = lplane(base, l, 1 + n), phi = lplane(base, l, 3 + n), cinv = lplane(base, l, 7);
        double p[5][5], r[3][3], c[3][3];
        bool ok[3][3];
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int b = 0; b < 5; ++b) p[a][b] = 0.0;                          // ring = walls (0), unknowns start from 0
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                ok[a][b] = a < nvy && b < nvx;
                r[a][b] = ok[a][b] ? rhs(l.b.vlx + b, l.b.vly + a) : 0.0;
                c[a][b] = ok[a][b] ? cinv(l.b.vlx + b, l.b.vly + a) : 0.0;
            }
        // one half-sweep: the points of colour `col` (compile-time), straight-line
        auto half = [&] (auto colc) {
            constexpr int col = decltype(colc)::value;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    if (((a + b + P0 + col) & 1) != 0) continue;                // (i + j + is) even  <=>  (a + b + P0 + is) even
                    const int i = l.b.vlx + b, j = l.b.vly + a;
                    const double w = p[a + 1][b], e = p[a + 1][b + 2], so = p[a][b + 1], no = p[a + 2][b + 1];
                    double lx = facx*(w + e), ly = facy*(so + no);
                    if (CC) {
                        const double fx43 = facx*(4./3.), fy43 = facy*(4./3.);
                        lx = (i == l.b.lox) ? fx43*e : ((i == l.b.hix) ? fx43*w : lx);
                        ly = (j == l.b.loy) ? fy43*no : ((j == l.b.hiy) ? fy43*so : ly);
                    }
                    const double v = (r[a][b] - (lx + ly))*c[a][b];
                    p[a + 1][b + 1] = ok[a][b] ? v : p[a + 1][b + 1];
                }
        };
        int is = 0;
        for (; is + 1 < nsweeps; is += 2) { half(std::integral_constant<int, 0>{}); half(std::integral_constant<int, 1>{}); }
        if (is < nsweeps) half(std::integral_constant<int, 0>{});
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b)
                if (ok[a][b]) phi(l.b.vlx + b, l.b.vly + a) = p[a + 1][b + 1];
    }
}
template <bool CC>
__device__ void low_bottom_lane (lds_double* base, const LowLev& l, double facx, double facy, int nsweeps, int n0, int n1)
{
    if (((l.b.vlx + l.b.vly) & 1) == 0) low_bottom_regs_p<CC, 0>(base, l, facx, facy, nsweeps, n0, n1);
    else low_bottom_regs_p<CC, 1>(base, l, facx, facy, nsweeps, n0, n1);
    __syncthreads();
}

// levels lv[0..nl-1] (finest first): cor[0] = lower-V(res[0]); mirrors the single-block bottom
// solver of the reference (HpMultiGrid.cpp:854-1033), 16+ sweeps on the last level.  Level 0's
// coefficient and residual come from HBM (acf_g, res_g), its correction goes back (cor_g); the
// coefficients of the lower levels are re-derived in LDS (average_down_acoef).
template <bool CC>
__global__ __launch_bounds__(1024)
void k_lower_v (const LowLev* __restrict__ lv, int nl, const double* __restrict__ acf_g, const double* __restrict__ res_g,
                double* __restrict__ cor_g, double facx0, double facy0, int nsweeps_bottom, StopRule sr, FView fine_res = FView{})
{
    if (!vcycle_active(sr)) return;
    extern __shared__ __attribute__((aligned(16))) double lds_raw[];
    lds_double* base = (lds_double*)lds_raw;
    // grid = 2 on node-centred grids (round 6): one field component per workgroup -- the components only meet in norms this
    // kernel does not take, so two CUs need no synchronisation and every barrier-separated phase carries half the LDS traffic
    // (Bx/By solve at 1023^2 375 -> 361 us per slice; 512 threads the same, 256 slower: profiles/r06_lowv_ab.txt)
    const int n0 = gridDim.x == 2 ? (int)blockIdx.x : 0, n1 = gridDim.x == 2 ? n0 + 1 : 2;
    MG_STAMP(8);
    {   // every plane of every level starts from zero (walls, corrections, the coefficient planes' rims)
        const LowLev last = lv[nl - 1];
        const int total = last.off + 8*last.cells;
        for (int s = threadIdx.x; s < total; s += blockDim.x) base[s] = 0.0;
        __syncthreads();
    }
    {
        const LowLev l = lv[0];
        if (fine_res.p) {
            // the top level's right-hand side = R(residual of the level above), formed here (no k_restrict launch ahead of this
            // kernel); cells outside the unknowns' box read as 0
            for (int s = threadIdx.x; s < l.cells; s += blockDim.x) base[l.off + s] = acf_g[s];
            HPS_LOW_FOR_VALID(l, i, j) {
                for (int n = n0; n < n1; ++n) lplane(base, l, 1 + n)(i, j) = restrict_at<CC>(fine_res, i, j, n);
            }
        } else
        for (int s = threadIdx.x; s < l.cells; s += blockDim.x) {
            base[l.off + s] = acf_g[s];
            base[l.off + l.cells + s] = res_g[s];
            base[l.off + 2*l.cells + s] = res_g[l.cells + s];
        }
        __syncthreads();
    }
    // (every level's descriptor is copied out of global memory ONCE per use below: handed on as a reference to lv[il] itself, each
    //  phase behind a barrier began with three to four dependent scalar loads of its fields -- a third of a phase's ~900 clocks)
    // coefficient hierarchy and inverse diagonals (one division per point and V-cycle)
    for (int il = 1; il < nl; ++il) { const LowLev f = lv[il - 1], c = lv[il]; low_hier_level<CC>(base, f, c); }
    MG_STAMP(9);
    for (int il = 0; il < nl; ++il) { const LowLev l = lv[il]; low_cinv_level<CC>(base, l, low_fac(facx0, il), low_fac(facy0, il)); }
    __syncthreads();
    MG_STAMP(10);
    for (int il = 0; il < nl - 1; ++il) { const LowLev l = lv[il], c = lv[il + 1]; low_down_level<CC>(base, l, c, low_fac(facx0, il), low_fac(facy0, il), n0, n1); }
    MG_STAMP(11);
    {
        const LowLev l = lv[nl - 1];
        if (l.b.vhx - l.b.vlx < 3 && l.b.vhy - l.b.vly < 3)
            low_bottom_lane<CC>(base, l, low_fac(facx0, nl - 1), low_fac(facy0, nl - 1), nsweeps_bottom, n0, n1);
        else
        low_sweeps<CC>(base, l, low_fac(facx0, nl - 1), low_fac(facy0, nl - 1), nsweeps_bottom, n0, n1);
    }
    MG_STAMP(12);
    for (int il = nl - 2; il >= 0; --il) { const LowLev l = lv[il], c = lv[il + 1]; low_up_level<CC>(base, l, c, low_fac(facx0, il), low_fac(facy0, il), n0, n1); }
    MG_STAMP(13);
    {
        const LowLev l = lv[0];
        for (int s = n0*l.cells + threadIdx.x; s < n1*l.cells; s += blockDim.x) cor_g[s] = base[l.off + 3*l.cells + s];
    }
    MG_STAMP(14);
}

// ---------------------------------------------------------------------------------------------
// Cell-centred lower V (k_lower_v3), register/LDS resident, from the first level with at most 64 x 64 cells, ONE field
// component per workgroup (grid = 2).  The two components of the solve only meet in the norm, which the lower V does not
// take, so two workgroups on two CUs need no synchronisation at all, and every barrier phase of the 64 x 64 and 32 x 32
// levels carries half the LDS traffic and half the fp64 instruction stream of one workgroup for both (one CU's LDS pipe and
// VALUs were what bounded those phases: ~1800 cycles per half-sweep).
// Every level is worked in 2 x 2 cell blocks, one thread per block: the block's correction, rhs and inverse diagonal sit in
// registers, so a red-black half-sweep updates two cells with two LDS reads each (the other two neighbours are the thread's
// own cells), the residual's 4-average for the restriction and the piecewise-constant prolongation are thread-local, and
// the 2 x 2 bottom level is one lane's registers.  LDS per level: level A one ringed plane (cor); below it four: cor | res |
// acf | 1/diag (level A keeps its rhs in registers).  Levels of at most 64 blocks run in wave 0 alone without workgroup
// barriers.  The first sweep of every down-leg level starts from cor = 0, where the update is rhs/diag exactly.
// Level A's inverse diagonals come from k_acf_pyramid (cinv_g: 4 divisions per thread and V-cycle less).  The gate of
// the speculative V-cycle is evaluated AFTER the level-A loads have been issued: a kernel's first dependent read of
// global memory costs ~1.5 us behind a kernel boundary (scripts/ubench/launch_floor.hip), and the two now overlap.
constexpr int LOW2_MAXLEV = 8;
struct Low2 { int nl; int total; int nx[LOW2_MAXLEV], ny[LOW2_MAXLEV], off[LOW2_MAXLEV];
              int coff[LOW2_MAXLEV], cbase, ctot; };      // the levels' [acf | 1/diag] planes, one contiguous image from cbase

__device__ __forceinline__ LevBox cc_box (int nx, int ny) { return LevBox{0, 0, nx - 1, ny - 1, 0, 0, nx - 1, ny - 1}; }

template <bool WAVE>
__device__ __forceinline__ void lvl_sync ()
{
    // one wave: its DS instructions reach the LDS in program order, so a read issued behind a write sees it without the
    // wave waiting for the write to retire -- only the compiler has to be kept in order (the s_waitcnt that stood here
    // stalled every one of the ~60 phases of the one-wave levels for the write's round trip)
    if (WAVE) asm volatile("" ::: "memory");
    else __syncthreads();
}

// a thread's 2 x 2 block: cells k = 0:(i,j) 1:(i+1,j) 2:(i,j+1) 3:(i+1,j+1); 0 and 3 have colour 0
struct Blk {
    lds_double* c0;           // the block's cell 0 in the correction plane
    int pitch;
    bool act;                 // this thread has a block on this level
    bool ok[4];               // cell inside the level (odd sizes)
    double fxm[2], fym[2];    // wall multipliers of the block's two columns / rows
    double v0[4];             // correction
    double r0[4], ci[4];
};

// half-sweep of parity P (0: cells 0 and 3, 1: cells 1 and 2) + publication of the new values
template <int P, bool WAVE>
__device__ __forceinline__ void blk_sweep (Blk& B)
{
    if (B.act) {
        const int pt = B.pitch;
        if (P == 0) {
            {   const double w0 = B.c0[-1], s0 = B.c0[-pt];
                const double n0 = (B.r0[0] - (B.fxm[0]*(w0 + B.v0[1]) + B.fym[0]*(s0 + B.v0[2])))*B.ci[0];
                if (B.ok[0]) { B.v0[0] = n0; B.c0[0] = n0; } }
            {   const double e0 = B.c0[pt + 2], t0 = B.c0[2*pt + 1];
                const double n0 = (B.r0[3] - (B.fxm[1]*(B.v0[2] + e0) + B.fym[1]*(B.v0[1] + t0)))*B.ci[3];
                if (B.ok[3]) { B.v0[3] = n0; B.c0[pt + 1] = n0; } }
        } else {
            {   const double e0 = B.c0[2], s0 = B.c0[1 - pt];
                const double n0 = (B.r0[1] - (B.fxm[1]*(B.v0[0] + e0) + B.fym[0]*(s0 + B.v0[3])))*B.ci[1];
                if (B.ok[1]) { B.v0[1] = n0; B.c0[1] = n0; } }
            {   const double w0 = B.c0[pt - 1], t0 = B.c0[2*pt];
                const double n0 = (B.r0[2] - (B.fxm[0]*(w0 + B.v0[3]) + B.fym[1]*(B.v0[0] + t0)))*B.ci[2];
                if (B.ok[2]) { B.v0[2] = n0; B.c0[pt] = n0; } }
        }
    }
    lvl_sync<WAVE>();
}

// down-leg sweeps from cor = 0: sweep 0 is rhs/diag on the colour-0 cells, then sweeps 1 .. nsw-1 (nsw even)
template <bool WAVE>
__device__ __forceinline__ void blk_down_sweeps (Blk& B, int nsw)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) B.v0[k] = 0.0;
    if (B.act) {
        if (B.ok[0]) { B.v0[0] = B.r0[0]*B.ci[0]; B.c0[0] = B.v0[0]; }
        if (B.ok[3]) { B.v0[3] = B.r0[3]*B.ci[3]; B.c0[B.pitch + 1] = B.v0[3]; }
    }
    lvl_sync<WAVE>();
    blk_sweep<1, WAVE>(B);
    for (int s = 2; s < nsw; s += 2) { blk_sweep<0, WAVE>(B); blk_sweep<1, WAVE>(B); }
}

// The whole level is this one block (2 x 2 cells or fewer): every neighbour outside the block is the
// zero ring, so all nsw sweeps from cor = 0 run in the lane's registers; published once at the end.
__device__ __forceinline__ void blk_single_sweeps (Blk& B, int nsw)
{
    // (every neighbour outside the block is the zero ring: 0 + v == v exactly, so the sums with it are left out -- this is a
    //  chain of 2 nsw dependent half-sweeps in one lane, every instruction of it is on the V-cycle's critical path)
#pragma unroll
    for (int k = 0; k < 4; ++k) B.v0[k] = 0.0;
    if (B.act) {
        for (int s = 0; s < nsw; s += 2) {
            {   const double a0 = (B.r0[0] - (B.fxm[0]*B.v0[1] + B.fym[0]*B.v0[2]))*B.ci[0];
                const double b0 = (B.r0[3] - (B.fxm[1]*B.v0[2] + B.fym[1]*B.v0[1]))*B.ci[3];
                if (B.ok[0]) B.v0[0] = a0;
                if (B.ok[3]) B.v0[3] = b0; }
            {   const double a0 = (B.r0[1] - (B.fxm[1]*B.v0[0] + B.fym[0]*B.v0[3]))*B.ci[1];
                const double b0 = (B.r0[2] - (B.fxm[0]*B.v0[3] + B.fym[1]*B.v0[0]))*B.ci[2];
                if (B.ok[1]) B.v0[1] = a0;
                if (B.ok[2]) B.v0[2] = b0; }
        }
        const int ok[4] = {0, 1, B.pitch, B.pitch + 1};
#pragma unroll
        for (int k = 0; k < 4; ++k) if (B.ok[k]) B.c0[ok[k]] = B.v0[k];
    }
}

// residuals of the block's four cells (0 for cells outside the level)
__device__ __forceinline__ void blk_residual (const Blk& B, int i, int j, const LevBox& b, const double (&a)[4],
                                              double fx, double fy, double (&q0)[4])
{
    const int pt = B.pitch;
    const double w00 = B.c0[-1], s00 = B.c0[-pt], e01 = B.c0[2], s01 = B.c0[1 - pt];
    const double w02 = B.c0[pt - 1], n02 = B.c0[2*pt], e03 = B.c0[pt + 2], n03 = B.c0[2*pt + 1];
    q0[0] = residual_v<false>(B.v0[0], w00, B.v0[1], s00, B.v0[2], i, j, b, B.r0[0], a[0], fx, fy);
    q0[1] = residual_v<false>(B.v0[1], B.v0[0], e01, s01, B.v0[3], i + 1, j, b, B.r0[1], a[1], fx, fy);
    q0[2] = residual_v<false>(B.v0[2], w02, B.v0[3], B.v0[0], n02, i, j + 1, b, B.r0[2], a[2], fx, fy);
    q0[3] = residual_v<false>(B.v0[3], B.v0[2], e03, B.v0[1], n03, i + 1, j + 1, b, B.r0[3], a[3], fx, fy);
#pragma unroll
    for (int k = 0; k < 4; ++k) if (!B.ok[k]) q0[k] = 0.0;
}

// geometry of thread t's block on a level of nx x ny cells whose plane starts at `lev` (pitch nx + 2)
__device__ __forceinline__ void blk_geometry (Blk& B, lds_double* lev, int nx, int ny, int t, double fx, double fy, int& i, int& j)
{
    const int nbx = (nx + 1) >> 1, nby = (ny + 1) >> 1;
    const int lg = (nbx <= 1) ? 0 : 32 - __clz(nbx - 1);       // blocks per row rounded up to a power of two
    const int bi = t & ((1 << lg) - 1), bj = t >> lg;
    B.act = (bi < nbx) && (bj < nby);
    i = 2*bi; j = 2*bj;
    B.pitch = nx + 2;
    const int o = B.act ? (j + 1)*B.pitch + i + 1 : B.pitch + 1;
    B.c0 = lev + o;
    B.ok[0] = B.act; B.ok[1] = B.act && (i + 1 < nx); B.ok[2] = B.act && (j + 1 < ny); B.ok[3] = B.ok[1] && B.ok[2];
    B.fxm[0] = wall_mult<true>(i, 0, nx - 1, fx); B.fxm[1] = wall_mult<true>(i + 1, 0, nx - 1, fx);
    B.fym[0] = wall_mult<true>(j, 0, ny - 1, fy); B.fym[1] = wall_mult<true>(j + 1, 0, ny - 1, fy);
}

__device__ __forceinline__ double lvl_fac (double f0, int l) { for (int k = 0; k < l; ++k) f0 *= 0.25; return f0; }

template <bool WAVE>
__device__ __forceinline__ void low_down_s (lds_double* base, const Low2& d, int l, int t, double fx, double fy, int nsw, bool last)
{
    const int nx = d.nx[l], ny = d.ny[l];
    Blk B; int i, j;
    blk_geometry(B, base + d.off[l], nx, ny, t, fx, fy, i, j);
    const int ps = B.pitch*(ny + 2);
    const lds_double* r = B.c0 + ps;
    const lds_double* cf = base + d.coff[l] + (B.c0 - (base + d.off[l]));      // the block's cell 0 in the acf plane
    const int ok[4] = {0, 1, B.pitch, B.pitch + 1};
    double a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int o = B.ok[k] ? ok[k] : 0;
        B.r0[k] = r[o]; a[k] = cf[o]; B.ci[k] = cf[ps + o];
    }
    if (last && nx <= 2 && ny <= 2) { blk_single_sweeps(B, nsw); lvl_sync<WAVE>(); }
    else blk_down_sweeps<WAVE>(B, nsw);
    if (!last) {
        double q0[4];
        blk_residual(B, i, j, cc_box(nx, ny), a, fx, fy, q0);
        if (B.act) {
            const int pn = d.nx[l+1] + 2, psn = pn*(d.ny[l+1] + 2);
            base[d.off[l+1] + psn + ((j >> 1) + 1)*pn + (i >> 1) + 1] = 0.25*(q0[0] + q0[1] + q0[2] + q0[3]);
        }
        lvl_sync<WAVE>();
    }
}

template <bool WAVE>
__device__ __forceinline__ void low_up_s (lds_double* base, const Low2& d, int l, int t, double fx, double fy)
{
    const int nx = d.nx[l], ny = d.ny[l];
    Blk B; int i, j;
    blk_geometry(B, base + d.off[l], nx, ny, t, fx, fy, i, j);
    const int ps = B.pitch*(ny + 2);
    const lds_double* r = B.c0 + ps;
    const lds_double* cf = base + d.coff[l] + (B.c0 - (base + d.off[l]));
    const int ok[4] = {0, 1, B.pitch, B.pitch + 1};
    const int pn = d.nx[l+1] + 2;
    const lds_double* kc = base + d.off[l+1] + ((j >> 1) + 1)*pn + (i >> 1) + 1;
    const double k0 = B.act ? kc[0] : 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int o = B.ok[k] ? ok[k] : 0;
        B.r0[k] = r[o]; B.ci[k] = cf[ps + o];
        const double c0 = B.c0[o];
        B.v0[k] = B.ok[k] ? c0 + k0 : 0.0;
        if (B.ok[k]) B.c0[o] = B.v0[k];
    }
    lvl_sync<WAVE>();
    blk_sweep<0, WAVE>(B); blk_sweep<1, WAVE>(B); blk_sweep<0, WAVE>(B); blk_sweep<1, WAVE>(B);
}

// levels of at most 8 x 8 cells in one wave, one lane per cell
__device__ __forceinline__ void tiny_down_s (lds_double* base, const Low2& d, int l, int t, double fx, double fy)
{
    const int nx = d.nx[l], ny = d.ny[l], pitch = nx + 2, ps = pitch*(ny + 2);
    const int i = t & 7, j = t >> 3;
    const bool ok = (i < nx) && (j < ny);
    const int o = ok ? (j + 1)*pitch + i + 1 : pitch + 1;
    lds_double* c0 = base + d.off[l] + o;
    const lds_double* cf = base + d.coff[l] + o;
    const double r0 = c0[ps], a = cf[0], ci = cf[ps];
    const double fxm = wall_mult<true>(i, 0, nx - 1, fx), fym = wall_mult<true>(j, 0, ny - 1, fy);
    if (ok && (((i + j) & 1) == 0)) c0[0] = r0*ci;                          // sweep 0 from cor = 0
    lvl_sync<true>();
    for (int s = 1; s < 4; ++s) {
        if (ok && (((i + j + s) & 1) == 0)) c0[0] = (r0 - offdiag_m((const lds_double*)c0, pitch, fxm, fym))*ci;
        lvl_sync<true>();
    }
    const LevBox b = cc_box(nx, ny);
    const double u0 = residual_at<false>((const lds_double*)c0, pitch, i, j, b, r0, a, fx, fy);
    const double q0 = ok ? u0 : 0.0;
    const double b0 = __shfl_down(q0, 1), g0 = __shfl_down(q0, 8), e0 = __shfl_down(q0, 9);
    if (ok && !(i & 1) && !(j & 1)) {
        const int pn = d.nx[l+1] + 2, psn = pn*(d.ny[l+1] + 2);
        base[d.off[l+1] + psn + ((j >> 1) + 1)*pn + (i >> 1) + 1] = 0.25*(q0 + b0 + g0 + e0);
    }
    lvl_sync<true>();
}

__device__ __forceinline__ void tiny_up_s (lds_double* base, const Low2& d, int l, int t, double fx, double fy)
{
    const int nx = d.nx[l], ny = d.ny[l], pitch = nx + 2, ps = pitch*(ny + 2);
    const int i = t & 7, j = t >> 3;
    const bool ok = (i < nx) && (j < ny);
    const int o = ok ? (j + 1)*pitch + i + 1 : pitch + 1;
    lds_double* c0 = base + d.off[l] + o;
    const double r0 = c0[ps], ci = base[d.coff[l] + ps + o];
    const double fxm = wall_mult<true>(i, 0, nx - 1, fx), fym = wall_mult<true>(j, 0, ny - 1, fy);
    if (ok) {
        const int pn = d.nx[l+1] + 2;
        c0[0] = c0[0] + base[d.off[l+1] + ((j >> 1) + 1)*pn + (i >> 1) + 1];
    }
    lvl_sync<true>();
    for (int s = 0; s < 4; ++s) {
        if (ok && (((i + j + s) & 1) == 0)) c0[0] = (r0 - offdiag_m((const lds_double*)c0, pitch, fxm, fym))*ci;
        lvl_sync<true>();
    }
}

// Guests of the lower V (the engine's HPS_EARLY_INIT): workgroups 2 .. of the first V-cycle's launch run the slab's shift /
// zero pass for the next slice on the compute units the two solver workgroups leave idle.  They share nothing with the
// solver workgroups and do not read the stop rule.
__device__ __forceinline__ void lower_v_guest (const ShiftInit& a, int guest, int nguests)
{
    for (long s = (long)guest*1024 + threadIdx.x; s < a.plane; s += (long)nguests*1024) shift_init_cell(a, s);
}

// Guest of a solve's initial level-0 pass (k_smooth's GUEST): the [acf | 1/diag] image of the levels below k_lower_v3's top
// level A, which depends on level A's coefficient plane only (the pyramid's, a whole launch earlier in the stream) -- derived
// here, beside the pass's tiles, the first lower V of the solve does not derive it on the V-cycle's critical path.  Cell for
// cell the expressions of k_lower_v3's own derivation (which grids without this guest keep), block by block as there; the
// image is staged in the host kernel's static LDS (s_img, nt threads) and left in g.img, where every lower V copies it in.
struct CoefGuest { const Low2* low; const double* acfA; double* img; double facx0, facy0; };

__device__ void coef_guest_derive (double* s_img, const CoefGuest& g, int nt)
{
    lds_double* img = (lds_double*)s_img;
    const Low2& d = *g.low;
    const int t = threadIdx.x;
    const int nl = d.nl, ctot = d.ctot, cbase = d.cbase;
    for (int q = t; q < ctot; q += nt) img[q] = 0.0;       // (the rings: never read, but the image is the same every time)
    __syncthreads();
    if (nl > 1) {
        const int nxA = d.nx[0], nyA = d.ny[0], nbx = (nxA + 1) >> 1, nby = (nyA + 1) >> 1, p1 = d.nx[1] + 2;
        for (int q = t; q < nbx*nby; q += nt) {
            const int bj = q / nbx, i = 2*(q - bj*nbx), j = 2*bj;
            double a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ik = i + (k & 1), jk = j + (k >> 1);
                const double v = g.acfA[min(ik, nxA - 1) + min(jk, nyA - 1)*nxA];
                a[k] = (ik < nxA && jk < nyA) ? v : 0.0;
            }
            img[d.coff[1] - cbase + ((j >> 1) + 1)*p1 + (i >> 1) + 1] = 0.25*(a[0] + a[1] + a[2] + a[3]);
        }
    }
    __syncthreads();
    for (int l = 1; l < nl; ++l) {
        const double fx = lvl_fac(g.facx0, l), fy = lvl_fac(g.facy0, l);
        const int nx = d.nx[l], ny = d.ny[l], nbx = (nx + 1) >> 1, nby = (ny + 1) >> 1, pitch = nx + 2, ps = pitch*(ny + 2);
        lds_double* lev = img + (d.coff[l] - cbase);
        const int ok[4] = {0, 1, pitch, pitch + 1};
        for (int q = t; q < nbx*nby; q += nt) {
            const int bj = q / nbx, i = 2*(q - bj*nbx), j = 2*bj;
            lds_double* acf = lev + (j + 1)*pitch + i + 1;
            const bool in[4] = {true, i + 1 < nx, j + 1 < ny, i + 1 < nx && j + 1 < ny};
            double a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = in[k] ? acf[ok[k]] : 0.0;
            if (l + 1 < nl) {
                const int pn = d.nx[l+1] + 2;
                img[d.coff[l+1] - cbase + ((j >> 1) + 1)*pn + (i >> 1) + 1] = 0.25*(a[0] + a[1] + a[2] + a[3]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (in[k]) acf[ps + ok[k]] = 1.0/diag_c0<true>(i + (k & 1), j + (k >> 1), cc_box(nx, ny), a[k], fx, fy);
        }
        __syncthreads();
    }
    for (int q = t; q < ctot; q += nt) g.img[q] = img[q];
}

__global__ __launch_bounds__(1024)
void k_lower_v3 (const Low2* __restrict__ dp, const double* __restrict__ acf_g, const double* __restrict__ cinv_g,
                 const double* __restrict__ res_g, double* __restrict__ cor_g, double* __restrict__ coef_g, int nxA, int nyA, int ctot,
                 double facx0, double facy0, int nsweeps_bottom, StopRule sr, ShiftInit guest, int derive_first)
{
    if (blockIdx.x >= 2) { lower_v_guest(guest, (int)blockIdx.x - 2, (int)gridDim.x - 2); return; }
    extern __shared__ __attribute__((aligned(16))) double lds_raw[];
    lds_double* base = (lds_double*)lds_raw;
    const int t = threadIdx.x;
    const Low2& d = *dp;          // (level A's size and the image's length come by value: the first loads must not wait for this read)
    const int nl = d.nl;
    const int cellsA = nxA*nyA;
    res_g += (long)blockIdx.x*cellsA; cor_g += (long)blockIdx.x*cellsA;      // this workgroup's component
    const LevBox bA = cc_box(nxA, nyA);
    Blk A; int iA, jA;
    blk_geometry(A, base, nxA, nyA, t, facx0, facy0, iA, jA);       // (d.off[0] = 0)
    // ---- level A: rhs, coefficient and inverse diagonal of the thread's block from HBM, issued before the gate is read
    double aA[4], rA[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = iA + (k & 1), j = jA + (k >> 1);
        const int g = min(i, nxA - 1) + min(j, nyA - 1)*nxA;
        const double v0 = res_g[g], v2 = acf_g[g], v3 = cinv_g[g];
        rA[k] = A.ok[k] ? v0 : 0.0; aA[k] = A.ok[k] ? v2 : 0.0; A.ci[k] = A.ok[k] ? v3 : 0.0;
        A.r0[k] = rA[k];
    }
    // The [acf | 1/diag] planes of the levels below A depend on the coefficient only: the guest of the solve's initial level-0
    // pass has left their image in coef_g (coef_guest_derive) and every V-cycle copies it in.  derive_first (grids whose
    // initial pass cannot host the guest, HPS_MG_COEF_GUEST=0): the first V-cycle of a solve derives them here
    // (average_down_acoef + one division per cell) and leaves the image in coef_g for the later ones.
    const bool derive = derive_first && (sr.k <= 0);
    constexpr int NIMG = 4;      // image words per thread (LOW2 levels below 64 x 64: 3264 doubles)
    double img[NIMG];
#pragma unroll
    for (int m = 0; m < NIMG; ++m) { const int q = min(t + 1024*m, ctot - 1); img[m] = derive ? 0.0 : coef_g[q]; }
    const bool active = vcycle_active(sr);
#pragma unroll
    for (int k = 0; k < 4; ++k) { HPS_KEEP(rA[k]); HPS_KEEP(aA[k]); HPS_KEEP(A.ci[k]); }
#pragma unroll
    for (int m = 0; m < NIMG; ++m) HPS_KEEP(img[m]);
    if (!active) return;
    MG_STAMP(8);
    // only the correction planes need zeros (ring + the cells of the colour the first half-sweep skips)
    for (int l = 0; l < nl; ++l) {
        const int n1 = (d.nx[l] + 2)*(d.ny[l] + 2);
        lds_double* c = base + d.off[l];
        for (int s = t; s < n1; s += 1024) c[s] = 0.0;
    }
    if (!derive) {
#pragma unroll
        for (int m = 0; m < NIMG; ++m) if (t + 1024*m < ctot) base[d.cbase + t + 1024*m] = img[m];
        for (int q = t + 1024*NIMG; q < ctot; q += 1024) base[d.cbase + q] = coef_g[q];      // (larger level sets)
    }
    __syncthreads();
    if (derive) {
        // ---- coefficient hierarchy (average_down_acoef) and inverse diagonals of the levels below
        if (nl > 1 && A.act) {
            const int p1 = d.nx[1] + 2;
            base[d.coff[1] + ((jA >> 1) + 1)*p1 + (iA >> 1) + 1] = 0.25*(aA[0] + aA[1] + aA[2] + aA[3]);
        }
        __syncthreads();
        for (int l = 1; l < nl; ++l) {
            const double fx = lvl_fac(facx0, l), fy = lvl_fac(facy0, l);
            const int nx = d.nx[l], ny = d.ny[l];
            Blk B; int i, j;
            blk_geometry(B, base + d.coff[l], nx, ny, t, fx, fy, i, j);     // c0 = the block's cell 0 in the acf plane
            const int ps = B.pitch*(ny + 2);
            lds_double* acf = B.c0;
            const int ok[4] = {0, 1, B.pitch, B.pitch + 1};
            if (B.act) {          // (whole waves have no block on the small levels: they skip the divisions)
                double a[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) a[k] = B.ok[k] ? acf[ok[k]] : 0.0;
                if (l + 1 < nl) {     // the next level's coefficient first: the divisions below are off the critical path
                    const int pn = d.nx[l+1] + 2;
                    base[d.coff[l+1] + ((j >> 1) + 1)*pn + (i >> 1) + 1] = 0.25*(a[0] + a[1] + a[2] + a[3]);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (B.ok[k]) acf[ps + ok[k]] = 1.0/diag_c0<true>(i + (k & 1), j + (k >> 1), cc_box(nx, ny), a[k], fx, fy);
            }
            __syncthreads();
        }
        if (blockIdx.x == 0) for (int q = t; q < ctot; q += 1024) coef_g[q] = base[d.cbase + q];
    }
    MG_STAMP(9);
    // ---- level A down-leg
    const bool bottomA = (nl == 1);
    blk_down_sweeps<false>(A, bottomA ? nsweeps_bottom : 4);
    if (!bottomA) {
        double q0[4];
        blk_residual(A, iA, jA, bA, aA, facx0, facy0, q0);
        if (A.act) {
            const int p1 = d.nx[1] + 2, ps1 = p1*(d.ny[1] + 2);
            base[d.off[1] + ps1 + ((jA >> 1) + 1)*p1 + (iA >> 1) + 1] = 0.25*(q0[0] + q0[1] + q0[2] + q0[3]);
        }
        __syncthreads();
    }
    MG_STAMP(10);
    if (!bottomA) {
        // lw = first level whose blocks (and those of every level below it) fit wave 0
        int lw = 1;
        for (; lw < nl; ++lw) {
            const int nbx = (d.nx[lw] + 1) >> 1, nby = (d.ny[lw] + 1) >> 1;
            int lg = 0; while ((1 << lg) < nbx) ++lg;
            if ((nby << lg) <= 64) break;
        }
        for (int l = 1; l < lw; ++l)
            low_down_s<false>(base, d, l, t, lvl_fac(facx0, l), lvl_fac(facy0, l), (l == nl - 1) ? nsweeps_bottom : 4, l == nl - 1);
        MG_STAMP(11);
        if (lw < nl) {
            if (t < 64) {
                for (int l = lw; l < nl; ++l) {
                    MG_STAMP(16 + l);
                    const bool tiny = (d.nx[l] <= 8 && d.ny[l] <= 8 && l < nl - 1);
                    if (tiny) tiny_down_s(base, d, l, t, lvl_fac(facx0, l), lvl_fac(facy0, l));
                    else low_down_s<true>(base, d, l, t, lvl_fac(facx0, l), lvl_fac(facy0, l), (l == nl - 1) ? nsweeps_bottom : 4, l == nl - 1);
                }
                for (int l = nl - 2; l >= lw; --l) {
                    MG_STAMP(32 + l);
                    if (d.nx[l] <= 8 && d.ny[l] <= 8) tiny_up_s(base, d, l, t, lvl_fac(facx0, l), lvl_fac(facy0, l));
                    else low_up_s<true>(base, d, l, t, lvl_fac(facx0, l), lvl_fac(facy0, l));
                }
            }
            __syncthreads();
        }
        MG_STAMP(12);
        for (int l = min(lw - 1, nl - 2); l >= 1; --l)
            low_up_s<false>(base, d, l, t, lvl_fac(facx0, l), lvl_fac(facy0, l));
        // ---- level A up-leg: correction back from LDS, prolongation, 4 sweeps
        const int p1 = d.nx[1] + 2;
        const lds_double* kc = base + d.off[1] + ((jA >> 1) + 1)*p1 + (iA >> 1) + 1;
        const double k0 = A.act ? kc[0] : 0.0;
        const int ok[4] = {0, 1, A.pitch, A.pitch + 1};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int o = A.ok[k] ? ok[k] : 0;
            const double c0 = A.c0[o];
            A.v0[k] = A.ok[k] ? c0 + k0 : 0.0;
            if (A.ok[k]) A.c0[o] = A.v0[k];
            A.r0[k] = rA[k];
        }
        __syncthreads();
        blk_sweep<0, false>(A); blk_sweep<1, false>(A); blk_sweep<0, false>(A); blk_sweep<1, false>(A);
    }
    MG_STAMP(13);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int g = min(iA + (k & 1), nxA - 1) + min(jA + (k >> 1), nyA - 1)*nxA;
        if (A.ok[k]) cor_g[g] = A.v0[k];
    }
    MG_STAMP(14);
}

// Coefficient pyramid, cell-centred (average_down_acoef, HpMultiGrid.cpp:1640-1700): one launch
// derives levels 1..nlev_out from level 0.  A workgroup owns a 32 x 32 block of level-0 cells;
// thread t holds the level-1 cell (t & 15, t >> 4) of the block and levels 2.. go through LDS.
// The nested 0.25*(((a+b)+c)+d) order of restrict_cc is kept at every level.
struct PyrOut { double* p[5]; int nx[5], ny[5];      // levels 1..5, row pitch = nx
                double* cinv; int cinv_l; double cfx, cfy; };      // inverse diagonals of level 1 + cinv_l (k_lower_v3's level A), or null

__device__ __forceinline__ void acf_pyramid_block (const FView& acf0, int nx0, int ny0, const PyrOut& out, int nlev_out, unsigned long long* zero, int nzero,
                                                   int bx, int by)
{
    // the first launch of a solve: it also clears the norm slots (saves a memset launch)
    if (bx == 0 && by == 0) for (int q = threadIdx.x; q < nzero; q += 256) zero[q] = 0ULL;
    __shared__ double s_a[2][16*16];
    const int t = threadIdx.x;
    const int bi = bx*32, bj = by*32;       // level-0 origin of the block
    int li = t & 15, lj = t >> 4;
    double v = 0.0;
    {
        const int i = bi + 2*li, j = bj + 2*lj;
        if (i + 1 < nx0 && j + 1 < ny0) v = 0.25*(acf0(i, j, 0) + acf0(i+1, j, 0) + acf0(i, j+1, 0) + acf0(i+1, j+1, 0));
        const int ic = (bi >> 1) + li, jc = (bj >> 1) + lj;
        if (ic < out.nx[0] && jc < out.ny[0]) {
            out.p[0][ic + (long)jc*out.nx[0]] = v;
            if (out.cinv && out.cinv_l == 0) out.cinv[ic + (long)jc*out.nx[0]] = 1.0/diag_c0<true>(ic, jc, cc_box(out.nx[0], out.ny[0]), v, out.cfx, out.cfy);
        }
        s_a[0][t] = v;
    }
    int n = 16, cur = 0;
    for (int l = 1; l < nlev_out; ++l) {
        __syncthreads();
        n >>= 1;
        if (t < n*n) {
            li = t % n; lj = t / n;
            const double* f = s_a[cur];
            const int w = 2*n;
            v = 0.25*(f[2*li + 2*lj*w] + f[2*li + 1 + 2*lj*w] + f[2*li + (2*lj + 1)*w] + f[2*li + 1 + (2*lj + 1)*w]);
            const int ic = (bi >> (l + 1)) + li, jc = (bj >> (l + 1)) + lj;
            if (ic < out.nx[l] && jc < out.ny[l]) {
                out.p[l][ic + (long)jc*out.nx[l]] = v;
                if (out.cinv && out.cinv_l == l) out.cinv[ic + (long)jc*out.nx[l]] = 1.0/diag_c0<true>(ic, jc, cc_box(out.nx[l], out.ny[l]), v, out.cfx, out.cfy);
            }
            s_a[cur ^ 1][t] = v;
        }
        cur ^= 1;
    }
}

__global__ __launch_bounds__(256)
void k_acf_pyramid (FView acf0, int nx0, int ny0, PyrOut out, int nlev_out, unsigned long long* zero, int nzero)
{
    acf_pyramid_block(acf0, nx0, ny0, out, nlev_out, zero, nzero, (int)blockIdx.x, (int)blockIdx.y);
}

// the pyramid's blocks (the first gx*gy workgroups) and, behind them, a pass of the engine's slab that is due at the same point of
// a slice: -grad Psi and the Sx / Sy initialisation (slab_ops.h), 256 cells of a padded row per workgroup -- the coefficient
// hierarchy costs the slice no launch of its own
__global__ __launch_bounds__(256)
void k_hierarchy_gradpsi (FView acf0, int nx0, int ny0, PyrOut out, int nlev_out, unsigned long long* zero, int nzero, int gx, int gy,
                          SlabView f, GradPsiSxSy ga, int nbx)
{
    const int b = (int)blockIdx.x;
    if (b < gx*gy) { acf_pyramid_block(acf0, nx0, ny0, out, nlev_out, zero, nzero, b % gx, b / gx); return; }
    const int q = b - gx*gy;
    const int row = q / nbx, bxs = q - row*nbx;
    gradpsi_sxsy_cell(f, ga, bxs*256 + (int)threadIdx.x - f.ng, row - f.ng);
}

// ---- node-centred coefficient hierarchy in one launch (round 6) ------------------------------------------------------------
// average_down_acoef on the 2^K - 1 grids (HpMultiGrid.cpp:1640-1700 with the 9-point full weighting of the nodal levels) was one
// k_restrict launch per level: five dependent 5-us launches per solve at 1023^2 (26 us of the slice).  Here a workgroup owns
// NB x NB nodes of the coarsest level wanted (level np) and everything below them: with s = np - l, level l's nodes
// [T0 2^s, (T0 + NB) 2^s) are its to write, and it needs [T0 2^s - c_l, (T0 + NB) 2^s) with c_l = 2^s - 1 of them (the 3 x 3
// stencils of the nodes above reach one node further down-left per level): a (NB 2^np + 2^np - 1)^2 window of level 0 goes to
// LDS (95^2 for np = 5, NB = 2: 2.2 x the plane's 8 MB, once), every level is formed there with the same expression and
// operand order as restrict_at<false> -- the nodes outside a level's unknowns are never needed by a coarser unknown -- and
// the owned unknowns go to their level's plane.  Fine window index of node 2i - 1 is 2 (i - lo_l): no index arithmetic.
constexpr int NPYR_MAX = 5, NPYR_NB = 2;
struct NodalPyr { FView lev[NPYR_MAX]; int vhx[NPYR_MAX + 1], vhy[NPYR_MAX + 1]; int np; };      // vh*[l]: last unknown of level l (first: 1)

template <int NP>       // (compile-time level count: the window widths are constants, the index divisions multiplications)
__global__ __launch_bounds__(256)
void k_nodal_acf_pyramid (FView f0, NodalPyr o, unsigned long long* zero, int nzero)
{
    extern __shared__ double npyr_lds[];
    constexpr int np = NP;
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && blockIdx.y == 0) for (int w = tid; w < nzero; w += 256) zero[w] = 0ULL;      // the solve's norm slots
    const int T0x = blockIdx.x*NPYR_NB, T0y = blockIdx.y*NPYR_NB;
    // level 0 window
    int w = NPYR_NB*(1 << np) + (1 << np) - 1;
    int lox = T0x*(1 << np) - ((1 << np) - 1), loy = T0y*(1 << np) - ((1 << np) - 1);
    double* cur = npyr_lds;
    // (eight loads of a thread in flight before the first LDS store: one load per trip was 35 dependent round trips per workgroup
    //  -- the launch took what the five k_restrict launches it replaces had taken)
    for (int e0 = tid; e0 < w*w; e0 += 8*256) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = min(e0 + 256*u, w*w - 1);
            const int lj = e / w, li = e - lj*w;
            const int i = lox + li, j = loy + lj;
            const bool in = (i >= 1 && i <= o.vhx[0] && j >= 1 && j <= o.vhy[0]);
            const double x = f0(min(max(i, 1), o.vhx[0]), min(max(j, 1), o.vhy[0]), 0);
            v[u] = in ? x : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int e = e0 + 256*u; if (e < w*w) cur[e] = v[u]; }
    }
    __syncthreads();
#pragma unroll
    for (int l = 1; l <= np; ++l) {
        const int s = np - l;
        const int wl = NPYR_NB*(1 << s) + (1 << s) - 1;
        const int lxl = T0x*(1 << s) - ((1 << s) - 1), lyl = T0y*(1 << s) - ((1 << s) - 1);
        const int ox = T0x*(1 << s), oy = T0y*(1 << s);          // first owned node
        double* nxt = cur + w*w;
        const FView& out = o.lev[l - 1];
        for (int e = tid; e < wl*wl; e += 256) {
            const int lj = e / wl, li = e - lj*wl;
            const int i = lxl + li, j = lyl + lj;
            double v = 0.0;
            if (i >= 1 && i <= o.vhx[l] && j >= 1 && j <= o.vhy[l]) {
                const double* f = cur + (2*lj)*w + 2*li;             // node (2i - 1, 2j - 1) of the finer window
                v = (1./16.)*(f[0] + 2.*f[1] + f[2]
                            + 2.*f[w] + 4.*f[w + 1] + 2.*f[w + 2]
                            + f[2*w] + 2.*f[2*w + 1] + f[2*w + 2]);
                if (i >= ox && j >= oy) out(i, j, 0) = v;
            }
            if (l < np) nxt[e] = v;
        }
        __syncthreads();
        cur = nxt; w = wl;
    }
}
static size_t nodal_pyramid_lds (int np)
{
    size_t n = 0;
    for (int l = 0; l < np; ++l) { const int s = np - l; const size_t w = (size_t)NPYR_NB*(1 << s) + (1 << s) - 1; n += w*w; }
    return n*sizeof(double);
}

// inverse diagonals of a cell-centred level (grids whose level A lies below the pyramid kernel's five levels)
__global__ void k_level_cinv (const double* __restrict__ acf, double* __restrict__ cinv, int nx, int ny, double fx, double fy)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i < nx && j < ny) cinv[i + (long)j*nx] = 1.0/diag_c0<true>(i, j, cc_box(nx, ny), acf[i + (long)j*nx], fx, fy);
}

__global__ void k_copy2 (LevBox b, FView dst, FView src)
{
    const int i = b.vlx + blockIdx.x*blockDim.x + threadIdx.x;
    const int j = b.vly + blockIdx.y;
    if (i > b.vhx || j > b.vhy) return;
    dst(i, j, 0) = src(i, j, 0); dst(i, j, 1) = src(i, j, 1);
}

// The generic bottom: the reference's CPU branch (bottomsolve, HpMultiGrid.cpp:1583-1593), taken when the lower V would need
// more LDS than one workgroup has (no level of at most LOWV_MAX_CELLS: the coarsest level is large).  The coarsest level's
// correction is zeroed (is < 0), then swept once per launch, colour (i + j + is) % 2 == 0 in level index space, in global
// memory.  Neighbours outside a cell-centred box are not read (the wall stencil does not use them); node-centred walls hold 0.
template <bool CC>
__global__ __launch_bounds__(256)
void k_bottom_sweep (LevBox b, FView cor, FView rhs, FView acf, double facx, double facy, int is, StopRule sr)
{
    if (!vcycle_active(sr)) return;
    const int i = b.vlx + blockIdx.x*blockDim.x + threadIdx.x;
    const int j = b.vly + blockIdx.y;
    if (i > b.vhx || j > b.vhy) return;
    if (is < 0) { cor(i, j, 0) = 0.0; cor(i, j, 1) = 0.0; return; }
    if ((i + j + is) & 1) return;
    const double ci = 1.0/diag_c0<CC>(i, j, b, acf(i, j, 0), facx, facy);
    for (int n = 0; n < 2; ++n) {
        const double w = (i > b.lox) ? cor(i-1, j, n) : 0.0, e = (i < b.hix) ? cor(i+1, j, n) : 0.0;
        const double s = (j > b.loy) ? cor(i, j-1, n) : 0.0, no = (j < b.hiy) ? cor(i, j+1, n) : 0.0;
        double lx = facx*(w + e), ly = facy*(s + no);
        if (CC) {
            lx = (i == b.lox) ? facx*(4./3.)*e : ((i == b.hix) ? facx*(4./3.)*w : lx);
            ly = (j == b.loy) ? facy*(4./3.)*no : ((j == b.hiy) ? facy*(4./3.)*s : ly);
        }
        cor(i, j, n) = (rhs(i, j, n) - (lx + ly))*ci;
    }
}

struct MGLevelDev { LevBox b; long cells; double *acf, *res, *cor, *rescor; };

constexpr long LOWV_MAX_CELLS = 34*34;     // levels with at most ~32x32 unknowns run in k_lower_v (LDS resident)
constexpr long SMALL_TILE_CELLS = 300L*300L;      // levels up to this many cells are smoothed on TileSmall, larger ones on TileBig

constexpr int MG_GO_WORD = 8;      // int word of the header slot that k_post_norms sets: 1 = the solve is over
struct SolveRun { int enq, nspec, nzeroed, max_iters; double tol_rel, tol_abs; bool cc; };

struct Multigrid {
    bool cc; int nx, ny; double dx, dy;
    bool hierarchy_ready = false;               // mg_solve1_prepare has enqueued the coefficient hierarchy of the next solve
    bool nodal_pull1 = false;                   // node-centred: level 1's down-leg smoother forms its right-hand side from level 0's residual itself
    std::vector<MGLevelDev> L;
    int lowv_begin = 1;                         // first level handled by k_lower_v
    LowLev* d_low = nullptr; size_t low_lds = 0;
    bool bottom = false;                        // the lower V does not fit: lowv_begin = coarsest level, swept by k_bottom_sweep
    // device / pinned buffers: one header slot (MG_NSUB words: a caller's counters ride along with the norm
    // read-back, see hps_mg_rider) followed by the norm slots; d_norms / h_norms point at slot 0
    unsigned long long *d_buf = nullptr, *h_buf = nullptr;
    unsigned long long* h_buf_dev = nullptr;    // device address of the (mapped) pinned buffer: k_post_norms writes it
    long dbg_trips = 0, dbg_solves = 0, dbg_hist[8] = {0,0,0,0,0,0,0,0};
    unsigned long long* h_seq = nullptr; unsigned long long* h_seq_dev = nullptr; unsigned long long seq = 0;
    unsigned long long* d_norms = nullptr;      // [0] residual, [1] rhs
    unsigned long long* h_norms = nullptr;      // pinned copy of d_norms (2 + MG_MAX_VCYCLES slots)
    int last_iters = 1;                         // V-cycles of the previous solve = speculation depth
    SolveRun run{};                             // the solve between mg_solve1_begin and mg_solve1_finish
    bool defer_post = false; bool deferred_valid = false; MgPost deferred{};      // mg_defer_post / mg_take_deferred_post
    bool use_low3 = false; Low2 low3{}; Low2* d_low3 = nullptr; size_t low3_lds = 0;   // cell-centred register/LDS lower V (k_lower_v3)
    bool ride_on = false; ShiftInit ride{}; int ride_guests = 0;      // mg_ride_shift_init: guests of the next solve's first k_lower_v3 launch
    double* cinvA = nullptr;                    // inverse diagonals of level lowv_begin (written with the coefficient pyramid)
    double* coef_img = nullptr;                 // [acf | 1/diag] planes of the levels below it (left by the initial pass's guest, or by the first V-cycle of a solve)
    bool coef_guest = false;                    // the image is derived by a guest workgroup of the initial level-0 pass (HPS_MG_COEF_GUEST)
    int up_fused = 0;                           // mid levels 1 .. up_fused make their up-leg in one k_up_fused launch (0: one launch each; HPS_MG_UP_FUSED)
    double* tmp0 = nullptr;                     // level-0 scratch: smoothed solution before the last GSRB^4
    bool cor_in_tmp = false;                    // which buffer holds cor[0] (the fused 8-sweep end of the V-cycle is out of place)
    FView sol, rhs, acf0;                       // level-0 user views (set per solve)

    ~Multigrid () {
        for (auto& l : L) { (void)hipFree(l.acf); (void)hipFree(l.res); (void)hipFree(l.cor); (void)hipFree(l.rescor); }
        if (getenv("HPS_MG_DEBUG")) fprintf(stderr, "mg: solves %ld trips %ld hist %ld %ld %ld %ld %ld %ld\n", dbg_solves, dbg_trips, dbg_hist[0], dbg_hist[1], dbg_hist[2], dbg_hist[3], dbg_hist[4], dbg_hist[5]);
        (void)hipFree(d_buf); (void)hipFree(d_low); (void)hipFree(tmp0); (void)hipFree(d_low3); (void)hipFree(cinvA); (void)hipFree(coef_img);
        if (h_buf) (void)hipHostFree(h_buf);
    }
    FView lv (int il, double* p) const {
        const MGLevelDev& l = L[il];
        const long nxb = l.b.hix - l.b.lox + 1;
        return FView{p, nxb, l.cells, -l.b.lox, -l.b.loy};
    }
    int nlev () const { return (int)L.size(); }
    bool pulls (int il) const {
        return !cc && ((il >= 2 && ((il < lowv_begin && L[il].cells <= SMALL_TILE_CELLS) ||
                                    (il == lowv_begin && !use_low3 && !bottom))) ||      // (il == lowv_begin: k_lower_v's own load)
                       (il == 1 && nodal_pull1));
    }
};

// LDS one workgroup may have (163 840 B on MI355X); queried once.  (The opt-in attribute as well: where a runtime reports a
// smaller default per-block figure, launches up to the opt-in limit still work after hipFuncSetAttribute.)
static size_t device_max_lds ()
{
    static const size_t lim = [] {
        int dev = 0, a = 0, b = 0;
        if (hipGetDevice(&dev) != hipSuccess) return (size_t)0;
        if (hipDeviceGetAttribute(&a, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) a = 0;
        if (hipDeviceGetAttribute(&b, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess) b = 0;
        return (size_t)std::max(a, b);
    }();
    return lim;
}

int mg_create (int nx, int ny, double dx, double dy, Multigrid** out)
{
    if (nx % 2 != ny % 2) { set_error("hps_mg_create: nx and ny must have the same parity"); return HPS_ERR_ARG; }
    HPS_REQUIRE((long)(nx + 16)*(ny + 16) < (1L << 27), "hps_mg_create: the kernels address a two-component plane pair by 32-bit byte offsets (at most 2^27 cells per plane)");
    Multigrid* M = new Multigrid;
    M->cc = (nx % 2 == 0); M->nx = nx; M->ny = ny; M->dx = dx; M->dy = dy;
    // level boxes (ctor, HpMultiGrid.cpp:1043-1072)
    int hx = M->cc ? nx - 1 : nx + 1, hy = M->cc ? ny - 1 : ny + 1;
    for (int il = 0; il < 31; ++il) {
        MGLevelDev l{};
        l.b.lox = 0; l.b.loy = 0; l.b.hix = hx; l.b.hiy = hy;
        if (M->cc) { l.b.vlx = 0; l.b.vly = 0; l.b.vhx = hx; l.b.vhy = hy; }
        else       { l.b.vlx = 1; l.b.vly = 1; l.b.vhx = hx - 1; l.b.vhy = hy - 1; }
        l.cells = (long)(hx + 1)*(hy + 1);
        HPS_HIP_CHECK(hipMalloc(&l.acf, l.cells*sizeof(double)));
        HPS_HIP_CHECK(hipMalloc(&l.res, 2*l.cells*sizeof(double)));
        HPS_HIP_CHECK(hipMalloc(&l.cor, 2*l.cells*sizeof(double)));
        HPS_HIP_CHECK(hipMalloc(&l.rescor, 2*l.cells*sizeof(double)));
        HPS_HIP_CHECK(hipMemset(l.acf, 0, l.cells*sizeof(double)));
        HPS_HIP_CHECK(hipMemset(l.res, 0, 2*l.cells*sizeof(double)));
        HPS_HIP_CHECK(hipMemset(l.cor, 0, 2*l.cells*sizeof(double)));
        HPS_HIP_CHECK(hipMemset(l.rescor, 0, 2*l.cells*sizeof(double)));
        M->L.push_back(l);
        bool ok;
        const int nxl = hx + 1, nyl = hy + 1;
        if (M->cc) { ok = nxl >= 4 && nyl >= 4 && nxl % 2 == 0 && nyl % 2 == 0; if (ok) { hx = nxl/2 - 1; hy = nyl/2 - 1; } }
        else       { ok = nxl >= 8 && nyl >= 8 && hx % 2 == 0 && hy % 2 == 0;   if (ok) { hx /= 2; hy /= 2; } }
        if (!ok) break;
    }
    if (M->nlev() < 2) { delete M; set_error("hps_mg_create: grid too small to coarsen"); return HPS_ERR_ARG; }
    if (!M->cc)
        HPS_HIP_CHECK(hipFuncSetAttribute((const void*)k_nodal_acf_pyramid<5>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)nodal_pyramid_lds(NPYR_MAX)));
    const int nl = M->nlev();
    M->lowv_begin = nl - 1;
    for (int il = nl - 1; il >= 1; --il) if (M->L[il].cells <= LOWV_MAX_CELLS) M->lowv_begin = il;
    if (M->cc) {
        // k_lower_v3 from the first level with at most 64 x 64 cells whose coarser levels all fit 32 x 32 (none: k_lower_v)
        for (int il = 1; il < nl; ++il) {
            const LevBox& b = M->L[il].b;
            const bool fits = (b.hix + 1 <= 64) && (b.hiy + 1 <= 64) && (nl - il <= LOW2_MAXLEV)
                           && (il + 1 >= nl || (M->L[il+1].b.hix + 1 <= 32 && M->L[il+1].b.hiy + 1 <= 32));
            if (!fits) continue;
            // one component per workgroup: level A one plane, the others cor | res, then their acf | 1/diag planes
            M->use_low3 = true; M->lowv_begin = il;
            Low2& e = M->low3;
            e.nl = nl - il;
            int off3 = 0;
            for (int k = 0; k < e.nl; ++k) {
                const LevBox& bk = M->L[il + k].b;
                e.nx[k] = bk.hix + 1; e.ny[k] = bk.hiy + 1; e.off[k] = off3;
                off3 += (k == 0 ? 1 : 2)*(e.nx[k] + 2)*(e.ny[k] + 2);      // cor [| res]
            }
            e.cbase = off3; e.coff[0] = off3;
            for (int k = 1; k < e.nl; ++k) { e.coff[k] = off3; off3 += 2*(e.nx[k] + 2)*(e.ny[k] + 2); }      // acf | 1/diag
            e.ctot = std::max(off3 - e.cbase, 1);
            e.total = off3;
            HPS_HIP_CHECK(hipMalloc(&M->coef_img, (size_t)e.ctot*sizeof(double)));
            HPS_HIP_CHECK(hipMemset(M->coef_img, 0, (size_t)e.ctot*sizeof(double)));
            M->low3_lds = (size_t)off3*sizeof(double);
            if (M->low3_lds > 64*1024)
                HPS_HIP_CHECK(hipFuncSetAttribute((const void*)k_lower_v3, hipFuncAttributeMaxDynamicSharedMemorySize, (int)M->low3_lds));
            HPS_HIP_CHECK(hipMalloc(&M->d_low3, sizeof(Low2)));
            HPS_HIP_CHECK(hipMemcpy(M->d_low3, &e, sizeof(Low2), hipMemcpyHostToDevice));
            HPS_HIP_CHECK(hipMalloc(&M->cinvA, (size_t)e.nx[0]*e.ny[0]*sizeof(double)));
            // guests: one per compute unit that the two solver workgroups leave free
            int dev = 0, ncu = 0;
            HPS_HIP_CHECK(hipGetDevice(&dev));
            HPS_HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
            M->ride_guests = std::max(ncu - 2, 1);
            // the image's guest needs the initial pass on 64 x 32 tiles (its static LDS holds the image; 32 x 16 tiles: too small)
            const char* sw = getenv("HPS_MG_COEF_GUEST");
            M->coef_guest = !(sw && atoi(sw) == 0) && M->L[0].cells > SMALL_TILE_CELLS && e.nl > 1 && e.ctot <= COEF_GUEST_MAX_IMG;
            break;
        }
    }
    if (!M->use_low3) {
        long cells = 0;
        for (int il = M->lowv_begin; il < nl; ++il) cells += M->L[il].cells;
        M->low_lds = (size_t)(8*cells)*sizeof(double);
        hipFuncAttributes fa{};
        HPS_HIP_CHECK(hipFuncGetAttributes(&fa, M->cc ? (const void*)k_lower_v<true> : (const void*)k_lower_v<false>));
        if (M->low_lds + fa.sharedSizeBytes > device_max_lds()) { M->bottom = true; M->lowv_begin = nl - 1; M->low_lds = 0; }
    }
    // the up-leg of levels 1 .. min(3, lowv_begin - 1) in one launch: cell-centred grids with k_lower_v3 and at least two mid levels
    {
        const char* sw = getenv("HPS_MG_UP_FUSED");
        if (!(sw && atoi(sw) == 0) && M->cc && M->use_low3 && M->lowv_begin >= 3) M->up_fused = std::min(3, M->lowv_begin - 1);
    }
    // node-centred: level 1 pulls (vcycle: pulls) when it is a smoother level of its own, not the lower V's top
    M->nodal_pull1 = !M->cc && M->lowv_begin > 1;
    if (!M->use_low3 && !M->bottom) {
        std::vector<LowLev> low;
        int off = 0;
        for (int il = M->lowv_begin; il < nl; ++il) {
            const MGLevelDev& l = M->L[il];
            low.push_back(LowLev{l.b, l.b.hix - l.b.lox + 1, (int)l.cells, off});
            off += 8*(int)l.cells;
        }
        if (M->low_lds > 64*1024) {
            HPS_HIP_CHECK(hipFuncSetAttribute((const void*)k_lower_v<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)M->low_lds));
            HPS_HIP_CHECK(hipFuncSetAttribute((const void*)k_lower_v<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)M->low_lds));
        }
        HPS_HIP_CHECK(hipMalloc(&M->d_low, low.size()*sizeof(LowLev)));
        HPS_HIP_CHECK(hipMemcpy(M->d_low, low.data(), low.size()*sizeof(LowLev), hipMemcpyHostToDevice));
    }
    HPS_HIP_CHECK(hipMalloc(&M->d_buf, (3 + MG_MAX_VCYCLES)*MG_NSUB*sizeof(unsigned long long)));
    HPS_HIP_CHECK(hipHostMalloc(&M->h_buf, ((3 + MG_MAX_VCYCLES)*MG_NSUB + 8)*sizeof(unsigned long long), hipHostMallocMapped));
    HPS_HIP_CHECK(hipHostGetDevicePointer((void**)&M->h_buf_dev, M->h_buf, 0));
    M->h_seq = M->h_buf + (3 + MG_MAX_VCYCLES)*MG_NSUB; M->h_seq_dev = M->h_buf_dev + (3 + MG_MAX_VCYCLES)*MG_NSUB;
    *M->h_seq = 0ULL;
    HPS_HIP_CHECK(hipMemset(M->d_buf, 0, (3 + MG_MAX_VCYCLES)*MG_NSUB*sizeof(unsigned long long)));
    memset(M->h_buf, 0, (3 + MG_MAX_VCYCLES)*MG_NSUB*sizeof(unsigned long long));
    M->d_norms = M->d_buf + MG_NSUB; M->h_norms = M->h_buf + MG_NSUB;
    HPS_HIP_CHECK(hipMalloc(&M->tmp0, 2*M->L[0].cells*sizeof(double)));
    HPS_HIP_CHECK(hipMemset(M->tmp0, 0, 2*M->L[0].cells*sizeof(double)));
    *out = M;
    return HPS_OK;
}

template <class TS, bool CC, int SRC, bool DO_RES, int NSW = 4, bool RPULL = false>
static void launch_smooth_ts (Multigrid* M, int il, FView phi_out, FView phi_out2, FView rhs, FView acf, FView phi_in, FView crse,
                              FView res_out, FView cres_out, unsigned long long* resnorm, unsigned long long* rhsnorm,
                              const StopRule& sr, hipStream_t st)
{
    const LevBox& b = M->L[il].b;
    constexpr int E = DO_RES ? NSW : NSW - 1;
    constexpr int FX = TS::TX - 2*E, FY = TS::TY - 2*E;
    const int ntx = ceil_div(b.vhx - b.vlx + 1, FX), nty = ceil_div(b.vhy - b.vly + 1, FY);
    const double fac = (double)(1 << il);
    const double ldx = M->dx*fac, ldy = M->dy*fac;
    const double facx = 1.0/(ldx*ldx), facy = 1.0/(ldy*ldy);
    constexpr bool FUSE = CC && DO_RES;
    hipLaunchKernelGGL((k_smooth<TS, CC, SRC, DO_RES, FUSE, NSW, RPULL>), dim3(ntx*nty), dim3(TS::NT), 0, st, b, phi_out, phi_out2, rhs, acf,
                       phi_in, crse, res_out, cres_out, facx, facy, ntx, resnorm, rhsnorm, sr);
}

template <bool CC, int SRC, bool DO_RES>
static void launch_smooth (Multigrid* M, int il, FView phi_out, FView phi_out2, FView rhs, FView acf, FView phi_in, FView crse,
                           FView res_out, FView cres_out, unsigned long long* resnorm, unsigned long long* rhsnorm,
                           const StopRule& sr, hipStream_t st)
{
    if (M->L[il].cells <= SMALL_TILE_CELLS)
        launch_smooth_ts<TileSmall, CC, SRC, DO_RES>(M, il, phi_out, phi_out2, rhs, acf, phi_in, crse, res_out, cres_out, resnorm, rhsnorm, sr, st);
    else
        launch_smooth_ts<TileBig, CC, SRC, DO_RES>(M, il, phi_out, phi_out2, rhs, acf, phi_in, crse, res_out, cres_out, resnorm, rhsnorm, sr, st);
}

// k_up_fused for levels 1 .. M->up_fused: level 1's tiling and tile shape are launch_smooth's
template <class TS, int NL>
static void launch_up_fused_ts (Multigrid* M, int lb, const StopRule& sr, hipStream_t st)
{
    UpArgs A{};
    for (int k = 0; k < NL; ++k) {
        const int il = 1 + k;
        const double fac = (double)(1 << il);
        const double ldx = M->dx*fac, ldy = M->dy*fac;
        A.l[k] = UpLevArg{M->L[il].b, M->lv(il, M->L[il].res), M->lv(il, M->L[il].acf), M->lv(il, M->L[il].cor), 1.0/(ldx*ldx), 1.0/(ldy*ldy)};
    }
    A.crse = M->lv(NL + 1, (NL + 1 == lb) ? M->L[NL+1].cor : M->L[NL+1].rescor);
    A.out = M->lv(1, M->L[1].rescor);
    const LevBox& b = M->L[1].b;
    constexpr int FX = TS::TX - 6, FY = TS::TY - 6;
    const int ntx = ceil_div(b.vhx - b.vlx + 1, FX), nty = ceil_div(b.vhy - b.vly + 1, FY);
    A.ntx = ntx;
    hipLaunchKernelGGL((k_up_fused<TS, NL>), dim3(ntx*nty), dim3(TS::NT), 0, st, A, sr);
}

static void launch_up_fused (Multigrid* M, int lb, const StopRule& sr, hipStream_t st)
{
    const bool small = M->L[1].cells <= SMALL_TILE_CELLS;
    if (M->up_fused == 3) { if (small) launch_up_fused_ts<TileSmall, 3>(M, lb, sr, st); else launch_up_fused_ts<TileBig, 3>(M, lb, sr, st); }
    else                  { if (small) launch_up_fused_ts<TileSmall, 2>(M, lb, sr, st); else launch_up_fused_ts<TileBig, 2>(M, lb, sr, st); }
}

template <bool CC>
static void restrict_residual_if_nodal (Multigrid* M, int il, const StopRule& sr, hipStream_t st)
{
    if (CC) return;     // fused into k_smooth
    const LevBox& cb = M->L[il+1].b;
    hipLaunchKernelGGL(k_restrict<CC>, dim3(ceil_div(cb.vhx - cb.vlx + 1, 64), cb.vhy - cb.vly + 1), dim3(64), 0, st,
                       cb, M->lv(il+1, M->L[il+1].res), M->lv(il, M->L[il].rescor), 2, sr);
}

// V-cycle k (vcycle :1429-1512).  On entry res[1] = R(rhs - L(cor[0])); on exit again, plus
// tmp0 = smoothed solution, cor[0] = sol = GSRB^4(tmp0) and the residual norm in d_norms[2+k].
template <bool CC>
static void vcycle (Multigrid* M, int k, double tol_rel, double tol_abs, hipStream_t st)
{
    const int nl = M->nlev();
    const int lb = M->lowv_begin;
    const FView none{};
    const StopRule sr{M->d_norms, k, tol_rel, tol_abs};
    // node-centred levels: the smoother of level il >= 2 forms its right-hand side from level il - 1's residual itself (RPULL);
    // the launch of k_restrict stays where the next consumer is not a smoother (level 0 -> 1 behind the fused pass, the lower V's input)
    // (levels on 32 x 16 tiles only: with the nine reads per cell in flight the 64 x 32 variant spills 108 registers under its cap)
    // (round 6: level 1 too -- on 32 x 32 tiles of 256 threads where it is too large for the 32 x 16 ones: the 64 x 32 variant's 512
    //  threads are what capped its registers -- so the level 0 -> 1 restriction launch is gone as well: M->nodal_pull1)
    for (int il = 1; il < lb; ++il) {
        if (!M->pulls(il))
            launch_smooth<CC, SRC_ZERO, true>(M, il, M->lv(il, M->L[il].cor), none, M->lv(il, M->L[il].res), M->lv(il, M->L[il].acf), none,
                                              none, M->lv(il, M->L[il].rescor), M->lv(il+1, M->L[il+1].res), nullptr, nullptr, sr, st);
        else if constexpr (!CC) {
            if (M->L[il].cells > SMALL_TILE_CELLS)
                launch_smooth_ts<TileMid, CC, SRC_ZERO, true, 4, true>(M, il, M->lv(il, M->L[il].cor), none, M->lv(il, M->L[il].res), M->lv(il, M->L[il].acf), none,
                                                                       M->lv(il-1, M->L[il-1].rescor), M->lv(il, M->L[il].rescor), M->lv(il+1, M->L[il+1].res), nullptr, nullptr, sr, st);
            else
                launch_smooth_ts<TileSmall, CC, SRC_ZERO, true, 4, true>(M, il, M->lv(il, M->L[il].cor), none, M->lv(il, M->L[il].res), M->lv(il, M->L[il].acf), none,
                                                                         M->lv(il-1, M->L[il-1].rescor), M->lv(il, M->L[il].rescor), M->lv(il+1, M->L[il+1].res), nullptr, nullptr, sr, st);
        }
        if (!M->pulls(il + 1)) restrict_residual_if_nodal<CC>(M, il, sr, st);
    }
    {
        const double fac = (double)(1 << lb);
        const double ldx = M->dx*fac, ldy = M->dy*fac;
        const LevBox& bb = M->L[nl-1].b;
        const int nsweeps = std::max(16, (std::max(bb.hix - bb.lox + 1, bb.hiy - bb.loy + 1) + 1)/2*2);
        if (M->bottom) {
            const FView cor = M->lv(lb, M->L[lb].cor), rhs = M->lv(lb, M->L[lb].res), acf = M->lv(lb, M->L[lb].acf);
            const dim3 grid(ceil_div(bb.vhx - bb.vlx + 1, 64), bb.vhy - bb.vly + 1);
            for (int is = -1; is < nsweeps; ++is)
                hipLaunchKernelGGL(k_bottom_sweep<CC>, grid, dim3(64), 0, st, bb, cor, rhs, acf, 1.0/(ldx*ldx), 1.0/(ldy*ldy), is, sr);
        } else if (M->use_low3) {
            // one field component per workgroup; behind them the guests of this solve (mg_ride_shift_init), in V-cycle 0 only
            const int guests = (k == 0 && M->ride_on) ? M->ride_guests : 0;
            M->ride_on = false;
            hipLaunchKernelGGL(k_lower_v3, dim3(2 + guests), dim3(1024), M->low3_lds, st, M->d_low3, M->L[lb].acf, M->cinvA, M->L[lb].res, M->L[lb].cor,
                               M->coef_img, M->low3.nx[0], M->low3.ny[0], M->low3.ctot, 1.0/(ldx*ldx), 1.0/(ldy*ldy), nsweeps, sr, M->ride,
                               M->coef_guest ? 0 : 1);
        } else      // (node-centred: one field component per workgroup)
            hipLaunchKernelGGL(k_lower_v<CC>, dim3(CC ? 1 : 2), dim3(1024), M->low_lds, st, M->d_low, nl - lb, M->L[lb].acf, M->L[lb].res,
                               M->L[lb].cor, 1.0/(ldx*ldx), 1.0/(ldy*ldy), nsweeps, sr, M->pulls(lb) ? M->lv(lb-1, M->L[lb-1].rescor) : FView{});
    }
    // up-leg: the smoothed correction of level il lands in rescor[il] (out of place)
    // (cell-centred, M->up_fused = NL > 0: levels NL .. 1 in one launch behind the deeper levels' own)
    for (int il = lb - 1; il > (CC ? M->up_fused : 0); --il) {
        double* crse = (il + 1 == lb) ? M->L[il+1].cor : M->L[il+1].rescor;
        launch_smooth<CC, SRC_PROLONG, false>(M, il, M->lv(il, M->L[il].rescor), none, M->lv(il, M->L[il].res), M->lv(il, M->L[il].acf),
                                              M->lv(il, M->L[il].cor), M->lv(il+1, crse), none, none, nullptr, nullptr, sr, st);
    }
    if constexpr (CC) if (M->up_fused) launch_up_fused(M, lb, sr, st);
    {
        // level 0: cor[0] + P(correction), GSRB^4 (the smoothed solution), GSRB^4 + residual (solve_doit's
        // iterate) in one pass: out of place between cor[0] and tmp0 (other tiles read the rims), the
        // iterate also goes to the caller's slab
        double* crse = (1 == lb) ? M->L[1].cor : M->L[1].rescor;
        double* in = M->cor_in_tmp ? M->tmp0 : M->L[0].cor;
        double* out = M->cor_in_tmp ? M->L[0].cor : M->tmp0;
        launch_smooth_ts<typename HugeTileOf<CC>::type, CC, SRC_PROLONG, true, 8>(M, 0, M->lv(0, out), M->sol, M->rhs, M->acf0, M->lv(0, in), M->lv(1, crse),
                                                             M->lv(0, M->L[0].rescor), M->lv(1, M->L[1].res), M->d_norms + (2 + k)*MG_NSUB,
                                                             nullptr, sr, st);
        M->cor_in_tmp = !M->cor_in_tmp;
    }
    if (!M->nodal_pull1) restrict_residual_if_nodal<CC>(M, 0, sr, st);
}

// norm slots (and the rider words) -> mapped host memory, sequence number last behind a system-scope fence: the host
// polls it instead of a DMA copy + stream synchronise (one round trip per solve, two when the speculation fell short)
__global__ __launch_bounds__(256)
void k_post_norms (const unsigned long long* __restrict__ src, volatile unsigned long long* dst, int nwords,
                   volatile unsigned long long* seq_slot, unsigned long long seq, int* go_word, StopRule after)
{
    // one word for the kernels enqueued behind this solve before the host has seen its norms (the gated plasma push):
    // is the solve over after the V-cycles enqueued so far?
    {   const bool act = vcycle_active(after);      // (whole waves: the rule is read lane-parallel)
        if (threadIdx.x == 0) *go_word = act ? 0 : 1; }
    for (int w = threadIdx.x; w < nwords; w += blockDim.x) dst[w] = src[w];
    HPS_HOST_STORES_ACKNOWLEDGED();
    __syncthreads();
    if (threadIdx.x == 0) { *seq_slot = seq; }
}

// one batch of (gated) V-cycles and the post of all norms so far to the host
template <bool CC>
static void enqueue_cycles (Multigrid* M, hipStream_t st)
{
    SolveRun& r = M->run;
    for (int v = 0; v < r.nspec && r.enq < r.max_iters; ++v, ++r.enq) {
        if (r.enq >= r.nzeroed) {        // more slots than foreseen: zero the next batch (rare)
            const int more = std::min(r.max_iters - r.nzeroed, 64);
            (void)hipMemsetAsync(M->d_norms + (2 + r.nzeroed)*MG_NSUB, 0, more*MG_NSUB*sizeof(unsigned long long), st);
            r.nzeroed += more;
        }
        vcycle<CC>(M, r.enq, r.tol_rel, r.tol_abs, st);
    }
    ++M->seq; ++M->dbg_trips;
    if (M->defer_post) {
        // the caller's next kernel on this stream posts (mg_take_deferred_post): no launch of its own between the last V-cycle and it
        M->defer_post = false; M->deferred_valid = true;
        M->deferred = MgPost{M->d_buf, (volatile unsigned long long*)M->h_buf_dev, (3 + r.enq)*MG_NSUB, (volatile unsigned long long*)M->h_seq_dev, M->seq,
                             StopRule{M->d_norms, r.enq, r.tol_rel, r.tol_abs}};
        return;
    }
    hipLaunchKernelGGL(k_post_norms, dim3(1), dim3(256), 0, st, M->d_buf, (volatile unsigned long long*)M->h_buf_dev,
                       (3 + r.enq)*MG_NSUB, (volatile unsigned long long*)M->h_seq_dev, M->seq,
                       reinterpret_cast<int*>(M->d_buf) + MG_GO_WORD, StopRule{M->d_norms, r.enq, r.tol_rel, r.tol_abs});
}

// The coefficient hierarchy of a solve (average_down_acoef, HpMultiGrid.cpp:1640-1700; level 0 reads the slab) and the zeroing
// of its norm slots.  It needs the coefficient (chi) only, not the right-hand side: mg_solve1_prepare lets the caller
// enqueue it early, on a stream of its own, beside whatever produces the right-hand side.
struct GuestPass { bool on = false; SlabView f{hps_slab{}}; GradPsiSxSy ga{}; };

template <bool CC>
static int solve1_hierarchy (Multigrid* M, int max_iters, hipStream_t st, const GuestPass* guest = nullptr)
{
    const int lb = M->lowv_begin;
    max_iters = std::min(max_iters, MG_MAX_VCYCLES);
    const StopRule always{nullptr, -1, 0.0, 0.0};
    // speculate as many V-cycles as the previous solve needed; each one is a no-op once converged
    int nspec = std::min(std::max(M->last_iters, 1), std::max(max_iters, 1));
    int nzeroed = std::min(max_iters, nspec + 8);
    const int nzero_words = (2 + nzeroed)*MG_NSUB;
    int first = 1;
    if (CC) {
        PyrOut po{};
        const int np = std::min(lb, 5);
        for (int il = 1; il <= np; ++il) { po.p[il-1] = M->L[il].acf; po.nx[il-1] = M->L[il].b.hix + 1; po.ny[il-1] = M->L[il].b.hiy + 1; }
        const double lfac = (double)(1 << lb), lfx = 1.0/(M->dx*lfac*M->dx*lfac), lfy = 1.0/(M->dy*lfac*M->dy*lfac);
        if (M->use_low3 && lb <= np) { po.cinv = M->cinvA; po.cinv_l = lb - 1; po.cfx = lfx; po.cfy = lfy; }
        if (guest) {
            const int gx = ceil_div(M->nx, 32), gy = ceil_div(M->ny, 32);
            const SlabView& f = guest->f;
            const int nbx = ceil_div(f.js, 256), rows = f.ny + 2*f.ng;
            hipLaunchKernelGGL(k_hierarchy_gradpsi, dim3(gx*gy + nbx*rows), dim3(256), 0, st, M->acf0, M->nx, M->ny, po, np, M->d_norms, nzero_words,
                               gx, gy, f, guest->ga, nbx);
        } else
        hipLaunchKernelGGL(k_acf_pyramid, dim3(ceil_div(M->nx, 32), ceil_div(M->ny, 32)), dim3(256), 0, st, M->acf0, M->nx, M->ny, po, np,
                           M->d_norms, nzero_words);
        first = np + 1;
    } else {
        // node-centred: levels 1..min(lb, 5) in one launch (lb >= 1), the norm slots zeroed by it too
        NodalPyr o{};
        const int np = std::min(lb, NPYR_MAX);
        o.np = np;
        o.vhx[0] = M->L[0].b.vhx; o.vhy[0] = M->L[0].b.vhy;
        for (int il = 1; il <= np; ++il) { o.lev[il-1] = M->lv(il, M->L[il].acf); o.vhx[il] = M->L[il].b.vhx; o.vhy[il] = M->L[il].b.vhy; }
        const int tx = ceil_div(M->L[np].b.hix, NPYR_NB), ty = ceil_div(M->L[np].b.hiy, NPYR_NB);      // top-level nodes 0..hi - 1 (0: wall)
        switch (np) {
            case 1: hipLaunchKernelGGL(k_nodal_acf_pyramid<1>, dim3(tx, ty), dim3(256), nodal_pyramid_lds(np), st, M->acf0, o, M->d_norms, nzero_words); break;
            case 2: hipLaunchKernelGGL(k_nodal_acf_pyramid<2>, dim3(tx, ty), dim3(256), nodal_pyramid_lds(np), st, M->acf0, o, M->d_norms, nzero_words); break;
            case 3: hipLaunchKernelGGL(k_nodal_acf_pyramid<3>, dim3(tx, ty), dim3(256), nodal_pyramid_lds(np), st, M->acf0, o, M->d_norms, nzero_words); break;
            case 4: hipLaunchKernelGGL(k_nodal_acf_pyramid<4>, dim3(tx, ty), dim3(256), nodal_pyramid_lds(np), st, M->acf0, o, M->d_norms, nzero_words); break;
            default: hipLaunchKernelGGL(k_nodal_acf_pyramid<5>, dim3(tx, ty), dim3(256), nodal_pyramid_lds(np), st, M->acf0, o, M->d_norms, nzero_words); break;
        }
        first = np + 1;
    }
    for (int il = first; il <= lb; ++il) {
        const LevBox& cb = M->L[il].b;
        FView fine = (il == 1) ? M->acf0 : M->lv(il-1, M->L[il-1].acf);
        hipLaunchKernelGGL(k_restrict<CC>, dim3(ceil_div(cb.vhx - cb.vlx + 1, 64), cb.vhy - cb.vly + 1), dim3(64), 0, st,
                           cb, M->lv(il, M->L[il].acf), fine, 1, always);
    }
    if (CC && M->use_low3 && lb > 5) {
        const double lfac = (double)(1 << lb);
        const int lnx = M->L[lb].b.hix + 1, lny = M->L[lb].b.hiy + 1;
        hipLaunchKernelGGL(k_level_cinv, dim3(ceil_div(lnx, 64), lny), dim3(64), 0, st, M->L[lb].acf, M->cinvA, lnx, lny,
                           1.0/(M->dx*lfac*M->dx*lfac), 1.0/(M->dy*lfac*M->dy*lfac));
    }
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

// the initial pass of a cell-centred solve (launch_smooth<true, SRC_DIRECT, true> on level 0's 64 x 32 tiles) with one workgroup
// more: the guest that derives k_lower_v3's coefficient image (coef_guest_derive).  The hierarchy's launches are ahead of it
// on this stream, or on the stream the caller has joined (mg_solve1_prepare*); the first lower V is behind it.
static void launch_initial_with_guest (Multigrid* M, const StopRule& sr, hipStream_t st)
{
    using TS = TileBig;
    const LevBox& b = M->L[0].b;
    constexpr int FX = TS::TX - 2*4, FY = TS::TY - 2*4;
    const int ntx = ceil_div(b.vhx - b.vlx + 1, FX), nty = ceil_div(b.vhy - b.vly + 1, FY);
    const int lb = M->lowv_begin;
    const double lfac = (double)(1 << lb), ldx = M->dx*lfac, ldy = M->dy*lfac;
    const CoefGuest g{M->d_low3, M->L[lb].acf, M->coef_img, 1.0/(ldx*ldx), 1.0/(ldy*ldy)};
    hipLaunchKernelGGL((k_smooth<TS, true, SRC_DIRECT, true, true, 4, false, CoefGuest>), dim3(ntx*nty + 1), dim3(TS::NT), 0, st, b,
                       M->lv(0, M->L[0].cor), FView{}, M->rhs, M->acf0, M->sol, FView{}, M->lv(0, M->L[0].rescor), M->lv(1, M->L[1].res),
                       1.0/(M->dx*M->dx), 1.0/(M->dy*M->dy), ntx, M->d_norms, M->d_norms + MG_NSUB, sr, g);
}

template <bool CC>
static int solve1_begin (Multigrid* M, double tol_rel, double tol_abs, int max_iters, hipStream_t st)
{
    max_iters = std::min(max_iters, MG_MAX_VCYCLES);
    M->cor_in_tmp = false;
    const StopRule always{nullptr, -1, 0.0, 0.0};
    int nspec = std::min(std::max(M->last_iters, 1), std::max(max_iters, 1));
    int nzeroed = std::min(max_iters, nspec + 8);
    if (M->hierarchy_ready) M->hierarchy_ready = false;       // (mg_solve1_prepare has enqueued it; the caller has ordered the streams)
    else if (int e = solve1_hierarchy<CC>(M, max_iters, st)) return e;
    // cor[0] = GSRB^4(sol), residual norm, rhs norm, res[1] = R(residual)  (solve_doit :1319-1346)
    if (CC && M->coef_guest)
        launch_initial_with_guest(M, always, st);
    else
    launch_smooth<CC, SRC_DIRECT, true>(M, 0, M->lv(0, M->L[0].cor), FView{}, M->rhs, M->acf0, M->sol, FView{}, M->lv(0, M->L[0].rescor),
                                        M->lv(1, M->L[1].res), M->d_norms, M->d_norms + MG_NSUB, always, st);
    if (!M->nodal_pull1) restrict_residual_if_nodal<CC>(M, 0, always, st);
    M->run = SolveRun{0, nspec, nzeroed, max_iters, tol_rel, tol_abs, CC};
    enqueue_cycles<CC>(M, st);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

// read the norms back, replay the stopping rule on the host (solve_doit :1352-1398), enqueue one more V-cycle at a time
// while it says so.  *extra: did that happen (then kernels gated on gate_after_enqueued() have not run)?
template <bool CC>
static int solve1_finish (Multigrid* M, int* iters_out, double* resnorm_out, int* extra, hipStream_t st)
{
    SolveRun& r = M->run;
    int status = HPS_OK;
    int iters = 0;
    double last_norm = 0.0;
    bool converged = false, diverged = false, first_trip = true;
    if (extra) *extra = 0;
    auto slot_value = [M] (int slot) {
        unsigned long long m = 0ULL;
        for (int q = 0; q < MG_NSUB; ++q) m = std::max(m, M->h_norms[slot*MG_NSUB + q]);
        double dd; memcpy(&dd, &m, 8); return dd;
    };
    while (true) {
        {   volatile unsigned long long* hs = M->h_seq;
            long spins = 0;
            while (*hs != M->seq) {
                if ((++spins & 0xfffff) == 0 && hipStreamQuery(st) != hipErrorNotReady) {      // a failed launch must not hang us
                    if (*hs == M->seq) break;
                    HPS_HIP_CHECK(hipStreamSynchronize(st));
                    if (*hs != M->seq) { set_error("hps_mg_solve1: the norm read-back never arrived"); return HPS_ERR_HIP; }
                }
            }
            __atomic_thread_fence(__ATOMIC_ACQUIRE); }
        const double res0 = slot_value(0), rhs0 = slot_value(1);
        const double max_norm = (rhs0 >= res0) ? rhs0 : res0;
        const double target = std::max(r.tol_abs, std::max(r.tol_rel, 1.e-16)*max_norm);
        last_norm = res0; iters = 0;
        converged = (res0 <= target); diverged = false;
        for (int k = 0; k < r.enq && !converged && !diverged; ++k) {
            last_norm = slot_value(2 + k); ++iters;
            if (last_norm <= target) converged = true;
            else if (!(last_norm <= 1.e20*max_norm)) diverged = true;
        }
        if (first_trip) {
            // what the device-side gate of the kernels enqueued behind the first batch has seen (vcycle_active, k = enq)
            const double prev = (r.enq == 0) ? res0 : slot_value(2 + r.enq - 1);
            const bool gate_active = prev > target && prev <= 1.e20*max_norm;
            if (gate_active != !(converged || diverged)) { set_error("hps_mg_solve1: host and device stopping rules disagree"); return HPS_ERR_HIP; }
            if (extra) *extra = gate_active ? 1 : 0;
            first_trip = false;
        }
        if (converged || diverged) break;
        if (r.enq >= r.max_iters) { set_error("hps_mg_solve1: not converged after max_iters V-cycles"); status = HPS_ERR_MG_MAXITER; break; }
        r.nspec = 1;
        enqueue_cycles<CC>(M, st);
    }
    if (diverged) { set_error("hps_mg_solve1: diverging"); status = HPS_ERR_MG_DIVERGED; }
    M->last_iters = std::max(1, iters); ++M->dbg_solves; ++M->dbg_hist[std::min(iters, 7)];
    if (iters == 0) {
        // converged on entry: solution = cor[0] of the initial smoothing (solve_doit :1419-1426)
        const LevBox& b0 = M->L[0].b;
        hipLaunchKernelGGL(k_copy2, dim3(ceil_div(b0.vhx - b0.vlx + 1, 64), b0.vhy - b0.vly + 1), dim3(64), 0, st,
                           b0, M->sol, M->lv(0, M->L[0].cor));
    }
    HPS_HIP_CHECK(hipGetLastError());
    if (iters_out) *iters_out = iters;
    if (resnorm_out) *resnorm_out = last_norm;
    return status;
}

static void set_views (Multigrid* M, const hps_slab& s, int sol_comp, int rhs_comp, int acf_comp)
{
    // centre the slab box on the level-0 box (center_box, HpMultiGrid.H:168-175)
    const int sh = M->cc ? 0 : 1;
    const int o = s.ng - sh;
    M->sol  = FView{s.p + (long)sol_comp*s.nstride, s.jstride, s.nstride, o, o};
    M->rhs  = FView{s.p + (long)rhs_comp*s.nstride, s.jstride, s.nstride, o, o};
    M->acf0 = FView{s.p + (long)acf_comp*s.nstride, s.jstride, s.nstride, o, o};
}

// the solve in two halves: begin enqueues the speculated V-cycles and the post of their norms; finish waits for the
// norms.  Kernels enqueued in between must be gated on the word at mg_gate_after_enqueued (they run iff it is 1: the solve is over).
int mg_solve1_begin (void* handle, hps_slab s, int sol_comp, int rhs_comp, int acf_comp, double tol_rel, double tol_abs,
                     int max_iters, hipStream_t st)
{
    Multigrid* M = static_cast<Multigrid*>(handle);
    HPS_REQUIRE(s.nstride < (1L << 27) && s.ng <= 8, "mg_solve1_begin: planes of at most 2^27 doubles and at most 8 guard cells (32-bit byte offsets in the kernels)");
    set_views(M, s, sol_comp, rhs_comp, acf_comp);
    return M->cc ? solve1_begin<true>(M, tol_rel, tol_abs, max_iters, st) : solve1_begin<false>(M, tol_rel, tol_abs, max_iters, st);
}
// the coefficient hierarchy of the NEXT mg_solve1_begin (same slab, same components, same max_iters) on stream `st`, which
// the caller orders: behind whatever writes the coefficient, ahead of mg_solve1_begin's stream
int mg_solve1_prepare (void* handle, hps_slab s, int sol_comp, int rhs_comp, int acf_comp, int max_iters, hipStream_t st)
{
    Multigrid* M = static_cast<Multigrid*>(handle);
    set_views(M, s, sol_comp, rhs_comp, acf_comp);
    if (int e = M->cc ? solve1_hierarchy<true>(M, max_iters, st) : solve1_hierarchy<false>(M, max_iters, st)) return e;
    M->hierarchy_ready = true;
    return HPS_OK;
}
int mg_solve1_prepare_with (void* handle, hps_slab s, int sol_comp, int rhs_comp, int acf_comp, int max_iters, SlabView f, GradPsiSxSy ga,
                            hipStream_t st, bool* done)
{
    Multigrid* M = static_cast<Multigrid*>(handle);
    *done = false;
    if (!M->cc) return HPS_OK;                       // (the nodal hierarchy has no pyramid kernel)
    set_views(M, s, sol_comp, rhs_comp, acf_comp);
    GuestPass g; g.on = true; g.f = f; g.ga = ga;
    if (int e = solve1_hierarchy<true>(M, max_iters, st, &g)) return e;
    M->hierarchy_ready = true;
    *done = true;
    return HPS_OK;
}
// a hierarchy enqueued by mg_solve1_prepare* that no mg_solve1_begin followed (the caller failed in between) is dropped
// (and so is a pass handed to mg_ride_shift_init)
void mg_solve1_forget_hierarchy (void* handle)
{
    if (!handle) return;
    Multigrid* M = static_cast<Multigrid*>(handle);
    M->hierarchy_ready = false; M->ride_on = false;
}
// mg_defer_post ahead of mg_solve1_begin: the post of the first batch's norms is not launched but handed out by
// mg_take_deferred_post -- the caller MUST then enqueue, next on the same stream, a kernel that performs it (k_advance_tiled's
// MgPost argument), or the solve's finish never sees its norms.  (Without mg_defer_post k_post_norms has posted already:
// mg_take_deferred_post returns false and the caller gates on mg_gate_after_enqueued.)
void mg_defer_post (void* handle) { Multigrid* M = static_cast<Multigrid*>(handle); M->defer_post = true; M->deferred_valid = false; }
bool mg_take_deferred_post (void* handle, MgPost* out)
{
    Multigrid* M = static_cast<Multigrid*>(handle);
    M->defer_post = false;
    if (!M->deferred_valid) return false;
    M->deferred_valid = false; *out = M->deferred;
    return true;
}
// mg_ride_shift_init ahead of mg_solve1_begin: the slab's shift / zero pass for the next slice rides in the launch of that
// solve's first lower V (k_lower_v3's guests; V-cycle 0 is always enqueued).  false: this grid's lower V is another kernel and
// nothing will be done -- the caller keeps its own launch.
bool mg_ride_shift_init (void* handle, const ShiftInit& pass)
{
    Multigrid* M = static_cast<Multigrid*>(handle);
    if (!M->cc || !M->use_low3 || M->bottom) return false;
    M->ride = pass; M->ride_on = true;
    return true;
}
const int* mg_gate_after_enqueued (void* handle)
{
    return reinterpret_cast<const int*>(static_cast<Multigrid*>(handle)->d_buf) + MG_GO_WORD;
}
// have the norms of the batch enqueued by mg_solve1_begin arrived (mg_solve1_finish would not wait)?
bool mg_solve1_ready (void* handle)
{
    Multigrid* M = static_cast<Multigrid*>(handle);
    return *(volatile unsigned long long*)M->h_seq == M->seq;
}
int mg_solve1_finish (void* handle, int* iters_out, double* resnorm_out, int* extra, hipStream_t st)
{
    Multigrid* M = static_cast<Multigrid*>(handle);
    return M->cc ? solve1_finish<true>(M, iters_out, resnorm_out, extra, st) : solve1_finish<false>(M, iters_out, resnorm_out, extra, st);
}

int mg_solve1 (Multigrid* M, hps_slab s, int sol_comp, int rhs_comp, int acf_comp, double tol_rel, double tol_abs,
               int max_iters, int* iters_out, double* resnorm_out, hipStream_t st)
{
    if (int e = mg_solve1_begin(M, s, sol_comp, rhs_comp, acf_comp, tol_rel, tol_abs, max_iters, st)) return e;
    return mg_solve1_finish(M, iters_out, resnorm_out, nullptr, st);
}

} // namespace hps

using namespace hps;

extern "C" int hps_mg_create (int nx, int ny, double dx, double dy, void** handle)
{
    HPS_REQUIRE(nx >= 2 && ny >= 2 && handle, "hps_mg_create: bad size");
    Multigrid* M = nullptr;
    if (int e = mg_create(nx, ny, dx, dy, &M)) return e;
    *handle = M;
    return HPS_OK;
}

extern "C" int hps_mg_info (void* handle, int* cc, int* nlev, int* lowv_begin, int* lowv_kind, long* lowv_lds, int* tiles,
                            int* nodal_pull1, int* pyr_levels, int* pyr_restricts)
{
    HPS_REQUIRE(handle, "hps_mg_info: null handle");
    const Multigrid* M = static_cast<const Multigrid*>(handle);
    const int lb = M->lowv_begin;
    if (cc) *cc = M->cc;
    if (nlev) *nlev = M->nlev();
    if (lowv_begin) *lowv_begin = lb;
    if (lowv_kind) *lowv_kind = M->bottom ? HPS_MG_LOWV_BOTTOM : M->use_low3 ? HPS_MG_LOWV_V3 : M->cc ? HPS_MG_LOWV_CC : HPS_MG_LOWV_NODAL;
    if (lowv_lds) *lowv_lds = (long)(M->use_low3 ? M->low3_lds : M->low_lds);
    if (tiles) {
        // as launch_smooth and vcycle's pulls choose them: level 0's initial pass, then the down-leg of levels 1 .. lb - 1
        for (int il = 0; il < HPS_MG_MAXLEV; ++il) {
            int t = -1;
            if (il < lb) {
                const bool small = M->L[il].cells <= SMALL_TILE_CELLS;
                t = M->pulls(il) ? (small ? HPS_MG_TILE_SMALL_PULL : HPS_MG_TILE_MID_PULL) : (small ? HPS_MG_TILE_SMALL : HPS_MG_TILE_BIG);
            }
            tiles[il] = t;
        }
    }
    if (nodal_pull1) *nodal_pull1 = M->nodal_pull1;
    if (pyr_levels) *pyr_levels = std::min(lb, M->cc ? 5 : NPYR_MAX);
    if (pyr_restricts) *pyr_restricts = lb - std::min(lb, M->cc ? 5 : NPYR_MAX);
    return HPS_OK;
}

extern "C" int hps_mg_info_schedule (void* handle, int* coef_guest)
{
    HPS_REQUIRE(handle, "hps_mg_info_schedule: null handle");
    if (coef_guest) *coef_guest = static_cast<const Multigrid*>(handle)->coef_guest ? 1 : 0;
    return HPS_OK;
}

extern "C" int hps_mg_info_upleg (void* handle, int* fused_levels)
{
    HPS_REQUIRE(handle, "hps_mg_info_upleg: null handle");
    if (fused_levels) *fused_levels = static_cast<const Multigrid*>(handle)->up_fused;
    return HPS_OK;
}

extern "C" int hps_mg_solve1 (void* handle, hps_slab slab, int sol_comp, int rhs_comp, int acoef_comp, double tol_rel,
                              double tol_abs, int max_iters, int* iters_host, double* resnorm_host, hps_stream stream)
{
    HPS_REQUIRE(handle && slab.p, "hps_mg_solve1: null argument");
    Multigrid* M = static_cast<Multigrid*>(handle);
    HPS_REQUIRE(slab.nx == M->nx && slab.ny == M->ny, "hps_mg_solve1: slab size does not match the solver");
    HPS_REQUIRE(sol_comp >= 0 && sol_comp + 1 < slab.ncomp && rhs_comp >= 0 && rhs_comp + 1 < slab.ncomp &&
                acoef_comp >= 0 && acoef_comp < slab.ncomp, "hps_mg_solve1: bad component");
    HPS_REQUIRE(M->cc || slab.ng >= 1, "hps_mg_solve1: node-centred solve needs >= 1 guard cell");
    HPS_REQUIRE(slab.nstride < (1L << 27) && slab.ng <= 8, "hps_mg_solve1: planes of at most 2^27 doubles and at most 8 guard cells (32-bit byte offsets in the kernels)");
    return mg_solve1(M, slab, sol_comp, rhs_comp, acoef_comp, tol_rel, tol_abs, max_iters, iters_host, resnorm_host,
                     (hipStream_t)stream);
}

// hpmg::MultiGrid::solve1 with its own argument list (HpMultiGrid.H:64-66: FArrayBox& sol, FArrayBox const& rhs,
// FArrayBox const& acoef): three separate views -- sol and rhs with two components each, acoef with one -- that need
// not live in one slab.  Each view is centred on the solver's box as center_box does (HpMultiGrid.H:168-175).
extern "C" int hps_mg_solve1_fabs (void* handle, hps_slab sol2, hps_slab rhs2, hps_slab acoef1, double tol_rel, double tol_abs,
                                   int max_iters, int* iters_host, double* resnorm_host, hps_stream stream)
{
    HPS_REQUIRE(handle && sol2.p && rhs2.p && acoef1.p, "hps_mg_solve1_fabs: null argument");
    Multigrid* M = static_cast<Multigrid*>(handle);
    for (const hps_slab* s : {&sol2, &rhs2, &acoef1}) {
        HPS_REQUIRE(s->nx == M->nx && s->ny == M->ny, "hps_mg_solve1_fabs: view size does not match the solver");
        HPS_REQUIRE(M->cc || s->ng >= 1, "hps_mg_solve1_fabs: node-centred solve needs >= 1 guard cell in every view");
    }
    HPS_REQUIRE(sol2.ncomp >= 2 && rhs2.ncomp >= 2 && acoef1.ncomp >= 1, "hps_mg_solve1_fabs: sol and rhs need two components, acoef one");
    const int sh = M->cc ? 0 : 1;
    HPS_REQUIRE(sol2.nstride < (1L << 27) && rhs2.nstride < (1L << 27) && acoef1.nstride < (1L << 27), "hps_mg_solve1_fabs: planes of at most 2^27 doubles (32-bit byte offsets in the kernels)");
    M->sol  = FView{sol2.p, sol2.jstride, sol2.nstride, sol2.ng - sh, sol2.ng - sh};
    M->rhs  = FView{rhs2.p, rhs2.jstride, rhs2.nstride, rhs2.ng - sh, rhs2.ng - sh};
    M->acf0 = FView{acoef1.p, acoef1.jstride, acoef1.nstride, acoef1.ng - sh, acoef1.ng - sh};
    hipStream_t st = (hipStream_t)stream;
    if (int e = M->cc ? solve1_begin<true>(M, tol_rel, tol_abs, max_iters, st) : solve1_begin<false>(M, tol_rel, tol_abs, max_iters, st)) return e;
    return mg_solve1_finish(M, iters_host, resnorm_host, nullptr, st);
}

// debug: first call arms the stamps, later calls read the 16 slots back
// A header slot of the norm buffer for the caller's own device counters: they reach the host with the read-back
// every solve does anyway (the engine's halo-fallback counter uses word 0).
void mg_rider (void* handle, int** dev_words, const int** host_words)
{
    Multigrid* M = static_cast<Multigrid*>(handle);
    *dev_words = reinterpret_cast<int*>(M->d_buf);
    *host_words = reinterpret_cast<const int*>(M->h_buf);
}

extern "C" int hps_mg_debug_stamps (long long* stamps16_host)
{
#ifndef HPS_STAMPS
    (void)stamps16_host; set_error("hps_mg_debug_stamps: the library was built without -DHPS_STAMPS (make stamps)"); return HPS_ERR_UNSUPPORTED;
#else
    static long long* d = nullptr;
    if (!d) {
        HPS_HIP_CHECK(hipMalloc(&d, 48*sizeof(long long)));
        HPS_HIP_CHECK(hipMemset(d, 0, 48*sizeof(long long)));
        HPS_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_mg_dbg), &d, sizeof(d)));
        return HPS_OK;
    }
    HPS_HIP_CHECK(hipDeviceSynchronize());
    HPS_HIP_CHECK(hipMemcpy(stamps16_host, d, 48*sizeof(long long), hipMemcpyDeviceToHost));
    return HPS_OK;
#endif
}

extern "C" int hps_mg_destroy (void* handle)
{
    delete static_cast<Multigrid*>(handle);
    return HPS_OK;
}
