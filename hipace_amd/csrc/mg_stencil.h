// mg_stencil.h -- what every kernel family of multigrid.hip shares: the level views and boxes (FView, LevBox), the smoother's
// tile shapes, the operator's stencil at a cell (diag_c0, offdiag*, wall_mult, residual_*, gs_cell), the transfer operators
// (prolong_at, restrict_at), the workgroup max-norm (block_max_to), the HPS_KEEP / MG_STAMP macros and the small helpers of
// the lower Vs and the pyramid (lds_double, cc_box, lvl_fac).  It owns no kernel and needs none of the other mg_*.h.
#ifndef HPS_MG_STENCIL_H_
#define HPS_MG_STENCIL_H_

#include "common.h"
#include "mg_gate.h"

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

// coarse = R(fine): 4-average (cell-centred) or 9-point full weighting (nodal)
template <bool CC>
__device__ __forceinline__ double restrict_at (const FView& fine, int i, int j, int n)
{
    if (CC) return 0.25*(fine(2*i, 2*j, n) + fine(2*i+1, 2*j, n) + fine(2*i, 2*j+1, n) + fine(2*i+1, 2*j+1, n));
    return (1./16.)*(fine(2*i-1, 2*j-1, n) + 2.*fine(2*i, 2*j-1, n) + fine(2*i+1, 2*j-1, n)
                   + 2.*fine(2*i-1, 2*j, n) + 4.*fine(2*i, 2*j, n) + 2.*fine(2*i+1, 2*j, n)
                   + fine(2*i-1, 2*j+1, n) + 2.*fine(2*i, 2*j+1, n) + fine(2*i+1, 2*j+1, n));
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

// ---- shared by the LDS-resident lower Vs (mg_lower_v.h, mg_lower_v3.h) and the coefficient pyramid (mg_pyramid.h)
typedef __attribute__((address_space(3))) double lds_double;

__device__ __forceinline__ LevBox cc_box (int nx, int ny) { return LevBox{0, 0, nx - 1, ny - 1, 0, 0, nx - 1, ny - 1}; }

// facx / facy of level l below a level with f0: a quarter per level (exact: powers of two)
__device__ __forceinline__ double lvl_fac (double f0, int l) { for (int k = 0; k < l; ++k) f0 *= 0.25; return f0; }

} // namespace hps
#endif
