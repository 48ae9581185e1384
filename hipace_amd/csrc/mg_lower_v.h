// mg_lower_v.h -- k_lower_v<CC>: every level of at most ~32 x 32 unknowns in one 1024-thread workgroup, all arrays in LDS (the
// node-centred lower V, and the cell-centred one of the grids k_lower_v3 does not take), with its LowLev / LView views and
// low_* phases.  Needs mg_stencil.h only.
#ifndef HPS_MG_LOWER_V_H_
#define HPS_MG_LOWER_V_H_

#include "mg_stencil.h"
#include <type_traits>

namespace hps {

// ---- all small levels in one workgroup, LDS resident --------------------------------------------
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
    for (int il = 0; il < nl; ++il) { const LowLev l = lv[il]; low_cinv_level<CC>(base, l, lvl_fac(facx0, il), lvl_fac(facy0, il)); }
    __syncthreads();
    MG_STAMP(10);
    for (int il = 0; il < nl - 1; ++il) { const LowLev l = lv[il], c = lv[il + 1]; low_down_level<CC>(base, l, c, lvl_fac(facx0, il), lvl_fac(facy0, il), n0, n1); }
    MG_STAMP(11);
    {
        const LowLev l = lv[nl - 1];
        if (l.b.vhx - l.b.vlx < 3 && l.b.vhy - l.b.vly < 3)
            low_bottom_lane<CC>(base, l, lvl_fac(facx0, nl - 1), lvl_fac(facy0, nl - 1), nsweeps_bottom, n0, n1);
        else
        low_sweeps<CC>(base, l, lvl_fac(facx0, nl - 1), lvl_fac(facy0, nl - 1), nsweeps_bottom, n0, n1);
    }
    MG_STAMP(12);
    for (int il = nl - 2; il >= 0; --il) { const LowLev l = lv[il], c = lv[il + 1]; low_up_level<CC>(base, l, c, lvl_fac(facx0, il), lvl_fac(facy0, il), n0, n1); }
    MG_STAMP(13);
    {
        const LowLev l = lv[0];
        for (int s = n0*l.cells + threadIdx.x; s < n1*l.cells; s += blockDim.x) cor_g[s] = base[l.off + 3*l.cells + s];
    }
    MG_STAMP(14);
}

} // namespace hps
#endif
