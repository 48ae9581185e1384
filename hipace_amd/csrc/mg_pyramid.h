// mg_pyramid.h -- the coefficient hierarchy of a solve: k_acf_pyramid (cell-centred, five levels per launch),
// k_hierarchy_gradpsi (the same with the engine's -grad Psi / Sx, Sy pass behind its blocks), k_nodal_acf_pyramid<NP>
// (node-centred) and k_level_cinv.  Needs mg_stencil.h, and slab_ops.h for the engine's pass.
#ifndef HPS_MG_PYRAMID_H_
#define HPS_MG_PYRAMID_H_

#include "mg_stencil.h"
#include "slab_ops.h"

namespace hps {

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

} // namespace hps
#endif
