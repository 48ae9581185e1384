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
//
// This file is the host side: the Multigrid state, mg_create, the launchers, vcycle, the solve in two halves, the engine-facing
// interface (multigrid.h) and the C ABI.  The kernels are in headers it includes, one per family -- one translation unit,
// because they share inline device code and vcycle names instances of all of them: mg_stencil.h (views, tile shapes, the
// stencil), mg_smooth.h (k_smooth, k_restrict, k_copy2, k_bottom_sweep), mg_up_fused.h (k_up_fused), mg_lower_v.h
// (k_lower_v), mg_lower_v3.h (k_lower_v3 and the coefficient guest), mg_pyramid.h (the coefficient pyramids).
#include "common.h"
#include "multigrid.h"
#include "mg_stencil.h"
#include "mg_lower_v.h"
#include "mg_lower_v3.h"
#include "mg_smooth.h"
#include "mg_up_fused.h"
#include "mg_pyramid.h"

#include <vector>
#include <memory>
#include <algorithm>
#include <cmath>
#include <cstring>

namespace hps {

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
    int down_tile[HPS_MG_MAXLEV];               // HPS_MG_TILE_* of level 0's initial pass and of the down-leg smoother of levels 1 .. lowv_begin - 1; -1 from lowv_begin on (mg_create)
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

static int mg_create (int nx, int ny, double dx, double dy, Multigrid** out)
{
    if (nx % 2 != ny % 2) { set_error("hps_mg_create: nx and ny must have the same parity"); return HPS_ERR_ARG; }
    HPS_REQUIRE((long)(nx + 16)*(ny + 16) < (1L << 27), "hps_mg_create: the kernels address a two-component plane pair by 32-bit byte offsets (at most 2^27 cells per plane)");
    std::unique_ptr<Multigrid> M(new Multigrid);      // (a failure below frees what has been allocated: ~Multigrid)
    M->cc = (nx % 2 == 0); M->nx = nx; M->ny = ny; M->dx = dx; M->dy = dy;
    // level boxes (ctor, HpMultiGrid.cpp:1043-1072)
    int hx = M->cc ? nx - 1 : nx + 1, hy = M->cc ? ny - 1 : ny + 1;
    for (int il = 0; il < 31; ++il) {
        M->L.push_back(MGLevelDev{});
        MGLevelDev& l = M->L.back();
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
        bool ok;
        const int nxl = hx + 1, nyl = hy + 1;
        if (M->cc) { ok = nxl >= 4 && nyl >= 4 && nxl % 2 == 0 && nyl % 2 == 0; if (ok) { hx = nxl/2 - 1; hy = nyl/2 - 1; } }
        else       { ok = nxl >= 8 && nyl >= 8 && hx % 2 == 0 && hy % 2 == 0;   if (ok) { hx /= 2; hy /= 2; } }
        if (!ok) break;
    }
    if (M->nlev() < 2) { set_error("hps_mg_create: grid too small to coarsen"); return HPS_ERR_ARG; }
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
    // the smoother tiles, decided here once: vcycle's down-leg switches on them, hps_mg_info reports them.  A level that pulls
    // sweeps 32 x 16 tiles, or 32 x 32 where it is too large for those (vcycle); the others follow launch_smooth's rule
    for (int il = 0; il < HPS_MG_MAXLEV; ++il) {
        M->down_tile[il] = -1;
        if (il >= M->lowv_begin) continue;
        const bool small = M->L[il].cells <= SMALL_TILE_CELLS;
        M->down_tile[il] = M->pulls(il) ? (small ? HPS_MG_TILE_SMALL_PULL : HPS_MG_TILE_MID_PULL) : (small ? HPS_MG_TILE_SMALL : HPS_MG_TILE_BIG);
    }
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
    *out = M.release();
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
        const FView cor = M->lv(il, M->L[il].cor), res = M->lv(il, M->L[il].res), acf = M->lv(il, M->L[il].acf), rescor = M->lv(il, M->L[il].rescor);
        const FView cres = M->lv(il+1, M->L[il+1].res);
        switch (M->down_tile[il]) {       // (mg_create)
        case HPS_MG_TILE_SMALL:
            launch_smooth_ts<TileSmall, CC, SRC_ZERO, true>(M, il, cor, none, res, acf, none, none, rescor, cres, nullptr, nullptr, sr, st);
            break;
        case HPS_MG_TILE_BIG:
            launch_smooth_ts<TileBig, CC, SRC_ZERO, true>(M, il, cor, none, res, acf, none, none, rescor, cres, nullptr, nullptr, sr, st);
            break;
        case HPS_MG_TILE_SMALL_PULL:
            if constexpr (!CC)
                launch_smooth_ts<TileSmall, CC, SRC_ZERO, true, 4, true>(M, il, cor, none, res, acf, none, M->lv(il-1, M->L[il-1].rescor), rescor, cres, nullptr, nullptr, sr, st);
            break;
        case HPS_MG_TILE_MID_PULL:
            if constexpr (!CC)
                launch_smooth_ts<TileMid, CC, SRC_ZERO, true, 4, true>(M, il, cor, none, res, acf, none, M->lv(il-1, M->L[il-1].rescor), rescor, cres, nullptr, nullptr, sr, st);
            break;
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

static int mg_solve1 (Multigrid* M, hps_slab s, int sol_comp, int rhs_comp, int acf_comp, double tol_rel, double tol_abs,
               int max_iters, int* iters_out, double* resnorm_out, hipStream_t st)
{
    if (int e = mg_solve1_begin(M, s, sol_comp, rhs_comp, acf_comp, tol_rel, tol_abs, max_iters, st)) return e;
    return mg_solve1_finish(M, iters_out, resnorm_out, nullptr, st);
}

// A header slot of the norm buffer for the caller's own device counters: they reach the host with the read-back
// every solve does anyway (the engine's halo-fallback counter uses word 0).
void mg_rider (void* handle, int** dev_words, const int** host_words)
{
    Multigrid* M = static_cast<Multigrid*>(handle);
    *dev_words = reinterpret_cast<int*>(M->d_buf);
    *host_words = reinterpret_cast<const int*>(M->h_buf);
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
    if (tiles) std::copy(M->down_tile, M->down_tile + HPS_MG_MAXLEV, tiles);
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

// debug: first call arms the stamps, later calls read the 48 slots back
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
