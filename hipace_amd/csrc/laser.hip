// laser.hip -- laser envelope on the device: the Gaussian initial envelope, |a|^2 for the plasma operators and the
// FFT envelope solver that advances the pulse by one time step, slice by slice.
//
// Reference: laser/MultiLaser.cpp -- InitLaserSlice :803-921 (Gaussian branch :881-919, Laser.H defaults: no
// carrier-envelope phase, no propagation angle, no pulse-front tilt), UpdateLaserAabs :214-291, AdvanceSliceFFT
// :609-801 (Benedetti et al. 2017 scheme with the on-axis phase terms of lasers.use_phase), and the hand-over of the
// time levels between two steps, utils/MultiBuffer.cpp:840-852, 913-925.
// Several pulses with CEP, propagation angle and pulse-front tilt, envelopes from samples (Laser.cpp:117-341) and the in-situ
// reductions (InSituComputeDiags :923-1003) are DESIGN 8k: k_laser_init_pulses, k_laser_add, k_laser_resample, k_insitu_laser.
//
// Layout: three complex arrays [nz][ny][nx] (a at time steps n-1, n, n+1), 16 B per cell, resident in HBM for the whole
// run -- 1024^2 x 2048 slices are 3 x 34 GB, which is what 288 GB per GPU are for; the reference streams them through
// host buffers.  Without lasers.n_cell / patch_* the laser grid is the field grid and lasers.interp_order = 1, so chi
// and |a|^2 pass between the two grids cell by cell.  With them (hps_engine_set_laser_grid) the arrays are
// [zeta_hi - zeta_lo + 1][nyl][nxl] on the laser's patch and two interpolation kernels carry |a|^2 to the field grid
// (UpdateLaserAabs :253-284) and chi to the laser grid (SetInitialChi :293-332, InterpolateChi :334-407).
#include "common.h"
#include "engine.h"
#include "expr.h"
#include "multigrid.h"

#include <rocfft/rocfft.h>
#include <algorithm>
#include <cmath>

namespace hps {

struct LaserPhase { double2 exp1, exp2; double djn, pad; };

struct LaserState {
    int nx = 0, ny = 0, nz = 0;                                    // cells of the laser grid (the field grid's unless a grid is set)
    int zlo = 0;                                                   // field slice of the laser's slice 0
    double dx = 0.0, dy = 0.0, xoff = 0.0, yoff = 0.0, lenx = 0.0, leny = 0.0;      // cell size, GetPosOffset, patch length
    bool grid = false;                                             // hps_engine_set_laser_grid
    double *chi = nullptr, *chi_initial = nullptr;                 // [ny][nx], grid only: chi the envelope solver reads, chi of the unperturbed plasma
    double2 *nm1 = nullptr, *n00 = nullptr, *np1 = nullptr;      // [nz][ny][nx]
    double2* work = nullptr;                                       // [ny][nx] right-hand side / solution
    LaserPhase* phase = nullptr;
    rocfft_plan fwd = nullptr, bwd = nullptr; rocfft_execution_info info = nullptr; void* fft_work = nullptr;
    // lasers.solver_type = multigrid (multigrid2.hip): planar [2][ny][nx] solution (kept from slice to slice: the next
    // solve's initial guess, as np1j00 in the reference) and right-hand side, Re of the coefficient, its Im (one double)
    void* mg = nullptr; double *mg_sol = nullptr, *mg_rhs = nullptr, *mg_acf_real = nullptr, *mg_acf_imag = nullptr; long mg_vcycles = 0;
    double *insitu = nullptr, *insitu_part = nullptr;              // hps_engine_set_insitu_laser: [8][nz] rows, [INSITU_GROUPS][8] partial rows
    int steps = 0; bool initialised = false;
    bool import_mode = false;        // ring pipeline: a_n, a_{n-1} of the coming step arrive through laser_import_slice
    ~LaserState () {
        if (fwd) rocfft_plan_destroy(fwd);
        if (bwd) rocfft_plan_destroy(bwd);
        if (info) rocfft_execution_info_destroy(info);
        (void)hipFree(nm1); (void)hipFree(n00); (void)hipFree(np1); (void)hipFree(work); (void)hipFree(phase); (void)hipFree(fft_work);
        if (mg) mg2_destroy_internal(mg);
        (void)hipFree(mg_sol); (void)hipFree(mg_rhs); (void)hipFree(mg_acf_real); (void)hipFree(mg_acf_imag);
        (void)hipFree(chi); (void)hipFree(chi_initial);
        (void)hipFree(insitu); (void)hipFree(insitu_part);
    }
};

__device__ __forceinline__ double2 cmul (double2 a, double2 b) { return make_double2(a.x*b.x - a.y*b.y, a.x*b.y + a.y*b.x); }
__device__ __forceinline__ double2 cadd (double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub (double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cscale (double s, double2 a) { return make_double2(s*a.x, s*a.y); }

struct LaserPars { double a0, w0, L0, k0, x0, y0, z0, zfoc; };

// Gaussian envelope of every slice (InitLaserSlice :881-919)
__global__ __launch_bounds__(256)
void k_laser_init (double2* a, int nx, int ny, int nz, LaserPars L, double dx, double dy, double dz, double xoff, double yoff, double zoff)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    const int j = blockIdx.y, k = blockIdx.z;
    if (i >= nx) return;
    const double x = i*dx + xoff - L.x0, y = j*dy + yoff - L.y0, zp = k*dz + zoff - L.z0;
    // diffract_factor D = 1 + i q, q = (zp - zfoc + z0) 2/(k0 w0^2)
    const double q = (zp - L.zfoc + L.z0)*2.0/(L.k0*L.w0*L.w0);
    const double den = 1.0 + q*q;
    const double dr = 1.0/den, di = -q/den;                     // 1/D
    const double wr = dr/(L.w0*L.w0), wi = di/(L.w0*L.w0);       // 1/(w0^2 D)
    const double r2 = x*x + y*y;
    const double er = -r2*wr - zp*zp/(L.L0*L.L0), ei = -r2*wi;   // exponent
    const double m = exp(er);
    double sn, cs; sincos(ei, &sn, &cs);
    const double ar = L.a0*dr, ai = L.a0*di;                     // prefactor a0/D
    a[((long)k*ny + j)*nx + i] = make_double2(m*(ar*cs - ai*sn), m*(ar*sn + ai*cs));
}

// The same for a list of pulses (hps_engine_set_laser_pulses), each with carrier-envelope phase, propagation angle and pulse-front
// tilt, literally InitLaserSlice :876-915: rotation of (y, z) by rot = propagation_angle_yz + (PFT_yz - pi/2), z0 cos(angle) in
// the diffraction factor and the factor exp(i yp k0 angle + CEP) -- CEP is added to the exponent as a real number there, so it
// scales the pulse by e^CEP; restated, not corrected.  One exp and one sincos per pulse and cell; the list is a kernel argument.
struct LaserPulse { double a0, w0, L0, x0, y0, z0, zfoc, cep, angle, cos_angle, cos_rot, sin_rot; };
struct LaserPulseList { int n; LaserPulse p[8]; };

__global__ __launch_bounds__(256)
void k_laser_init_pulses (double2* a, int nx, int ny, int nz, LaserPulseList P, double k0, double dx, double dy, double dz, double xoff, double yoff,
                          double zoff)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    const int j = blockIdx.y, k = blockIdx.z;
    if (i >= nx) return;
    double sr = 0.0, si = 0.0;
    for (int q = 0; q < P.n; ++q) {
        const LaserPulse& L = P.p[q];
        const double x = i*dx + xoff - L.x0, y = j*dy + yoff - L.y0, z = k*dz + zoff - L.z0;
        const double yp = L.cos_rot*y - L.sin_rot*z, zp = L.sin_rot*y + L.cos_rot*z;
        const double qd = (zp - L.zfoc + L.z0*L.cos_angle)*2.0/(k0*L.w0*L.w0);       // diffract_factor D = 1 + i qd
        const double den = 1.0 + qd*qd;
        const double dr = 1.0/den, di = -qd/den;                     // 1/D
        const double wr = dr/(L.w0*L.w0), wi = di/(L.w0*L.w0);       // 1/(w0^2 D)
        const double r2 = x*x + yp*yp;
        const double er = -r2*wr - zp*zp/(L.L0*L.L0) + L.cep, ei = -r2*wi + yp*k0*L.angle;   // exponent
        const double m = exp(er);
        double sn, cs; sincos(ei, &sn, &cs);
        const double ar = L.a0*dr, ai = L.a0*di;                     // prefactor a0/D
        sr += m*(ar*cs - ai*sn); si += m*(ar*sn + ai*cs);
    }
    a[((long)k*ny + j)*nx + i] = make_double2(sr, si);
}

// samples on the laser grid itself (geometry 0, the reference's parser type :856-874): a plain add
__global__ __launch_bounds__(256)
void k_laser_add (double2* __restrict__ a, const double2* __restrict__ s, long n)
{
    const long o = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (o < n) { const double2 v = a[o], w = s[o]; a[o] = make_double2(v.x + w.x, v.y + w.y); }
}

// order-1 shape factor of a sample axis with n samples (compute_shape_factor<1>): false = the stencil lies wholly outside
// 0 .. n-1 (also keeps floor() in int range)
__device__ __forceinline__ bool sample_stencil (double mid, long n, int* cell, double* s)
{
    if (!(mid > -2.0 && mid < (double)n + 1.0)) return false;
    *cell = shape_weights<1>(mid, s);
    return true;
}

// Envelope from a file's samples (Laser::GetEnvelopeFromFile, Laser.cpp:177-336), one thread per laser cell, added to a.
// geometry 1 "xyt": data [nt][ny][nx], 2 "xyz": [nz][ny][nx], 3 "rt": [modes][nt][nr]; off = position of sample 0 per axis in
// the file's order (t of xyt and rt starts at the laser's last slice: tmid = (zmax - z)/c/spacing[0]); samples outside the
// extent count as zero.  The sums run in the reference's order: t or z outermost, then y, then x; per (t, r) mode 0, then cos
// and sin part of m = 1 .. modes/2.
struct LaserFile { int geometry; int e0, e1, e2; double off0, off1, off2, sp0, sp1, sp2, unit; };

__global__ __launch_bounds__(256)
void k_laser_resample (double2* __restrict__ a, int nx, int ny, int nz, const double2* __restrict__ data, LaserFile F, double clight,
                       double dx, double dy, double dz, double xoff, double yoff, double zoff)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    const int j = blockIdx.y, k = blockIdx.z;
    if (i >= nx) return;
    const double x = i*dx + xoff, y = j*dy + yoff, z = k*dz + zoff, zmax = (nz - 1)*dz + zoff;
    double vr = 0.0, vi = 0.0;
    if (F.geometry == 3) {
        const double r = sqrt(x*x + y*y), theta = atan2(y, x);
        double sr[2], st[2]; int ic, kc;
        if (sample_stencil((r - F.off1)/F.sp1, F.e2, &ic, sr) && sample_stencil((zmax - z)/clight/F.sp0, F.e1, &kc, st)) {
            for (int it = 0; it <= 1; ++it)
                for (int ir = 0; ir <= 1; ++ir) {
                    const int cr = ic + ir, ct = kc + it;
                    if (cr < 0 || cr >= F.e2 || ct < 0 || ct >= F.e1) continue;       // (cr < 0 is refused on the host)
                    const long o = (long)ct*F.e2 + cr, mode = (long)F.e1*F.e2;
                    const double w = sr[ir]*st[it];
                    const double2 d0 = data[o];
                    vr += w*(d0.x*F.unit); vi += w*(d0.y*F.unit);
                    for (int im = 1; im <= F.e0/2; ++im) {
                        double sn, cs; sincos(im*theta, &sn, &cs);
                        const double2 dc = data[(2*im - 1)*mode + o], ds = data[2*im*mode + o];
                        vr += w*cs*(dc.x*F.unit); vi += w*cs*(dc.y*F.unit);
                        vr += w*sn*(ds.x*F.unit); vi += w*sn*(ds.y*F.unit);
                    }
                }
        }
    } else {
        const double zmid = (F.geometry == 1) ? (zmax - z)/clight/F.sp0 : (z - F.off0)/F.sp0;
        double sx[2], sy[2], sz[2]; int ic, jc, kc;
        if (sample_stencil((x - F.off2)/F.sp2, F.e2, &ic, sx) && sample_stencil((y - F.off1)/F.sp1, F.e1, &jc, sy) &&
            sample_stencil(zmid, F.e0, &kc, sz)) {
            for (int iz = 0; iz <= 1; ++iz)
                for (int iy = 0; iy <= 1; ++iy)
                    for (int ix = 0; ix <= 1; ++ix) {
                        const int cx = ic + ix, cy = jc + iy, cz = kc + iz;
                        if (cx < 0 || cx >= F.e2 || cy < 0 || cy >= F.e1 || cz < 0 || cz >= F.e0) continue;
                        const double2 d = data[((long)cz*F.e1 + cy)*F.e2 + cx];
                        const double w = sx[ix]*sy[iy]*sz[iz];
                        vr += w*(d.x*F.unit); vi += w*(d.y*F.unit);
                    }
        }
    }
    const long o = ((long)k*ny + j)*nx + i;
    const double2 v = a[o];
    a[o] = make_double2(v.x + vr, v.y + vi);
}

// In-situ reductions of one laser plane (InSituComputeDiags :923-1003): max |a|^2, the sums of |a|^2 {1, x, x^2, y, y^2} and of a
// over the middle cells.  Eight values per lane over a grid-stride loop, through the wave with __shfl_xor, through LDS, one
// partial row per workgroup; k_insitu_laser_fold adds the rows in index order.  No floating-point atomics: the launch shape
// depends on the plane's size alone, so the result is a function of the plane, bit for bit.
constexpr int INSITU_GROUPS = 32;

__global__ __launch_bounds__(256)
void k_insitu_laser (const double2* __restrict__ a, int nx, int ny, double dx, double dy, double xoff, double yoff, double* __restrict__ part)
{
    const int xmid_lo = (nx - 1)/2, xmid_hi = nx/2, ymid_lo = (ny - 1)/2, ymid_hi = ny/2;
    const long plane = (long)nx*ny;
    double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    // a lane takes the cells o, o + S, o + 2 S, ... in this order, four loads in flight at a time; (i, j) of the next cell by
    // carry from (S mod nx, S div nx) instead of a division per cell
    const long S = (long)gridDim.x*blockDim.x;
    const int di = (int)(S % nx), dj = (int)(S/nx);
    long o = (long)blockIdx.x*blockDim.x + threadIdx.x;
    int j = (int)(o/nx), i = (int)(o - (long)j*nx);
    for (; o < plane; o += 4*S) {
        double2 e[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) e[u] = (o + u*S < plane) ? a[o + u*S] : make_double2(0.0, 0.0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (o + u*S >= plane) break;
            const double s = e[u].x*e[u].x + e[u].y*e[u].y;
            const double x = i*dx + xoff, y = j*dy + yoff;
            const bool on_axis = (i == xmid_lo || i == xmid_hi) && (j == ymid_lo || j == ymid_hi);
            v[0] = s > v[0] ? s : v[0];
            v[1] += s; v[2] += s*x; v[3] += s*x*x; v[4] += s*y; v[5] += s*y*y;
            v[6] += on_axis ? e[u].x : 0.0; v[7] += on_axis ? e[u].y : 0.0;
            i += di; j += dj;
            if (i >= nx) { i -= nx; ++j; }
        }
    }
    for (int m = 32; m > 0; m >>= 1) {
        const double w = __shfl_xor(v[0], m);
        v[0] = w > v[0] ? w : v[0];
        for (int q = 1; q < 8; ++q) v[q] += __shfl_xor(v[q], m);
    }
    __shared__ double wave[4][8];
    if ((threadIdx.x & 63) == 0) for (int q = 0; q < 8; ++q) wave[threadIdx.x >> 6][q] = v[q];
    __syncthreads();
    if (threadIdx.x < 8) {
        const int q = threadIdx.x;
        double r = wave[0][q];
        for (int w = 1; w < 4; ++w) r = (q == 0) ? (wave[w][q] > r ? wave[w][q] : r) : r + wave[w][q];
        part[(long)blockIdx.x*8 + q] = r;
    }
}

// one wave: lane q < 8 folds row q of the partials in index order and writes column `col` of out[8][ncol]
__global__ __launch_bounds__(64)
void k_insitu_laser_fold (const double* __restrict__ part, int groups, double dxdydz, double mid_factor, double* __restrict__ out, int ncol, int col)
{
    const int q = threadIdx.x;
    if (q >= 8) return;
    double r = part[q];
    for (int g = 1; g < groups; ++g) { const double w = part[(long)g*8 + q]; r = (q == 0) ? (w > r ? w : r) : r + w; }
    out[(long)q*ncol + col] = (q == 0) ? r : (q < 6 ? r*dxdydz : r*mid_factor);
}

// UpdateLaserAabs (:214-291): aabs = |a_n|^2 on the valid cells, 0 in the guard cells; optionally sum |a_n|
__global__ __launch_bounds__(256)
void k_laser_aabs (SlabView f, int c_aabs, const double2* __restrict__ a, double* sum_abs)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x - f.ng;
    const int j = blockIdx.y - f.ng;
    double mag = 0.0;
    if (i < f.nx + f.ng) {
        double v = 0.0;
        if (i >= 0 && i < f.nx && j >= 0 && j < f.ny) {
            const double2 e = a[(long)j*f.nx + i];
            v = e.x*e.x + e.y*e.y;
            mag = sqrt(v);
        }
        f.p[c_aabs*f.ns + f.off(i, j)] = v;
    }
    if (sum_abs) {
        for (int o = 32; o > 0; o >>= 1) mag += __shfl_xor(mag, o);
        __shared__ double part[4];
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mag;
        __syncthreads();
        if (threadIdx.x == 0) atomic_add_f64(sum_abs, part[0] + part[1] + part[2] + part[3]);
    }
}

// UpdateLaserAabs on a laser grid of its own (:253-284): one thread per field cell, guard cells included (the reference
// runs over the grown box); |a|^2 is formed in the gather -- the laser plane is small and stays in L2, no |a|^2 plane is
// written.  Laser cells outside 0 .. nxl-1 x 0 .. nyl-1 contribute nothing, so a field cell away from the patch gets 0.
template <int ORDER>
__global__ __launch_bounds__(256)
void k_laser_interp_aabs (SlabView f, int c_aabs, const double2* __restrict__ a, int nxl, int nyl, double dxf, double dyf,
                          double xofff, double yofff, double dxl_inv, double dyl_inv, double xoffl, double yoffl)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x - f.ng;
    const int j = blockIdx.y - f.ng;
    if (i >= f.nx + f.ng) return;
    const double xmid = (i*dxf + xofff - xoffl)*dxl_inv;
    const double ymid = (j*dyf + yofff - yoffl)*dyl_inv;
    double v = 0.0;
    // (the stencil of a point further than 3 cells from the patch holds no laser cell; also keeps floor() in int range)
    if (xmid > -3.0 && xmid < nxl + 2.0 && ymid > -3.0 && ymid < nyl + 2.0) {
        double sx[4], sy[4];
        const int i0 = shape_weights<ORDER>(xmid, sx), j0 = shape_weights<ORDER>(ymid, sy);
        for (int iy = 0; iy <= ORDER; ++iy) {
            const int cy = j0 + iy;
            if (cy < 0 || cy >= nyl) continue;
            for (int ix = 0; ix <= ORDER; ++ix) {
                const int cx = i0 + ix;
                if (cx < 0 || cx >= nxl) continue;
                const double2 e = a[(long)cy*nxl + cx];
                v += sx[ix]*sy[iy]*(e.x*e.x + e.y*e.y);
            }
        }
    }
    f.p[c_aabs*f.ns + f.off(i, j)] = v;
}

// sum |a_n| over the cells of one laser plane (the "laserEnvelope" checksum with a laser grid)
__global__ __launch_bounds__(256)
void k_laser_sum_abs (const double2* __restrict__ a, long n, double* sum_abs)
{
    const long o = (long)blockIdx.x*blockDim.x + threadIdx.x;
    double mag = 0.0;
    if (o < n) { const double2 e = a[o]; mag = sqrt(e.x*e.x + e.y*e.y); }
    for (int s = 32; s > 0; s >>= 1) mag += __shfl_xor(mag, s);
    __shared__ double part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mag;
    __syncthreads();
    if (threadIdx.x == 0) atomic_add_f64(sum_abs, part[0] + part[1] + part[2] + part[3]);
}

// SetInitialChi (:293-332): chi of the unperturbed plasma on the laser grid, "as if it were deposited there" -- the sum over
// the species of density(x, y, c t) q^2 mu0 / m (times init_level^2 for the ionisable one), with the engine's density:
// <plasma>.density, radius, hollow_core_radius and the tabulated f_r f_t.  f0, f1: density q^2 mu0 / m of the two species.
__global__ __launch_bounds__(256)
void k_laser_chi_initial (double* __restrict__ out, int nxl, int nyl, double dxl, double dyl, double xoffl, double yoffl, double f0, double f1,
                          const double* __restrict__ prof, int nr, double ft, double radius_sq, double hollow_sq)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= nxl) return;
    const double x = i*dxl + xoffl, y = j*dyl + yoffl;
    const double rsq = x*x + y*y;
    const double fac = (rsq > radius_sq || rsq < hollow_sq) ? 0.0 : ft*table_value(prof, prof + nr, nr, sqrt(rsq));
    out[(long)j*nxl + i] = fac*f0 + fac*f1;
}

// ... where a species' density is its program (hps_engine_set_density_expr): that species contributes
// prog(x, y, c t) f with f = q^2 mu0 / m (times init_level^2) alone, inside the radius and outside the hollow core; min_density
// is not applied (SetInitialChi does not).  A species whose p.n_ins is 0 contributes fac f as above.  Dynamic LDS: the
// programs' stack, [level][lane], the deeper of the two.
__global__ __launch_bounds__(256)
void k_laser_chi_initial_prog (double* __restrict__ out, int nxl, int nyl, double dxl, double dyl, double xoffl, double yoffl, double f0, double f1,
                               DensityProgram p0, DensityProgram p1, const double* __restrict__ prof, int nr, double ft, double radius_sq,
                               double hollow_sq)
{
    extern __shared__ double s_chi_stack[];
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= nxl) return;
    const double x = i*dxl + xoffl, y = j*dyl + yoffl;
    const double rsq = x*x + y*y;
    const bool in = !(rsq > radius_sq || rsq < hollow_sq);
    const double fac = in ? ft*table_value(prof, prof + nr, nr, sqrt(rsq)) : 0.0;
    ExprLdsStack st{s_chi_stack + threadIdx.x, (int)blockDim.x};
    double n0 = fac, n1 = fac;
    if (p0.n_ins > 0) { const ExprXyz v{x, y, p0.z}; const double val = expr_run(p0.ins, p0.n_ins, p0.consts, v, st); n0 = in ? val : 0.0; }
    if (p1.n_ins > 0) { const ExprXyz v{x, y, p1.z}; const double val = expr_run(p1.ins, p1.n_ins, p1.consts, v, st); n1 = in ? val : 0.0; }
    out[(long)j*nxl + i] = n0*f0 + n1*f1;
}

// ... and one further species (hps_engine_add_plasma_species) on top of the two: += n f, n its program's value or the
// tables', as above.  One launch per further species: the two kernels above stay what an engine without one launches.
__global__ __launch_bounds__(256)
void k_laser_chi_initial_add (double* __restrict__ out, int nxl, int nyl, double dxl, double dyl, double xoffl, double yoffl, double f,
                              DensityProgram p, const double* __restrict__ prof, int nr, double ft, double radius_sq, double hollow_sq)
{
    extern __shared__ double s_chi_stack[];
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= nxl) return;
    const double x = i*dxl + xoffl, y = j*dyl + yoffl;
    const double rsq = x*x + y*y;
    const bool in = !(rsq > radius_sq || rsq < hollow_sq);
    double n = in ? ft*table_value(prof, prof + nr, nr, sqrt(rsq)) : 0.0;
    if (p.n_ins > 0) {
        ExprLdsStack st{s_chi_stack + threadIdx.x, (int)blockDim.x};
        const ExprXyz v{x, y, p.z};
        const double val = expr_run(p.ins, p.n_ins, p.consts, v, st);
        n = in ? val : 0.0;
    }
    out[(long)j*nxl + i] += n*f;
}

// InterpolateChi (:334-407): one thread per laser cell.  Inside x_lo .. x_hi, y_lo .. y_hi (the laser cells on the field box
// shrunk by the guard width, :358-372) chi of the slab, interpolated; outside, chi of the unperturbed plasma.
template <int ORDER>
__global__ __launch_bounds__(256)
void k_laser_interp_chi (SlabView f, int c_chi, const double* __restrict__ chi_initial, double* __restrict__ chi_out, int nxl, int nyl,
                         double dxl, double dyl, double xoffl, double yoffl, double dxf_inv, double dyf_inv, double xofff, double yofff,
                         int x_lo, int x_hi, int y_lo, int y_hi)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= nxl) return;
    const long o = (long)j*nxl + i;
    if (!(x_lo <= i && i <= x_hi && y_lo <= j && j <= y_hi)) { chi_out[o] = chi_initial[o]; return; }
    const double xmid = (i*dxl + xoffl - xofff)*dxf_inv;
    const double ymid = (j*dyl + yoffl - yofff)*dyf_inv;
    double sx[4], sy[4];
    const int i0 = shape_weights<ORDER>(xmid, sx), j0 = shape_weights<ORDER>(ymid, sy);
    const double* __restrict__ src = f.p + c_chi*f.ns;
    double chi = 0.0;
    for (int iy = 0; iy <= ORDER; ++iy) {
        const int cy = j0 + iy;
        if (cy < -f.ng || cy >= f.ny + f.ng) continue;        // (a stencil wider than shrink + guard width: never in the engine)
        for (int ix = 0; ix <= ORDER; ++ix) {
            const int cx = i0 + ix;
            if (cx < -f.ng || cx >= f.nx + f.ng) continue;
            chi += sx[ix]*sy[iy]*src[f.off(cx, cy)];
        }
    }
    chi_out[o] = chi;
}

// on-axis phases of a_n on slices j, j+1, j+2 (the sum of the 1, 2 or 4 cells nearest the axis, as Wake-T; :651-697)
// -> exp(i(t_j - t_j+1)), exp(i(t_j - t_j+2)) and D_j^n.  One lane.
__global__ void k_laser_phase (const double2* j00, const double2* jp1, const double2* jp2, int nx, int ny, int use_phase, double dz,
                               LaserPhase* out)
{
    const int imid = (nx + 1)/2, jmid = (ny + 1)/2;
    double t[3] = {0.0, 0.0, 0.0};
    if (use_phase) {
        const double2* src[3] = {j00, jp1, jp2};
        for (int q = 0; q < 3; ++q) {
            double sr = 0.0, si = 0.0;
            if (src[q]) {
                for (int j = (ny % 2 == 0 ? jmid - 1 : jmid); j <= jmid; ++j)
                    for (int i = (nx % 2 == 0 ? imid - 1 : imid); i <= imid; ++i) { const double2 v = src[q][(long)j*nx + i]; sr += v.x; si += v.y; }
            }
            t[q] = atan2(si, sr);
        }
    }
    const double pi = 3.14159265358979323846;
    double dt1 = t[0] - t[1], dt2 = t[1] - t[2];
    if (dt1 < -1.5*pi) dt1 += 2.0*pi;
    if (dt1 >  1.5*pi) dt1 -= 2.0*pi;
    if (dt2 < -1.5*pi) dt2 += 2.0*pi;
    if (dt2 >  1.5*pi) dt2 -= 2.0*pi;
    LaserPhase p;
    double s, c;
    sincos(t[0] - t[1], &s, &c); p.exp1 = make_double2(c, s);
    sincos(t[0] - t[2], &s, &c); p.exp2 = make_double2(c, s);
    p.djn = (-3.0*dt1 + dt2)/(2.0*dz); p.pad = 0.0;
    *out = p;
}

struct LaserSlices { const double2 *n00j00, *n00jp1, *n00jp2, *nm1j00, *nm1jp1, *nm1jp2, *np1jp1, *np1jp2; };   // null = beyond the head: 0

// right-hand side of the envelope equation (:700-749)
__global__ __launch_bounds__(256)
void k_laser_rhs (LaserSlices S, SlabView f, int c_chi, double chi0, int gshrink, const double* __restrict__ chi_plane, int nx, int ny,
                  const LaserPhase* ph, int step, double dx, double dy, double dz, double c, double dt, double k0, double2* rhs,
                  double* mg_rhs, double* mg_acf_real, double* mg_acf_imag)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= nx) return;
    const long o = (long)j*nx + i;
    auto ld = [o] (const double2* p) { return p ? p[o] : make_double2(0.0, 0.0); };
    const double2 exp1 = ph->exp1, exp2 = ph->exp2; const double djn = ph->djn;
    const double2* ls = (step == 0) ? S.n00j00 : S.nm1j00;
    double2 lap = make_double2(0.0, 0.0);
    if (i > 0 && i < nx - 1 && j > 0 && j < ny - 1) {
        const double2 c0 = ls[o], xp = ls[o + 1], xm = ls[o - 1], yp = ls[o + nx], ym = ls[o - nx];
        lap.x = (xp.x + xm.x - 2.0*c0.x)/(dx*dx) + (yp.x + ym.x - 2.0*c0.x)/(dy*dy);
        lap.y = (xp.y + xm.y - 2.0*c0.y)/(dx*dx) + (yp.y + ym.y - 2.0*c0.y)/(dy*dy);
    }
    // InterpolateChi (:334-407): chi of the slab inside the box shrunk by the guard width, the initial chi outside; on a laser
    // grid of its own k_laser_interp_chi has done that (nx, ny are the laser's, the slab is not read)
    const bool inside = i >= gshrink && i < nx - gshrink && j >= gshrink && j < ny - gshrink;
    const double chi = chi_plane ? chi_plane[o] : (inside ? f.p[c_chi*f.ns + f.off(i, j)] : chi0);
    const double2 an00j00 = ld(S.n00j00), anp1jp1 = ld(S.np1jp1), anp1jp2 = ld(S.np1jp2);
    const double cdz = 1.0/(c*dt*dz), cdt = 1.0/(c*dt);
    // chi term: 2 chi a_n on the right-hand side (fft, :713-740); multigrid with MG_average_rhs = 1: chi a_n (first step)
    // or chi a_{n-1}, the other half in the operator (:575-598)
    const bool mgs = (mg_rhs != nullptr);
    double2 r;
    if (step == 0) {
        const double2 an00jp1 = ld(S.n00jp1), an00jp2 = ld(S.n00jp2);
        r = cscale(8.0*cdz, cmul(csub(an00jp1, anp1jp1), exp1));
        r = cadd(r, cscale(2.0*cdz, cmul(csub(anp1jp2, an00jp2), exp2)));
        r = cadd(r, cscale((mgs ? 1.0 : 2.0)*chi, an00j00));
        r = csub(r, lap);
        r = cadd(r, cmul(make_double2(-6.0*cdz, 4.0*djn*cdt + 4.0*k0*cdt), an00j00));
    } else {
        const double2 anm1jp1 = ld(S.nm1jp1), anm1jp2 = ld(S.nm1jp2), anm1j00 = ld(S.nm1j00);
        r = cscale(4.0*cdz, cmul(csub(anm1jp1, anp1jp1), exp1));
        r = cadd(r, cscale(1.0*cdz, cmul(csub(anp1jp2, anm1jp2), exp2)));
        r = csub(r, cscale(4.0*cdt*cdt, an00j00));
        r = cadd(r, mgs ? cscale(chi, anm1j00) : cscale(2.0*chi, an00j00));
        r = csub(r, lap);
        r = cadd(r, cmul(make_double2(-3.0*cdz + 2.0*cdt*cdt, 2.0*djn*cdt + 2.0*k0*cdt), anm1j00));
    }
    if (!mgs) { rhs[o] = r; return; }
    const long plane = (long)nx*ny;
    mg_rhs[o] = r.x; mg_rhs[plane + o] = r.y;
    mg_acf_real[o] = ((step == 0) ? 6.0*cdz : 3.0*cdz + 2.0*cdt*cdt) + chi;                 // :520-523, 571-572
    if (o == 0) *mg_acf_imag = (step == 0) ? -4.0*(k0 + djn)*cdt : -2.0*(k0 + djn)*cdt;    // :524-525
}

// planar (Re plane, Im plane) -> complex
__global__ __launch_bounds__(256)
void k_laser_from_planar (const double* __restrict__ p, double2* __restrict__ out, long plane)
{
    const long o = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (o < plane) out[o] = make_double2(p[o], p[plane + o]);
}

// divide by -(k^2 + a) in Fourier space (:754-772)
__global__ __launch_bounds__(256)
void k_laser_divide (double2* rhs, int nx, int ny, double dkx, double dky, const LaserPhase* ph, int step,
                     double dz, double c, double dt, double k0)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= nx) return;
    const int imid = (nx + 1)/2, jmid = (ny + 1)/2;
    const double djn = ph->djn;
    const double cdz = 1.0/(c*dt*dz), cdt = 1.0/(c*dt);
    const double2 ac = (step == 0) ? make_double2(6.0*cdz, -4.0*(k0 + djn)*cdt)
                                   : make_double2(3.0*cdz + 2.0*cdt*cdt, -2.0*(k0 + djn)*cdt);
    const double kx = (i < imid) ? dkx*i : dkx*(i - nx);
    const double ky = (j < jmid) ? dky*j : dky*(j - ny);
    const double dr = kx*kx + ky*ky + ac.x, di = ac.y;
    const double m2 = dr*dr + di*di;
    const double2 inv = (m2 > 0.0) ? make_double2(dr/m2, -di/m2) : make_double2(0.0, 0.0);
    const long o = (long)j*nx + i;
    rhs[o] = cscale(-1.0, cmul(rhs[o], inv));
}

__global__ __launch_bounds__(256)
void k_laser_store (const double2* sol, double2* np1, long n, double inv_n)
{
    const long o = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (o < n) np1[o] = cscale(inv_n, sol[o]);
}

static LaserPars laser_pars (const hps_deck& d)
{
    return LaserPars{d.laser_a0, d.laser_w0, d.laser_L0, 2.0*3.14159265358979323846/d.laser_lambda0, d.laser_pos[0], d.laser_pos[1],
                     d.laser_pos[2], d.laser_zfoc};
}

int laser_create (Engine& E)
{
    LaserState* L = new LaserState;
    E.laser = L;
    const hps_deck& d = E.d;
    const Engine::LaserGrid& G = E.lgrid;
    L->grid = G.set;
    if (G.set) {
        L->nx = G.nx; L->ny = G.ny; L->nz = G.zhi - G.zlo + 1; L->zlo = G.zlo;
        L->dx = G.dx; L->dy = G.dy; L->xoff = G.xoff; L->yoff = G.yoff; L->lenx = G.hi[0] - G.lo[0]; L->leny = G.hi[1] - G.lo[1];
    } else {
        L->nx = d.nx; L->ny = d.ny; L->nz = d.nz; L->zlo = 0;
        L->dx = E.gm.dx; L->dy = E.gm.dy; L->xoff = E.gm.xoff; L->yoff = E.gm.yoff; L->lenx = d.hi[0] - d.lo[0]; L->leny = d.hi[1] - d.lo[1];
    }
    const size_t plane = (size_t)L->nx*L->ny, tot = plane*L->nz;
    HPS_HIP_CHECK(hipMalloc(&L->n00, tot*sizeof(double2)));
    HPS_HIP_CHECK(hipMalloc(&L->phase, sizeof(LaserPhase)));
    if (d.laser_solver >= 1 && d.dt != 0.0) {
        HPS_HIP_CHECK(hipMalloc(&L->nm1, tot*sizeof(double2)));
        HPS_HIP_CHECK(hipMalloc(&L->np1, tot*sizeof(double2)));
        HPS_HIP_CHECK(hipMemset(L->nm1, 0, tot*sizeof(double2)));
        HPS_HIP_CHECK(hipMemset(L->np1, 0, tot*sizeof(double2)));
        if (L->grid) {
            HPS_HIP_CHECK(hipMalloc(&L->chi, plane*sizeof(double)));
            HPS_HIP_CHECK(hipMalloc(&L->chi_initial, plane*sizeof(double)));
            HPS_HIP_CHECK(hipMemset(L->chi, 0, plane*sizeof(double)));
            HPS_HIP_CHECK(hipMemset(L->chi_initial, 0, plane*sizeof(double)));
        }
    }
    if (d.laser_solver == 2 && d.dt != 0.0) {
        if (L->nx % 2 || L->ny % 2) { set_error("laser: the multigrid envelope solver needs even nx, ny (cell-centred hpmg box)"); return HPS_ERR_UNSUPPORTED; }
        if (int e = mg2_create_internal(L->nx, L->ny, L->dx, L->dy, &L->mg)) return e;
        HPS_HIP_CHECK(hipMalloc(&L->mg_sol, 2*plane*sizeof(double)));
        HPS_HIP_CHECK(hipMemset(L->mg_sol, 0, 2*plane*sizeof(double)));
        HPS_HIP_CHECK(hipMalloc(&L->mg_rhs, 2*plane*sizeof(double)));
        HPS_HIP_CHECK(hipMalloc(&L->mg_acf_real, plane*sizeof(double)));
        HPS_HIP_CHECK(hipMalloc(&L->mg_acf_imag, sizeof(double)));
    }
    if (d.laser_solver == 1 && d.dt != 0.0) {
        HPS_HIP_CHECK(hipMalloc(&L->work, plane*sizeof(double2)));
        static bool setup = false;
        if (!setup) { rocfft_setup(); setup = true; }
        const size_t len[2] = {(size_t)L->nx, (size_t)L->ny};
        if (rocfft_plan_create(&L->fwd, rocfft_placement_inplace, rocfft_transform_type_complex_forward, rocfft_precision_double, 2, len, 1, nullptr) != rocfft_status_success ||
            rocfft_plan_create(&L->bwd, rocfft_placement_inplace, rocfft_transform_type_complex_inverse, rocfft_precision_double, 2, len, 1, nullptr) != rocfft_status_success) {
            set_error("laser: rocfft_plan_create failed"); return HPS_ERR_FFT;
        }
        size_t wf = 0, wb = 0;
        rocfft_plan_get_work_buffer_size(L->fwd, &wf);
        rocfft_plan_get_work_buffer_size(L->bwd, &wb);
        rocfft_execution_info_create(&L->info);
        if (std::max(wf, wb) > 0) {
            HPS_HIP_CHECK(hipMalloc(&L->fft_work, std::max(wf, wb)));
            rocfft_execution_info_set_work_buffer(L->info, L->fft_work, std::max(wf, wb));
        }
        rocfft_execution_info_set_stream(L->info, E.laser_stream());
    }
    if (E.insitu_laser) {                                      // (the grid was set after the switch)
        if (int e = laser_set_insitu(E, 1)) { E.insitu_laser = false; return e; }
    }
    return HPS_OK;
}

void laser_destroy (Engine& E) { delete E.laser; E.laser = nullptr; }

void laser_sizes (Engine& E, int* nx, int* ny, int* nz) { *nx = E.laser->nx; *ny = E.laser->ny; *nz = E.laser->nz; }

// what hps_engine_add_laser_samples refuses beyond its own argument checks (needs the laser grid: checked again at the top of
// the first begin_step, since hps_engine_set_laser_grid may have come in between)
int laser_check_samples (Engine& E, const Engine::LaserSamples& S)
{
    LaserState* L = E.laser;
    for (int q = 0; q < (S.geometry == 3 ? 2 : 3); ++q)
        HPS_REQUIRE(S.geometry == 0 || (S.spacing[q] > 0.0 && std::isfinite(S.spacing[q]) && std::isfinite(S.offset[q])),
                    "hps_engine_add_laser_samples: the spacings must be positive and the offsets finite");
    if (S.geometry == 0)
        HPS_REQUIRE(S.extent[0] == L->nz && S.extent[1] == L->ny && S.extent[2] == L->nx,
                    "hps_engine_add_laser_samples: geometry 0 needs the extents of the laser grid, [nzl][nyl][nxl]");
    if (S.geometry == 3) {
        HPS_REQUIRE(S.extent[0] % 2 == 1, "hps_engine_add_laser_samples: rt needs an odd extent[0] (mode 0 and a cos and a sin part per further mode)");
        // the grid's smallest r: the cell nearest the axis in x and in y (Laser.cpp:303 asserts i_cell + ir >= 0)
        double ax = INFINITY, ay = INFINITY;
        for (int i = 0; i < L->nx; ++i) ax = std::min(ax, std::fabs(i*L->dx + L->xoff));
        for (int j = 0; j < L->ny; ++j) ay = std::min(ay, std::fabs(j*L->dy + L->yoff));
        const double rmid = (std::sqrt(ax*ax + ay*ay) - S.offset[1])/S.spacing[1];
        HPS_REQUIRE(std::floor(rmid) >= 0.0, "hps_engine_add_laser_samples: rt: a laser cell would reach a sample index < 0 in r (r < 0: offset[1] lies beyond the grid's smallest r)");
    }
    return HPS_OK;
}

// the initial envelope from the pulse list (or the deck's pulse) and the sample sets, in that order (InitLaserSlice :828-918)
static int laser_init_from_lists (Engine& E, double zoff)
{
    LaserState* L = E.laser;
    const hps_deck& d = E.d;
    const double pi = 3.14159265358979323846, k0 = 2.0*pi/d.laser_lambda0;
    const size_t tot = (size_t)L->nx*L->ny*L->nz;
    const dim3 grid(ceil_div(L->nx, 256), L->ny, L->nz), block(256);
    LaserPulseList P; P.n = 0;
    auto push = [&] (const hps_laser_pulse& p) {
        const double rot = p.propagation_angle_yz + (p.pft_yz - pi/2.0);
        P.p[P.n++] = LaserPulse{p.a0, p.w0, p.L0, p.pos[0], p.pos[1], p.pos[2], p.zfoc, p.cep, p.propagation_angle_yz,
                                std::cos(p.propagation_angle_yz), std::cos(rot), std::sin(rot)};
    };
    if (E.laser_pulses_set) { for (const hps_laser_pulse& p : E.laser_pulses) push(p); }
    else push(hps_laser_pulse{d.laser_a0, d.laser_w0, d.laser_L0, {d.laser_pos[0], d.laser_pos[1], d.laser_pos[2]}, d.laser_zfoc, 0.0, 0.0, pi/2.0});
    hipLaunchKernelGGL(k_laser_init_pulses, grid, block, 0, E.st, L->n00, L->nx, L->ny, L->nz, P, k0, L->dx, L->dy, E.gm.dz, L->xoff, L->yoff, zoff);
    HPS_HIP_CHECK(hipGetLastError());
    for (const Engine::LaserSamples& S : E.laser_samples) {        // (checked against this grid by Engine::begin_step)
        const size_t n = (size_t)S.extent[0]*S.extent[1]*S.extent[2];
        double2* dev = nullptr;
        HPS_HIP_CHECK(hipMalloc(&dev, n*sizeof(double2)));
        hipError_t err = hipMemcpy(dev, S.data.data(), n*sizeof(double2), hipMemcpyHostToDevice);
        if (err == hipSuccess) {
            if (S.geometry == 0) {
                hipLaunchKernelGGL(k_laser_add, dim3((unsigned)ceil_div((long)tot, 256)), block, 0, E.st, L->n00, dev, (long)tot);
            } else {
                const LaserFile F{S.geometry, (int)S.extent[0], (int)S.extent[1], (int)S.extent[2], S.offset[0], S.offset[1], S.offset[2],
                                  S.spacing[0], S.spacing[1], S.spacing[2], S.unit};
                hipLaunchKernelGGL(k_laser_resample, grid, block, 0, E.st, L->n00, L->nx, L->ny, L->nz, dev, F, E.gm.c, L->dx, L->dy, E.gm.dz,
                                   L->xoff, L->yoff, zoff);
            }
            err = hipGetLastError();
            if (err == hipSuccess) err = hipStreamSynchronize(E.st);
        }
        (void)hipFree(dev);
        HPS_HIP_CHECK(err);
    }
    E.laser_samples.clear(); E.laser_samples.shrink_to_fit();
    return HPS_OK;
}

// start of a time step: the first one evaluates the Gaussian on every slice, later ones hand the time levels on
// (a_{n+1} -> a_n -> a_{n-1}; MultiBuffer.cpp:840-852, 913-925)
int laser_begin_step (Engine& E)
{
    LaserState* L = E.laser;
    const hps_deck& d = E.d;
    if (L->import_mode) {
        L->initialised = true;       // levels are filled slice by slice; the driver has set the step index
        E.laser_samples.clear();     // (the initial envelope is the first stage's business)
    } else if (!L->initialised) {
        // a laser slice with global index k sits at the z of field slice k (the patch's z limits are snapped to whole field cells)
        const double zoff = 0.5*(d.lo[2] + d.hi[2] - E.gm.dz*(d.nz - 1)) + L->zlo*E.gm.dz;
        if (!E.laser_pulses_set && E.laser_samples.empty()) {
            hipLaunchKernelGGL(k_laser_init, dim3(ceil_div(L->nx, 256), L->ny, L->nz), dim3(256), 0, E.st, L->n00, L->nx, L->ny, L->nz, laser_pars(d),
                               L->dx, L->dy, E.gm.dz, L->xoff, L->yoff, zoff);
        } else if (int e = laser_init_from_lists(E, zoff)) return e;
        L->initialised = true; L->steps = 0;
    } else if (L->np1) {
        double2* old = L->nm1; L->nm1 = L->n00; L->n00 = L->np1; L->np1 = old;
        ++L->steps;
    }
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

// SetInitialChi (Hipace.cpp, once per step): needs the density profile's time factor of the step that begins
int laser_chi_initial (Engine& E)
{
    LaserState* L = E.laser;
    if (!L->chi_initial) return HPS_OK;
    const hps_deck& d = E.d;
    // per species: n q^2 mu0 / m, an ionisable one at its initial level; a program's value is the density itself
    const DensityProgram p[2] = {E.density_program(0), E.density_program(1)};
    double fac[2] = {0.0, 0.0};
    for (int k = 0; k < 2; ++k) if (E.sp[k].present()) {
        const Engine::Species& s = E.sp[k];
        const double n = p[s.index].n_ins > 0 ? 1.0 : s.density, lev = s.can_ionize ? (double)s.init_level : 1.0;
        fac[s.index] = n*s.charge*s.charge*E.gm.mu0/s.mass*lev*lev;
    }
    const double radius_sq = d.plasma_radius > 0.0 ? d.plasma_radius*d.plasma_radius : INFINITY;
    // the further species are added on top of the two, in index order, behind whichever kernel writes the two
    auto add_further = [&] () -> int {
        for (int k = 2; k < E.n_sp; ++k) {
            const Engine::Species& s = E.sp[k];
            const DensityProgram q = E.density_program(k);
            const double f = (q.n_ins > 0 ? 1.0 : s.density)*s.charge*s.charge*E.gm.mu0/s.mass;
            hipLaunchKernelGGL(k_laser_chi_initial_add, dim3(ceil_div(L->nx, 256), L->ny), dim3(256), E.density_lds(k), E.st, L->chi_initial, L->nx, L->ny,
                               L->dx, L->dy, L->xoff, L->yoff, f, q, E.d_prof_r, (int)E.prof_r.size(), E.prof_ft, radius_sq,
                               E.hollow_core_radius*E.hollow_core_radius);
            HPS_HIP_CHECK(hipGetLastError());
        }
        return HPS_OK;
    };
    if (p[0].n_ins > 0 || p[1].n_ins > 0) {
        hipLaunchKernelGGL(k_laser_chi_initial_prog, dim3(ceil_div(L->nx, 256), L->ny), dim3(256), std::max(E.density_lds(0), E.density_lds(1)), E.st,
                           L->chi_initial, L->nx, L->ny, L->dx, L->dy, L->xoff, L->yoff, fac[0], fac[1], p[0], p[1], E.d_prof_r, (int)E.prof_r.size(), E.prof_ft,
                           radius_sq, E.hollow_core_radius*E.hollow_core_radius);
        HPS_HIP_CHECK(hipGetLastError());
        return add_further();
    }
    hipLaunchKernelGGL(k_laser_chi_initial, dim3(ceil_div(L->nx, 256), L->ny), dim3(256), 0, E.st, L->chi_initial, L->nx, L->ny, L->dx, L->dy,
                       L->xoff, L->yoff, fac[0], fac[1], E.d_prof_r, (int)E.prof_r.size(), E.prof_ft, radius_sq, E.hollow_core_radius*E.hollow_core_radius);
    HPS_HIP_CHECK(hipGetLastError());
    return add_further();
}

static int launch_interp_aabs (SlabView f, int c_aabs, const double2* a, int nxl, int nyl, double dxl, double dyl, double xoffl, double yoffl,
                               const hps_geom& gm, int order, hipStream_t st)
{
    const dim3 grid(ceil_div(f.js, 256), f.ny + 2*f.ng), block(256);
#define HPS_LAUNCH_AABS(O) hipLaunchKernelGGL(k_laser_interp_aabs<O>, grid, block, 0, st, f, c_aabs, a, nxl, nyl, gm.dx, gm.dy, gm.xoff, gm.yoff, \
                                              1.0/dxl, 1.0/dyl, xoffl, yoffl)
    switch (order) {
        case 0: HPS_LAUNCH_AABS(0); break;
        case 1: HPS_LAUNCH_AABS(1); break;
        case 2: HPS_LAUNCH_AABS(2); break;
        default: HPS_LAUNCH_AABS(3); break;
    }
#undef HPS_LAUNCH_AABS
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

static int launch_interp_chi (SlabView f, int c_chi, const double* chi_initial, double* chi_out, int nxl, int nyl, double dxl, double dyl,
                              double xoffl, double yoffl, const hps_geom& gm, int shrink, int order, hipStream_t st)
{
    // the laser cells where the field box, shrunk by the guard width, ends (:358-372)
    const double pos_x_lo = shrink*gm.dx + gm.xoff, pos_x_hi = (f.nx - 1 - shrink)*gm.dx + gm.xoff;
    const double pos_y_lo = shrink*gm.dy + gm.yoff, pos_y_hi = (f.ny - 1 - shrink)*gm.dy + gm.yoff;
    const double dxl_inv = 1.0/dxl, dyl_inv = 1.0/dyl;
    auto clamp = [] (double v, int n) { return (int)std::min(std::max(v, -1.0), (double)n); };
    const int x_lo = clamp(std::ceil((pos_x_lo - xoffl)*dxl_inv), nxl), x_hi = clamp(std::floor((pos_x_hi - xoffl)*dxl_inv), nxl);
    const int y_lo = clamp(std::ceil((pos_y_lo - yoffl)*dyl_inv), nyl), y_hi = clamp(std::floor((pos_y_hi - yoffl)*dyl_inv), nyl);
    const dim3 grid(ceil_div(nxl, 256), nyl), block(256);
#define HPS_LAUNCH_CHI(O) hipLaunchKernelGGL(k_laser_interp_chi<O>, grid, block, 0, st, f, c_chi, chi_initial, chi_out, nxl, nyl, dxl, dyl, xoffl, yoffl, \
                                             1.0/gm.dx, 1.0/gm.dy, gm.xoff, gm.yoff, x_lo, x_hi, y_lo, y_hi)
    switch (order) {
        case 0: HPS_LAUNCH_CHI(0); break;
        case 1: HPS_LAUNCH_CHI(1); break;
        case 2: HPS_LAUNCH_CHI(2); break;
        default: HPS_LAUNCH_CHI(3); break;
    }
#undef HPS_LAUNCH_CHI
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

// InSituComputeDiags of the plane a_n of a slice (column k of the [8][nz] rows), on the engine's stream
static int launch_insitu (Engine& E, const double2* a, int k)
{
    LaserState* L = E.laser;
    const long plane = (long)L->nx*L->ny;
    const int groups = (int)std::min<long>(ceil_div(plane, 256), INSITU_GROUPS);
    const double mid_factor = (L->nx % 2 ? 1.0 : 0.5)*(L->ny % 2 ? 1.0 : 0.5);
    hipLaunchKernelGGL(k_insitu_laser, dim3(groups), dim3(256), 0, E.st, a, L->nx, L->ny, L->dx, L->dy, L->xoff, L->yoff, L->insitu_part);
    hipLaunchKernelGGL(k_insitu_laser_fold, dim3(1), dim3(64), 0, E.st, L->insitu_part, groups, L->dx*L->dy*E.gm.dz, mid_factor, L->insitu, L->nz, k);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

int laser_update_aabs (Engine& E, int islice, double* sum_abs)
{
    LaserState* L = E.laser;
    SlabView f(E.slab);
    if (L->insitu && E.laser_has_slice(islice)) {
        if (int e = launch_insitu(E, L->n00 + (size_t)(islice - L->zlo)*L->nx*L->ny, islice - L->zlo)) return e;
    }
    if (!L->grid) {
        hipLaunchKernelGGL(k_laser_aabs, dim3(ceil_div(E.slab.jstride, 256), E.d.ny + 2*E.g), dim3(256), 0, E.st, f, E.c_aabs,
                           L->n00 + (size_t)islice*L->nx*L->ny, sum_abs);
        return HPS_OK;
    }
    if (!E.laser_has_slice(islice)) {        // no laser on this slice: aabs = 0 (:223-230)
        HPS_HIP_CHECK(hipMemsetAsync(E.slab.p + (size_t)E.c_aabs*E.slab.nstride, 0, (size_t)E.slab.nstride*sizeof(double), E.st));
        return HPS_OK;
    }
    const size_t plane = (size_t)L->nx*L->ny;
    const double2* a = L->n00 + (size_t)(islice - L->zlo)*plane;
    if (sum_abs) hipLaunchKernelGGL(k_laser_sum_abs, dim3(ceil_div((long)plane, 256)), dim3(256), 0, E.st, a, (long)plane, sum_abs);
    return launch_interp_aabs(f, E.c_aabs, a, L->nx, L->ny, L->dx, L->dy, L->xoff, L->yoff, E.gm, E.lgrid.order, E.st);
}

// MultiLaser::AdvanceSlice: lasers.solver_type = fft (AdvanceSliceFFT) or multigrid (AdvanceSliceMG)
int laser_advance_slice (Engine& E, int islice)
{
    LaserState* L = E.laser;
    if (!L->np1 || !E.laser_has_slice(islice)) return HPS_OK;       // UseLaser(islice)
    const hipStream_t ls = E.laser_stream();       // ordered against the engine's stream by Engine::fork_laser / join_laser
    const hps_deck& d = E.d;
    const size_t plane = (size_t)L->nx*L->ny;
    const int nx = L->nx, ny = L->ny, k = islice - L->zlo;
    // beyond the head = beyond the laser's last slice (zeta_hi)
    auto at = [&] (const double2* base, int sl) -> const double2* { return sl < L->nz ? base + (size_t)sl*plane : nullptr; };
    const LaserSlices S{at(L->n00, k), at(L->n00, k + 1), at(L->n00, k + 2),
                        at(L->nm1, k), at(L->nm1, k + 1), at(L->nm1, k + 2),
                        at(L->np1, k + 1), at(L->np1, k + 2)};
    const double k0 = 2.0*3.14159265358979323846/d.laser_lambda0;
    if (L->grid) {
        if (int e = launch_interp_chi(SlabView(E.slab), (int)HPS_C_CHI, L->chi_initial, L->chi, nx, ny, L->dx, L->dy, L->xoff, L->yoff, E.gm,
                                      E.g, E.lgrid.order, ls)) return e;
    }
    hipLaunchKernelGGL(k_laser_phase, dim3(1), dim3(1), 0, ls, S.n00j00, S.n00jp1, S.n00jp2, nx, ny, d.laser_use_phase, E.gm.dz, L->phase);
    const dim3 grid(ceil_div(nx, 256), ny), block(256);
    const double chi0 = E.el.present() ? E.el.density*E.el.charge*E.el.charge*E.gm.mu0/E.el.mass : 0.0;
    hipLaunchKernelGGL(k_laser_rhs, grid, block, 0, ls, S, SlabView(E.slab), (int)HPS_C_CHI, chi0, E.g, L->chi, nx, ny, L->phase, L->steps,
                       L->dx, L->dy, E.gm.dz, E.gm.c, d.dt, k0, L->work, L->mg_rhs, L->mg_acf_real, L->mg_acf_imag);
    if (L->mg) {
        // MultiLaser::AdvanceSliceMG (:430-608): hpmg system type 2, at most 200 V-cycles; the initial guess is the solution
        // of the slice solved before this one (np1j00 is left in place by ShiftLaserSlices, :208)
        int iters = 0;
        if (int e = mg2_solve_internal(L->mg, L->mg_sol, L->mg_rhs, L->mg_acf_real, L->mg_acf_imag,
                                       d.laser_mg_tol_rel > 0.0 ? d.laser_mg_tol_rel : 1.0e-4, d.laser_mg_tol_abs, 200, &iters, ls)) return e;
        L->mg_vcycles += iters;
        hipLaunchKernelGGL(k_laser_from_planar, dim3(ceil_div((long)plane, 256)), block, 0, ls, L->mg_sol, L->np1 + (size_t)k*plane, (long)plane);
        HPS_HIP_CHECK(hipGetLastError());
        return HPS_OK;
    }
    void* buf[1] = {L->work};
    if (rocfft_execute(L->fwd, buf, nullptr, L->info) != rocfft_status_success) { set_error("laser: forward FFT failed"); return HPS_ERR_FFT; }
    hipLaunchKernelGGL(k_laser_divide, grid, block, 0, ls, L->work, nx, ny, 2.0*3.14159265358979323846/L->lenx,
                       2.0*3.14159265358979323846/L->leny, L->phase, L->steps, E.gm.dz, E.gm.c, d.dt, k0);
    if (rocfft_execute(L->bwd, buf, nullptr, L->info) != rocfft_status_success) { set_error("laser: backward FFT failed"); return HPS_ERR_FFT; }
    hipLaunchKernelGGL(k_laser_store, dim3(ceil_div((long)plane, 256)), block, 0, ls, L->work, L->np1 + (size_t)k*plane, (long)plane,
                       1.0/(double)plane);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

// ring hand-off of the envelope (MultiBuffer.cpp:840-852, 913-925): a stage passes {a_{n+1}, a_n} of a slice on, the next
// one stores them as its {a_n, a_{n-1}}.  msg = [2][ny][nx] complex of the laser grid on the device; both asynchronous on the
// stream.  A slice without a laser (outside the grid's zeta range) has no message: nothing is done.
int laser_set_import (Engine& E, int on, int step)
{
    E.laser->import_mode = (on != 0); E.laser->steps = step;
    return HPS_OK;
}
int laser_export_slice (Engine& E, int islice, double* msg_dev)
{
    if (!E.laser_has_slice(islice)) return HPS_OK;
    if (int e = E.join_laser()) return e;
    LaserState* L = E.laser;
    const size_t plane = (size_t)L->nx*L->ny, k = (size_t)(islice - L->zlo);
    const double2* newest = L->np1 ? L->np1 : L->n00;
    HPS_HIP_CHECK(hipMemcpyAsync(msg_dev, newest + k*plane, plane*sizeof(double2), hipMemcpyDeviceToDevice, E.st));
    HPS_HIP_CHECK(hipMemcpyAsync(msg_dev + 2*plane, L->n00 + k*plane, plane*sizeof(double2), hipMemcpyDeviceToDevice, E.st));
    return HPS_OK;
}
int laser_import_slice (Engine& E, int islice, const double* msg_dev)
{
    if (!E.laser_has_slice(islice)) return HPS_OK;
    LaserState* L = E.laser;
    const size_t plane = (size_t)L->nx*L->ny, k = (size_t)(islice - L->zlo);
    HPS_HIP_CHECK(hipMemcpyAsync(L->n00 + k*plane, msg_dev, plane*sizeof(double2), hipMemcpyDeviceToDevice, E.st));
    if (L->nm1) HPS_HIP_CHECK(hipMemcpyAsync(L->nm1 + k*plane, msg_dev + 2*plane, plane*sizeof(double2), hipMemcpyDeviceToDevice, E.st));
    return HPS_OK;
}

// in-process hand-off (several steps in flight on one device): the same two planes straight from the engine that ran
// the previous step, on the receiving engine's stream (the caller has made it wait for the sender's slice event)
int laser_import_from (Engine& E, int islice, Engine& src)
{
    if (!E.laser_has_slice(islice)) return HPS_OK;
    LaserState* L = E.laser; LaserState* P = src.laser;
    const size_t plane = (size_t)L->nx*L->ny, k = (size_t)(islice - L->zlo);
    const double2* newest = P->np1 ? P->np1 : P->n00;
    // a_n -> a_{n-1} first: with one stage in flight source and destination are the same engine
    if (L->nm1) HPS_HIP_CHECK(hipMemcpyAsync(L->nm1 + k*plane, P->n00 + k*plane, plane*sizeof(double2), hipMemcpyDeviceToDevice, E.st));
    if (newest != L->n00) HPS_HIP_CHECK(hipMemcpyAsync(L->n00 + k*plane, newest + k*plane, plane*sizeof(double2), hipMemcpyDeviceToDevice, E.st));
    return HPS_OK;
}

int laser_set_insitu (Engine& E, int on)
{
    LaserState* L = E.laser;
    (void)hipFree(L->insitu); (void)hipFree(L->insitu_part); L->insitu = L->insitu_part = nullptr;
    if (!on) return HPS_OK;
    hipError_t err = hipMalloc(&L->insitu, (size_t)8*L->nz*sizeof(double));
    if (err == hipSuccess) err = hipMemset(L->insitu, 0, (size_t)8*L->nz*sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&L->insitu_part, (size_t)8*INSITU_GROUPS*sizeof(double));
    if (err == hipSuccess) err = hipMemset(L->insitu_part, 0, (size_t)8*INSITU_GROUPS*sizeof(double));
    if (err != hipSuccess) {       // both or neither: launch_insitu goes by L->insitu
        (void)hipFree(L->insitu); (void)hipFree(L->insitu_part); L->insitu = L->insitu_part = nullptr;
    }
    HPS_HIP_CHECK(err);
    return HPS_OK;
}
int laser_clear_insitu (Engine& E)
{
    LaserState* L = E.laser;
    if (L->insitu) HPS_HIP_CHECK(hipMemsetAsync(L->insitu, 0, (size_t)8*L->nz*sizeof(double), E.st));
    return HPS_OK;
}
int laser_copy_insitu (Engine& E, double* out_host)
{
    LaserState* L = E.laser;
    HPS_REQUIRE(L->insitu, "hps_engine_insitu_laser: not switched on");
    HPS_HIP_CHECK(hipStreamSynchronize(E.st));
    HPS_HIP_CHECK(hipMemcpy(out_host, L->insitu, (size_t)8*L->nz*sizeof(double), hipMemcpyDeviceToHost));
    return HPS_OK;
}

long laser_mg_vcycles (Engine& E) { return E.laser ? E.laser->mg_vcycles : 0; }

int laser_copy_envelope (Engine& E, double* out_host)
{
    if (int e = E.join_laser()) return e;
    LaserState* L = E.laser;
    HPS_HIP_CHECK(hipStreamSynchronize(E.st));
    HPS_HIP_CHECK(hipMemcpy(out_host, L->n00, (size_t)L->nx*L->ny*L->nz*sizeof(double2), hipMemcpyDeviceToHost));
    return HPS_OK;
}

int laser_copy_chi (Engine& E, double* out_host)
{
    LaserState* L = E.laser;
    HPS_REQUIRE(L && L->chi, "hps_engine_laser_chi: needs a laser grid (hps_engine_set_laser_grid) and an evolving envelope (laser_solver >= 1, dt != 0)");
    if (int e = E.join_laser()) return e;
    HPS_HIP_CHECK(hipStreamSynchronize(E.st));
    HPS_HIP_CHECK(hipMemcpy(out_host, L->chi, (size_t)L->nx*L->ny*sizeof(double), hipMemcpyDeviceToHost));
    return HPS_OK;
}

// MultiLaser::MakeLaserGeometry (laser/MultiLaser.cpp:58-115): the field grid and box unless given; zeta snapped to whole field
// cells, so that laser slice k sits at the z of field slice k
int Engine::set_laser_grid (const int* n_cell, const double* patch_lo, const double* patch_hi, int interp_order)
{
    HPS_REQUIRE(laser, "hps_engine_set_laser_grid: the deck has no laser (laser_on)");
    HPS_REQUIRE(!step_begun, "hps_engine_set_laser_grid: must be called before the first hps_engine_begin_step");
    HPS_REQUIRE(interp_order >= 0 && interp_order <= 3, "hps_engine_set_laser_grid: lasers.interp_order must be 0, 1, 2 or 3");
    LaserGrid G;
    G.set = true; G.order = interp_order;
    G.nx = n_cell ? n_cell[0] : d.nx; G.ny = n_cell ? n_cell[1] : d.ny;
    for (int q = 0; q < 3; ++q) { G.lo[q] = patch_lo ? patch_lo[q] : d.lo[q]; G.hi[q] = patch_hi ? patch_hi[q] : d.hi[q]; }
    HPS_REQUIRE(G.nx >= 1 && G.ny >= 1, "hps_engine_set_laser_grid: lasers.n_cell must be positive");
    for (int q = 0; q < 3; ++q) HPS_REQUIRE(std::isfinite(G.lo[q]) && std::isfinite(G.hi[q]), "hps_engine_set_laser_grid: lasers.patch_lo / patch_hi must be finite");
    const double poff_z = 0.5*(d.lo[2] + d.hi[2] - gm.dz*(d.nz - 1)), dz_inv = 1.0/gm.dz;
    const double zl = std::max(0.0, std::round((G.lo[2] - poff_z)*dz_inv)), zh = std::min((double)(d.nz - 1), std::round((G.hi[2] - poff_z)*dz_inv));
    HPS_REQUIRE(zl <= zh, "hps_engine_set_laser_grid: the laser patch holds no field slice (empty zeta range)");
    G.zlo = (int)zl; G.zhi = (int)zh;
    G.lo[2] = (G.zlo - 0.5)*gm.dz + poff_z; G.hi[2] = (G.zhi + 0.5)*gm.dz + poff_z;
    HPS_REQUIRE(G.hi[0] > G.lo[0] && G.hi[1] > G.lo[1] && G.hi[2] > G.lo[2], "hps_engine_set_laser_grid: Laser box must have positive volume");
    G.dx = (G.hi[0] - G.lo[0])/G.nx; G.dy = (G.hi[1] - G.lo[1])/G.ny;
    G.xoff = 0.5*(G.lo[0] + G.hi[0] - G.dx*(G.nx - 1));
    G.yoff = 0.5*(G.lo[1] + G.hi[1] - G.dy*(G.ny - 1));
    if (d.laser_solver == 2 && d.dt != 0.0 && (G.nx % 2 || G.ny % 2)) {
        set_error("hps_engine_set_laser_grid: the multigrid envelope solver needs even lasers.n_cell (cell-centred hpmg box)"); return HPS_ERR_UNSUPPORTED; }
    HPS_HIP_CHECK(hipStreamSynchronize(st));
    laser_destroy(*this);
    lgrid = G;
    return laser_create(*this);
}

} // namespace hps

// The two grid-to-grid interpolations of the laser grid as operators of their own (the engine's kernels and launch code).
// a_plane: [nyl][nxl] complex (re, im interleaved) on the device; the laser grid is nxl x nyl cells of dxl x dyl with cell 0 at
// xoffl, yoffl; geom is the field slab's geometry.
extern "C" int hps_laser_interp_aabs (hps_slab slab, int c_aabs, const double* a_plane, int nxl, int nyl, double dxl, double dyl,
                                      double xoffl, double yoffl, hps_geom geom, int order, void* stream)
{
    using namespace hps;
    HPS_REQUIRE(slab.p && a_plane && c_aabs >= 0 && c_aabs < slab.ncomp, "hps_laser_interp_aabs: bad slab, plane or component");
    HPS_REQUIRE(nxl > 0 && nyl > 0 && dxl > 0.0 && dyl > 0.0, "hps_laser_interp_aabs: the laser grid needs cells of positive size");
    HPS_REQUIRE(order >= 0 && order <= 3, "hps_laser_interp_aabs: lasers.interp_order must be 0, 1, 2 or 3");
    return launch_interp_aabs(SlabView(slab), c_aabs, reinterpret_cast<const double2*>(a_plane), nxl, nyl, dxl, dyl, xoffl, yoffl, geom, order,
                              static_cast<hipStream_t>(stream));
}

extern "C" int hps_laser_interp_chi (hps_slab slab, int c_chi, const double* chi_initial, double* chi_out, int nxl, int nyl, double dxl,
                                     double dyl, double xoffl, double yoffl, hps_geom geom, int shrink, int order, void* stream)
{
    using namespace hps;
    HPS_REQUIRE(slab.p && chi_initial && chi_out && c_chi >= 0 && c_chi < slab.ncomp, "hps_laser_interp_chi: bad slab, plane or component");
    HPS_REQUIRE(nxl > 0 && nyl > 0 && dxl > 0.0 && dyl > 0.0, "hps_laser_interp_chi: the laser grid needs cells of positive size");
    HPS_REQUIRE(order >= 0 && order <= 3 && shrink >= 0, "hps_laser_interp_chi: lasers.interp_order must be 0, 1, 2 or 3 and shrink must not be negative");
    return launch_interp_chi(SlabView(slab), c_chi, chi_initial, chi_out, nxl, nyl, dxl, dyl, xoffl, yoffl, geom, shrink, order,
                             static_cast<hipStream_t>(stream));
}

// ---- the engine's laser entry points: arguments checked, then the laser_* functions above --------------------------------------
using namespace hps;

extern "C" int hps_engine_set_laser_import (void* h, int on, int step)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E->laser, "hps_engine_set_laser_import: no laser");
    return laser_set_import(*E, on, step);
}
extern "C" int hps_engine_export_laser_slice (void* h, int islice, double* msg_dev)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E->laser && msg_dev && islice >= 0 && islice < E->d.nz, "hps_engine_export_laser_slice: bad argument");
    return laser_export_slice(*E, islice, msg_dev);
}
extern "C" int hps_engine_import_laser_slice (void* h, int islice, const double* msg_dev)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E->laser && msg_dev && islice >= 0 && islice < E->d.nz, "hps_engine_import_laser_slice: bad argument");
    return laser_import_slice(*E, islice, msg_dev);
}
extern "C" int hps_engine_import_laser_from (void* h, int islice, void* src)
{
    Engine* E = static_cast<Engine*>(h); Engine* S = static_cast<Engine*>(src);
    HPS_REQUIRE(E->laser && S && S->laser && islice >= 0 && islice < E->d.nz && S->d.nx == E->d.nx && S->d.ny == E->d.ny && S->d.nz == E->d.nz,
                "hps_engine_import_laser_from: bad argument");
    {   const Engine::LaserGrid &a = E->lgrid, &b = S->lgrid;
        HPS_REQUIRE(a.set == b.set && (!a.set || (a.nx == b.nx && a.ny == b.ny && a.zlo == b.zlo && a.zhi == b.zhi)),
                    "hps_engine_import_laser_from: the two engines' laser grids differ"); }
    return laser_import_from(*E, islice, *S);
}
extern "C" int hps_engine_laser_envelope (void* h, double* out_host)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E->laser && out_host, "hps_engine_laser_envelope: no laser");
    return laser_copy_envelope(*E, out_host);
}
extern "C" int hps_engine_set_laser_grid (void* h, const int* n_cell, const double* patch_lo, const double* patch_hi, int interp_order)
{
    HPS_REQUIRE(h, "hps_engine_set_laser_grid: null handle");
    return static_cast<Engine*>(h)->set_laser_grid(n_cell, patch_lo, patch_hi, interp_order);
}
extern "C" int hps_engine_laser_grid (void* h, int* nxl, int* nyl, int* zeta_lo, int* zeta_hi)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E && E->laser, "hps_engine_laser_grid: no laser");
    int nx = 0, ny = 0, nz = 0;
    laser_sizes(*E, &nx, &ny, &nz);
    if (nxl) *nxl = nx;
    if (nyl) *nyl = ny;
    if (zeta_lo) *zeta_lo = E->lgrid.set ? E->lgrid.zlo : 0;
    if (zeta_hi) *zeta_hi = E->lgrid.set ? E->lgrid.zhi : E->d.nz - 1;
    return HPS_OK;
}
// several Gaussian pulses, envelopes from samples, in-situ reductions
extern "C" int hps_engine_set_laser_pulses (void* h, int n, const hps_laser_pulse* pulses)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E && E->laser, "hps_engine_set_laser_pulses: the deck has no laser (laser_on)");
    HPS_REQUIRE(!E->step_begun, "hps_engine_set_laser_pulses: must be called before the first hps_engine_begin_step");
    HPS_REQUIRE(n >= 0 && n <= 8, "hps_engine_set_laser_pulses: 0 to 8 pulses");
    HPS_REQUIRE(n == 0 || pulses, "hps_engine_set_laser_pulses: null pulse list");
    for (int q = 0; q < n; ++q) {
        const hps_laser_pulse& P = pulses[q];
        HPS_REQUIRE(P.w0 > 0.0 && P.L0 > 0.0, "hps_engine_set_laser_pulses: w0 and L0 must be positive");
        const double v[10] = {P.a0, P.w0, P.L0, P.pos[0], P.pos[1], P.pos[2], P.zfoc, P.cep, P.propagation_angle_yz, P.pft_yz};
        for (double x : v) HPS_REQUIRE(std::isfinite(x), "hps_engine_set_laser_pulses: the pulse parameters must be finite");
    }
    E->laser_pulses.assign(pulses, pulses + n);
    E->laser_pulses_set = true;
    return HPS_OK;
}
extern "C" int hps_engine_add_laser_samples (void* h, int geometry, const double* data_host, const long extent[3], const double offset[3],
                                             const double spacing[3], double unit)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E && E->laser, "hps_engine_add_laser_samples: the deck has no laser (laser_on)");
    HPS_REQUIRE(!E->step_begun, "hps_engine_add_laser_samples: must be called before the first hps_engine_begin_step");
    HPS_REQUIRE(geometry >= 0 && geometry <= 3, "hps_engine_add_laser_samples: geometry must be 0 (laser grid), 1 (xyt), 2 (xyz) or 3 (rt)");
    HPS_REQUIRE(extent && offset && spacing, "hps_engine_add_laser_samples: null argument");
    HPS_REQUIRE(E->laser_samples.size() < 4, "hps_engine_add_laser_samples: at most 4 sets of samples");
    HPS_REQUIRE(std::isfinite(unit), "hps_engine_add_laser_samples: unit must be finite");
    Engine::LaserSamples S;
    S.geometry = geometry; S.unit = unit;
    for (int q = 0; q < 3; ++q) {
        HPS_REQUIRE(extent[q] > 0 && extent[q] < (1L << 30), "hps_engine_add_laser_samples: the extents must be positive");
        S.extent[q] = extent[q]; S.offset[q] = offset[q]; S.spacing[q] = spacing[q];
    }
    // each extent is below 2^30, so the product of two fits a long; the product of all three is held below 2^31
    HPS_REQUIRE(extent[0]*extent[1] <= ((1L << 31) - 1)/extent[2], "hps_engine_add_laser_samples: more than 2^31 - 1 samples in a set");
    HPS_REQUIRE(data_host, "hps_engine_add_laser_samples: null argument");
    if (int e = laser_check_samples(*E, S)) return e;
    const size_t n = (size_t)extent[0]*extent[1]*extent[2];
    // no host memory for the copy is no fault of the arguments: the code of a failed device allocation
    try { S.data.assign(data_host, data_host + 2*n); E->laser_samples.push_back(std::move(S)); }
    catch (const std::exception&) { set_error("hps_engine_add_laser_samples: no host memory for the copy of the samples"); return HPS_ERR_HIP; }
    return HPS_OK;
}
extern "C" int hps_engine_set_insitu_laser (void* h, int on)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E && E->laser, "hps_engine_set_insitu_laser: the deck has no laser (laser_on)");
    if ((on != 0) == E->insitu_laser) return HPS_OK;      // on -> on keeps the rows collected so far
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    if (int e = laser_set_insitu(*E, on)) return e;       // (a failed allocation leaves it off)
    E->insitu_laser = (on != 0);
    return HPS_OK;
}
extern "C" int hps_engine_insitu_laser (void* h, double* out)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E && E->laser && E->insitu_laser && out, "hps_engine_insitu_laser: not switched on");
    return laser_copy_insitu(*E, out);
}
extern "C" int hps_engine_laser_chi (void* h, double* out_host)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E && E->laser && out_host, "hps_engine_laser_chi: no laser");
    return laser_copy_chi(*E, out_host);
}
extern "C" int hps_engine_laser_info (void* h, int* aabs_comp, double* sum_host)
{
    Engine* E = static_cast<Engine*>(h);
    if (aabs_comp) *aabs_comp = E->c_aabs;
    if (sum_host) {
        HPS_HIP_CHECK(hipStreamSynchronize(E->st));
        HPS_HIP_CHECK(hipMemcpy(sum_host, E->d_laser_sum, sizeof(double), hipMemcpyDeviceToHost));
    }
    return HPS_OK;
}
extern "C" int hps_engine_laser_vcycles (void* h, long* vcycles)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(vcycles, "hps_engine_laser_vcycles: null argument");
    *vcycles = E->laser ? laser_mg_vcycles(*E) : 0;
    return HPS_OK;
}
