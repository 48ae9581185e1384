// open_boundary.hip -- boundary.field = Open: restates Fields::SetBoundaryCondition (fields/Fields.cpp:678-735) with the
// multipole expansion of fields/OpenBoundary.H as two kernels on the staged Poisson sources.  Owns Engine::open_boundary
// and the stand-alone entry point hps_open_boundary.
#include "common.h"
#include "engine.h"

#include <algorithm>
#include <cmath>

namespace hps {

// boundary.field = Open (Fields::SetBoundaryCondition, fields/Fields.cpp:678-735): the free-space Green's function
// ln|r - r'|^2 / (4 pi) expanded to order 18 about the origin (fields/OpenBoundary.H: 37 real moments; here in complex form,
// z = x + i y:  ln|z - z'|^2 = ln|z|^2 - sum_n (2/n) Re((z'/z)^n), so with M_n = sum_src s z'^n the potential outside the
// sources is dx dy/(4 pi) [M_0 ln|z|^2 - sum_n (2/n) Re(M_n z^-n)]).  Coordinates scaled by 3/|diagonal|; sources beyond 95 % of
// the distance to the nearest wall are left out.  k_multipole_moments: mom[b][workgroup][2 n], [2 n + 1] = that workgroup's share of
// Re, Im M_n of plane b.
constexpr int OPEN_ORDER = 18, OPEN_PARTS = 256;      // order of the expansion; workgroups (= partial sums) per source
__global__ __launch_bounds__(256)
void k_multipole_moments (const double* __restrict__ staging, long nval, int nx, double dx, double dy, double xoff, double yoff,
                          double scale, double cutoff_sq, double* mom)
{
    const double* s = staging + (long)blockIdx.y*nval;
    double re[OPEN_ORDER + 1], im[OPEN_ORDER + 1];
#pragma unroll
    for (int n = 0; n <= OPEN_ORDER; ++n) { re[n] = 0.0; im[n] = 0.0; }
    // (eight loads in flight per thread: with two or three waves per SIMD one load per trip leaves the memory latency bare)
    const long stride = (long)gridDim.x*blockDim.x;
    for (long c0 = (long)blockIdx.x*blockDim.x + threadIdx.x; c0 < nval; c0 += 8*stride) {
        double sv8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const long c = c0 + u*stride; sv8[u] = c < nval ? s[c] : 0.0; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long c = c0 + u*stride;
            if (c >= nval) break;
            const int j = (int)(c / nx), i = (int)(c - (long)j*nx);
            const double x = (i*dx + xoff)*scale, y = (j*dy + yoff)*scale;
            if (x*x + y*y > cutoff_sq) continue;
            const double sv = sv8[u];
            double zr = 1.0, zi = 0.0;
#pragma unroll
            for (int n = 0; n <= OPEN_ORDER; ++n) {
                re[n] += sv*zr; im[n] += sv*zi;
                const double t = zr*x - zi*y; zi = zr*y + zi*x; zr = t;
            }
        }
    }
    // the workgroup's sum through LDS (38 values x 256 threads; 38 x 6 wave-shuffle steps of doubles took longer than the pass):
    // six threads per value add 43 entries each, one of them the six
    constexpr int NM = 2*(OPEN_ORDER + 1), LD = 257;
    __shared__ double part[NM*LD];
#pragma unroll
    for (int n = 0; n <= OPEN_ORDER; ++n) { part[(2*n)*LD + threadIdx.x] = re[n]; part[(2*n + 1)*LD + threadIdx.x] = im[n]; }
    __syncthreads();
    const int v = threadIdx.x / 6, q = threadIdx.x - 6*v;
    double a = 0.0;
    if (v < NM) for (int k = q; k < 256; k += 6) a += part[v*LD + k];
    __syncthreads();
    if (v < NM) part[v*LD + q] = a;
    __syncthreads();
    // (one partial sum per workgroup, added up by the consumer in a fixed order)
    if (threadIdx.x < NM) {
        const double* r = part + threadIdx.x*LD;
        mom[((long)blockIdx.y*gridDim.x + blockIdx.x)*NM + threadIdx.x] = ((r[0] + r[1]) + (r[2] + r[3])) + (r[4] + r[5]);
    }
}

// SetDirichletBoundaries (fields/Fields.cpp:627-669) with offset = factor = 1: the outermost rows and columns of the source get
// -phi(one cell outside)/h^2, corners from both sides.  One thread per boundary point: 2 nx + 2 ny of them per plane.
__global__ __launch_bounds__(256)
void k_open_boundary_apply (double* staging, long nval, int nx, int ny, double dx, double dy, double xoff, double yoff,
                            double scale, double pref, const double* __restrict__ mom, int nparts, unsigned no_monopole_mask)
{
    const int b = blockIdx.y;
    constexpr int NM = 2*(OPEN_ORDER + 1);
    __shared__ double Msh[6][NM];
    {   // the workgroups' partial moments, in a fixed order
        const int v = threadIdx.x % NM, q = threadIdx.x / NM;
        if (q < 6) {
            double a = 0.0;
            for (int k = q; k < nparts; k += 6) a += mom[((long)b*nparts + k)*NM + v];
            Msh[q][v] = a;
        }
        __syncthreads();
        if (threadIdx.x < NM) Msh[0][threadIdx.x] = ((Msh[0][threadIdx.x] + Msh[1][threadIdx.x]) + (Msh[2][threadIdx.x] + Msh[3][threadIdx.x]))
                                                    + (Msh[4][threadIdx.x] + Msh[5][threadIdx.x]);
        __syncthreads();
    }
    const int t = blockIdx.x*blockDim.x + threadIdx.x;
    if (t >= 2*nx + 2*ny) return;
    double xd, yd, hh; long target;
    if (t < nx)               { xd = t*dx + xoff;            yd = -dy + yoff;              hh = dy*dy; target = t; }
    else if (t < 2*nx)        { xd = (t - nx)*dx + xoff;     yd = ny*dy + yoff;            hh = dy*dy; target = (long)(ny - 1)*nx + (t - nx); }
    else if (t < 2*nx + ny)   { xd = -dx + xoff;             yd = (t - 2*nx)*dy + yoff;    hh = dx*dx; target = (long)(t - 2*nx)*nx; }
    else                      { xd = nx*dx + xoff;           yd = (t - 2*nx - ny)*dy + yoff; hh = dx*dx; target = (long)(t - 2*nx - ny)*nx + (nx - 1); }
    const double* M = Msh[0];
    const double zx = xd*scale, zy = yd*scale, nrm = zx*zx + zy*zy;
    const double ix = zx/nrm, iy = -zy/nrm;                   // 1/z
    double v = ((no_monopole_mask >> b) & 1u) ? 0.0 : M[0]*log(nrm);
    double pr = ix, pi_ = iy;
    for (int n = 1; n <= OPEN_ORDER; ++n) {
        v -= (2.0/n)*(M[2*n]*pr - M[2*n + 1]*pi_);
        const double q = pr*ix - pi_*iy; pi_ = pr*iy + pi_*ix; pr = q;
    }
    atomic_add_f64(staging + (long)b*nval + target, -(pref*v)/hh);
}

constexpr size_t OPEN_MOM_DOUBLES = (size_t)4*OPEN_PARTS*2*(OPEN_ORDER + 1);      // mom: [source][OPEN_PARTS][2 (OPEN_ORDER + 1)]

// The two launches on nbatch (1..4) contiguous planes [ny][nx] of the box lo .. hi (x, y), with the geometry derived as
// Engine::create derives gm (GetPosOffset); bit b of no_monopole_mask drops M_0 of plane b.  mom: OPEN_MOM_DOUBLES doubles on
// the device.  The engine's path and hps_open_boundary's.
static void open_boundary_planes (double* planes, int nbatch, int nx, int ny, const double* lo, const double* hi,
                                  unsigned no_monopole_mask, double* mom, hipStream_t st)
{
    const long nval = (long)nx*ny;
    const double dx = (hi[0] - lo[0])/nx, dy = (hi[1] - lo[1])/ny;
    const double xoff = 0.5*(lo[0] + hi[0] - dx*(nx - 1));
    const double yoff = 0.5*(lo[1] + hi[1] - dy*(ny - 1));
    const double Lx = hi[0] - lo[0], Ly = hi[1] - lo[1];
    const double scale = 3.0/std::sqrt(Lx*Lx + Ly*Ly);
    const double radius = std::min(std::min(std::fabs(lo[0]), std::fabs(hi[0])), std::min(std::fabs(lo[1]), std::fabs(hi[1])));
    const double cutoff_sq = (0.95*radius*scale)*(0.95*radius*scale);
    hipLaunchKernelGGL(k_multipole_moments, dim3(OPEN_PARTS, nbatch), dim3(256), 0, st, planes, nval, nx, dx, dy, xoff, yoff,
                       scale, cutoff_sq, mom);
    hipLaunchKernelGGL(k_open_boundary_apply, dim3(ceil_div(2*nx + 2*ny, 256), nbatch), dim3(256), 0, st, planes, nval, nx, ny,
                       dx, dy, xoff, yoff, scale, dx*dy/(4.0*3.14159265358979323846), mom, OPEN_PARTS, no_monopole_mask);
}

int Engine::open_boundary (int nbatch, unsigned no_monopole_mask)
{
    if (d.field_bc != 1) return HPS_OK;
    open_boundary_planes(staging, nbatch, d.nx, d.ny, d.lo, d.hi, no_monopole_mask, d_open_mom, st);
    return HPS_OK;
}

} // namespace hps

using namespace hps;

extern "C" int hps_open_boundary (double* staging_dev, int nbatch, int nx, int ny, const double lo[2], const double hi[2],
                                  unsigned no_monopole_mask, void* stream)
{
    HPS_REQUIRE(staging_dev && lo && hi, "hps_open_boundary: null argument");
    HPS_REQUIRE(nbatch >= 1 && nbatch <= 4, "hps_open_boundary: nbatch must be 1..4");
    HPS_REQUIRE(nx >= 2 && ny >= 2, "hps_open_boundary: nx and ny must be at least 2");
    HPS_REQUIRE(hi[0] > lo[0] && hi[1] > lo[1], "hps_open_boundary: the box needs hi > lo in x and y");
    HPS_REQUIRE(lo[0] < 0.0 && hi[0] > 0.0 && lo[1] < 0.0 && hi[1] > 0.0, "hps_open_boundary: boundary.field = Open needs x = y = 0 inside the box");
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* mom = nullptr;
    HPS_HIP_CHECK(hipMalloc(&mom, OPEN_MOM_DOUBLES*sizeof(double)));
    open_boundary_planes(staging_dev, nbatch, nx, ny, lo, hi, no_monopole_mask, mom, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(mom);
    HPS_HIP_CHECK(e);
    return HPS_OK;
}
