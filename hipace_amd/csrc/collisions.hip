// collisions.hip -- binary Coulomb collisions between plasma species, and between the moving beam and a plasma species (gfx950).
//
// Restates particles/collisions/CoulombCollision.cpp::doPlasmaPlasmaCoulombCollision with ElasticCollisionPerez.H,
// UpdateMomentumPerez.H, ComputeTemperature.H and ShuffleFisherYates.H of the reference (Perez et al., Phys. Plasmas 19,
// 083104 (2012)).  Bins are single cells of the particles' current x, y.  The reference draws from amrex::Random; here every
// draw is a function of (seed, collision, time step, slice, cell, pair, draw) -- coll_uniform below -- and every cell's list is
// put in the order of the particles' id bits before it is shuffled, so the result does not depend on the order of the sheet.
//
// Two kernel templates.  k_coll_list<Src, FILL> builds a cell-sorted index list of one source of particles, a sheet (CollSheet) or
// a beam slice (CollBeam): the count pass (integer atomics per cell), an exclusive scan (rocprim), the fill pass -- three
// launches per list, coll_build_list.  k_coll_cells<Side0> then collides the cells: ONE LANE PER CELL runs the reference's
// serial per-cell loop (order, shuffle, densities, temperatures, pairs).
// The wrap-around pairing makes the pairs of a cell depend on each other (a particle collides twice), and the reference's
// running charge product is serial too, so a cell is not split over lanes.  A cell's index list is staged in LDS
// (COLL_LDS_CAP = 64 entries per lane, lane-interleaved so that the lanes of a wave hit different banks: 16 KB per 64-lane
// workgroup, ten workgroups per CU); a cell with more particles works on its
// segment of the global index list in place and is counted (overfull cells).  Momenta are written by the lane that owns
// the pair; the only device-wide atomics are the integer cell counters and the two statistics words.
//
// Beam-plasma (doBeamPlasmaCoulombCollision, CoulombCollision.cpp:238-348; every is_beam_coll branch of ElasticCollisionPerez.H and
// ComputeTemperature.H): side 0 of the cell kernel is a beam slice -- BeamSoA, with a range that the list kernel reads on the
// device -- which carries uz where a plasma particle carries psi.  The functions below take side 0's type as a template
// argument (hps_plasma or BeamSoA); side 1 is always a sheet.  A beam particle carries no id: a cell's
// beam list is put in the lexicographic order of the bit patterns of (x, y, z, ux, uy, uz, w).  The beam's cell list is
// built first, and the plasma's count and fill passes enter a particle only where the beam has one (the gate of
// coll_cell_of), so the plasma list and the cell kernel's work follow the beam's footprint, not the sheet.
#include "engine.h"
#include <rocprim/device/device_scan.hpp>
#include <cfloat>
#include <type_traits>

namespace hps {

constexpr int COLL_LDS_CAP = 64;        // index entries per lane in LDS (both species of a cell together)
constexpr int COLL_WG = 64;             // one wave per workgroup

// side 1 is a sheet (p1); side 0's particles are the cell kernel's second argument, a sheet or a beam slice
struct CollSide { double q, m; int can_ionize; const unsigned* off; unsigned* perm; };
struct CollArgs {
    CollSide s[2]; hps_plasma p1; int same;
    int nx, ny; double plo0, plo1, dxi, dyi;
    double dt, L, dens_fac, c, inv_c, inv_c2; int normalized;
    unsigned long long key;              // coll_hash chain of (seed, collision, step, slice)
    unsigned long long* stats;           // {pairs collided, overfull cells}
};


// ---- counter-based generator: coll_hash / coll_unit (particle_math.h) ----------------------------------------------------
// stream 0: the pairs' draws (a = pair k, b = draw index); stream 1 + slot: the shuffle of species slot (a = position, b = 0)
__device__ __forceinline__ double coll_uniform (unsigned long long cell_key, unsigned stream, unsigned a, unsigned b)
{
    return coll_unit(coll_hash(coll_hash(coll_hash(cell_key, stream), a), b));
}

// ---- the cell lists: the two kinds of source, each with its range, x, y and who takes part ----------------------------------
// A sheet, [0, n): invalid particles (valid bit clear) and particles without weight are in no cell.
struct CollSheet {
    hps_plasma p;
    static constexpr bool thread_per_particle = true;
    __device__ __forceinline__ void range (long* first, long* count) const { *first = 0; *count = p.n; }
    __device__ __forceinline__ double x (long ip) const { return p.x[ip]; }
    __device__ __forceinline__ double y (long ip) const { return p.y[ip]; }
    __device__ __forceinline__ bool takes_part (long ip) const { return (p.idcpu[ip] & HPS_ID_VALID) && p.w[ip] != 0.0; }
};
// A beam slice: slice p of the moving beam, [B[p], B[p + 1]) read on the device -- behind k_beam_partition of that slice, so
// particles that slipped on to slice p + 1 are outside it --, or [0, n) of the free operator (B null).  size: length of the
// SoA's arrays; cap: entries the index list has room for.  Both clamp the range: the launch is sized from a host-side bound.
// Absorbed particles (nsub < 0) and particles without weight are in no cell.
struct CollBeam {
    BeamSoA b; const long* B; int p; long n, size, cap;
    static constexpr bool thread_per_particle = false;      // the range is known on the device only: at most 2048 workgroups stride over it
    __device__ __forceinline__ void range (long* first, long* count) const
    {
        long f = 0, c = n;
        if (B) { f = B[p]; c = B[p + 1] - f; }
        if (f < 0) f = 0;
        if (f > size) f = size;
        if (c > size - f) c = size - f;
        if (c > cap) c = cap;
        if (c < 0) c = 0;
        *first = f; *count = c;
    }
    __device__ __forceinline__ double x (long ip) const { return b.x[ip]; }
    __device__ __forceinline__ double y (long ip) const { return b.y[ip]; }
    __device__ __forceinline__ bool takes_part (long ip) const { return !(b.nsub && b.nsub[ip] < 0) && b.w[ip] != 0.0; }
};

// The cell of particle ip of src, or false if it is in none.  The cell comes from x, y alone -- findParticlesInEachTile(bx, 1,
// ...): int((pos - plo)*dxi), truncation as the reference's static_cast; a particle outside the box is in no bin.  gate, where
// not null, is the final cell offsets of the beam's list: the plasma side of a beam collision enters a particle only where
// the beam has one, and the loads that say whether the particle takes part come last, so a plasma particle outside the
// beam's footprint costs two loads and no atomic.
template <class Src>
__device__ __forceinline__ bool coll_cell_of (const CollArgs& a, const Src& src, long ip, const unsigned* gate, int* cell)
{
    const double x = src.x(ip), y = src.y(ip);
    const int i = (int)((x - a.plo0)*a.dxi), j = (int)((y - a.plo1)*a.dyi);
    if (x < a.plo0 || y < a.plo1 || i < 0 || i >= a.nx || j < 0 || j >= a.ny) return false;
    const int c = i + j*a.nx;
    if (gate && gate[c + 1] == gate[c]) return false;
    if (!src.takes_part(ip)) return false;
    *cell = c;
    return true;
}

// The count pass (FILL = false) and the fill pass of species slot's list, grid-stride over the source's range.  A sheet's
// launch has a thread per particle, and its one trip is compiled as one: most lanes of a gated pass are done after two or
// three dependent loads, the pass is bound by that latency, and without a loop head to come back to the compiler keeps the
// early exits and loads each kernel argument where it is first needed.  The fill pass counts cnt down to 0
// again: position = off[cell] + (what is left of the cell's count) - 1.
template <class Src, bool FILL>
__global__ __launch_bounds__(256)
void k_coll_list (CollArgs a, Src src, int slot, const unsigned* gate, unsigned* cnt)
{
    long first, count;
    src.range(&first, &count);
    for (long t = (long)blockIdx.x*blockDim.x + threadIdx.x; t < count; t += (long)gridDim.x*blockDim.x) {
        int cell;
        if (coll_cell_of(a, src, first + t, gate, &cell)) {
            if constexpr (FILL) a.s[slot].perm[a.s[slot].off[cell] + atomicSub(cnt + cell, 1u) - 1u] = (unsigned)(first + t);
            else atomicAdd(cnt + cell, 1u);
        }
        if constexpr (Src::thread_per_particle) break;
    }
}


// index lists: lane-interleaved LDS (entry i of this lane at b[i*COLL_WG]) or a segment of the global list
struct IdxLds { unsigned* b; __device__ __forceinline__ unsigned& operator[] (int i) const { return b[i*COLL_WG]; } };
struct IdxGlb { unsigned* b; __device__ __forceinline__ unsigned& operator[] (int i) const { return b[i]; } };

__device__ __forceinline__ unsigned long long coll_pkey (const hps_plasma& p, unsigned ip)
{
    return (p.idcpu[ip] >> 24) & ((1ULL << 39) - 1);
}
// a beam particle's key: the bit patterns of (x, y, z, ux, uy, uz, w), compared lexicographically as unsigned integers.
// Two particles that tie on all seven are interchangeable, so the order of a list is a function of the set of particles.
struct BeamKey {
    unsigned long long k[7];
    __device__ __forceinline__ bool operator> (const BeamKey& o) const
    {
        for (int q = 0; q < 7; ++q) if (k[q] != o.k[q]) return k[q] > o.k[q];
        return false;
    }
    __device__ __forceinline__ bool operator<= (const BeamKey& o) const { return !(*this > o); }
};
__device__ __forceinline__ BeamKey coll_pkey (const BeamSoA& b, unsigned ip)
{
    return BeamKey{{(unsigned long long)__double_as_longlong(b.x[ip]), (unsigned long long)__double_as_longlong(b.y[ip]),
                    (unsigned long long)__double_as_longlong(b.z[ip]), (unsigned long long)__double_as_longlong(b.ux[ip]),
                    (unsigned long long)__double_as_longlong(b.uy[ip]), (unsigned long long)__double_as_longlong(b.uz[ip]),
                    (unsigned long long)__double_as_longlong(b.w[ip])}};
}
// the three momentum rows a collision rewrites: (ux_half, uy_half, psi_half) of a sheet, (ux, uy, uz) of a beam slice
__device__ __forceinline__ double* coll_ux (const hps_plasma& p) { return p.ux_half; }
__device__ __forceinline__ double* coll_uy (const hps_plasma& p) { return p.uy_half; }
__device__ __forceinline__ double* coll_u3 (const hps_plasma& p) { return p.psi_half; }
__device__ __forceinline__ double* coll_ux (const BeamSoA& b) { return b.ux; }
__device__ __forceinline__ double* coll_uy (const BeamSoA& b) { return b.uy; }
__device__ __forceinline__ double* coll_u3 (const BeamSoA& b) { return b.uz; }

// canonical order: ascending keys (a sheet's id bits, unique within the species; a beam slice's BeamKey).  Insertion sort
// for short lists, heap sort beyond.
template <class Idx, class Side>
__device__ void coll_order (const Idx& I, int n, const Side& p)
{
    if (n <= COLL_LDS_CAP) {
        for (int i = 1; i < n; ++i) {
            const unsigned v = I[i]; const auto kv = coll_pkey(p, v);
            int j = i - 1;
            while (j >= 0 && coll_pkey(p, I[j]) > kv) { I[j + 1] = I[j]; --j; }
            I[j + 1] = v;
        }
        return;
    }
    auto sift = [&] (int root, int end) {
        const unsigned v = I[root]; const auto kv = coll_pkey(p, v);
        for (;;) {
            int ch = 2*root + 1;
            if (ch >= end) break;
            auto kc = coll_pkey(p, I[ch]);
            if (ch + 1 < end) { const auto k2 = coll_pkey(p, I[ch + 1]); if (k2 > kc) { kc = k2; ++ch; } }
            if (kc <= kv) break;
            I[root] = I[ch]; root = ch;
        }
        I[root] = v;
    };
    for (int i = n/2 - 1; i >= 0; --i) sift(i, n);
    for (int e = n - 1; e > 0; --e) { const unsigned t = I[0]; I[0] = I[e]; I[e] = t; sift(0, e); }
}

// ShuffleFisherYates over entries [0, n): i = n-1 .. 1, j uniform in [0, i]
template <class Idx>
__device__ void coll_shuffle (const Idx& I, int n, unsigned long long cell_key, unsigned slot)
{
    for (int i = n - 1; i >= 1; --i) {
        const int j = (int)(coll_uniform(cell_key, 1u + slot, (unsigned)i, 0u)*(double)(i + 1));
        const unsigned t = I[i]; I[i] = I[j]; I[j] = t;
    }
}

// ComputeTemperature: the plasma branch for a sheet, the beam branch (is_beam_coll, :30-34) for a beam slice
template <class Idx, class Side>
__device__ double coll_temperature (const Idx& I, int n, const Side& p, double m, double c, double inv_c2)
{
    constexpr bool BEAM = std::is_same<Side, BeamSoA>::value;
    if (n == 0) return 0.0;
    double vx = 0.0, vy = 0.0, vz = 0.0, vs = 0.0;
    for (int i = 0; i < n; ++i) {
        const unsigned ip = I[i];
        const double ux = coll_ux(p)[ip], uy = coll_uy(p)[ip], psi = coll_u3(p)[ip];
        const double gm = BEAM ? sqrt(1.0 + (ux*ux + uy*uy + psi*psi)*inv_c2) : (1.0 + (ux*ux + uy*uy)*inv_c2 + psi*psi)/(2.0*psi);
        const double uz = BEAM ? psi : c*(gm - psi);
        const double us = ux*ux + uy*uy + uz*uz;
        vx += ux/gm; vy += uy/gm; vz += uz/gm; vs += us/gm/gm;
    }
    vx = vx/n; vy = vy/n; vz = vz/n; vs = vs/n;
    return m/3.0*(vs - (vx*vx + vy*vy + vz*vz));
}

constexpr double SI_C = 299792458.0, SI_EP0 = 8.8541878128e-12, SI_QE = 1.602176634e-19, SI_ME = 9.1093837015e-31,
                 SI_HBAR = 1.054571817e-34, COLL_PI = 3.14159265358979323846;

// UpdateMomentumPerezElastic.  Returns false if the pair does not collide (no relative momentum).
__device__ bool coll_update (double& u1x, double& u1y, double& u1z, const double g1, double& u2x, double& u2y, double& u2z, const double g2,
                             const double n1, const double n2, const double n12, const double q1, double m1, const double w1,
                             const double q2, double m2, const double w2, const double dt, const double L, const double lmdD,
                             const bool normalized, unsigned long long cell_key, unsigned k)
{
    const double inv_c_SI = 1.0/SI_C, inv_c2_SI = 1.0/(SI_C*SI_C);
    unsigned draw = 0;
    const double diffx = fabs(u1x - u2x), diffy = fabs(u1y - u2y), diffz = fabs(u1z - u2z);
    const double diffm = sqrt(diffx*diffx + diffy*diffy + diffz*diffz);
    const double summm = sqrt(u1x*u1x + u1y*u1y + u1z*u1z) + sqrt(u2x*u2x + u2y*u2y + u2z*u2z);
    if (diffm < DBL_MIN || diffm/summm < 1.0e-10) return false;

    if (normalized) {
        m1 *= SI_ME; m2 *= SI_ME;
        u1x *= SI_C; u1y *= SI_C; u1z *= SI_C; u2x *= SI_C; u2y *= SI_C; u2z *= SI_C;
    }
    const double p1x = u1x*m1, p1y = u1y*m1, p1z = u1z*m1, p2x = u2x*m2, p2y = u2y*m2, p2z = u2z*m2;

    // centre-of-mass velocity and gamma
    const double mass_g = m1*g1 + m2*g2;
    const double vcx = (p1x + p2x)/mass_g, vcy = (p1y + p2y)/mass_g, vcz = (p1z + p2z)/mass_g;
    const double vcms = vcx*vcx + vcy*vcy + vcz*vcz;
    const double gc = 1.0/sqrt(1.0 - vcms*inv_c2_SI);
    const double vcDv1 = (vcx*u1x + vcy*u1y + vcz*u1z)/g1;
    const double vcDv2 = (vcx*u2x + vcy*u2y + vcz*u2z)/g2;

    double p1sx, p1sy, p1sz;
    if (vcms > DBL_MIN) {
        const double lf = ((gc - 1.0)/vcms*vcDv1 - gc)*m1*g1;
        p1sx = p1x + vcx*lf; p1sy = p1y + vcy*lf; p1sz = p1z + vcz*lf;
    } else { p1sx = p1x; p1sy = p1y; p1sz = p1z; }
    const double p1sm = sqrt(p1sx*p1sx + p1sy*p1sy + p1sz*p1sz);

    const double g1s = (1.0 - vcDv1*inv_c2_SI)*gc*g1;
    const double g2s = (1.0 - vcDv2*inv_c2_SI)*gc*g2;

    double lnLmd;
    if (L > 0.0) lnLmd = L;
    else {
        const double b0 = fabs(q1*q2)*inv_c2_SI/(4.0*COLL_PI*SI_EP0)*gc/mass_g*(m1*g1s*m2*g2s/(p1sm*p1sm*inv_c2_SI) + 1.0);
        const double bmin = fmax(SI_HBAR*COLL_PI/p1sm, b0);
        lnLmd = fmax(2.0, 0.5*log(1.0 + lmdD*lmdD/(bmin*bmin)));
    }

    const double tts = m1*g1s*m2*g2s/(inv_c2_SI*p1sm*p1sm) + 1.0;
    const double tts2 = tts*tts;
    const double charge_fac = normalized ? SI_QE*SI_QE*SI_QE*SI_QE : 1.0;
    double s = n1*n2/n12*dt*lnLmd*q1*q1*q2*q2*charge_fac*inv_c2_SI*inv_c2_SI/(4.0*COLL_PI*SI_EP0*SI_EP0*m1*g1*m2*g2)*gc*p1sm/mass_g*tts2;

    const double cbrt_n1 = cbrt(n1), cbrt_n2 = cbrt(n2);
    const double coeff = pow(4.0*COLL_PI/3.0, 1.0/3.0);
    const double vrel = mass_g*p1sm/(m1*g1s*m2*g2s*gc);
    const double sp = coeff*n1*n2/n12*dt*vrel*(m1 + m2)/fmax(m1*cbrt_n1*cbrt_n1, m2*cbrt_n2*cbrt_n2);
    s = fmin(s, sp);

    double r = coll_uniform(cell_key, 0u, k, draw++);
    double cosXs;
    if (s <= 0.1) {
        // the reference redraws while cosXs < -1: r < exp(-2/s) <= exp(-20), once in 5e8 pairs at s = 0.1.  The loop is bounded so
        // that no input (a NaN that slipped into s) can keep a lane spinning: after 64 redraws the pair scatters by pi
        for (int redraw = 0; ; ++redraw) {
            cosXs = 1.0 + s*log(r);
            if (cosXs >= -1.0) break;
            if (redraw == 64) { cosXs = -1.0; break; }
            r = coll_uniform(cell_key, 0u, k, draw++);
        }
    } else if (s <= 3.0) {
        const double Ainv = 0.0056958 + 0.9560202*s - 0.508139*s*s + 0.47913906*s*s*s - 0.12788975*s*s*s*s + 0.02389567*s*s*s*s*s;
        cosXs = Ainv*log(exp(-1.0/Ainv) + 2.0*r*sinh(1.0/Ainv));
    } else if (s <= 6.0) {
        const double A = 3.0*exp(-s);
        cosXs = 1.0/A*log(exp(-A) + 2.0*r*sinh(A));
    } else {
        cosXs = 2.0*r - 1.0;
    }
    const double sinXs = sqrt(1.0 - cosXs*cosXs);

    const double phis = coll_uniform(cell_key, 0u, k, draw++)*2.0*COLL_PI;
    const double cosphis = cos(phis), sinphis = sin(phis);

    double p1fsx, p1fsy, p1fsz;
    double p1sp = sqrt(p1sx*p1sx + p1sy*p1sy);
    if (p1sp > DBL_MIN) {
        p1fsx = (p1sx*p1sz/p1sp)*sinXs*cosphis + (p1sy*p1sm/p1sp)*sinXs*sinphis + p1sx*cosXs;
        p1fsy = (p1sy*p1sz/p1sp)*sinXs*cosphis + (-p1sx*p1sm/p1sp)*sinXs*sinphis + p1sy*cosXs;
        p1fsz = (-p1sp)*sinXs*cosphis + 0.0*sinXs*sinphis + p1sz*cosXs;
    } else {
        p1sp = sqrt(p1sy*p1sy + p1sz*p1sz);
        p1fsy = (p1sy*p1sx/p1sp)*sinXs*cosphis + (p1sz*p1sm/p1sp)*sinXs*sinphis + p1sy*cosXs;
        p1fsz = (p1sz*p1sx/p1sp)*sinXs*cosphis + (-p1sy*p1sm/p1sp)*sinXs*sinphis + p1sz*cosXs;
        p1fsx = (-p1sp)*sinXs*cosphis + 0.0*sinXs*sinphis + p1sx*cosXs;
    }
    const double p2fsx = -p1fsx, p2fsy = -p1fsy, p2fsz = -p1fsz;

    double p1fx, p1fy, p1fz, p2fx, p2fy, p2fz;
    if (vcms > DBL_MIN) {
        const double vcDp1fs = vcx*p1fsx + vcy*p1fsy + vcz*p1fsz;
        const double vcDp2fs = vcx*p2fsx + vcy*p2fsy + vcz*p2fsz;
        const double factor = (gc - 1.0)/vcms;
        const double factor1 = factor*vcDp1fs + m1*g1s*gc;
        const double factor2 = factor*vcDp2fs + m2*g2s*gc;
        p1fx = p1fsx + vcx*factor1; p1fy = p1fsy + vcy*factor1; p1fz = p1fsz + vcz*factor1;
        p2fx = p2fsx + vcx*factor2; p2fy = p2fsy + vcy*factor2; p2fz = p2fsz + vcz*factor2;
    } else {
        p1fx = p1fsx; p1fy = p1fsy; p1fz = p1fsz; p2fx = p2fsx; p2fy = p2fsy; p2fz = p2fsz;
    }

    // rejection for unequal weights (eq. 14): each side on a draw of its own
    r = coll_uniform(cell_key, 0u, k, draw++);
    if (w2 > r*fmax(w1, w2)) { u1x = p1fx/m1; u1y = p1fy/m1; u1z = p1fz/m1; }
    r = coll_uniform(cell_key, 0u, k, draw++);
    if (w1 > r*fmax(w1, w2)) { u2x = p2fx/m2; u2y = p2fy/m2; u2z = p2fz/m2; }
    if (normalized) {
        u1x *= inv_c_SI; u1y *= inv_c_SI; u1z *= inv_c_SI; u2x *= inv_c_SI; u2y *= inv_c_SI; u2z *= inv_c_SI;
    }
    return true;
}

// ElasticCollisionPerez over the lists I1[0, NI1) of species side 0 (P1: a sheet, or a beam slice -- is_beam_coll) and
// I2[0, NI2) of species side 1
template <class Idx, class Side>
__device__ unsigned coll_elastic (const CollArgs& a, const Side& P1, const Idx& I1, int NI1, const Idx& I2, int NI2, unsigned long long cell_key)
{
    constexpr bool BEAM = std::is_same<Side, BeamSoA>::value;
    const hps_plasma& P2 = a.p1;
    double q1 = a.s[0].q, q2 = a.s[1].q;
    const double m1 = a.s[0].m, m2 = a.s[1].m;
    double T1t = -1.0, T2t = -1.0;
    if (a.L <= 0.0) {
        T1t = coll_temperature(I1, NI1, P1, m1, a.c, a.inv_c2);
        T2t = coll_temperature(I2, NI2, P2, m2, a.c, a.inv_c2);
    }
    double n1 = 0.0, n2 = 0.0, n12 = 0.0;
    for (int i = 0; i < NI1; ++i) n1 += P1.w[I1[i]];
    for (int i = 0; i < NI2; ++i) n2 += P2.w[I2[i]];
    if (a.same) { n1 = n1 + n2; n2 = n1; }
    if (n1 == 0.0 || n2 == 0.0) return 0;
    const int NK = NI1 > NI2 ? NI1 : NI2;
    {   int i1 = 0, i2 = 0;
        for (int k = 0; k < NK; ++k) {
            n12 += fmin(P1.w[I1[i1]], P2.w[I2[i2]]);
            ++i1; if (i1 == NI1) i1 = 0;
            ++i2; if (i2 == NI2) i2 = 0;
        }
        if (a.same) n12 *= 2.0; }
    n1 *= a.dens_fac; n2 *= a.dens_fac; n12 *= a.dens_fac;

    double lmdD;
    if (T1t <= 0.0 || T2t <= 0.0) lmdD = 0.0;
    else lmdD = 1.0/sqrt(n1*q1*q1/(T1t*SI_EP0) + n2*q2*q2/(T2t*SI_EP0));
    const double rmin = pow(4.0*COLL_PI/3.0*fmax(n1, n2), -1.0/3.0);
    lmdD = fmax(lmdD, rmin);

    unsigned collided = 0;
    int i1 = 0, i2 = 0;
    for (int k = 0; k < NK; ++k) {
        const unsigned a1 = I1[i1], a2 = I2[i2];
        // the charge follows the ion's level; the reference's product runs on from pair to pair
        if constexpr (!BEAM) { if (a.s[0].can_ionize) q1 *= P1.ion_lev[a1]; }      // (can_ionize1 = false for a beam)
        if (a.s[1].can_ionize) q2 *= P2.ion_lev[a2];
        double u1x = coll_ux(P1)[a1], u1y = coll_uy(P1)[a1]; const double psi1 = coll_u3(P1)[a1];      // a beam's "psi1" is its uz
        double u2x = P2.ux_half[a2], u2y = P2.uy_half[a2]; const double psi2 = P2.psi_half[a2];
        double g1 = BEAM ? sqrt(1.0 + (u1x*u1x + u1y*u1y + psi1*psi1)*a.inv_c2)
                         : (1.0 + u1x*u1x*a.inv_c2 + u1y*u1y*a.inv_c2 + psi1*psi1)/(2.0*psi1);
        double g2 = (1.0 + u2x*u2x*a.inv_c2 + u2y*u2y*a.inv_c2 + psi2*psi2)/(2.0*psi2);
        double u1z = BEAM ? psi1 : a.c*(g1 - psi1), u2z = a.c*(g2 - psi2);
        const double dt_fac = BEAM ? 1.0 : 0.5*(g1/psi1 + g2/psi2);
        if (coll_update(u1x, u1y, u1z, g1, u2x, u2y, u2z, g2, n1, n2, n12, q1, m1, P1.w[a1], q2, m2, P2.w[a2],
                        a.dt*dt_fac, a.L, lmdD, a.normalized != 0, cell_key, (unsigned)k)) ++collided;
        g1 = sqrt(1.0 + (u1x*u1x + u1y*u1y + u1z*u1z)*a.inv_c2);
        coll_ux(P1)[a1] = u1x; coll_uy(P1)[a1] = u1y; coll_u3(P1)[a1] = BEAM ? u1z : g1 - u1z*a.inv_c;
        g2 = sqrt(1.0 + (u2x*u2x + u2y*u2y + u2z*u2z)*a.inv_c2);
        P2.ux_half[a2] = u2x; P2.uy_half[a2] = u2y; P2.psi_half[a2] = g2 - u2z*a.inv_c;
        ++i1; if (i1 == NI1) i1 = 0;
        ++i2; if (i2 == NI2) i2 = 0;
    }
    return collided;
}

// One cell: both lists in canonical order, shuffled (slot 0 is side 0, slot 1 the sheet of side 1), then the pairs.  Same
// species (sheets only): the one list is split at its middle, the first half shuffled, the halves collided.
template <class Idx, class Side>
__device__ unsigned coll_cell (const CollArgs& a, const Side& p0, const Idx& IA, int nA, const Idx& IB, int nB, unsigned long long cell_key)
{
    if constexpr (std::is_same<Side, hps_plasma>::value) if (a.same) {
        coll_order(IA, nA, p0);
        const int half = nA/2;                       // (start + stop)/2 of the reference, relative to start
        coll_shuffle(IA, half, cell_key, 0u);
        Idx I2 = IA; I2.b = &IA[half];
        return coll_elastic(a, p0, IA, half, I2, nA - half, cell_key);
    }
    coll_order(IA, nA, p0); coll_order(IB, nB, a.p1);
    coll_shuffle(IA, nA, cell_key, 0u); coll_shuffle(IB, nB, cell_key, 1u);
    return coll_elastic(a, p0, IA, nA, IB, nB, cell_key);
}

template <class Side0>
__global__ __launch_bounds__(COLL_WG)
void k_coll_cells (CollArgs a, Side0 p0)
{
    __shared__ unsigned lds[COLL_LDS_CAP*COLL_WG];
    const int cell = blockIdx.x*COLL_WG + threadIdx.x;
    if (cell >= a.nx*a.ny) return;
    const unsigned sA = a.s[0].off[cell], nA = a.s[0].off[cell + 1] - sA;
    unsigned sB = 0, nB = 0;
    if (std::is_same<Side0, hps_plasma>::value && a.same) { if (nA <= 1) return; }
    else {
        if (nA < 1) return;                          // (no beam particle here: the gated plasma list is empty too)
        sB = a.s[1].off[cell]; nB = a.s[1].off[cell + 1] - sB;
        if (nB < 1) return;
    }
    const unsigned long long cell_key = coll_hash(a.key, (unsigned long long)cell);
    unsigned collided;
    if (nA + nB <= (unsigned)COLL_LDS_CAP) {
        IdxLds IA{lds + threadIdx.x}, IB{lds + threadIdx.x + nA*COLL_WG};
        for (unsigned i = 0; i < nA; ++i) IA[i] = a.s[0].perm[sA + i];
        for (unsigned i = 0; i < nB; ++i) IB[i] = a.s[1].perm[sB + i];
        collided = coll_cell(a, p0, IA, (int)nA, IB, (int)nB, cell_key);
    } else {
        atomicAdd(a.stats + 1, 1ULL);
        IdxGlb IA{a.s[0].perm + sA}, IB{a.s[1].perm + sB};
        collided = coll_cell(a, p0, IA, (int)nA, IB, (int)nB, cell_key);
    }
    if (collided) atomicAdd(a.stats, (unsigned long long)collided);
}


// ---- host side -------------------------------------------------------------------------------------------------------
CollScratch::~CollScratch ()
{
    for (int s = 0; s < 2; ++s) { (void)hipFree(off[s]); (void)hipFree(perm[s]); }
    (void)hipFree(cnt); (void)hipFree(temp); (void)hipFree(stats);
}

static int coll_reserve (CollScratch& S, int ncells, long n0, long n1)
{
    if (!S.stats) { HPS_HIP_CHECK(hipMalloc(&S.stats, 2*sizeof(unsigned long long))); HPS_HIP_CHECK(hipMemset(S.stats, 0, 2*sizeof(unsigned long long))); }
    if (ncells > S.ncells) {
        (void)hipFree(S.cnt); (void)hipFree(S.off[0]); (void)hipFree(S.off[1]); (void)hipFree(S.temp);
        S.cnt = nullptr; S.off[0] = S.off[1] = nullptr; S.temp = nullptr; S.ncells = 0;
        // the scan runs over ncells + 1 counters (the last one 0) so that off[ncells] is the total
        HPS_HIP_CHECK(hipMalloc(&S.cnt, (size_t)(ncells + 1)*sizeof(unsigned)));
        HPS_HIP_CHECK(hipMemset(S.cnt, 0, (size_t)(ncells + 1)*sizeof(unsigned)));
        for (int s = 0; s < 2; ++s) HPS_HIP_CHECK(hipMalloc(&S.off[s], (size_t)(ncells + 1)*sizeof(unsigned)));
        S.temp_bytes = 0;
        HPS_HIP_CHECK(rocprim::exclusive_scan(nullptr, S.temp_bytes, S.cnt, S.off[0], 0u, (size_t)(ncells + 1), rocprim::plus<unsigned>(), (hipStream_t)0));
        HPS_HIP_CHECK(hipMalloc(&S.temp, std::max<size_t>(S.temp_bytes, 16)));
        S.ncells = ncells;
    }
    const long want[2] = {n0, n1};
    for (int s = 0; s < 2; ++s) if (want[s] > S.cap[s]) {
        (void)hipFree(S.perm[s]); S.perm[s] = nullptr; S.cap[s] = 0;
        HPS_HIP_CHECK(hipMalloc(&S.perm[s], (size_t)want[s]*sizeof(unsigned)));
        S.cap[s] = want[s];
    }
    return HPS_OK;
}

// what a plasma-plasma and a beam-plasma collision share: geometry, units, dt in seconds, the slice key
static CollArgs coll_args (CollScratch& S, const hps_geom& gm, int nx, int ny, double dt, double coulomb_log, double background_density_SI,
                           unsigned long long seed, int collision, int step, int islice)
{
    CollArgs a{};
    a.nx = nx; a.ny = ny; a.plo0 = gm.plo[0]; a.plo1 = gm.plo[1]; a.dxi = 1.0/gm.dx; a.dyi = 1.0/gm.dy;
    a.dt = dt;
    a.L = coulomb_log;
    // normalised weights are densities in units of the background density; SI weights are numbers of particles
    a.dens_fac = gm.normalized ? background_density_SI : (1.0/gm.dx)*(1.0/gm.dy)*(1.0/gm.dz);
    a.c = gm.c; a.inv_c = 1.0/gm.c; a.inv_c2 = 1.0/(gm.c*gm.c); a.normalized = gm.normalized;
    a.key = coll_hash(coll_hash(coll_hash(coll_hash(seed, 0ULL), (unsigned long long)collision), (unsigned long long)step), (unsigned long long)islice);
    a.stats = S.stats;
    return a;
}

// the refusals of both kinds.  n0, n1: the sizes of the two sides' arrays
static int coll_check (const hps_geom& gm, int nx, int ny, long n0, long n1, double background_density_SI)
{
    HPS_REQUIRE(nx > 0 && ny > 0 && (long)nx*ny < (1L << 31) - 1, "collisions: bad grid");
    HPS_REQUIRE(n0 >= 0 && n1 >= 0 && n0 < (1L << 32) - 1 && n1 < (1L << 32) - 1, "collisions: sheets and beams of up to 2^32 - 2 particles");
    HPS_REQUIRE(!gm.normalized || background_density_SI > 0.0, "collisions: normalised units need hipace.background_density_SI (Hipace.cpp:239-243)");
    return HPS_OK;
}

// Species slot's cell list of src: count, scan, fill, with `threads` threads in the two passes.  gate: see coll_cell_of.
template <class Src>
static int coll_build_list (CollScratch& S, const CollArgs& a, const Src& src, int slot, long threads, const unsigned* gate, hipStream_t st)
{
    const dim3 grid((unsigned)((threads + 255)/256));
    // (cnt is all zero here: allocated so, and the fill pass counts it down again)
    hipLaunchKernelGGL((k_coll_list<Src, false>), grid, dim3(256), 0, st, a, src, slot, gate, S.cnt);
    size_t tb = S.temp_bytes;
    HPS_HIP_CHECK(rocprim::exclusive_scan(S.temp, tb, S.cnt, S.off[slot], 0u, (size_t)(a.nx*a.ny + 1), rocprim::plus<unsigned>(), st));
    hipLaunchKernelGGL((k_coll_list<Src, true>), grid, dim3(256), 0, st, a, src, slot, gate, S.cnt);
    return HPS_OK;
}

template <class Side0>
static int coll_cells (const CollArgs& a, const Side0& p0, hipStream_t st)
{
    hipLaunchKernelGGL(k_coll_cells<Side0>, dim3((unsigned)((a.nx*a.ny + COLL_WG - 1)/COLL_WG)), dim3(COLL_WG), 0, st, a, p0);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

// One collision over two sheets (the same sheet twice: same species), enqueued on st.  S keeps the cell lists.
int collide_plasma (CollScratch& S, const hps_plasma& pa, const hps_plasma& pb, bool same, const hps_geom& gm, int nx, int ny,
                    double qa, double ma, int can_ionize_a, double qb, double mb, int can_ionize_b, double coulomb_log,
                    double background_density_SI, unsigned long long seed, int collision, int step, int islice, hipStream_t st)
{
    if (int e = coll_check(gm, nx, ny, pa.n, pb.n, background_density_SI)) return e;
    if (pa.n == 0 || pb.n == 0) return HPS_OK;
    if (int e = coll_reserve(S, nx*ny, pa.n, same ? 0 : pb.n)) return e;
    const double wp = std::sqrt(background_density_SI*SI_QE*SI_QE/(SI_EP0*SI_ME));
    CollArgs a = coll_args(S, gm, nx, ny, gm.normalized ? gm.dz/wp : gm.dz/SI_C, coulomb_log, background_density_SI, seed, collision, step, islice);
    a.s[0] = CollSide{qa, ma, can_ionize_a, S.off[0], S.perm[0]};
    a.s[1] = same ? a.s[0] : CollSide{qb, mb, can_ionize_b, S.off[1], S.perm[1]};
    a.p1 = same ? pa : pb;
    a.same = same ? 1 : 0;
    if (int e = coll_build_list(S, a, CollSheet{pa}, 0, pa.n, nullptr, st)) return e;
    if (!same) if (int e = coll_build_list(S, a, CollSheet{pb}, 1, pb.n, nullptr, st)) return e;
    return coll_cells(a, pa, st);
}

// One collision between a beam slice (side 0) and a sheet, enqueued on st.  bound: host-side upper bound of the slice's
// size (it sizes the beam's launches, at most 2048 workgroups; the kernels read the range on the device); dt: the run's time
// step in seconds.  Seven launches: the beam's count, scan and fill, the plasma's gated on the beam's offsets, the cell kernel.
int collide_beam_plasma (CollScratch& S, CollBeam m, long bound, const hps_plasma& pl, const hps_geom& gm, int nx, int ny,
                         double q_beam, double m_beam, double q_pl, double m_pl, int can_ionize_pl, double coulomb_log,
                         double background_density_SI, double dt, unsigned long long seed, int collision, int step, int islice, hipStream_t st)
{
    if (int e = coll_check(gm, nx, ny, m.size, pl.n, background_density_SI)) return e;
    if (bound <= 0 || m.size == 0 || pl.n == 0) return HPS_OK;
    // the beam's index list has room for the whole beam: the bound grows from slice to slice, the list is allocated once
    if (int e = coll_reserve(S, nx*ny, m.size, pl.n)) return e;
    m.cap = S.cap[0];
    CollArgs a = coll_args(S, gm, nx, ny, dt, coulomb_log, background_density_SI, seed, collision, step, islice);
    a.s[0] = CollSide{q_beam, m_beam, 0, S.off[0], S.perm[0]};
    a.s[1] = CollSide{q_pl, m_pl, can_ionize_pl, S.off[1], S.perm[1]};
    a.p1 = pl;
    a.same = 0;
    if (int e = coll_build_list(S, a, m, 0, std::min<long>(std::min(bound, m.size), 2048L*256), nullptr, st)) return e;
    if (int e = coll_build_list(S, a, CollSheet{pl}, 1, pl.n, S.off[0], st)) return e;
    return coll_cells(a, m.b, st);
}

int coll_read_stats (CollScratch& S, long* pairs, long* overfull, hipStream_t st)
{
    unsigned long long h[2] = {0, 0};
    HPS_HIP_CHECK(hipStreamSynchronize(st));
    if (S.stats) HPS_HIP_CHECK(hipMemcpy(h, S.stats, sizeof(h), hipMemcpyDeviceToHost));
    if (pairs) *pairs = (long)h[0];
    if (overfull) *overfull = (long)h[1];
    return HPS_OK;
}

// doCoulombCollision (Hipace.cpp:1034-1064): the configured collisions in order
int Engine::collide_slice (int islice)
{
    for (size_t i = 0; i < coll.size(); ++i) {
        const Collision& c = coll[i];
        const Species &A = sp[c.a], &B = sp[c.b];
        if (c.beam) {
            // Species 1 is the beam's slice behind its push and the slipped-particle shift (Hipace.cpp:704-712).  A static beam
            // (hipace.dt = 0) sits in the per-slice blocks, and every pair's s is 0 there: nothing is launched.  No beam: nothing.
            if (!moving || nbeam <= 0) continue;
            const int p = d.nz - 1 - islice;
            const long bound = beam_bound(p);
            if (bound <= 0) continue;
            const double wp = std::sqrt(d.background_density_SI*SI_QE*SI_QE/(SI_EP0*SI_ME));
            const double dt = gm.normalized ? step_dt/wp : step_dt;      // m_dt, the time step of the run (not dz)
            const CollBeam bs{bm, d_B, p, 0, nbeam, 0};
            if (int e = collide_beam_plasma(coll_scratch, bs, bound, B.pl, gm, d.nx, d.ny, d.beam_charge, d.beam_mass != 0.0 ? d.beam_mass : 1.0,
                                            B.charge, B.mass, B.can_ionize, c.coulomb_log, d.background_density_SI, dt, c.seed, (int)i, step_index, islice, st)) return e;
            continue;
        }
        if (int e = collide_plasma(coll_scratch, A.pl, B.pl, c.a == c.b, gm, d.nx, d.ny, A.charge, A.mass, A.can_ionize, B.charge, B.mass, B.can_ionize,
                                   c.coulomb_log, d.background_density_SI, c.seed, (int)i, step_index, islice, st)) return e;
    }
    return HPS_OK;
}

} // namespace hps

using namespace hps;

extern "C" int hps_collide_plasma (hps_plasma a, void* tiling_a, hps_plasma b, void* tiling_b, hps_geom geom, int nx, int ny,
                                   double charge_a, double mass_a, int can_ionize_a, double charge_b, double mass_b, int can_ionize_b,
                                   double coulomb_log, double background_density_SI, unsigned long long seed, int collision,
                                   int step, int islice, long* pairs_collided_host, long* overfull_cells_host, hps_stream stream)
{
    (void)tiling_a; (void)tiling_b;      // the cell lists are built from x, y: the order of the sheets does not enter
    const bool same = a.x == b.x && a.ux_half == b.ux_half;
    HPS_REQUIRE(!same || a.n == b.n, "hps_collide_plasma: the same sheet twice must have the same size");
    hipStream_t st = (hipStream_t)stream;
    CollScratch S;
    if (int e = collide_plasma(S, a, b, same, geom, nx, ny, charge_a, mass_a, can_ionize_a, charge_b, mass_b, can_ionize_b, coulomb_log,
                               background_density_SI, seed, collision, step, islice, st)) return e;
    return coll_read_stats(S, pairs_collided_host, overfull_cells_host, st);
}

// the refusals that hps_engine_add_collision and hps_engine_add_beam_collision share, in the words of fn.  species_ok /
// species_msg: the caller's own check of its species arguments, which comes second; ion: the collision names species 1
static int coll_add_check (const void* h, const std::string& fn, bool species_ok, const char* species_msg, bool ion, const char* at_most)
{
    HPS_REQUIRE(h, fn + ": null engine");
    const Engine* E = static_cast<const Engine*>(h);
    HPS_REQUIRE(species_ok, fn + species_msg);
    HPS_REQUIRE(!E->step_begun, fn + ": call before the first hps_engine_begin_step");
    HPS_REQUIRE((int)E->coll.size() < HPS_MAX_COLLISIONS, fn + at_most);
    HPS_REQUIRE(E->d.si_units || E->d.background_density_SI > 0.0, fn + ": collisions in normalised units need hipace.background_density_SI");
    HPS_REQUIRE(!ion || E->d.ion_on, fn + ": species 1 needs the species \"ion\" (ion_on)");
    if (E->d.ion_on && E->d.ion_init_level < E->d.ion_Z) {
        set_error(fn + ": the species \"ion\" can still ionise, and the electrons it releases carry no unique key for the collision draws");
        return HPS_ERR_UNSUPPORTED;
    }
    return HPS_OK;
}

extern "C" int hps_engine_add_collision (void* h, int species_a, int species_b, double coulomb_log, unsigned long long seed)
{
    const Engine* E = static_cast<const Engine*>(h);
    if (int e = coll_add_check(h, "hps_engine_add_collision", E && E->plasma_species_ok(species_a) && E->plasma_species_ok(species_b),
                               ": species are 0 (plasma), 1 (ion) or the index of an added species", species_a == 1 || species_b == 1,
                               ": at most HPS_MAX_COLLISIONS collisions")) return e;
    static_cast<Engine*>(h)->coll.push_back(Engine::Collision{species_a, species_b, coulomb_log, seed});
    return HPS_OK;
}

extern "C" int hps_collide_beam_plasma (hps_beam_slice beam, hps_plasma plasma, hps_geom geom, int nx, int ny, double charge_beam,
                                        double mass_beam, double charge_plasma, double mass_plasma, int can_ionize_plasma,
                                        double coulomb_log, double background_density_SI, unsigned long long seed, int collision,
                                        int step, int islice, double dt, long* pairs_collided_host, long* overfull_cells_host,
                                        hps_stream stream)
{
    HPS_REQUIRE(beam.n >= 0 && (beam.n == 0 || (beam.x && beam.y && beam.z && beam.ux && beam.uy && beam.uz && beam.w)),
                "hps_collide_beam_plasma: the beam slice needs its seven arrays");
    hipStream_t st = (hipStream_t)stream;
    CollScratch S;
    const CollBeam bs{BeamSoA{beam.x, beam.y, beam.z, beam.ux, beam.uy, beam.uz, beam.w, beam.nsub, nullptr, nullptr, nullptr},
                      nullptr, 0, beam.n, beam.n, 0};
    if (int e = collide_beam_plasma(S, bs, beam.n, plasma, geom, nx, ny, charge_beam, mass_beam, charge_plasma, mass_plasma, can_ionize_plasma,
                                    coulomb_log, background_density_SI, dt, seed, collision, step, islice, st)) return e;
    return coll_read_stats(S, pairs_collided_host, overfull_cells_host, st);
}

extern "C" int hps_engine_add_beam_collision (void* h, int plasma_species, double coulomb_log, unsigned long long seed)
{
    if (h && plasma_species >= 2 && static_cast<const Engine*>(h)->plasma_species_ok(plasma_species)) {
        set_error("hps_engine_add_beam_collision: a beam collision with a further plasma species (index >= 2) is not supported");
        return HPS_ERR_UNSUPPORTED;
    }
    if (int e = coll_add_check(h, "hps_engine_add_beam_collision", plasma_species == 0 || plasma_species == 1,
                               ": the plasma species is 0 (plasma) or 1 (ion)", plasma_species == 1,
                               ": at most HPS_MAX_COLLISIONS collisions, of both kinds together")) return e;
    Engine* E = static_cast<Engine*>(h);
    if (E->multi_beam()) {
        set_error("hps_engine_add_beam_collision: the engine holds several beam species (hps_engine_add_beam_species); the collision takes one beam's charge and mass");
        return HPS_ERR_UNSUPPORTED;
    }
    if (E->d.dt_adaptive) {
        set_error("hps_engine_add_beam_collision: hipace.dt = adaptive is not supported with a beam collision: the reference gathers the beam's "
                  "moments behind the collisions (GatherMinUzSlice, Hipace.cpp:713-716), the engine reduces them inside k_beam_partition, ahead of them");
        return HPS_ERR_UNSUPPORTED;
    }
    Engine::Collision c{0, plasma_species, coulomb_log, seed};
    c.beam = true;
    E->coll.push_back(c);
    return HPS_OK;
}

extern "C" int hps_engine_collision_stats (void* h, long* pairs_collided, long* overfull_cells)
{
    HPS_REQUIRE(h, "hps_engine_collision_stats: null engine");
    Engine* E = static_cast<Engine*>(h);
    return coll_read_stats(E->coll_scratch, pairs_collided, overfull_cells, E->st);
}
