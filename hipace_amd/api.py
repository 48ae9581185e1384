"""Host-side mirror of the reference's operator interface for the slice hot path, on top of the
C ABI (include/hpslice.h).  Names, argument meaning and error behaviour follow the reference's
C++ seams:

    DepositCurrent(plasma, fields, ...)          particles/deposition/PlasmaDepositCurrent.H:28-32
    ExplicitDeposition(plasma, fields, ...)      particles/deposition/ExplicitDeposition.H:20-22
    AdvancePlasmaParticles(plasma, fields, ...)  particles/pusher/PlasmaParticleAdvance.H:23-26
    FFTPoissonSolver.SolvePoissonEquation(lhs)   fields/fft_poisson_solver/FFTPoissonSolver.H:26-57
    MultiGrid.solve1(sol, rhs, acoef, ...)       mg_solver/HpMultiGrid.H:64-66
    SliceEngine                                  Hipace::Evolve / SolveOneSlice (Hipace.cpp:393-728)

PyTorch is used only to own device memory and streams; all arithmetic happens in libhpslice.so.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, decks as _decks, expr as _expr
from ._lib import CIDX, COMPS, ID_VALID, PL_REAL, check


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _iarr(vals):
    return (C.c_int * len(vals))(*[int(v) for v in vals])


class Geometry:
    """Slice geometry + physical constants + particle boundary (hps_geom)."""

    def __init__(self, nx, ny, lo, hi, dz, bc=1, normalized=True, consts=(1., 1., 1., 1., 1.), ng=None):
        self.nx, self.ny = nx, ny
        g = _lib.Geom()
        g.dx = (hi[0] - lo[0]) / nx
        g.dy = (hi[1] - lo[1]) / ny
        g.dz = dz
        # GetPosOffset (fields/Fields.H:71-77): independent of the number of guard cells
        g.xoff = 0.5 * (lo[0] + hi[0] - g.dx * (nx - 1))
        g.yoff = 0.5 * (lo[1] + hi[1] - g.dy * (ny - 1))
        g.c, g.ep0, g.mu0, g.q_e, g.m_e = consts
        g.plo = (C.c_double * 2)(lo[0], lo[1])
        g.phi = (C.c_double * 2)(hi[0], hi[1])
        g.bc = bc
        g.normalized = int(normalized)
        self.c = g


class Fields:
    """The field slab: ncomp planes of (ny+2ng, nx+2ng) doubles in HBM (fields/Fields.H:465)."""

    def __init__(self, nx, ny, ng, ncomp, device="cuda", data=None):
        self.nx, self.ny, self.ng, self.ncomp = nx, ny, ng, ncomp
        shape = (ncomp, ny + 2 * ng, nx + 2 * ng)
        if data is None:
            self.t = torch.zeros(shape, dtype=torch.float64, device=device)
        else:
            self.t = torch.as_tensor(np.ascontiguousarray(data), dtype=torch.float64).reshape(shape).to(device).contiguous()

    def struct(self):
        s = _lib.Slab()
        s.p = self.t.data_ptr()
        s.nx, s.ny, s.ng, s.ncomp = self.nx, self.ny, self.ng, self.ncomp
        s.jstride = self.nx + 2 * self.ng
        s.nstride = s.jstride * (self.ny + 2 * self.ng)
        return s

    def numpy(self):
        return self.t.cpu().numpy()


class PlasmaSheet:
    """Pure-SoA plasma sheet (particles/plasma/PlasmaParticleContainer.H:21-50)."""

    def __init__(self, real, valid=None, ion_lev=None, device="cuda", key=None):
        """key: per-particle integers, unique within the sheet, stored as key + 1 in the id bits of idcpu (what the
        engine's lattice particles carry: the key of the ionisation and collision draws); None: id 1 for every particle."""
        real = np.ascontiguousarray(real, dtype=np.float64)
        assert real.shape[0] == 11
        self.n = real.shape[1]
        self.real = torch.as_tensor(real).to(device).contiguous()
        if valid is None:
            valid = np.ones(self.n, dtype=np.int32)
        idcpu = np.where(np.asarray(valid) != 0, np.uint64(ID_VALID | (1 << 24)), np.uint64(1 << 24)).astype(np.uint64)
        if key is not None:
            ids = (np.asarray(key, dtype=np.uint64) + np.uint64(1)) << np.uint64(24)
            idcpu = (idcpu & np.uint64(ID_VALID)) | ids
        self.idcpu = torch.as_tensor(idcpu.view(np.int64)).to(device).contiguous()
        if ion_lev is None:
            ion_lev = np.zeros(self.n, dtype=np.int32)
        self.ion_lev = torch.as_tensor(np.asarray(ion_lev, dtype=np.int32)).to(device).contiguous()

    def struct(self):
        p = _lib.Plasma()
        base = self.real.data_ptr()
        for k, name in enumerate(PL_REAL):
            setattr(p, name, base + 8 * k * self.n)
        p.idcpu = self.idcpu.data_ptr()
        p.ion_lev = self.ion_lev.data_ptr()
        p.n = self.n
        return p

    def numpy(self):
        idc = self.idcpu.cpu().numpy().view(np.uint64)
        return self.real.cpu().numpy(), ((idc >> np.uint64(63)) & np.uint64(1)).astype(np.int32)


class BoxSorter:
    """BoxSorter::sortParticlesByBox (particles/sorting/BoxSort.H:18-48): beam particles -> longitudinal boxes."""

    def sortParticlesByBox(self, z, plo_z, dz, num_boxes):
        """z: float64 device tensor.  Fills boxCounts / boxOffsets (num_boxes + 1 each) and boxPermutations
        (perm[new] = old) as numpy uint64 arrays."""
        z = z.contiguous()
        n = z.numel()
        counts = torch.zeros(num_boxes + 1, dtype=torch.int64, device=z.device)
        offsets = torch.zeros(num_boxes + 1, dtype=torch.int64, device=z.device)
        perm = torch.zeros(max(n, 1), dtype=torch.int64, device=z.device)
        check(_lib.lib().hps_beam_sort_by_box(C.c_void_p(z.data_ptr() if n else 0), n, float(plo_z), float(dz), num_boxes,
                                              C.c_void_p(counts.data_ptr()), C.c_void_p(offsets.data_ptr()),
                                              C.c_void_p(perm.data_ptr()), _stream()))
        torch.cuda.synchronize()
        self.boxCounts = counts.cpu().numpy().astype(np.uint64)
        self.boxOffsets = offsets.cpu().numpy().astype(np.uint64)
        self.boxPermutations = perm[:n].cpu().numpy().astype(np.uint64)
        return self


class Tiling:
    """Tile binning of a plasma sheet (the reference's ReorderParticles hook)."""

    def __init__(self, nx, ny, tile_size, max_particles):
        self._h = C.c_void_p()
        check(_lib.lib().hps_tiling_create(nx, ny, tile_size, max_particles, C.byref(self._h)))
        self.fallback = torch.zeros(1, dtype=torch.int32, device="cuda")

    def reorder(self, plasma, geom):
        """Stable sort of `plasma` by tile; returns the reordered PlasmaSheet (a new SoA buffer)."""
        out = PlasmaSheet.__new__(PlasmaSheet)
        out.n = plasma.n
        out.real = torch.empty_like(plasma.real)
        out.idcpu = torch.empty_like(plasma.idcpu)
        out.ion_lev = torch.empty_like(plasma.ion_lev)
        check(_lib.lib().hps_reorder_particles(self._h, plasma.struct(), out.struct(), geom.c, _stream()))
        return out

    def set_validity(self, by_weight=False, by_psi_half=False):
        """The caller's promise that every invalid particle of the sheet has w == 0 (by_weight) / psi_half == 0
        (by_psi_half): the tiled operators then take the engine's variants that read validity from there."""
        check(_lib.lib().hps_tiling_set_validity(self._h, int(by_weight), int(by_psi_half)))

    def info(self):
        nt, off, perm = C.c_int(), C.c_void_p(), C.c_void_p()
        check(_lib.lib().hps_tiling_info(self._h, C.byref(nt), C.byref(off), C.byref(perm)))
        return nt.value, off.value, perm.value

    def offsets_and_perm(self, n):
        torch.cuda.synchronize()
        nt, off, perm = self.info()
        o = np.empty(nt + 2, dtype=np.int32)
        p = np.empty(n, dtype=np.uint32)
        check(_lib.lib().hps_memcpy_d2h(o.ctypes.data_as(C.c_void_p), C.c_void_p(off), o.nbytes))
        if n:
            check(_lib.lib().hps_memcpy_d2h(p.ctypes.data_as(C.c_void_p), C.c_void_p(perm), p.nbytes))
        return o, p

    def launch_order(self):
        """-> (order int32 (ntiles,), records int32 (ntiles, 4)): workgroup b of a tile kernel works on tile order[b];
        records[b] = {tile, first particle, end, 0}.  Read-only copies of what the last reorder left on the device."""
        torch.cuda.synchronize()
        nt, off, _ = self.info()
        order = np.empty(nt, dtype=np.int32)
        rec = np.empty((nt, 4), dtype=np.int32)
        check(_lib.lib().hps_memcpy_d2h(order.ctypes.data_as(C.c_void_p), C.c_void_p(off + 4 * (nt + 2)), order.nbytes))
        check(_lib.lib().hps_memcpy_d2h(rec.ctypes.data_as(C.c_void_p), C.c_void_p(off + 4 * ((2 * nt + 2 + 3) & ~3)), rec.nbytes))
        return order, rec

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.lib().hps_tiling_destroy(self._h)
            self._h = None


def DepositCurrent(plasma, fields, geom, charge, mass, depos_order, jx=-1, jy=-1, jz=-1, rho=-1, chi=-1,
                   rhomjz=-1, max_qsa_weighting_factor=35.0, can_ionize=False, n_qsa=None, tiling=None, aabs=-1):
    """aabs: slab component holding the laser's |a|^2 (-1: no laser)."""
    comp = _iarr([jx, jy, jz, rho, chi, rhomjz])
    nq = C.c_void_p(n_qsa.data_ptr()) if n_qsa is not None else None
    if tiling is None:
        check(_lib.lib().hps_deposit_current_laser(fields.struct(), plasma.struct(), geom.c, comp, aabs, charge, mass,
                                                   depos_order, max_qsa_weighting_factor, int(can_ionize), nq, _stream()))
    else:
        check(_lib.lib().hps_deposit_current_tiled_laser(fields.struct(), plasma.struct(), geom.c, comp, aabs, charge, mass,
                                                         depos_order, max_qsa_weighting_factor, int(can_ionize), nq,
                                                         tiling._h, C.c_void_p(tiling.fallback.data_ptr()), _stream()))


def ExplicitDeposition(plasma, fields, geom, charge, mass, depos_order, Bz, Ez, ExmBy, EypBx, Sy, Sx,
                       derivative_type=2, can_ionize=False, tiling=None, aabs=-1):
    if tiling is None:
        check(_lib.lib().hps_explicit_deposit_laser(fields.struct(), plasma.struct(), geom.c, _iarr([Bz, Ez, ExmBy, EypBx]),
                                                    aabs, _iarr([Sy, Sx]), charge, mass, depos_order, derivative_type,
                                                    int(can_ionize), _stream()))
    else:
        check(_lib.lib().hps_explicit_deposit_tiled_laser(fields.struct(), plasma.struct(), geom.c,
                                                          _iarr([Bz, Ez, ExmBy, EypBx]), aabs, _iarr([Sy, Sx]), charge, mass,
                                                          depos_order, derivative_type, int(can_ionize), tiling._h,
                                                          C.c_void_p(tiling.fallback.data_ptr()), _stream()))


def AdvancePlasmaParticles(plasma, fields, geom, charge, mass, depos_order, Psi, Ez, Bx, By, Bz,
                           temp_slice=False, n_subcycles=1, can_ionize=False, tiling=None, aabs=-1):
    if tiling is None:
        check(_lib.lib().hps_advance_plasma_laser(fields.struct(), plasma.struct(), geom.c, _iarr([Psi, Ez, Bx, By, Bz]),
                                                  aabs, charge, mass, depos_order, int(temp_slice), n_subcycles,
                                                  int(can_ionize), _stream()))
    else:
        check(_lib.lib().hps_advance_plasma_tiled_laser(fields.struct(), plasma.struct(), geom.c,
                                                        _iarr([Psi, Ez, Bx, By, Bz]), aabs, charge, mass, depos_order,
                                                        int(temp_slice), n_subcycles, int(can_ionize), tiling._h,
                                                        C.c_void_p(tiling.fallback.data_ptr()), _stream()))


def CoulombCollision(plasma_a, plasma_b, geom, charge_a, mass_a, charge_b=None, mass_b=None, can_ionize_a=False,
                     can_ionize_b=False, coulomb_log=-1.0, background_density_SI=0.0, seed=0, collision=0, step=0, islice=0,
                     tiling_a=None, tiling_b=None):
    """doPlasmaPlasmaCoulombCollision (particles/collisions/CoulombCollision.cpp:59-236) over two PlasmaSheets -- the same
    sheet twice collides a species with itself.  ux_half, uy_half, psi_half are rewritten in place.  Returns (pairs
    collided, overfull cells); see hps_collide_plasma."""
    if plasma_b is plasma_a or charge_b is None:
        charge_b, mass_b, can_ionize_b = charge_a, mass_a, can_ionize_a
    pairs, over = C.c_long(), C.c_long()
    check(_lib.lib().hps_collide_plasma(plasma_a.struct(), tiling_a._h if tiling_a is not None else None,
                                        plasma_b.struct(), tiling_b._h if tiling_b is not None else None, geom.c, geom.nx, geom.ny,
                                        charge_a, mass_a, int(can_ionize_a), charge_b, mass_b, int(can_ionize_b), coulomb_log,
                                        background_density_SI, seed, collision, step, islice, C.byref(pairs), C.byref(over),
                                        _stream()))
    return pairs.value, over.value


class BeamSlice:
    """A beam slice on the device for BeamPlasmaCollision: soa = (7, n) array x y z ux uy uz w (the rows of
    SliceEngine.beam_state), nsub = per-particle sub-cycle counters (< 0: absorbed) or None."""

    def __init__(self, soa, nsub=None, device="cuda"):
        soa = np.ascontiguousarray(soa, dtype=np.float64)
        assert soa.ndim == 2 and soa.shape[0] == 7
        self.n = soa.shape[1]
        self.soa = torch.as_tensor(soa).to(device).contiguous()
        self.nsub = None if nsub is None else torch.as_tensor(np.ascontiguousarray(nsub, dtype=np.int32)).to(device).contiguous()
        assert self.nsub is None or self.nsub.numel() == self.n

    def struct(self):
        b = _lib.BeamSlice()
        base = self.soa.data_ptr()
        for k, name in enumerate(("x", "y", "z", "ux", "uy", "uz", "w")):
            setattr(b, name, base + 8 * k * self.n)
        b.nsub = self.nsub.data_ptr() if self.nsub is not None else None
        b.n = self.n
        return b

    def numpy(self):
        return self.soa.cpu().numpy()


def BeamPlasmaCollision(beam, plasma, geom, charge_beam, mass_beam, charge_plasma, mass_plasma, dt, can_ionize_plasma=False,
                        coulomb_log=-1.0, background_density_SI=0.0, seed=0, collision=0, step=0, islice=0):
    """doBeamPlasmaCoulombCollision (particles/collisions/CoulombCollision.cpp:238-348) over a BeamSlice and a PlasmaSheet: the
    beam's ux, uy, uz and the sheet's ux_half, uy_half, psi_half are rewritten in place.  dt: the run's time step in seconds
    (hipace.dt over omega_p in normalised units).  Returns (pairs collided, overfull cells); see hps_collide_beam_plasma."""
    pairs, over = C.c_long(), C.c_long()
    check(_lib.lib().hps_collide_beam_plasma(beam.struct(), plasma.struct(), geom.c, geom.nx, geom.ny, charge_beam, mass_beam,
                                             charge_plasma, mass_plasma, int(can_ionize_plasma), coulomb_log, background_density_SI,
                                             seed, collision, step, islice, dt, C.byref(pairs), C.byref(over), _stream()))
    return pairs.value, over.value


def record_particle_dispatch(on=True):
    """Switch the dispatch record of the tiled particle kernels on (emptying it) or off (hps_particles_record)."""
    check(_lib.lib().hps_particles_record(int(on)))


def recorded_particle_dispatch():
    """The set of tiled particle kernel instances launched since record_particle_dispatch(True), such as
    'k_deposit_tiled<2,16,51,0,1>' (template arguments as integers)."""
    n = C.c_long()
    check(_lib.lib().hps_particles_recorded(None, 0, C.byref(n)))
    buf = C.create_string_buffer(n.value + 1)
    check(_lib.lib().hps_particles_recorded(buf, n.value + 1, C.byref(n)))
    return set(buf.value.decode().split())


class LaserInterp:
    """The two grid-to-grid interpolations of a laser envelope on a grid of its own (lasers.n_cell / patch_lo / patch_hi /
    interp_order) as operators: UpdateLaserAabs (laser/MultiLaser.cpp:253-284) and InterpolateChi (:334-407).  The laser grid
    is n_cell = (nxl, nyl) cells on patch_lo .. patch_hi (x, y); geom is the field slab's Geometry."""

    def __init__(self, n_cell, patch_lo, patch_hi, order=1):
        self.nxl, self.nyl = int(n_cell[0]), int(n_cell[1])
        self.dxl, self.dyl = (patch_hi[0] - patch_lo[0]) / self.nxl, (patch_hi[1] - patch_lo[1]) / self.nyl
        self.xoffl = 0.5 * (patch_lo[0] + patch_hi[0] - self.dxl * (self.nxl - 1))      # GetPosOffset of the laser box
        self.yoffl = 0.5 * (patch_lo[1] + patch_hi[1] - self.dyl * (self.nyl - 1))
        self.order = int(order)

    def _plane(self, t, dtype):
        assert t.is_cuda and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == (self.nyl, self.nxl)
        return C.c_void_p(t.data_ptr())

    def aabs(self, fields, geom, aabs_comp, a):
        """slab component aabs_comp (guard cells included) <- |a|^2 of the complex128 device tensor a (nyl, nxl)"""
        check(_lib.lib().hps_laser_interp_aabs(fields.struct(), int(aabs_comp), self._plane(a, torch.complex128), self.nxl, self.nyl,
                                               self.dxl, self.dyl, self.xoffl, self.yoffl, geom.c, self.order, _stream()))

    def chi(self, fields, geom, chi_comp, chi_initial, shrink=None):
        """-> float64 device tensor (nyl, nxl): slab component chi_comp interpolated on the laser cells that lie on the field box
        shrunk by `shrink` cells (default: the slab's guard width, as the engine), chi_initial (nyl, nxl) elsewhere"""
        out = torch.empty((self.nyl, self.nxl), dtype=torch.float64, device=chi_initial.device)
        check(_lib.lib().hps_laser_interp_chi(fields.struct(), int(chi_comp), self._plane(chi_initial, torch.float64),
                                              C.c_void_p(out.data_ptr()), self.nxl, self.nyl, self.dxl, self.dyl, self.xoffl, self.yoffl,
                                              geom.c, fields.ng if shrink is None else int(shrink), self.order, _stream()))
        return out


def open_boundary(planes, lo, hi, no_monopole_mask=0):
    """boundary.field = Open on source planes of the caller's (hps_open_boundary, the engine's own two kernels): planes is a
    CUDA float64 tensor (nbatch, ny, nx) on the box lo .. hi (x, y), updated in place -- the outermost rows and columns get the
    Dirichlet corrections of the sources' free-space potential; bit b of no_monopole_mask drops the monopole of plane b."""
    if not (isinstance(planes, torch.Tensor) and planes.is_cuda and planes.dtype == torch.float64 and planes.dim() == 3
            and planes.is_contiguous()):
        raise ValueError("open_boundary: planes must be a contiguous CUDA float64 tensor (nbatch, ny, nx)")
    nbatch, ny, nx = planes.shape
    check(_lib.lib().hps_open_boundary(C.c_void_p(planes.data_ptr()), nbatch, nx, ny, (C.c_double * 2)(lo[0], lo[1]),
                                       (C.c_double * 2)(hi[0], hi[1]), int(no_monopole_mask), _stream()))
    return planes


class FFTPoissonSolver:
    """Lap(F) = S, F = 0 one cell outside the box; S lives in the staging area."""

    def __init__(self, nx, ny, dx, dy, device="cuda"):
        self.nx, self.ny = nx, ny
        self._h = C.c_void_p()
        check(_lib.lib().hps_poisson_create(nx, ny, dx, dy, C.byref(self._h)))
        self.staging = torch.zeros((ny, nx), dtype=torch.float64, device=device)

    def StagingArea(self):
        return self.staging

    BACKENDS = ("own-sym", "own-pow2", "dense", "rocfft")      # HPS_POISSON_* of include/hpslice.h

    def info(self):
        """(backend, x_len, tri_rows) the size dispatch chose: backend one of BACKENDS, x_len the length nx + 1 of the own DST
        kernel along x (0: none), tri_rows the rows per thread M of k_tridiag_y<M, ..> along y (0: none, rocFFT)."""
        b, n, m = C.c_int(), C.c_int(), C.c_int()
        check(_lib.lib().hps_poisson_info(self._h, C.byref(b), C.byref(n), C.byref(m)))
        return self.BACKENDS[b.value], n.value, m.value

    def SolvePoissonEquation(self, lhs_fields, comp):
        check(_lib.lib().hps_poisson_solve(self._h, C.c_void_p(self.staging.data_ptr()), lhs_fields.struct(), comp,
                                           _stream()))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.lib().hps_poisson_destroy(self._h)
            self._h = None


class MultiGrid2:
    """hpmg::MultiGrid system type 2 (complex coefficient: the laser envelope solve), solve2 with an array Re and a scalar
    Im coefficient.  sol2 / rhs2: CUDA float64 tensors (2, ny, nx); acoef_real (ny, nx); acoef_imag a 1-element tensor."""

    def __init__(self, nx, ny, dx, dy):
        self._h = C.c_void_p()
        check(_lib.lib().hps_mg2_create(nx, ny, dx, dy, C.byref(self._h)))

    def solve2(self, sol2, rhs2, acoef_real, acoef_imag, tol_rel=1e-4, tol_abs=0.0, nummaxiter=200):
        it = C.c_int()
        rn = C.c_double()
        for t in (sol2, rhs2, acoef_real, acoef_imag):
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float64
        check(_lib.lib().hps_mg2_solve2(self._h, sol2.data_ptr(), rhs2.data_ptr(), acoef_real.data_ptr(), acoef_imag.data_ptr(),
                                        tol_rel, tol_abs, nummaxiter, C.byref(it), C.byref(rn), _stream()))
        return it.value, rn.value

    BOTTOMS = ("lower-v", "single-block", "per-sweep")      # HPS_MG2_BOTTOM_* of include/hpslice.h
    TILES = ("single-block", "32x16", "64x32")              # HPS_MG2_TILE_*

    def info(self):
        """What the size dispatch chose: {"nlev", "low_top" (first level of k2_lower_v, -1: none), "bottom" (one of BOTTOMS:
        k2_lower_v, or the generic bottom in one k2_sweeps launch or one launch per sweep), "tiles" (one of TILES for each
        level above the bottom part)}."""
        nl, top, b, t = C.c_int(), C.c_int(), C.c_int(), (C.c_int * 31)()
        check(_lib.lib().hps_mg2_info(self._h, C.byref(nl), C.byref(top), C.byref(b), t))
        return {"nlev": nl.value, "low_top": top.value, "bottom": self.BOTTOMS[b.value],
                "tiles": tuple(self.TILES[v] for v in t if v >= 0)}

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.lib().hps_mg2_destroy(self._h)
            self._h = None


class MultiGrid:
    """hpmg::MultiGrid system type 1.

    The levels from the first one with at most 34 x 34 cells down run in one workgroup with all their arrays in LDS
    (k_lower_v3 / k_lower_v).  Where no level is that small and the coarsest one does not fit one workgroup's LDS (160 KiB:
    300^2, 129^2 or 1025^2, whose coarsening stops early), the coarsest level is swept in global memory instead, with
    max(16, longest side rounded up to even) red-black sweeps: the reference's CPU branch, for which it prints the warning
    that the grid should be a power of two (cell-centred) or one more (node-centred) for the single-block bottom solver
    (HpMultiGrid.cpp:1076-1089, 1583-1593).  The solution is the reference's either way; info() reports the choice."""

    def __init__(self, nx, ny, dx, dy):
        self._h = C.c_void_p()
        check(_lib.lib().hps_mg_create(nx, ny, dx, dy, C.byref(self._h)))

    LOWV = ("v3", "v-cc", "v-nodal", "bottom")                      # HPS_MG_LOWV_* of include/hpslice.h
    TILES = ("TileSmall", "TileBig", "TileSmall-pull", "TileMid-pull")    # HPS_MG_TILE_*

    def info(self, schedule=False):
        """What the size dispatch chose: {"cc", "nlev", "lowv_begin", "lowv" (one of LOWV), "lowv_lds" (dynamic LDS bytes of the
        lower V, 0 for the bottom), "tiles" (one of TILES for level 0's initial pass and the down-leg of levels 1 ..
        lowv_begin - 1), "nodal_pull1", "pyramid" (levels k_acf_pyramid / k_nodal_acf_pyramid<n> derives), "restricts"
        (k_restrict launches behind it)}.  schedule=True adds what the schedule switches chose when the solver was created:
        "coef_guest" (k_lower_v3's coefficient image comes from a guest workgroup of the initial level-0 pass,
        HPS_MG_COEF_GUEST)."""
        cc, nl, lb, kind, npyr, nres, pull1 = (C.c_int() for _ in range(7))
        lds, t = C.c_long(), (C.c_int * 31)()
        check(_lib.lib().hps_mg_info(self._h, C.byref(cc), C.byref(nl), C.byref(lb), C.byref(kind), C.byref(lds), t,
                                     C.byref(pull1), C.byref(npyr), C.byref(nres)))
        out = {"cc": bool(cc.value), "nlev": nl.value, "lowv_begin": lb.value, "lowv": self.LOWV[kind.value],
               "lowv_lds": lds.value, "tiles": tuple(self.TILES[v] for v in t if v >= 0), "nodal_pull1": bool(pull1.value),
               "pyramid": npyr.value, "restricts": nres.value}
        if schedule:
            guest = C.c_int()
            check(_lib.lib().hps_mg_info_schedule(self._h, C.byref(guest)))
            out["coef_guest"] = bool(guest.value)
        return out

    def upleg_fused_levels(self):
        """n where the mid levels 1 .. n of a V-cycle make their up-leg in one launch (k_up_fused: 2 or 3; HPS_MG_UP_FUSED,
        read when the solver is created), 0 where every mid level has a launch of its own."""
        n = C.c_int()
        check(_lib.lib().hps_mg_info_upleg(self._h, C.byref(n)))
        return n.value

    def solve1(self, fields, sol_comp, rhs_comp, acoef_comp, tol_rel=1e-4, tol_abs=2.2250738585072014e-308,
               nummaxiter=200):
        it = C.c_int()
        rn = C.c_double()
        check(_lib.lib().hps_mg_solve1(self._h, fields.struct(), sol_comp, rhs_comp, acoef_comp, tol_rel, tol_abs,
                                       nummaxiter, C.byref(it), C.byref(rn), _stream()))
        return it.value, rn.value

    def solve1_fabs(self, sol, rhs, acoef, tol_rel=1e-4, tol_abs=2.2250738585072014e-308, nummaxiter=200):
        """hpmg::MultiGrid::solve1(sol, rhs, acoef, ...) with three separate `Fields` (HpMultiGrid.H:64-66): sol and rhs with
        two components, acoef with one; sol is the initial guess on entry."""
        it = C.c_int()
        rn = C.c_double()
        check(_lib.lib().hps_mg_solve1_fabs(self._h, sol.struct(), rhs.struct(), acoef.struct(), tol_rel, tol_abs, nummaxiter,
                                            C.byref(it), C.byref(rn), _stream()))
        return it.value, rn.value

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.lib().hps_mg_destroy(self._h)
            self._h = None


class Expression:
    """A parsed function of the input file as a device operator (hps_expr_eval): Expression("if(x > 0, sin(x), y^2)",
    variables=("x", "y"))(x, y) evaluates the compiled program (hipace_amd/expr.py) with one lane per element on float64
    device tensors of one shape.  evaluate_host runs the same routine on the CPU over numpy arrays (hps_expr_eval_host, no
    device); .program.evaluate is the numpy restatement."""

    def __init__(self, text, variables=("x", "y", "z", "t"), constants=None):
        self.program = text if isinstance(text, _expr.Program) else _expr.compile_expr(text, variables, constants)
        self._c, self._keep = self.program.c_struct()
        depth = C.c_int()
        check(_lib.lib().hps_expr_check(C.byref(self._c), len(self.program.variables), C.byref(depth)))
        self.depth = depth.value

    def __call__(self, *tensors, out=None):
        nv = len(self.program.variables)
        if len(tensors) != nv:
            raise ValueError(f"Expression: {nv} tensors expected ({', '.join(self.program.variables)}), got {len(tensors)}")
        if out is None and not tensors:
            raise ValueError("Expression: a program without variables needs out=")
        for t in tensors:
            assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.shape == tensors[0].shape
        if out is None:
            out = torch.empty_like(tensors[0])
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and (not tensors or out.shape == tensors[0].shape)
        ptrs = (C.c_void_p * max(nv, 1))(*[t.data_ptr() if t.numel() else None for t in tensors])
        check(_lib.lib().hps_expr_eval(C.byref(self._c), nv, out.numel(), ptrs, C.c_void_p(out.data_ptr() if out.numel() else None),
                                       _stream()))
        return out

    def evaluate_host(self, *arrays):
        nv = len(self.program.variables)
        if len(arrays) != nv:
            raise ValueError(f"Expression: {nv} arrays expected ({', '.join(self.program.variables)}), got {len(arrays)}")
        a = [np.ascontiguousarray(v, dtype=np.float64) for v in np.broadcast_arrays(*arrays)] if arrays else []
        out = np.empty(a[0].shape if a else (1,), dtype=np.float64)
        ptrs = (C.c_void_p * max(nv, 1))(*[v.ctypes.data for v in a])
        check(_lib.lib().hps_expr_eval_host(C.byref(self._c), nv, out.size, ptrs, out.ctypes.data_as(C.c_void_p)))
        return out


class AdaptiveTimeStep:
    """hipace.dt = adaptive: the reference's controller (utils/AdaptiveTimeStep.cpp) over hps_adaptive_* -- host code, no
    device.  One per rank / pipeline stage, all initialised alike."""

    def __init__(self, deck, density_profile=None, density_exprs=None, beams=None, plasma_species=None):
        """plasma_species: the further plasma species as decks.plasma_species gives them (default: the deck's own entry), each
        one more species of rho_max(z) (hps_adaptive_add_species).  density_exprs: {species: (text_or_table, constants)} of parsed densities; default: the deck's own
        (decks.DENSITY_EXPR_DEFAULT), as SliceEngine applies them.  beams: [dict(charge, mass, uz_mean, uz_std)], one per beam
        species (default: the deck's entry beam_species behind the deck's own beam); with more than one the controller runs per
        beam (hps_adaptive_*_beams): CalculateFromMinUz takes the moments [n][4] of SliceEngine.beam_moments(species=all)"""
        self.deck = dict(deck)
        if beams is None:
            more = [s["record"] for s in _decks.beam_species(deck)]
            beams = ([dict(charge=deck.get("beam_charge", -1.0), mass=deck.get("beam_mass", 1.0))] + more) if more else None
        self.beams = None if beams is None or len(beams) < 2 else [dict(b) for b in beams]
        self._dk = _lib.fill_struct(_lib.Deck(), deck)
        self._h = C.c_void_p()
        check(_lib.lib().hps_adaptive_create(C.byref(self._dk), C.byref(self._h)))
        if density_profile is not None:
            self.set_density_profile(*density_profile)
        more_sp = _decks.plasma_species(deck) if plasma_species is None else list(plasma_species)
        self.plasma_species_names = list(_decks.PLASMA_SPECIES_NAMES)
        own = density_exprs is None
        if own:
            density_exprs = {sp: spec[:2] for sp, spec in _decks.density_exprs(deck).items()}
        for spec in more_sp:
            k = self.add_species(spec["record"]["charge"], spec["record"]["density"], spec.get("name"))
            if own and spec.get("density") is not None:
                density_exprs[k] = spec["density"][:2]
        for sp, spec in density_exprs.items():
            self.set_density_expr(sp, *spec)

    @classmethod
    def for_engine(cls, engine):
        """a controller for `engine`'s deck, density profile and density programs"""
        exprs = {sp: ((progs[0] if pos is None else list(zip(pos, progs))), None)
                 for sp, (progs, pos, _) in getattr(engine, "density_exprs", {}).items()}
        names, _ = engine.beam_species()
        beams = [r for r in engine.beam_species_records] if len(names) > 1 else None
        return cls(engine.deck, getattr(engine, "density_profile", None), exprs, beams, getattr(engine, "plasma_species_specs", []))

    def add_species(self, charge, density, name=None):
        """one more plasma species for rho_max(z) (hps_adaptive_add_species) -> its index (2, 3, ...)"""
        k = _lib.lib().hps_adaptive_add_species(self._h, float(charge), float(density))
        if k < 0:
            raise _lib.HpsError(f"hps_adaptive_add_species: {_lib.lib().hps_last_error().decode()}")
        self.plasma_species_names.append(name or f"species{k}")
        return k

    def _beam_arrays(self):
        q = np.array([b["charge"] for b in self.beams], dtype=np.float64)
        m = np.array([b["mass"] for b in self.beams], dtype=np.float64)
        return q, m

    def set_density_expr(self, species, text_or_table, constants=None):
        """the species' parsed density (SliceEngine.set_density_expr): rho_max(z) takes |charge * density(0, 0, z)|"""
        sp = _decks.plasma_species_index(self.plasma_species_names, species) if isinstance(species, str) else int(species)
        progs, pos = _expr.compile_density(text_or_table, constants)
        arr, keep = _expr.c_programs(progs)
        z = (C.c_double * len(pos))(*pos) if pos is not None else None
        check(_lib.lib().hps_adaptive_set_density_expr(self._h, sp, len(progs), arr, z))

    def rho_max(self, z):
        """MultiPlasma::maxChargeDensity(z) as the controller takes it (hps_adaptive_rho_max)"""
        out = C.c_double()
        check(_lib.lib().hps_adaptive_rho_max(self._h, float(z), C.byref(out)))
        return out.value

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.lib().hps_adaptive_destroy(self._h)
            self._h = None

    def set_density_profile(self, r=(), fr=(), ct=(), ft=()):
        a = [np.ascontiguousarray(v, dtype=np.float64) for v in (r, fr, ct, ft)]
        assert len(a[0]) == len(a[1]) and len(a[2]) == len(a[3])
        p = [x.ctypes.data_as(C.c_void_p) if len(x) else None for x in a]
        check(_lib.lib().hps_adaptive_set_density_profile(self._h, len(a[0]), p[0], p[1], len(a[2]), p[2], p[3]))

    def initial_dt(self, uz_mean=None, uz_std=None, nstages=1):
        """the head rank's GatherMinUzSlice(beams, true) + CalculateFromMinUz + CalculateFromDensity (Hipace.cpp:275-279);
        default: the deck's u_mean[2] and beam_uz_std.  -> dt"""
        um = self.deck["beam_umean"][2] if uz_mean is None else uz_mean
        us = self.deck.get("beam_uz_std", 0.0) if uz_std is None else uz_std
        if uz_std is None and us == 0.0 and self.deck.get("beam_density_expr") is not None:
            us = (self.deck.get("beam_u_std") or (0, 0, 0))[2]      # decks.BEAM_INIT_DEFAULT: the fixed_ppc beam's own u_std[2]
        dt = C.c_double()
        if self.beams is not None:      # per beam: species 0 as above, the others from their own uz_mean / uz_std
            ums = np.array([um] + [b.get("uz_mean", 0.0) for b in self.beams[1:]], dtype=np.float64)
            uss = np.array([us] + [b.get("uz_std", 0.0) for b in self.beams[1:]], dtype=np.float64)
            q, m = self._beam_arrays()
            check(_lib.lib().hps_adaptive_initial_dt_beams(self._h, len(self.beams), ums.ctypes.data_as(C.c_void_p),
                                                           uss.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p),
                                                           m.ctypes.data_as(C.c_void_p), int(nstages), C.byref(dt)))
            return dt.value
        check(_lib.lib().hps_adaptive_initial_dt(self._h, float(um), float(us), int(nstages), C.byref(dt)))
        return dt.value

    def CalculateFromDensity(self, t):
        """start of the step at time t: phase-advance control, then hipace.max_time (Hipace.cpp:420-435).  -> its dt"""
        dt = C.c_double()
        check(_lib.lib().hps_adaptive_before_step(self._h, float(t), C.byref(dt)))
        return dt.value

    def next_time(self):
        """time of the step after the one CalculateFromDensity began (MultiBuffer::put_time; inf: no further step)"""
        t = C.c_double()
        check(_lib.lib().hps_adaptive_next_time(self._h, C.byref(t)))
        return t.value

    def CalculateFromMinUz(self, moments, t, nstages=1):
        """end of the step that started at t, from its moments (SliceEngine.beam_moments).  -> this controller's next dt"""
        m = np.ascontiguousarray(moments, dtype=np.float64)
        dt = C.c_double()
        if self.beams is not None:
            assert m.shape == (len(self.beams), 4)
            q, ms = self._beam_arrays()
            check(_lib.lib().hps_adaptive_after_step_beams(self._h, len(self.beams), m.ctypes.data_as(C.c_void_p),
                                                           q.ctypes.data_as(C.c_void_p), ms.ctypes.data_as(C.c_void_p), float(t),
                                                           int(nstages), C.byref(dt)))
            return dt.value
        assert m.shape == (4,)
        check(_lib.lib().hps_adaptive_after_step(self._h, m.ctypes.data_as(C.c_void_p), float(t), int(nstages), C.byref(dt)))
        return dt.value


class SliceEngine:
    """Device-resident slice loop for one deck (see hipace_amd/decks.py)."""

    def __init__(self, deck, device=0, tile_size=None, sort_period=None, fine_patch=None, fine_transition_cells=None):
        """fine_patch: plasmas.fine_patch(x,y) as a callable f(x, y) over numpy arrays (> 0 / True = fine) or a boolean
        (ny, nx) mask, with fine_transition_cells (default 5, the reference's) cells of transition around it; default: the
        deck's "fine_patch" / "fine_transition_cells" entries.  Needs plasma_fine_ppc and / or ion_fine_ppc in the deck."""
        self.deck = dict(deck)
        self.step_times = []            # hipace.dt = adaptive in a pipeline: (step, t, dt) of every step this engine began
        self._dk = _lib.fill_struct(_lib.Deck(), deck)
        # <beam>.density(x,y,z), min_density, u_std, random_ppc (decks.BEAM_INIT_DEFAULT): the device generator replaces the beam
        # of beam_profile, so the library is not asked to build that one first.  A deck without these keys changes nothing here.
        beam = _decks.beam_init(deck)
        if beam is not None:
            self._dk.beam_profile = -1
        # the fixed_weight beam (the deck's optional entry beam_fixed_weight, decks.BEAM_FIXED_WEIGHT_DEFAULT): likewise
        beam_fw = _decks.beam_fixed_weight(deck)
        if beam_fw is not None:
            self._dk.beam_profile = -1
        # ... and the fixed_weight_pdf beam (beam_fixed_weight_pdf, decks.BEAM_FIXED_WEIGHT_PDF_DEFAULT)
        beam_fwp = _decks.beam_fixed_weight_pdf(deck)
        if beam_fwp is not None:
            self._dk.beam_profile = -1
        self._h = C.c_void_p()
        check(_lib.lib().hps_engine_create(C.byref(self._dk), device, C.byref(self._h)))
        # SALAME on a witness species of a moving-beam engine (decks.SALAME_SPECIES_DEFAULT): announced ahead of every other
        # setter -- the engine allocates the SALAME slice now; a deck without the key and without a do_salame species makes no call
        if _decks.beam_species_salame(deck):
            self.deck["beam_species_salame"] = 1
            check(_lib.lib().hps_engine_set_beam_species_salame(self._h, 1))
        # the beam species: species 0 is the deck's beam; the deck's entry beam_species is applied further down
        self.beam_species_names = [deck.get("beam_name", "beam")]
        self.beam_species_records = [dict(charge=deck.get("beam_charge", -1.0), mass=deck.get("beam_mass", 1.0),
                                          uz_mean=deck["beam_umean"][2] if "beam_umean" in deck else 0.0,
                                          uz_std=deck.get("beam_uz_std", 0.0))]
        # the plasma species: 0 = "plasma", 1 = "ion"; the deck's entry plasma_species is appended here, ahead of the
        # setters that take a species' index or name (a deck without the entry makes no call)
        self.plasma_species_names = list(_decks.PLASMA_SPECIES_NAMES)
        self.plasma_species_specs = []
        if tile_size is not None:
            check(_lib.lib().hps_engine_set_tiling(self._h, tile_size, sort_period or 128))
        for spec in _decks.plasma_species(deck):
            self._add_plasma_species(spec)
        # not members of hps_deck: applied through the setters, fine_ppc ahead of the patch
        pf, jf = tuple(deck.get("plasma_fine_ppc", (0, 0))), tuple(deck.get("ion_fine_ppc", (0, 0)))
        hollow = float(deck.get("plasma_hollow_core_radius", 0.0))
        if any(pf) or any(jf) or hollow != 0.0:
            check(_lib.lib().hps_engine_set_plasma_init(self._h, (C.c_int * 2)(*pf), (C.c_int * 2)(*jf), hollow))
        # warm plasmas (decks.PLASMA_THERMAL_DEFAULT): a deck without these keys, or with all of them zero, makes no call
        for sp, name in enumerate(("plasma", "ion")):
            u_mean = tuple(float(v) for v in deck.get(name + "_u_mean", (0.0, 0.0, 0.0)))
            u_std = _decks.thermal_u_std(deck, name)
            if any(u_mean) or any(u_std):
                self.set_plasma_momentum(sp, u_mean, u_std, deck.get("plasma_seed", 0))
        sym, prevent = deck.get("plasmas_do_symmetrize", 0), deck.get("plasmas_prevent_centered_particle", 0)
        if sym or prevent:
            self.set_plasma_symmetry(sym, prevent)
        # lasers.n_cell / patch_lo / patch_hi / interp_order (decks.LASER_GRID_DEFAULT): a deck without these keys makes no call
        if _decks.has_laser_grid(deck):
            self.set_laser_grid(deck.get("laser_n_cell"), deck.get("laser_patch_lo"), deck.get("laser_patch_hi"),
                                deck.get("laser_interp_order", 1))
        # several pulses, parser profiles, in-situ laser reductions (decks.LASER_PULSE_DEFAULT): a deck without these keys makes no call
        if deck.get("lasers") is not None:
            self.set_laser_pulses(deck["lasers"])
        for fn in deck.get("laser_profiles", ()):
            self.add_laser_profile(fn)
        if deck.get("laser_insitu", 0):
            self.set_insitu_laser(True)
        if fine_patch is None:
            fine_patch = deck.get("fine_patch")
        if fine_patch is not None:
            if fine_transition_cells is None:
                fine_transition_cells = deck.get("fine_transition_cells", 5)
            self.set_fine_patch(fine_patch, fine_transition_cells)
        for a, b, coulomb_log, seed in deck.get("collisions", ()):      # not a member of hps_deck: applied through the setters
            if a == "beam":                                             # ("beam", plasma species, CoulombLog, seed)
                self.add_beam_collision(b, coulomb_log, seed)
            else:
                self.add_collision(a, b, coulomb_log, seed)
        ext = deck.get("beam_external_fields")      # beams.external_E / external_B: dict(E=(...), B=(...), constants={...})
        if ext is not None:
            unknown = set(ext) - {"E", "B", "constants"}
            if unknown:
                raise ValueError(f"beam_external_fields: unknown entries {sorted(unknown)}")
            self.set_beam_external_fields(ext.get("E"), ext.get("B"), ext.get("constants"))
        # <plasma>.density(x,y,z), min_density, density_table_file (decks.DENSITY_EXPR_DEFAULT): a deck without these keys makes no call
        for sp, spec in _decks.density_exprs(deck).items():
            self.set_density_expr(sp, *spec)
        if beam is not None:      # (a deck without the keys makes no call)
            self.set_beam_fixed_ppc(**beam)
        if beam_fw is not None:
            self.beam_left_out = self.set_beam_fixed_weight(**beam_fw)
        if beam_fwp is not None:
            self.beam_left_out = self.set_beam_fixed_weight_pdf(**beam_fwp)
        # further beam species (decks.BEAM_SPECIES_DEFAULT): a deck without the entry makes no call
        for spec in _decks.beam_species(deck):
            self._add_beam_species(spec)
        nc, ng, npart = C.c_int(), C.c_int(), C.c_long()
        check(_lib.lib().hps_engine_info(self._h, C.byref(nc), C.byref(ng), C.byref(npart)))
        self.ncomp, self.ng, self.nparticles = nc.value, ng.value, npart.value

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.lib().hps_engine_destroy(self._h)
            self._h = None

    def begin_step(self):
        check(_lib.lib().hps_engine_begin_step(self._h))

    def solve_slice(self, islice):
        check(_lib.lib().hps_engine_solve_slice(self._h, islice))

    def solve_slice_begin(self, islice):
        """the slice up to the Bx/By solve's norm read-back, enqueued without waiting (see hps_engine_solve_slice_begin)"""
        check(_lib.lib().hps_engine_solve_slice_begin(self._h, islice))

    def solve_slice_finish(self, islice):
        check(_lib.lib().hps_engine_solve_slice_finish(self._h, islice))

    def slice_ready(self):
        """would solve_slice_finish return without waiting for the device?"""
        return bool(_lib.lib().hps_engine_slice_ready(self._h))

    def run_step(self):
        check(_lib.lib().hps_engine_run_step(self._h))

    def sync(self):
        check(_lib.lib().hps_engine_sync(self._h))

    def set_tiling(self, tile_size=16, sort_period=128):
        check(_lib.lib().hps_engine_set_tiling(self._h, tile_size, sort_period))

    def fine_patch_mask(self, fine_patch):
        """plasmas.fine_patch(x,y) > 0 at the cell centres lo + (i + 0.5) dx as a (ny, nx) uint8 array; a mask is passed on"""
        nx, ny = self.deck["nx"], self.deck["ny"]
        if callable(fine_patch):
            lo, hi = self.deck["lo"], self.deck["hi"]
            dx, dy = (hi[0] - lo[0]) / nx, (hi[1] - lo[1]) / ny
            x = lo[0] + (np.arange(nx) + 0.5) * dx
            y = lo[1] + (np.arange(ny) + 0.5) * dy
            fine_patch = np.broadcast_to(np.asarray(fine_patch(x[None, :], y[:, None])), (ny, nx)) > 0
        m = np.ascontiguousarray(np.asarray(fine_patch) != 0, dtype=np.uint8)
        if m.shape != (ny, nx):
            raise ValueError(f"fine_patch: the mask must have the shape (ny, nx) = {(ny, nx)}, not {m.shape}")
        return m

    def set_fine_patch(self, fine_patch, transition_cells=5):
        """plasmas.fine_patch(x,y) and fine_transition_cells (hps_engine_set_fine_patch), before the first begin_step:
        fine_patch is a callable f(x, y) over numpy arrays or a boolean (ny, nx) mask."""
        m = self.fine_patch_mask(fine_patch)
        check(_lib.lib().hps_engine_set_fine_patch(self._h, m.ctypes.data_as(C.c_void_p), int(transition_cells)))
        npart = C.c_long()
        check(_lib.lib().hps_engine_info(self._h, None, None, C.byref(npart)))
        self.nparticles = npart.value

    def set_plasma_momentum(self, species=0, u_mean=(0.0, 0.0, 0.0), u_std=(0.0, 0.0, 0.0), seed=0):
        """<plasma>.u_mean / u_std of species 0 (plasma) / 1 (ion) / a further species (index or name) in units of c and the seed of its momentum draws
        (hps_engine_set_plasma_momentum), before the first begin_step."""
        check(_lib.lib().hps_engine_set_plasma_momentum(self._h, self._plasma_index(species), (C.c_double * 3)(*u_mean), (C.c_double * 3)(*u_std), int(seed)))

    # ---- further plasma species in one engine -------------------------------------------
    def _plasma_index(self, species):
        """a name -> its index (ValueError: unknown); a number passes as it is: the library refuses one it does not hold"""
        return _decks.plasma_species_index(self.plasma_species_names, species) if isinstance(species, str) else int(species)

    def _add_plasma_species(self, spec):
        rec = _lib.fill_struct(_lib.PlasmaSpecies(), spec["record"])
        k = C.c_int()
        check(_lib.lib().hps_engine_add_plasma_species(self._h, C.byref(rec), C.byref(k)))
        self.plasma_species_names.append(spec["name"] or f"species{k.value}")
        self.plasma_species_specs.append(spec)
        if any(spec["u_mean"]) or any(spec["u_std"]):
            self.set_plasma_momentum(k.value, spec["u_mean"], spec["u_std"], spec["seed"])
        if spec["density"] is not None:
            self.set_density_expr(k.value, *spec["density"])
        return k.value

    def add_plasma_species(self, **spec):
        """One more fixed-charge plasma species behind "plasma" (0) and "ion" (1) (hps_engine_add_plasma_species and the
        per-species setters), before the first begin_step.  spec: decks.PLASMA_SPECIES_DEFAULT -- name, charge (default: the
        opposite of the plasma's), mass, density, ppc, fine_ppc, neutralize_background, u_mean, u_std | temperature_in_ev, seed,
        density_expr | density_table, density_constants, min_density.  -> the species' index"""
        if spec.get("name") is not None and spec["name"] in self.plasma_species_names:
            raise ValueError(f"add_plasma_species: a name is given twice ({spec['name']!r})")
        return self._add_plasma_species(_decks.plasma_species_spec(self.deck, spec, "add_plasma_species"))

    def plasma_species(self):
        """-> (names, counts) of the engine's plasma species: "plasma", "ion" (count 0 in a deck without it), the further ones"""
        n = C.c_int()
        counts = (C.c_long * _decks.MAX_PLASMA_SPECIES)()
        check(_lib.lib().hps_engine_plasma_species_info(self._h, C.byref(n), counts))
        return list(self.plasma_species_names[:n.value]), [counts[k] for k in range(n.value)]

    def plasma(self, species=0):
        """The sheet of plasma species `species` (index or name): (real (11, n), valid (n,), ion_lev (n,), key (n,)) as ions()"""
        self.sync()
        p = _lib.lib().hps_engine_plasma_species(self._h, self._plasma_index(species))
        n = p.n
        real = np.empty((11, n), dtype=np.float64)
        idc = np.empty(n, dtype=np.uint64)
        lev = np.empty(n, dtype=np.int32)
        if n:
            for k, name in enumerate(PL_REAL):
                check(_lib.lib().hps_memcpy_d2h(real[k].ctypes.data_as(C.c_void_p), C.c_void_p(getattr(p, name)), real[k].nbytes))
            check(_lib.lib().hps_memcpy_d2h(idc.ctypes.data_as(C.c_void_p), C.c_void_p(p.idcpu), idc.nbytes))
            check(_lib.lib().hps_memcpy_d2h(lev.ctypes.data_as(C.c_void_p), C.c_void_p(p.ion_lev), lev.nbytes))
        key = ((idc >> np.uint64(24)) & np.uint64((1 << 39) - 1)).astype(np.int64) - 1
        return real, ((idc >> np.uint64(63)) & np.uint64(1)).astype(np.int32), lev, key

    def set_plasma_symmetry(self, do_symmetrize=False, prevent_centered_particle=False):
        """plasmas.do_symmetrize and prevent_centered_particle, one value for every species (hps_engine_set_plasma_symmetry),
        before the first begin_step; the particle count follows the four mirrored copies."""
        check(_lib.lib().hps_engine_set_plasma_symmetry(self._h, int(bool(do_symmetrize)), int(bool(prevent_centered_particle))))
        npart = C.c_long()
        check(_lib.lib().hps_engine_info(self._h, None, None, C.byref(npart)))
        self.nparticles = npart.value

    def set_laser_grid(self, n_cell=None, patch_lo=None, patch_hi=None, interp_order=1):
        """lasers.n_cell (2), patch_lo, patch_hi (3 each; None: the field grid's) and interp_order: the envelope on a grid of its
        own (hps_engine_set_laser_grid, decks.laser_geometry), before the first begin_step."""
        n = (C.c_int * 2)(*[int(v) for v in n_cell]) if n_cell is not None else None
        lo = (C.c_double * 3)(*[float(v) for v in patch_lo]) if patch_lo is not None else None
        hi = (C.c_double * 3)(*[float(v) for v in patch_hi]) if patch_hi is not None else None
        check(_lib.lib().hps_engine_set_laser_grid(self._h, n, lo, hi, int(1 if interp_order is None else interp_order)))
        # self.deck describes the grid the engine holds: laser_cell_centres and add_laser_profile go by it
        self.deck.update(laser_n_cell=None if n_cell is None else tuple(int(v) for v in n_cell),
                         laser_patch_lo=None if patch_lo is None else tuple(float(v) for v in patch_lo),
                         laser_patch_hi=None if patch_hi is None else tuple(float(v) for v in patch_hi),
                         laser_interp_order=int(1 if interp_order is None else interp_order))

    def laser_grid(self):
        """(nxl, nyl, zeta_lo, zeta_hi) as the engine holds them; without set_laser_grid (nx, ny, 0, nz - 1)"""
        v = [C.c_int() for _ in range(4)]
        check(_lib.lib().hps_engine_laser_grid(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def laser_chi(self):
        """chi on the laser grid as the last envelope advance read it: (nyl, nxl); needs set_laser_grid and an evolving envelope"""
        nxl, nyl, _, _ = self.laser_grid()
        out = np.empty((nyl, nxl), dtype=np.float64)
        check(_lib.lib().hps_engine_laser_chi(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def set_laser_pulses(self, pulses):
        """lasers.names with init_type = gaussian: a list of dicts with the reference's keys a0, w0, L0 | tau, position_mean,
        focal_distance, CEP, propagation_angle_yz, PFT_yz (decks.LASER_PULSE_DEFAULT) replaces the deck's own pulse; an empty
        list leaves only the envelopes of add_laser_profile / add_laser_samples.  At most 8; before the first begin_step.  CEP
        scales the pulse by e^CEP, as in the reference (MultiLaser.cpp:912)."""
        c = _decks.SI["c"] if self.deck.get("si_units", 0) else 1.0
        arr = (_lib.LaserPulse * max(len(pulses), 1))()
        for q, pulse in enumerate(pulses):
            a0, w0, L0, pos, zfoc, cep, angle, pft = _decks.laser_pulse(pulse, c)
            arr[q] = _lib.LaserPulse(a0, w0, L0, (C.c_double * 3)(*pos), zfoc, cep, angle, pft)
        check(_lib.lib().hps_engine_set_laser_pulses(self._h, len(pulses), arr))

    def laser_cell_centres(self):
        """x (nxl), y (nyl), z (nzl) of the laser grid's cells: decks.laser_cell_centres of self.deck, in which set_laser_grid
        records the grid it gave the engine"""
        x, y, z = _decks.laser_cell_centres(self.deck)
        nxl, nyl, zlo, zhi = self.laser_grid()
        if (x.size, y.size, z.size) != (nxl, nyl, zhi - zlo + 1):
            raise RuntimeError(f"the engine's laser grid {(nxl, nyl, zhi - zlo + 1)} is not the deck's {(x.size, y.size, z.size)}")
        return x, y, z

    def add_laser_profile(self, fn):
        """init_type = parser: fn(x, y, z) -> complex over numpy arrays, evaluated on the laser grid's cell centres on the host and
        added to the envelope cell by cell (geometry 0)."""
        x, y, z = self.laser_cell_centres()
        X, Y, Z = np.broadcast_arrays(x[None, None, :], y[None, :, None], z[:, None, None])
        data = np.empty(X.shape, dtype=np.complex128)
        data[...] = fn(X, Y, Z)
        self.add_laser_samples(0, data, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))

    def add_laser_samples(self, geometry, data, offset, spacing, unit=1.0):
        """init_type = from_file: complex samples [extent0][extent1][extent2] in the geometry 0 (the laser grid itself), 1 | "xyt",
        2 | "xyz" or 3 | "rt" ([modes][nt][nr]); offset, spacing per axis in the file's order (two values for rt); unit = unitSI.
        Added to the envelope by the first begin_step, after the pulses, in the order given (hps_engine_add_laser_samples)."""
        geometry = {"grid": 0, "xyt": 1, "xyz": 2, "rt": 3}.get(geometry, geometry)
        if geometry not in (0, 1, 2, 3):
            raise ValueError("laser samples: geometry must be 0, 'xyt', 'xyz' or 'rt'")
        a = np.ascontiguousarray(data, dtype=np.complex128)
        if a.ndim != 3:
            raise ValueError("laser samples: data must have three axes")
        off, sp = [float(v) for v in offset], [float(v) for v in spacing]
        need = 2 if geometry == 3 else 3
        if len(off) < need or len(sp) < need or len(off) > 3 or len(sp) > 3:
            raise ValueError(f"laser samples: offset and spacing need {need} values")
        off, sp = off + [0.0] * (3 - len(off)), sp + [1.0] * (3 - len(sp))
        check(_lib.lib().hps_engine_add_laser_samples(self._h, int(geometry), a.ctypes.data_as(C.c_void_p), (C.c_long * 3)(*a.shape),
                                                      (C.c_double * 3)(*off), (C.c_double * 3)(*sp), float(unit)))

    def add_laser_file(self, path, iteration=0, name="laserEnvelope"):
        """init_type = from_file: a lasy-layout openPMD file (openpmd_writer.read_laser); its wavelength must be the deck's."""
        from . import openpmd_writer
        geometry, data, offset, spacing, unit, lambda0 = openpmd_writer.read_laser(path, iteration, name)
        mine = float(self.deck["laser_lambda0"])
        if not abs(lambda0 - mine) <= 1.0e-12 * abs(mine):
            raise ValueError(f"{path}: the file's wavelength {lambda0!r} is not the deck's laser_lambda0 {mine!r}, which all "
                             "envelopes of an engine share")
        self.add_laser_samples(geometry, data, offset, spacing, unit)

    def set_insitu_laser(self, on=True):
        """lasers.insitu_period: per-slice reductions of MultiLaser::InSituComputeDiags."""
        check(_lib.lib().hps_engine_set_insitu_laser(self._h, int(on)))

    INSITU_LASER_NAMES = ("max(|a|^2)", "[|a|^2]", "[|a|^2*x]", "[|a|^2*x*x]", "[|a|^2*y]", "[|a|^2*y*y]")

    def insitu_laser_rows(self):
        """the raw (8, nzl) rows of hps_engine_insitu_laser"""
        _, _, zlo, zhi = self.laser_grid()
        out = np.empty((8, zhi - zlo + 1), dtype=np.float64)
        check(_lib.lib().hps_engine_insitu_laser(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def insitu_laser(self):
        """-> dict under the reference's names (MultiLaser.cpp:1039-1052), one value per laser slice, "axis(a)" complex; "sum": the
        per-step totals the reference writes as "integrated" (the maximum of max(|a|^2), the sums of the others)."""
        rows = self.insitu_laser_rows()
        out = {name: rows[q].copy() for q, name in enumerate(self.INSITU_LASER_NAMES)}
        out["axis(a)"] = rows[6] + 1j * rows[7]
        out["sum"] = {name: (rows[q].max() if q == 0 else rows[q].sum()) for q, name in enumerate(self.INSITU_LASER_NAMES)}
        return out

    def add_collision(self, species_a=0, species_b=0, coulomb_log=-1.0, seed=0):
        """hipace.collisions: one more Coulomb collision between species 0 (plasma) / 1 (ion) / further ones (indices or names), before the first begin_step
        (hps_engine_add_collision); coulomb_log <= 0 = computed per pair."""
        check(_lib.lib().hps_engine_add_collision(self._h, self._plasma_index(species_a), self._plasma_index(species_b), coulomb_log, seed))

    def add_beam_collision(self, plasma_species=0, coulomb_log=-1.0, seed=0):
        """hipace.collisions with <collision>.species = beam <plasma>: one more collision, between the moving beam and species
        0 (plasma) / 1 (ion), in the same ordered list as add_collision (hps_engine_add_beam_collision).  With a static beam
        (hipace.dt = 0) it is accepted and does nothing: every pair's scattering parameter is 0 there."""
        check(_lib.lib().hps_engine_add_beam_collision(self._h, self._plasma_index(plasma_species), coulomb_log, seed))

    def set_beam_external_fields(self, E=None, B=None, constants=None):
        """beams.external_E(x,y,z,t) / beams.external_B(x,y,z,t): three expressions (strings in the input file's syntax, or
        numbers) each, or None; constants: my_constants.  Compiled by hipace_amd/expr.py and handed to
        hps_engine_set_beam_external_fields before the first begin_step; components that fold to the constant 0 are skipped.
        The moving beam's push adds them at every sub-step's position and the step's time, on top of the deck's ext_E_slope /
        ext_Ez_slope; a static beam (hipace.dt = 0) is not changed by them."""
        progs = [_expr.compile_components(E, "beams.external_E", constants), _expr.compile_components(B, "beams.external_B", constants)]
        keep, arrs = [], []
        for three in progs:
            if three is None:
                arrs.append(None)
                continue
            a = (_lib.Expr * 3)()
            for q, prog in enumerate(three):
                a[q], k = prog.c_struct()
                keep.append(k)
            arrs.append(a)
        check(_lib.lib().hps_engine_set_beam_external_fields(self._h, arrs[0], arrs[1]))
        self.beam_external_fields = progs

    def collision_stats(self):
        a, b = C.c_long(), C.c_long()
        check(_lib.lib().hps_engine_collision_stats(self._h, C.byref(a), C.byref(b)))
        return dict(pairs_collided=a.value, overfull_cells=b.value)

    # ---- ring hand-off of a moving beam (hipace.dt != 0) ------------------------------------------
    @property
    def moving(self):
        return float(self.deck.get("dt", 0.0)) != 0.0 or self.adaptive

    @property
    def adaptive(self):
        """hipace.dt = adaptive: every step's time and dt come from the host (set_time, AdaptiveTimeStep)"""
        return bool(self.deck.get("dt_adaptive", 0))

    def set_time(self, t, dt):
        """physical time and dt of the step the next begin_step starts (hps_engine_set_time)"""
        check(_lib.lib().hps_engine_set_time(self._h, float(t), float(dt)))

    def beam_moments(self, species=None):
        """{sum w, sum w uz/c, sum w (uz/c)^2, min uz/c} of the step last solved, as a float64 array (synchronises).
        species: None -- the one beam's (refused by an engine with several species: their moments are never summed);
        "all" -- every species', [n][4]; k -- species k's."""
        if species is None:
            out = np.zeros(4, dtype=np.float64)
            check(_lib.lib().hps_engine_beam_moments(self._h, out.ctypes.data_as(C.c_void_p)))
            return out
        n = len(self.beam_species_names)
        out = np.zeros((n, 4), dtype=np.float64)
        check(_lib.lib().hps_engine_beam_moments_species(self._h, out.ctypes.data_as(C.c_void_p)))
        return out if isinstance(species, str) and species == "all" else out[self._species_index(species)]

    # ---- several beam species in one engine ---------------------------------------------
    def _species_index(self, species):
        if isinstance(species, str):
            if species not in self.beam_species_names:
                raise ValueError(f"no beam species named {species!r} (have {self.beam_species_names})")
            return self.beam_species_names.index(species)
        k = int(species)
        if not 0 <= k < len(self.beam_species_names):
            raise ValueError(f"no beam species {k} (the engine holds {len(self.beam_species_names)})")
        return k

    def _select_species(self, species):
        check(_lib.lib().hps_engine_select_beam_species(self._h, self._species_index(species or 0)))

    def _add_beam_species(self, spec):
        rec = _lib.fill_struct(_lib.BeamSpecies(), spec["record"])
        k = C.c_int(-1)
        check(_lib.lib().hps_engine_add_beam_species(self._h, C.byref(rec), C.byref(k)))
        name = spec["name"] if spec["name"] is not None else f"beam{k.value}"
        self.beam_species_names.append(name)
        self.beam_species_records.append(dict(spec["record"]))
        setter = dict(fixed_weight=self.set_beam_fixed_weight, fixed_weight_pdf=self.set_beam_fixed_weight_pdf,
                      density_expr=self.set_beam_fixed_ppc, particles=self.set_beam_particles)[spec["source"]]
        args = dict(spec["args"])
        if spec["source"] == "particles":
            args["allow_outside"] = True
        if not hasattr(self, "beam_species_left_out"):
            self.beam_species_left_out = {}
        self.beam_species_left_out[k.value] = setter(species=k.value, **args)
        if spec["source"] == "fixed_weight_pdf" and not (spec["record"]["uz_mean"] or spec["record"]["uz_std"]):
            self.beam_species_records[-1].update(uz_mean=self.beam_uz_moments[0], uz_std=self.beam_uz_moments[1])
        return k.value

    def add_beam_species(self, **spec):
        """One more beam species in this moving-beam engine (hps_engine_add_beam_species + the source's setter with species=):
        name, charge, mass, n_subcycles, do_z_push, radiation_reaction, spin_anom, do_spin_tracking, uz_mean, uz_std (defaults:
        the deck's beam's), do_salame (the species takes part in SALAME during step 0: needs a deck with beam_species_salame)
        and exactly one source -- fixed_weight=dict(...), fixed_weight_pdf=dict(...), density_expr=... (with
        constants, min_density, u_std, random_ppc, seed) or particles=(7, n) array (decks.BEAM_SPECIES_DEFAULT).  Before the
        first begin_step.  -> the species' index; what the source left out of the box: beam_species_left_out[index]."""
        return self._add_beam_species(_decks.beam_species_spec(self.deck, spec, "add_beam_species"))

    def beam_species(self):
        """-> (names, counts) of the engine's beam species, species 0 = the deck's beam"""
        n = C.c_int()
        counts = (C.c_long * _decks.MAX_BEAM_SPECIES)()
        check(_lib.lib().hps_engine_beam_species_info(self._h, C.byref(n), counts))
        return list(self.beam_species_names[:n.value]), [counts[k] for k in range(n.value)]

    def beam_container(self):
        """-> (boundaries int64 [nz+1], soa float64 [7, nbeam], tags uint8 [nbeam]) of the whole container, every species"""
        names, _ = self.beam_species()
        nz = self.deck["nz"]
        if len(names) == 1:
            bnd, soa = self.beam_state()
            return bnd, soa, np.zeros(soa.shape[1], dtype=np.uint8)
        n = C.c_long()
        check(_lib.lib().hps_engine_beam_state_species(self._h, -1, C.byref(n), None, None))
        bnd = np.zeros(nz + 1, dtype=np.int64)
        soa = np.zeros((7, max(n.value, 1)), dtype=np.float64)
        tags = np.zeros(max(n.value, 1), dtype=np.uint8)
        check(_lib.lib().hps_engine_beam_state_species(self._h, -1, C.byref(n), bnd.ctypes.data_as(C.c_void_p),
                                                       soa.ctypes.data_as(C.c_void_p) if n.value else None))
        check(_lib.lib().hps_engine_beam_tags(self._h, tags.ctypes.data_as(C.c_void_p)))
        return bnd, soa[:, :n.value], tags[:n.value]

    def beam_kernels(self):
        """-> (set of the beam kernel instances launched so far, e.g. "k_beam_push<2,0,0>" = ORDER, EXT, MULTI; does the
        container hold a species tag row)"""
        n, tagged = C.c_long(), C.c_int()
        check(_lib.lib().hps_engine_beam_kernels(self._h, None, 0, C.byref(n), C.byref(tagged)))
        buf = C.create_string_buffer(n.value + 1)
        check(_lib.lib().hps_engine_beam_kernels(self._h, buf, n.value + 1, C.byref(n), C.byref(tagged)))
        return set(buf.value.decode().split()), bool(tagged.value)

    def run_adaptive(self, n_steps=None, controller=None, on_step_end=None):
        """hipace.dt = adaptive on this one engine (Hipace::Evolve with one rank, Hipace.cpp:400-490): the head rank's
        initial dt, then per step CalculateFromDensity + max_time, the step at (t, dt), CalculateFromMinUz on its moments.
        Runs n_steps (default: the deck's) or stops where hipace.max_time drops the rest; on_step_end(step, t, dt) after each.
        Returns [(step, t, dt)] of the steps started -- the reference's "started step ... at time = ... with dt = ..." lines."""
        assert self.adaptive, "run_adaptive needs a deck with dt_adaptive"
        n = self.deck["n_steps"] if n_steps is None else int(n_steps)
        ats = controller or AdaptiveTimeStep.for_engine(self)
        ats.initial_dt(nstages=1)
        t, log = 0.0, []
        for step in range(n):
            if t == float("inf"):
                break
            dt = ats.CalculateFromDensity(t)
            log.append((step, t, dt))
            self.set_time(t, dt)
            self.run_step()
            ats.CalculateFromMinUz(self.beam_moments("all" if ats.beams is not None else None), t, 1)
            if on_step_end is not None:
                on_step_end(step, t, dt)
            t = ats.next_time()
        return log

    def beam_capacity(self):
        n = C.c_long()
        check(_lib.lib().hps_engine_beam_capacity(self._h, C.byref(n)))
        return n.value

    def set_beam_capacity(self, cap):
        """particles a slice's hand-off message has room for (default: twice the fullest injected slice); before the first step"""
        check(_lib.lib().hps_engine_set_beam_capacity(self._h, int(cap)))

    def beam_message_doubles(self):
        """Length of a hand-off message of the moving beam: 1 + rows*capacity (7 rows, 10 with spin tracking)."""
        r = C.c_int()
        check(_lib.lib().hps_engine_beam_message_rows(self._h, C.byref(r)))
        return 1 + r.value * self.beam_capacity()

    def beam_spin(self):
        """<beam>.do_spin_tracking: (3, nbeam) array sx sy sz in the particle order of beam_state()."""
        nbeam, _ = self.beam_layout()
        out = np.zeros((3, max(nbeam, 1)), dtype=np.float64)
        check(_lib.lib().hps_engine_beam_spin(self._h, out.ctypes.data_as(C.c_void_p) if nbeam else None))
        return out[:, :nbeam]

    def set_beam_import(self, on):
        check(_lib.lib().hps_engine_set_beam_import(self._h, int(on)))

    def export_beam_slice(self, islice, msg):
        """msg: float64 device tensor of 1 + 7*beam_capacity(); filled asynchronously on the engine's stream."""
        check(_lib.lib().hps_engine_export_beam_slice(self._h, islice, C.c_void_p(msg.data_ptr())))

    def import_beam_slice(self, islice, msg):
        check(_lib.lib().hps_engine_import_beam_slice(self._h, islice, C.c_void_p(msg.data_ptr())))

    def beam_state(self, species=None):
        """(boundaries int64 [nz+1], soa float64 [7, nbeam]) of the beam as it is now; slice p from the head is
        soa[:, boundaries[p]:boundaries[p+1]] (rows x y z ux uy uz w).  A static beam (hipace.dt = 0) comes in the same
        layout, with the weights SALAME has left.  species=k (index or name): that species' particles alone, in container
        order (an engine with several species refuses species=None)."""
        nz = self.deck["nz"]
        if species is not None:
            k = self._species_index(species)
            n = C.c_long()
            check(_lib.lib().hps_engine_beam_state_species(self._h, k, C.byref(n), None, None))
            bnd = np.zeros(nz + 1, dtype=np.int64)
            soa = np.zeros((7, max(n.value, 1)), dtype=np.float64)
            check(_lib.lib().hps_engine_beam_state_species(self._h, k, C.byref(n), bnd.ctypes.data_as(C.c_void_p),
                                                           soa.ctypes.data_as(C.c_void_p) if n.value else None))
            return bnd, soa[:, :n.value]
        nbeam, _ = self.beam_layout()
        bnd = np.zeros(nz + 1, dtype=np.int64)
        soa = np.zeros((7, max(nbeam, 1)), dtype=np.float64)
        check(_lib.lib().hps_engine_beam_state(self._h, bnd.ctypes.data_as(C.c_void_p), soa.ctypes.data_as(C.c_void_p) if nbeam else None))
        return bnd, soa[:, :nbeam].reshape(7, nbeam) if nbeam else soa[:, :0]

    def set_density_profile(self, r=(), fr=(), ct=(), ft=()):
        """n(x, y, ct) = density * f_r(r) * f_t(c t): piecewise-linear tables (hps_engine_set_density_profile)."""
        self.density_profile = (r, fr, ct, ft)
        a = [np.ascontiguousarray(v, dtype=np.float64) for v in (r, fr, ct, ft)]
        assert len(a[0]) == len(a[1]) and len(a[2]) == len(a[3])
        p = [x.ctypes.data_as(C.c_void_p) if len(x) else None for x in a]
        check(_lib.lib().hps_engine_set_density_profile(self._h, len(a[0]), p[0], p[1], len(a[2]), p[2], p[3]))

    def set_density_expr(self, species, text_or_table, constants=None, min_density=0.0):
        """<plasma>.density(x,y,z) of species 0 / "plasma", 1 / "ion" or a further species (index or name) as a parsed function: a string in the input file's
        syntax (or a number), or the density table as a list of (position, string) pairs in ascending order of position
        (decks.read_density_table reads density_table_file); constants: my_constants; min_density: <plasma>.min_density.
        Compiled by hipace_amd/expr.py over (x, y, z) and handed to hps_engine_set_density_expr before the first begin_step.
        The value is the density itself: for this species it replaces <species>_density f_r f_t of set_density_profile."""
        try:
            sp = self._plasma_index(species)
        except (ValueError, TypeError):
            raise ValueError(f"set_density_expr: species must be 0, 1, 'plasma', 'ion' or a further species' index or name, got {species!r}")
        progs, pos = _expr.compile_density(text_or_table, constants)
        arr, keep = _expr.c_programs(progs)
        z = (C.c_double * len(pos))(*pos) if pos is not None else None
        check(_lib.lib().hps_engine_set_density_expr(self._h, sp, len(progs), arr, z, float(min_density)))
        if not hasattr(self, "density_exprs"):
            self.density_exprs = {}
        self.density_exprs[sp] = (progs, pos, float(min_density))

    def set_fusion(self, on=True):
        """Push of slice k and deposition of slice k-1 in one pass over the sheet (include/hpslice.h: hps_engine_set_fusion)."""
        check(_lib.lib().hps_engine_set_fusion(self._h, int(on)))

    def fallbacks(self):
        n = C.c_long()
        check(_lib.lib().hps_engine_fallbacks(self._h, C.byref(n)))
        return n.value

    def sorts(self):
        n = C.c_long()
        check(_lib.lib().hps_engine_sorts(self._h, C.byref(n)))
        return n.value

    def set_diagnostics(self, on=True):
        check(_lib.lib().hps_engine_set_diagnostics(self._h, int(on)))

    def set_profiling(self, on=True, stride=1, light=False):
        """HIP-event phase timers; stride > 1 times every stride-th slice only (an event record costs ~3.4 us);
        light: only the deposition kernel and the kernel-free interval (4 records per slice instead of 11)."""
        check(_lib.lib().hps_engine_set_profiling_stride(self._h, int(stride)))
        check(_lib.lib().hps_engine_set_profiling(self._h, (2 if light else 1) if on else 0))

    def beam_layout(self):
        """-> (nbeam, offsets[nz+1]): block p (p-th slice from the head) holds particles offsets[p]:offsets[p+1]."""
        nb = C.c_long()
        off = (C.c_long * (self.deck["nz"] + 1))()
        check(_lib.lib().hps_engine_beam_info(self._h, C.byref(nb), off))
        return nb.value, np.array(off[:], dtype=np.int64)

    def set_beam_particles(self, soa, allow_outside=False, species=None):
        """A host-initialised beam in place of the deck's (any of the reference's injection types): soa = (7, n) array
        x y z ux uy uz w.  Before the first begin_step.  -> number of particles outside the box in z (left out).
        species=k: the particles fill beam species k (add_beam_species) instead of replacing the beam."""
        soa = np.ascontiguousarray(soa, dtype=np.float64)
        assert soa.ndim == 2 and soa.shape[0] == 7
        self._select_species(species)
        out = C.c_long(0)
        check(_lib.lib().hps_engine_set_beam_particles(self._h, soa.shape[1], soa.ctypes.data_as(C.c_void_p),
                                                       C.byref(out) if allow_outside else None))
        return out.value

    def set_beam_fixed_ppc(self, expr, constants=None, min_density=0.0, u_std=None, random_ppc=None, seed=1, species=None):
        """The general fixed_ppc beam in place of the deck's, generated on the device (hps_engine_set_beam_fixed_ppc):
        <beam>.density(x,y,z) as a string in the input file's syntax (or a number, or a Program over x, y, z), constants:
        my_constants, <beam>.min_density, u_std (3, units of c), random_ppc (3 flags) and the seed of the draws.  The deck gives
        beam_ppc, the window beam_zmin / beam_zmax / beam_radius around beam_pos_mean, beam_umean, charge and mass.  Before the
        first begin_step; whichever of this and set_beam_particles is called last holds."""
        if isinstance(expr, _expr.Program):
            prog = expr
            if len(prog.variables) > 3 and any(o == "var" and a >= 3 for o, a in prog.ins):
                raise ValueError("set_beam_fixed_ppc: the beam's density is a function of x, y, z and cannot read t")
            if len(prog.variables) != 3:
                prog = _expr.Program(prog.ins, prog.consts, ("x", "y", "z"), prog.text)
        else:
            try:
                prog = _expr.compile_expr(expr, ("x", "y", "z"), constants)
            except ValueError as e:
                if "unknown name: 't'" in str(e):
                    raise ValueError(f"set_beam_fixed_ppc: the beam's density is a function of x, y, z and cannot read t ({e})") from None
                raise
        c, keep = prog.c_struct()
        us = (C.c_double * 3)(*[float(v) for v in u_std]) if u_std is not None else None
        rp = (C.c_int * 3)(*[int(bool(v)) for v in random_ppc]) if random_ppc is not None else None
        self._select_species(species)      # (species=k: fills beam species k, add_beam_species)
        check(_lib.lib().hps_engine_set_beam_fixed_ppc(self._h, C.byref(c), float(min_density), us, rp, int(seed)))

    def set_beam_fixed_weight(self, num_particles, position_mean, position_std, u_mean=(0.0, 0.0, 0.0), u_std=(0.0, 0.0, 0.0),
                              density=None, total_charge=None, profile="gaussian", zmin=-np.inf, zmax=np.inf, radius=np.inf,
                              do_symmetrize=False, z_foc=0.0, duz_per_uz0_dzeta=0.0, seed=1, constants=None, species=None):
        """The fixed_weight beam (injection_type = fixed_weight, profile "gaussian" or "can") in place of the deck's, generated on
        the device (hps_engine_set_beam_fixed_weight): num_particles draws -- a quarter of them with do_symmetrize --
        with z normal about position_mean[2] with position_std[2] (gaussian) or uniform in [zmin, zmax] (can), x and y normal
        about position_mean[0](z), position_mean[1](z): numbers, strings in the input file's syntax over z (constants:
        my_constants) or Programs over ("z",).  Exactly one of density (the peak density) and total_charge (SI units only).
        u_mean, u_std in units of c.  The deck gives the grid, the units, beam_charge and beam_mass.  Before the first
        begin_step; whichever beam setter is called last holds.
        -> (particles of invalid draws, particles of valid draws outside the box in z): both left out."""
        if (density is None) == (total_charge is None):
            raise ValueError("set_beam_fixed_weight: specify exclusively either total_charge or density of the beam")
        prof = {"gaussian": 0, "can": 1}.get(profile)
        if prof is None:
            raise ValueError(f"set_beam_fixed_weight: only gaussian and can are supported with fixed_weight beam injection, got {profile!r}")
        if len(position_mean) != 3 or len(position_std) != 3 or len(u_mean) != 3 or len(u_std) != 3:
            raise ValueError("set_beam_fixed_weight: position_mean, position_std, u_mean and u_std have three entries each")
        progs = []
        for q in range(2):
            m = position_mean[q]
            if isinstance(m, _expr.Program):
                if tuple(m.variables) != ("z",):
                    raise ValueError(f"set_beam_fixed_weight: position_mean[{q}] is a function of z alone")
                progs.append(m)
                continue
            try:
                progs.append(_expr.compile_expr(m, ("z",), constants))
            except ValueError as e:
                raise ValueError(f"set_beam_fixed_weight: position_mean[{q}] is a function of z alone ({e})") from None
        spec = _lib.BeamFixedWeight(
            num_particles=int(num_particles), profile=prof, do_symmetrize=int(bool(do_symmetrize)), pos_mean_z=float(position_mean[2]),
            pos_std=(C.c_double * 3)(*[float(v) for v in position_std]), u_mean=(C.c_double * 3)(*[float(v) for v in u_mean]),
            u_std=(C.c_double * 3)(*[float(v) for v in u_std]), zmin=float(zmin), zmax=float(zmax), radius=float(radius),
            z_foc=float(z_foc), duz_per_uz0_dzeta=float(duz_per_uz0_dzeta), density=0.0 if density is None else float(density),
            total_charge=0.0 if total_charge is None else float(total_charge), charge_is_specified=int(total_charge is not None))
        (cx, keep_x), (cy, keep_y) = progs[0].c_struct(), progs[1].c_struct()
        out = (C.c_long * 2)(0, 0)
        self._select_species(species)      # (species=k: fills beam species k, add_beam_species)
        check(_lib.lib().hps_engine_set_beam_fixed_weight(self._h, C.byref(spec), C.byref(cx), C.byref(cy), int(seed), out))
        self.beam_mean_programs = (progs[0], progs[1])
        return out[0], out[1]

    def set_beam_fixed_weight_pdf(self, num_particles, pdf, position_mean, position_std, u_mean=(0.0, 0.0, 0.0), u_std=(0.0, 0.0, 0.0),
                                  density=None, total_charge=None, radius=np.inf, z_foc=0.0, do_symmetrize=False, pdf_ref_ratio=4,
                                  seed=1, constants=None, species=None):
        """The fixed_weight_pdf beam (injection_type = fixed_weight_pdf) in place of the deck's, generated on the device
        (hps_engine_set_beam_fixed_weight_pdf): num_particles particles of one weight -- a quarter as many draws with
        do_symmetrize -- with the longitudinal profile pdf(z), tabulated on nz pdf_ref_ratio sub-slices, x and y normal about
        position_mean[0 | 1](z) with position_std[0 | 1](z), u normal about u_mean[d](z) with u_std[d](z), in units of c.  pdf and
        the ten functions: numbers, strings in the input file's syntax over z (constants: my_constants) or Programs over ("z",).
        Exactly one of density (the peak density) and total_charge (SI units only): numbers, or strings over the constants.
        The deck gives the grid, the units, beam_charge and beam_mass.  Before the first begin_step; whichever beam setter is
        called last holds.  beam_uz_moments keeps the pdf-weighted (mean, standard deviation) of u_z: the arguments of
        adaptive_initial_dt.
        -> (particles of invalid draws, particles of valid draws outside the box in z): both left out."""
        name = "set_beam_fixed_weight_pdf"
        if (density is None) == (total_charge is None):
            raise ValueError(f"{name}: specify exclusively either total_charge or density of the beam")
        if len(position_mean) != 2 or len(position_std) != 2 or len(u_mean) != 3 or len(u_std) != 3:
            raise ValueError(f"{name}: position_mean and position_std have two entries each, u_mean and u_std three")

        def function(what, f):
            if isinstance(f, _expr.Program):
                if tuple(f.variables) != ("z",):
                    raise ValueError(f"{name}: {what} is a function of z alone")
                return f
            try:
                return _expr.compile_expr(f, ("z",), constants)
            except ValueError as e:
                raise ValueError(f"{name}: {what} is a function of z alone ({e})") from None

        def number(what, v):
            if not isinstance(v, str):
                return float(v)
            try:
                p = _expr.compile_expr(v, (), constants)
            except ValueError as e:
                raise ValueError(f"{name}: {what} is a number ({e})") from None
            return float(p.evaluate())

        prog_pdf = function("pdf", pdf)
        progs = [function(f"{k}[{q}]", v) for k, vals in (("position_mean", position_mean), ("position_std", position_std),
                                                          ("u_mean", u_mean), ("u_std", u_std)) for q, v in enumerate(vals)]
        spec = _lib.BeamFixedWeightPdf(
            num_particles=int(num_particles), do_symmetrize=int(bool(do_symmetrize)), pdf_ref_ratio=int(pdf_ref_ratio),
            radius=number("radius", radius), z_foc=number("z_foc", z_foc), density=0.0 if density is None else number("density", density),
            total_charge=0.0 if total_charge is None else number("total_charge", total_charge),
            charge_is_specified=int(total_charge is not None))
        cpdf, keep_pdf = prog_pdf.c_struct()
        arr, keep = _expr.c_programs(progs)
        out, mom = (C.c_long * 2)(0, 0), (C.c_double * 2)(0.0, 0.0)
        self._select_species(species)      # (species=k: fills beam species k, add_beam_species)
        check(_lib.lib().hps_engine_set_beam_fixed_weight_pdf(self._h, C.byref(spec), C.byref(cpdf), arr, int(seed), out, mom))
        self.beam_pdf_programs = (prog_pdf, tuple(progs))
        self.beam_uz_moments = (mom[0], mom[1])
        return out[0], out[1]

    def set_beam_storage(self, tensor, injected_beam_support=False):
        """Use `tensor` (float64, 7*nbeam, on this device) as the engine's beam blocks; None = own.
        injected_beam_support: the blocks are the injected beam handed along the ring (dt = 0), so the slab
        kernels may keep skipping the beam planes outside its transverse support."""
        check(_lib.lib().hps_engine_set_beam_storage(self._h, C.c_void_p(tensor.data_ptr()) if tensor is not None else None))
        if tensor is not None and injected_beam_support:
            check(_lib.lib().hps_engine_assume_initial_beam_support(self._h))

    def initial_beam_into(self, tensor):
        check(_lib.lib().hps_engine_initial_beam(self._h, C.c_void_p(tensor.data_ptr())))

    # ---- field diagnostics (Fields::Copy) -----------------------------------------------------------------
    def set_field_diagnostic(self, names, coarsening=(1, 1, 1), diag_type="xyz", patch_lo=None, patch_hi=None):
        """diagnostic.field_data = names, diagnostic.coarsening = cx cy cz, diagnostic.diag_type = xyz | xz | yz | xy,
        diagnostic.patch_lo / patch_hi (hps_engine_set_field_diagnostic_box)."""
        idx = _lib.CIDX_PC if self.deck.get("bxby_solver", 0) else _lib.CIDX
        cn = self.comp_names()
        comps = (C.c_int * len(names))(*[idx[n] if n in idx else cn.index(n) for n in names])
        co = (C.c_int * 3)(*coarsening)
        sd = {"xyz": -1, "yz": 0, "xz": 1, "xy": 2}[diag_type]
        plo = (C.c_double * 3)(*patch_lo) if patch_lo is not None else None
        phi = (C.c_double * 3)(*patch_hi) if patch_hi is not None else None
        check(_lib.lib().hps_engine_set_field_diagnostic_box(self._h, len(names), comps, co, sd, plo, phi))
        self._fd = (list(names), tuple(coarsening))

    def field_diagnostic_geometry(self):
        """-> (cells (nx, ny, nz), lo, hi) of the diagnostic grid"""
        n, lo, hi = (C.c_int * 3)(), (C.c_double * 3)(), (C.c_double * 3)()
        check(_lib.lib().hps_engine_field_diagnostic_geometry(self._h, n, lo, hi))
        return tuple(n), tuple(lo), tuple(hi)

    def field_diagnostic(self):
        """-> dict name -> array [nz, ny, nx] of the diagnostic grid, of the step that is being (or has just been) solved."""
        names, _ = self._fd
        n, _, _ = self.field_diagnostic_geometry()
        out = np.empty((len(names), n[2], n[1], n[0]))
        check(_lib.lib().hps_engine_field_diagnostic(self._h, out.ctypes.data_as(C.c_void_p)))
        return {k: out[i] for i, k in enumerate(names)}

    INSITU_FIELDS = ["[Ex^2]", "[Ey^2]", "[Ez^2]", "[Bx^2]", "[By^2]", "[Bz^2]", "[ExmBy^2]", "[EypBx^2]", "[jz_beam]",
                     "[Ez*jz_beam]"]

    INSITU_PLASMA = ["sum(w)", "[x]", "[x^2]", "[y]", "[y^2]", "[ux]", "[ux^2]", "[uy]", "[uy^2]", "[uz]", "[uz^2]", "[ga]",
                     "[ga^2]", "[(ga-1)*(1-vz)]", "Np"]

    INSITU_BEAM = ["sum(w)", "[x]", "[x^2]", "[y]", "[y^2]", "[z]", "[z^2]", "[ux]", "[ux^2]", "[uy]", "[uy^2]", "[uz]", "[uz^2]",
                   "[x*ux]", "[y*uy]", "[z*uz]", "[x*uy]", "[y*ux]", "[ux/uz]", "[uy/uz]", "[ga]", "[ga^2]", "Np"]

    def laser_vcycles(self):
        n = C.c_long()
        check(_lib.lib().hps_engine_laser_vcycles(self._h, C.byref(n)))
        return n.value

    def set_insitu_beam(self, radius=float("inf")):
        """<beam>.insitu_period / insitu_radius: per-slice moments of BeamParticleContainer::InSituComputeDiags."""
        check(_lib.lib().hps_engine_set_insitu_beam(self._h, min(float(radius), 1.0e300)))

    def insitu_beam(self, species=None):
        """-> dict name -> array[nz] (index = islice), names as the reference's in-situ file (BeamParticleContainer.cpp:625-650).
        species=k (index or name): that beam species' moments (an engine with several species refuses species=None)."""
        out = np.empty((23, self.deck["nz"]))
        if species is None:
            check(_lib.lib().hps_engine_insitu_beam(self._h, out.ctypes.data_as(C.c_void_p)))
        else:
            check(_lib.lib().hps_engine_insitu_beam_species(self._h, self._species_index(species), out.ctypes.data_as(C.c_void_p)))
        return {n: out[i] for i, n in enumerate(self.INSITU_BEAM)}

    def set_insitu_plasma(self, radius=float("inf")):
        """plasma.insitu_period / insitu_radius: per-slice moments of PlasmaParticleContainer::InSituComputeDiags."""
        check(_lib.lib().hps_engine_set_insitu_plasma(self._h, min(float(radius), 1.0e300)))

    def insitu_plasma(self, species=0):
        """species: 0 / "plasma", or a further species' index or name (hps_engine_insitu_plasma_species)"""
        out = np.empty((15, self.deck["nz"]))
        check(_lib.lib().hps_engine_insitu_plasma_species(self._h, self._plasma_index(species), out.ctypes.data_as(C.c_void_p)))
        return {n: out[i] for i, n in enumerate(self.INSITU_PLASMA)}

    def set_insitu_fields(self, on=True):
        """fields.insitu_period: per-slice reductions of Fields::InSituComputeDiags."""
        check(_lib.lib().hps_engine_set_insitu_fields(self._h, int(on)))

    def insitu_fields(self):
        """-> dict name -> array[nz] (index = islice) with the reference's names (Fields.cpp:1380-1389)."""
        out = np.empty((10, self.deck["nz"]))
        check(_lib.lib().hps_engine_insitu_fields(self._h, out.ctypes.data_as(C.c_void_p)))
        return {n: out[i] for i, n in enumerate(self.INSITU_FIELDS)}

    # ---- several steps in flight on one device (pipeline.run_local_pipeline) ----------------------------
    def stream_handle(self):
        """the engine's hipStream_t as an integer (torch.cuda.ExternalStream(handle) for timing events)"""
        return _lib.lib().hps_engine_stream(self._h)

    def record_event(self, slot):
        """Mark this engine's stream; returns the event another engine can wait for."""
        ev = C.c_void_p()
        check(_lib.lib().hps_engine_record_event(self._h, int(slot), C.byref(ev)))
        return ev.value

    def wait_event(self, event):
        """This engine's stream waits (on the device) for an event recorded by another engine."""
        if event is not None:
            check(_lib.lib().hps_engine_wait_event(self._h, C.c_void_p(event)))

    def copy_async(self, dst, src):
        """dst.copy_(src) for two float64 device tensors, on this engine's stream."""
        assert dst.numel() == src.numel()
        check(_lib.lib().hps_engine_copy_async(self._h, C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()),
                                               dst.numel() * 8))

    def phase_times(self):
        ms = (C.c_double * 8)()
        n = C.c_long()
        check(_lib.lib().hps_engine_phase_times(self._h, ms, C.byref(n)))
        names = ["deposit_current", "poisson", "explicit_deposit", "mg_solve1", "advance_plasma", "other", "sort", "empty_interval"]
        return {k: ms[i] for i, k in enumerate(names)}, n.value

    def checksums(self):
        out = (C.c_double * self.ncomp)()
        check(_lib.lib().hps_engine_checksums(self._h, out))
        names = self.comp_names()
        cs = {names[i]: out[i] for i in range(self.ncomp)}
        if "aabs" in cs:
            tot = C.c_double()
            check(_lib.lib().hps_engine_laser_info(self._h, None, C.byref(tot)))
            cs["laserEnvelope"] = tot.value
        return cs

    # ---- ring hand-off of the laser envelope ---------------------------------------------------------------
    @property
    def has_laser(self):
        return bool(self.deck.get("laser_on", 0))

    def laser_message_doubles(self):
        nxl, nyl, _, _ = self.laser_grid()
        return 4 * nxl * nyl

    def set_step(self, step):
        """physical time step of the next begin_step (pipeline stages run steps r, r + N, ...)"""
        check(_lib.lib().hps_engine_set_step(self._h, int(step)))

    def set_laser_import(self, on, step=0):
        check(_lib.lib().hps_engine_set_laser_import(self._h, int(on), int(step)))

    def export_laser_slice(self, islice, msg):
        check(_lib.lib().hps_engine_export_laser_slice(self._h, islice, C.c_void_p(msg.data_ptr())))

    def import_laser_slice(self, islice, msg):
        check(_lib.lib().hps_engine_import_laser_slice(self._h, islice, C.c_void_p(msg.data_ptr())))

    def import_laser_from(self, islice, src):
        check(_lib.lib().hps_engine_import_laser_from(self._h, islice, src._h))

    def laser_envelope(self):
        """a_n of the step that has begun: complex array [nz, ny, nx]; with a laser grid [zeta_hi - zeta_lo + 1, nyl, nxl]."""
        nxl, nyl, zlo, zhi = self.laser_grid()
        out = np.empty((zhi - zlo + 1, nyl, nxl), dtype=np.complex128)
        check(_lib.lib().hps_engine_laser_envelope(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def comp_names(self):
        """Names of the slab components of this engine (rho and aabs are optional and come last; behind them the twelve
        planes of the SALAME slice, "Salame_<name>", in a beam_do_salame or beam_species_salame deck -- slab() holds them,
        checksums() does not)."""
        if self.deck.get("bxby_solver", 0):
            return list(_lib.COMPS_PC[:22]) + (["rho"] if self.deck.get("deposit_rho", 0) else [])
        return list(COMPS[:21]) + (["rho"] if self.deck.get("deposit_rho", 0) else []) + \
            (["aabs"] if self.deck.get("laser_on", 0) else []) + \
            (["Salame_" + n for n in _lib.COMPS_SALAME] if self.deck.get("beam_do_salame", 0) or self.deck.get("beam_species_salame", 0) else [])

    def salame_stats(self):
        """<beam>.do_salame: dict of arrays [nz] (index = islice) -- "W" the last weight factor, "W_total" = W * sum(jz) of
        that iteration (SalameGetW), "iterations", "converged", "overloaded" -- of the slices SALAME ran on in step 0; zeros
        elsewhere ("ran" says where)."""
        nz = self.deck["nz"]
        out = np.zeros((nz, 4), dtype=np.float64)
        check(_lib.lib().hps_engine_salame_stats(self._h, out.ctypes.data_as(C.c_void_p)))
        flags = out[:, 3].astype(np.int64)
        return {"W": out[:, 0].copy(), "W_total": out[:, 1].copy(), "iterations": out[:, 2].astype(np.int64),
                "converged": (flags & 1) != 0, "overloaded": (flags & 2) != 0, "ran": out[:, 2] > 0}

    def deposit_beam_species(self, islice, species, jx=None, jy=None, jz=None):
        """hps_engine_deposit_beam_species: the moving beam's deposit of slice islice restricted to `species` (indices or names),
        added to the slab components named jx, jy (both or neither) and jz (comp_names(); None: none).  Enqueued on the engine's
        stream, behind begin_step."""
        names = self.comp_names()
        comp = [names.index(c) if c is not None else -1 for c in (jx, jy, jz)]
        mask = 0
        for s in species:
            mask |= 1 << self._species_index(s)
        check(_lib.lib().hps_engine_deposit_beam_species(self._h, int(islice), mask, *comp))

    def salame_scale_slice(self, islice, W):
        """hps_engine_salame_scale_slice: SalameMultiplyBeamWeight on slice islice of the moving beam's container (the do_salame
        species' particles that have not slipped in; W = 0 removes them).  Enqueued on the engine's stream, behind begin_step."""
        check(_lib.lib().hps_engine_salame_scale_slice(self._h, int(islice), float(W)))

    def pc_stats(self):
        """(predictor-corrector iterations so far, sum over slices of the final relative B-field error)."""
        its, err = C.c_long(), C.c_double()
        check(_lib.lib().hps_engine_pc_stats(self._h, C.byref(its), C.byref(err)))
        return its.value, err.value

    def pc_zero_b_slices(self):
        """slices on which the predictor-corrector loop left after one pass because sum |B| of its guess was 0 (the serial
        path's exact zeros ahead of the beam, which the engine reproduces: INTEGRATION.md)"""
        n = C.c_long()
        check(_lib.lib().hps_engine_pc_zero_b_slices(self._h, C.byref(n)))
        return n.value

    def stats(self):
        vc, sl = C.c_long(), C.c_long()
        check(_lib.lib().hps_engine_stats(self._h, C.byref(vc), C.byref(sl)))
        ei = C.c_long()      # slices whose shift / zero pass rode in the Bx/By solve's lower V (HPS_EARLY_INIT)
        check(_lib.lib().hps_engine_early_init_slices(self._h, C.byref(ei)))
        return dict(vcycles=vc.value, slices=sl.value, early_init=ei.value)

    def schedule(self):
        """What the schedule switches read at creation chose: {"mg_coef_guest" (MultiGrid.info(schedule=True)["coef_guest"] of
        the Bx/By solver), "valid_by_psi" (the electrons' tiled push reads validity off psi_half, HPS_VALID_BY_PSI)}."""
        g, v = C.c_int(), C.c_int()
        check(_lib.lib().hps_engine_schedule(self._h, C.byref(g), C.byref(v)))
        return dict(mg_coef_guest=bool(g.value), valid_by_psi=bool(v.value))

    def qsa_drops(self):
        """particles dropped by the depositions so far for violating the quasi-static approximation (max_qsa)"""
        n = C.c_long()
        check(_lib.lib().hps_engine_qsa_drops(self._h, C.byref(n)))
        return n.value

    def slab(self):
        self.sync()
        s = _lib.lib().hps_engine_slab(self._h)
        nx, ny, g = s.nx, s.ny, s.ng
        out = np.empty((s.ncomp, ny + 2 * g, nx + 2 * g), dtype=np.float64)
        check(_lib.lib().hps_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(s.p), out.nbytes))
        return out

    def ions(self):
        """Species "ion" (deck ion_on): (real (11, n), valid (n,), ion_lev (n,), key (n,)) -- key = the ion's lattice index,
        which the tile sort moves with the particle (the id bits of idcpu)."""
        self.sync()
        p = _lib.lib().hps_engine_ions(self._h)
        n = p.n
        real = np.empty((11, n), dtype=np.float64)
        idc = np.empty(n, dtype=np.uint64)
        lev = np.empty(n, dtype=np.int32)
        if n:
            for k, name in enumerate(PL_REAL):
                check(_lib.lib().hps_memcpy_d2h(real[k].ctypes.data_as(C.c_void_p), C.c_void_p(getattr(p, name)), real[k].nbytes))
            check(_lib.lib().hps_memcpy_d2h(idc.ctypes.data_as(C.c_void_p), C.c_void_p(p.idcpu), idc.nbytes))
            check(_lib.lib().hps_memcpy_d2h(lev.ctypes.data_as(C.c_void_p), C.c_void_p(p.ion_lev), lev.nbytes))
        key = ((idc >> np.uint64(24)) & np.uint64((1 << 39) - 1)).astype(np.int64) - 1
        return real, ((idc >> np.uint64(63)) & np.uint64(1)).astype(np.int32), lev, key

    def ion_stats(self):
        """(electrons released by the species "ion" since the engine was created, particles of the first species now)."""
        a, b = C.c_long(), C.c_long()
        check(_lib.lib().hps_engine_ion_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def particles(self):
        self.sync()
        p = _lib.lib().hps_engine_plasma(self._h)
        n = p.n
        real = np.empty((11, n), dtype=np.float64)
        idc = np.empty(n, dtype=np.uint64)
        if n:
            for k, name in enumerate(PL_REAL):       # x_prev / y_prev may alias x / y inside the engine
                check(_lib.lib().hps_memcpy_d2h(real[k].ctypes.data_as(C.c_void_p), C.c_void_p(getattr(p, name)), real[k].nbytes))
            check(_lib.lib().hps_memcpy_d2h(idc.ctypes.data_as(C.c_void_p), C.c_void_p(p.idcpu), idc.nbytes))
        return real, ((idc >> np.uint64(63)) & np.uint64(1)).astype(np.int32)
