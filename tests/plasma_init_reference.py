"""numpy restatement of PlasmaParticleContainer::InitParticles (particles/plasma/PlasmaParticleContainerInit.cpp:36-313) and
ParticleUtil::get_position_unit_cell_fine (particles/particles_utils/ParticleUtil.H:66-104) for what hipace_amd supports:
the fine patch with its transition (level map on the cell box cropped to the plasma radius), the weights, and the radius,
hollow_core_radius and density tests.  Not restated: prevent_centered_particle (offsets 0), do_symmetrize, the momentum draws
(u_mean = u_std = 0: ux = uy = 0, psi = 1).  No fused multiply-adds, every operation rounds once, as the reference's CPU build."""
import numpy as np


def round_half_away(v):
    """std::round"""
    return int(np.sign(v) * np.floor(abs(v) + 0.5))


def cell_box(nx, ny, lo, dx, dy, radius):
    """the tile box of lines 68-82: the whole domain, cropped to the plasma radius if that is finite.  (ilo, ihi, jlo, jhi),
    inclusive; empty if ihi < ilo or jhi < jlo"""
    ilo, ihi, jlo, jhi = 0, nx - 1, 0, ny - 1
    if radius != np.inf:
        ilo = max(ilo, round_half_away((-radius - lo[0]) / dx - 2))
        jlo = max(jlo, round_half_away((-radius - lo[1]) / dy - 2))
        ihi = min(ihi, round_half_away((radius - lo[0]) / dx + 2))
        jhi = min(jhi, round_half_away((radius - lo[1]) / dy + 2))
    return ilo, ihi, jlo, jhi


def level_map(mask, T, box):
    """lines 104-138 on the cells of `box`: T + 1 where the mask is set, then T passes of max(own, neighbour - 1) over the
    4-neighbourhood that do not look past the box.  Returns the map of the box, (jhi - jlo + 1, ihi - ilo + 1)."""
    ilo, ihi, jlo, jhi = box
    a = np.where(np.asarray(mask)[jlo:jhi + 1, ilo:ihi + 1] != 0, T + 1, 0).astype(np.int64)
    for _ in range(T):
        b = a
        a = b.copy()
        a[:, 1:] = np.maximum(a[:, 1:], b[:, :-1] - 1)      # i > lo.x
        a[:, :-1] = np.maximum(a[:, :-1], b[:, 1:] - 1)     # i < hi.x
        a[1:, :] = np.maximum(a[1:, :], b[:-1, :] - 1)      # j > lo.y
        a[:-1, :] = np.maximum(a[:-1, :], b[1:, :] - 1)     # j < hi.y
    return a


def position_unit_cell_fine(i_part, ppc, fine, T, L):
    """get_position_unit_cell_fine for an array L of levels: (rx, ry, do_init)"""
    L = np.asarray(L)
    nxc, nyc = ppc
    nxf, nyf = fine
    # L == 0
    do0 = np.full(L.shape, i_part < nxc * nyc)
    rx0 = np.full(L.shape, (0.5 + i_part % nxc) / nxc)
    ry0 = np.full(L.shape, (0.5 + i_part // nxc) / nyc)
    # L > 0
    ixf, iyf = i_part % nxf, i_part // nxf
    ixc, iyc = (ixf * nxc) // nxf, (iyf * nyc) // nyf
    s = L.astype(np.float64) / (T + 1)
    s = 1.5 * s - 0.5 * s * s * s
    rx1 = ((0.5 + ixc) / nxc) * (1.0 - s) + ((0.5 + ixf) / nxf) * s
    ry1 = ((0.5 + iyc) / nyc) * (1.0 - s) + ((0.5 + iyf) / nyf) * s
    coarse = L == 0
    return np.where(coarse, rx0, rx1), np.where(coarse, ry0, ry1), np.where(coarse, do0, True)


def init_particles(nx, ny, lo, hi, nz, ppc, fine_ppc=None, mask=None, T=5, density=1.0, radius=np.inf, hollow_core_radius=0.0,
                   normalized=True, density_func=None):
    """The particles InitParticles creates, in its order (i_part outermost, the box's cells x-fastest, only those created).
    lo, hi: the 3-d box; mask: (ny, nx) fine_patch(x, y) > 0 at the cell centres, None = no fine patch; density_func(x, y) ->
    density(x, y, c t), default the constant `density`.  Returns a dict of arrays: x, y, w, level (of the particle's cell), i,
    j (its cell), i_part, and "L", the (ny, nx) level map (0 outside the cropped box)."""
    dx, dy, dz = (hi[0] - lo[0]) / nx, (hi[1] - lo[1]) / ny, (hi[2] - lo[2]) / nz
    use_fine = mask is not None
    fine = tuple(fine_ppc) if use_fine else tuple(ppc)
    n_c, n_f = ppc[0] * ppc[1], fine[0] * fine[1]
    scale_c = 0.0 if n_c <= 0 else (1.0 / n_c if normalized else dx * dy * dz / n_c)
    scale_f = 0.0 if n_f <= 0 else (1.0 / n_f if normalized else dx * dy * dz / n_f)
    box = cell_box(nx, ny, lo, dx, dy, radius)
    ilo, ihi, jlo, jhi = box
    Lfull = np.zeros((ny, nx), dtype=np.int64)
    out = {k: [] for k in ("x", "y", "w", "level", "i", "j", "i_part")}
    if ihi >= ilo and jhi >= jlo:
        Lb = level_map(mask, T, box) if use_fine else np.zeros((jhi - jlo + 1, ihi - ilo + 1), dtype=np.int64)
        Lfull[jlo:jhi + 1, ilo:ihi + 1] = Lb
        jj, ii = np.meshgrid(np.arange(jlo, jhi + 1), np.arange(ilo, ihi + 1), indexing="ij")
        dens = density_func if density_func is not None else (lambda x, y: np.full(np.shape(x), float(density)))
        for i_part in range(n_f):
            rx, ry, do_init = position_unit_cell_fine(i_part, ppc, fine, T, Lb)
            x = lo[0] + (ii + rx) * dx
            y = lo[1] + (jj + ry) * dy
            rsq = x * x + y * y
            n_xy = dens(x, y)
            keep = do_init & ~((x >= hi[0]) | (x < lo[0]) | (y >= hi[1]) | (y < lo[1]) | (rsq > radius * radius)
                               | (rsq < hollow_core_radius * hollow_core_radius) | (n_xy <= 0.0))
            w = n_xy * np.where(Lb == 0, scale_c, scale_f)
            keep = keep.ravel()                      # x-fastest
            out["x"].append(x.ravel()[keep]); out["y"].append(y.ravel()[keep]); out["w"].append(w.ravel()[keep])
            out["level"].append(Lb.ravel()[keep]); out["i"].append(ii.ravel()[keep]); out["j"].append(jj.ravel()[keep])
            out["i_part"].append(np.full(int(keep.sum()), i_part))
    res = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in out.items()}
    for k in ("level", "i", "j", "i_part"):
        res[k] = res[k].astype(np.int64)
    res["L"] = Lfull
    return res


def sort_yx(x, y, *more, width=1.0):
    """the particles as a set: sorted by (y, x).  The keys are the coordinates in units of 1.2345e-10 of the box width, rounded:
    far below the lattice spacing and far above the rounding differences of two evaluations of the same lattice, so that
    both come out in the same order."""
    q = 1.2345e-10 * width
    o = np.lexsort((np.round(np.asarray(x) / q), np.round(np.asarray(y) / q)))
    return (x[o], y[o]) + tuple(m[o] for m in more)
