"""Seeded synthetic inputs shared by the CPU and GPU tests."""
import numpy as np

NCOMP = 21
G2 = 2     # guard cells for order-2 shapes (fields/Fields.cpp:63-64)


def thermal_sheet(nx, ny, lo, hi, ppc=2, seed=12345, u_std=0.1, jitter=1.0):
    """SURVEY 8(d) micro-benchmark sheet: lattice + uniform jitter, thermal momenta.

    Returns real (11, n) float64 in PlasmaIdx order, valid (n,) int32, ion_lev (n,) int32.
    """
    rng = np.random.default_rng(seed)
    dx = (hi[0] - lo[0]) / nx
    dy = (hi[1] - lo[1]) / ny
    xs, ys = [], []
    for ip in range(ppc * ppc):       # ppc index outermost (PlasmaParticleContainerInit.cpp:192)
        ixp, iyp = ip % ppc, ip // ppc
        ii, jj = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
        xs.append((lo[0] + (ii + (0.5 + ixp) / ppc) * dx).ravel())
        ys.append((lo[1] + (jj + (0.5 + iyp) / ppc) * dy).ravel())
    x = np.concatenate(xs)
    y = np.concatenate(ys)
    n = x.size
    x = x + jitter * (rng.random(n) - 0.5) * dx
    y = y + jitter * (rng.random(n) - 0.5) * dy
    eps = 1e-9
    x = np.clip(x, lo[0] + eps, hi[0] - eps)
    y = np.clip(y, lo[1] + eps, hi[1] - eps)
    ux = rng.normal(0.0, u_std, n)
    uy = rng.normal(0.0, u_std, n)
    uz = rng.normal(0.0, u_std, n)
    psi = np.sqrt(1.0 + ux * ux + uy * uy + uz * uz) - uz
    w = np.full(n, 1.0 / (ppc * ppc)) * (0.5 + rng.random(n))
    real = np.empty((11, n))
    real[0], real[1], real[2], real[3], real[4], real[5] = x, y, w, ux, uy, psi
    real[6], real[7] = x, y
    real[8] = ux + rng.normal(0.0, 0.01, n)
    real[9] = uy + rng.normal(0.0, 0.01, n)
    real[10] = psi * (1.0 + rng.normal(0.0, 0.01, n))
    return real, np.ones(n, dtype=np.int32), np.zeros(n, dtype=np.int32)


def smooth_slab(nx, ny, g, ncomp=NCOMP, seed=7, amp=0.3):
    """Random smooth fields in every component (a few Fourier modes), guards included."""
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(-g, ny + g), np.arange(-g, nx + g), indexing="ij")
    out = np.zeros((ncomp, ny + 2 * g, nx + 2 * g))
    for n in range(ncomp):
        for _ in range(4):
            kx, ky = rng.integers(1, 5, 2)
            ph = rng.random(2) * 2 * np.pi
            out[n] += amp * rng.normal() * np.sin(2 * np.pi * kx * ii / nx + ph[0]) * np.cos(2 * np.pi * ky * jj / ny + ph[1])
    return out


def rel_err(a, b):
    a = np.asarray(a)
    b = np.asarray(b)
    scale = max(np.abs(b).max(), 1e-300)
    return np.abs(a - b).max() / scale


def dst1(x, axis=-1):
    """DST-I along `axis` in FFTW's RODFT00 scaling, Y_k = 2 sum_j x_j sin(pi (j+1)(k+1) / (n+1)), from a real FFT of the
    odd extension (0, x, 0, -reversed x) of length 2(n+1): numpy only, independent of the oracle.  dst1(dst1(x)) = 2(n+1) x."""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, -1)
    n = x.shape[-1]
    z = np.zeros(x.shape[:-1] + (1,))
    ext = np.concatenate([z, x, z, -x[..., ::-1]], axis=-1)
    return np.moveaxis(-np.fft.rfft(ext, axis=-1).imag[..., 1:n + 1], -1, axis)


def poisson_dirichlet_ref(rhs, dx, dy):
    """Lap(F) = rhs on an (ny, nx) box, F = 0 one cell outside, with the 5-point Laplacian: DST-I along both directions,
    division by its eigenvalues -4/dx^2 sin^2(pi k / 2(nx+1)) - 4/dy^2 sin^2(pi l / 2(ny+1)), DST-I back."""
    ny, nx = rhs.shape
    sx = np.sin(np.pi * np.arange(1, nx + 1) / (2.0 * (nx + 1))) ** 2
    sy = np.sin(np.pi * np.arange(1, ny + 1) / (2.0 * (ny + 1))) ** 2
    eig = -4.0 * sx[None, :] / dx ** 2 - 4.0 * sy[:, None] / dy ** 2
    u = dst1(dst1(rhs, axis=1), axis=0) / eig
    return dst1(dst1(u, axis=1), axis=0) / (4.0 * (nx + 1) * (ny + 1))


# hpmg system type 1 (mg_solver/HpMultiGrid.cpp), restated in float64 numpy on the solve's own grid, independent of the oracle:
# -acf phi + Lap(phi) = rhs with homogeneous Dirichlet walls.  Cell-centred (even nx, ny): every cell is an unknown and a cell
# next to the wall takes the 4/3 stencil (laplacian :162-182, gs1 :265-292: the ghost value -2 phi_0 + phi_1 / 3).  Node-centred
# (odd nx, ny): the nx x ny user cells are the unknowns and the wall nodes one cell outside hold 0.  Arrays are (..., ny, nx).
WALL = 4.0 / 3.0


def _stencil_parts(phi, cc, facx, facy):
    """(off-diagonal part of Lap phi, diagonal factor of Lap at each cell without acf)."""
    p = np.asarray(phi, dtype=np.float64)
    pad = np.zeros(p.shape[:-2] + (p.shape[-2] + 2, p.shape[-1] + 2))
    pad[..., 1:-1, 1:-1] = p
    w, e = pad[..., 1:-1, :-2], pad[..., 1:-1, 2:]
    s, n = pad[..., :-2, 1:-1], pad[..., 2:, 1:-1]
    ny, nx = p.shape[-2:]
    lx, ly = facx * (w + e), facy * (s + n)
    dxx = np.full(nx, -2.0 * facx)
    dyy = np.full(ny, -2.0 * facy)
    if cc:
        lx[..., :, 0] = facx * WALL * e[..., :, 0]
        lx[..., :, -1] = facx * WALL * w[..., :, -1]
        ly[..., 0, :] = facy * WALL * n[..., 0, :]
        ly[..., -1, :] = facy * WALL * s[..., -1, :]
        dxx[[0, -1]] = -4.0 * facx
        dyy[[0, -1]] = -4.0 * facy
    return lx + ly, dxx[None, :] + dyy[:, None]


def helmholtz1_residual(sol, rhs, acf, dx, dy, cc):
    """rhs + acf phi - Lap(phi) (residual1 :184-190) at every unknown."""
    off, dlap = _stencil_parts(sol, cc, 1.0 / dx ** 2, 1.0 / dy ** 2)
    return rhs + acf * sol - (off + dlap * sol)


def helmholtz1_gsrb4(sol, rhs, acf, dx, dy, cc):
    """The four red-black half-sweeps (colour (i + j + c) % 2 == 0, c = 0..3) that solve_doit applies after each V-cycle; the
    parity is the same in user and in level index space.  Points of one colour do not read each other: one vector update each."""
    phi = np.array(sol, dtype=np.float64)
    ny, nx = phi.shape[-2:]
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    diag = None
    for c in range(4):
        off, dlap = _stencil_parts(phi, cc, 1.0 / dx ** 2, 1.0 / dy ** 2)
        if diag is None:
            diag = dlap - acf
        m = (ii + jj + c) % 2 == 0
        phi = np.where(m, (rhs - off) / diag, phi)
    return phi


def helmholtz1_matrix(acf, dx, dy, cc):
    """A = acf - Lap as a scipy.sparse matrix on the (ny, nx) unknowns, row-major: A phi = -rhs is the equation solved."""
    import scipy.sparse as sp
    ny, nx = acf.shape
    fx, fy = 1.0 / dx ** 2, 1.0 / dy ** 2
    def lap1(n, f):
        d = np.full(n, -2.0 * f)
        up = np.full(n - 1, f)
        lo = np.full(n - 1, f)
        if cc:
            d[[0, -1]] = -4.0 * f
            up[0] = WALL * f
            lo[-1] = WALL * f
        return sp.diags([lo, d, up], [-1, 0, 1], format="csr")
    lap = sp.kron(sp.identity(ny), lap1(nx, fx)) + sp.kron(lap1(ny, fy), sp.identity(nx))
    return (sp.diags(np.asarray(acf, dtype=np.float64).ravel()) - lap).tocsc()


def helmholtz1_direct(rhs, acf, dx, dy, cc):
    """(phi, ||A^-1||_inf): the exact solution of -acf phi + Lap(phi) = rhs by a sparse direct solve, for each leading plane of
    rhs, and the inverse's norm.  A = acf - Lap with acf >= 0 is a weakly diagonally dominant M-matrix, so A^-1 >= 0 entrywise
    and ||A^-1||_inf = ||A^-1 1||_inf: then ||x - phi||_inf <= ||A^-1||_inf ||r(x)||_inf for any x."""
    import scipy.sparse.linalg as spl
    ny, nx = acf.shape
    lu = spl.splu(helmholtz1_matrix(acf, dx, dy, cc))
    r = np.asarray(rhs, dtype=np.float64).reshape(-1, ny * nx)
    phi = np.stack([lu.solve(-b) for b in r]).reshape(np.shape(rhs))
    return phi, float(np.abs(lu.solve(np.ones(ny * nx))).max())


# DepositCurrent (particles/deposition/PlasmaDepositCurrent.cpp:155-246) restated in float64 numpy, independent of the oracle
# and of the kernels: the shape factors of orders 0 to 3 and the per-component weights of each particle.
DEP_COMPS = ("jx", "jy", "jz", "rho", "chi", "rhomjz")


def shape_factors(order, xmid):
    """(first cell, (n, order + 1) weights) of the plain shape of `order` at the positions xmid (in cells)."""
    xmid = np.asarray(xmid, dtype=np.float64)
    if order == 0:
        return np.floor(xmid + 0.5).astype(np.int64), np.ones(xmid.shape + (1,))
    if order == 1:
        j = np.floor(xmid)
        t = xmid - j
        return j.astype(np.int64), np.stack([1.0 - t, t], axis=-1)
    if order == 2:
        j = np.floor(xmid + 0.5)
        t = xmid - j
        return j.astype(np.int64) - 1, np.stack([0.5 * (0.5 - t) ** 2, 0.75 - t * t, 0.5 * (0.5 + t) ** 2], axis=-1)
    j = np.floor(xmid)
    t = xmid - j
    u = 1.0 - t
    return j.astype(np.int64) - 1, np.stack([u ** 3 / 6.0, 2.0 / 3.0 - t * t + 0.5 * t ** 3,
                                             2.0 / 3.0 - u * u + 0.5 * u ** 3, t ** 3 / 6.0], axis=-1)


def deposit_weights(real, valid, ion, slab, ng, geom, q, m, order, max_qsa=35.0, can_ionize=False, aabs=-1):
    """Per particle of the sheet: (survives, dropped, (6, n) per-component weight w_c, charge density q w level / vol,
    stencil (i0, sx, j0, sy)).  A valid particle whose gamma/psi fails the QSA test is dropped (NaN passes, as in the
    reference); w_c in DEP_COMPS order: ux/psi, uy/psi, (gamma_psi - 1) c, gamma_psi, q mu0 level/(m psi), 1.
    |a|^2 (slab component aabs) is gathered with the deposition's own shape, times laser_norm (times level^2)."""
    x, y, w, ux, uy, psi = (np.asarray(real[k], dtype=np.float64) for k in range(6))
    lev = np.asarray(ion, dtype=np.float64) if can_ionize else np.ones(x.size)
    vol_inv = 1.0 if geom.normalized else 1.0 / (geom.dx * geom.dy * geom.dz)
    i0, sx = shape_factors(order, (x - geom.xoff) / geom.dx)
    j0, sy = shape_factors(order, (y - geom.yoff) / geom.dy)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        psi_inv = 1.0 / psi
        vx, vy = ux * psi_inv, uy * psi_inv
        A = np.zeros(x.size)
        if aabs >= 0:
            on = np.asarray(valid) != 0
            for iy in range(order + 1):
                for ix in range(order + 1):
                    jj = np.where(on, j0 + iy + ng, 0)
                    ii = np.where(on, i0 + ix + ng, 0)
                    A += sx[:, ix] * sy[:, iy] * slab[aabs][jj, ii]
            A *= ((q / geom.q_e) * (geom.m_e / m)) ** 2 * lev * lev
        c = geom.c
        gp = 0.5 * ((1.0 + 0.5 * A) * psi_inv ** 2 + (vx / c) ** 2 + (vy / c) ** 2 + 1.0)
        bad = (gp < 0.0) | (gp > max_qsa) | (psi_inv < 0.0)
        wc = np.stack([vx, vy, (gp - 1.0) * c, gp, q * geom.mu0 * lev / m * psi_inv, np.ones(x.size)])
    valid = np.asarray(valid) != 0
    dropped = valid & bad
    return valid & ~bad, dropped, wc, q * vol_inv * w * lev, (i0, sx, j0, sy)


def deposit_current_ref(slab, ng, real, valid, ion, geom, comp, q, m, order, max_qsa=35.0, can_ionize=False, aabs=-1):
    """DepositCurrent into a copy of slab (ncomp, ny + 2 ng, nx + 2 ng): comp = slab component per DEP_COMPS entry (-1: not
    deposited).  Returns (slab, valid, w, n_qsa): the dropped particles lose their valid bit and their weight."""
    out = np.array(slab, dtype=np.float64)
    live, dropped, wc, rho, (i0, sx, j0, sy) = deposit_weights(real, valid, ion, slab, ng, geom, q, m, order, max_qsa,
                                                               can_ionize, aabs)
    idx = np.nonzero(live)[0]
    for iy in range(order + 1):
        for ix in range(order + 1):
            cd = rho[idx] * sx[idx, ix] * sy[idx, iy]
            jj, ii = j0[idx] + iy + ng, i0[idx] + ix + ng
            for k, c in enumerate(comp):
                if c >= 0:
                    np.add.at(out[c], (jj, ii), cd * wc[k, idx])
    v = np.where(dropped, 0, np.asarray(valid)).astype(np.int32)
    w = np.where(dropped, 0.0, np.asarray(real[2], dtype=np.float64))
    return out, v, w, int(dropped.sum())
