"""numpy restatement of the fixed_weight_pdf beam (injection_type = fixed_weight_pdf: BeamParticleContainer.cpp:200-240,
InitBeamFixedWeightPDF3D / InitBeamFixedWeightPDFSlice, BeamParticleContainerInit.cpp:477-695) as hipace_amd generates it on the
device (hps_engine_set_beam_fixed_weight_pdf), written from the reference's formulae and the table of draws:

    key(tag, i) = hash(hash(seed, tag), i);  unit(k, c) = coll_unit(hash(k, c));  pair(k, c) = Box-Muller of unit(k, c), unit(k, c + 1)
    tag 1 (momentum)   m_x, m_y = pair(key, 0), m_z = cosine branch of pair(key, 2)       (tests/beam_init_reference.normal_deviates)
    tag 3 (x, y)       attempt k: n_x, n_y = pair(key, 2 k)
    tag 4 (pdf z)      t = unit(key, 0) cum[ns] -> the sub-slice s;  w = unit(key, 1) -> z inside it

pe, the pdf at the ns + 1 edges, is an argument: the tests take it from the library's own host routine
(api.Expression(pdf, ("z",)).evaluate_host(edges(...))), so that from the table on nothing depends on a libm.  The ten functions of
z are numbers, strings over z or Programs (hipace_amd/expr.py: Program.evaluate)."""
import numpy as np

from hipace_amd import decks, expr
from tests import beam_fixed_weight_reference as F
from tests import beam_init_reference as B
from tests import plasma_thermal_reference as W

U64 = np.uint64
TAG_XY, TAG_PDF_Z = 3, 4
MAX_ATTEMPTS = 4096
small_deck, cell_size, binned, slice_coordinate = F.small_deck, F.cell_size, F.binned, F.slice_coordinate


def weight_roundings(ns):
    """roundings between the table pe and the weight (table() below), as a bound in eps on the relative error: lw (2 per sub-slice,
    carried into a sum of positive terms: 2) and the sum's ns additions (ns); max_density: dz and zs (3), zs std_x std_y pi (3), the
    division (1), lw (2); density integral / max_density (2); the cell sizes (hi - lo)/n (6), their inverses (3), the product of
    the three and the product with the total (3); the division by N (1)"""
    return ns + 26


def function(f, constants=None):
    prog = f if isinstance(f, expr.Program) else expr.compile_expr(f, ("z",), constants)
    return prog.evaluate


def edges(deck, pdf_ref_ratio=4):
    """the ns + 1 edges lo_z + s zs of the sub-slices"""
    zs = cell_size(deck)[2] / pdf_ref_ratio
    return deck["lo"][2] + np.arange(deck["nz"] * pdf_ref_ratio + 1) * zs


def table(deck, pe, num_particles, position_std, u_mean_z=0.0, u_std_z=0.0, density=None, total_charge=None, pdf_ref_ratio=4,
          constants=None):
    """the host part (:489-542), sequentially and in the reference's order -> dict(ns, zs, lw, integral, max_density, weight,
    uz_mean, uz_std, cum (ns + 1), last: the last sub-slice of positive weight)"""
    pe = np.asarray(pe, dtype=np.float64)
    ns = deck["nz"] * pdf_ref_ratio
    assert pe.shape == (ns + 1,) and (pe >= 0.0).all(), "PDF must be >= 0 everywhere"
    lo_z, zs = deck["lo"][2], cell_size(deck)[2] / pdf_ref_ratio
    sx, sy = function(position_std[0], constants), function(position_std[1], constants)
    um, us = function(u_mean_z, constants), function(u_std_z, constants)
    lw = 0.5 * (pe[:-1] + pe[1:])
    integral = max_density = avg_uz = avg_uz_sq = 0.0
    for s in range(ns - 1, -1, -1):
        zmin, zmax = lo_z + s * zs, lo_z + (s + 1) * zs
        zmid = 0.5 * (zmin + zmax)
        if lw[s] > 0.0 and total_charge is None:
            max_density = max(max_density, float(lw[s] / (zs * sx(zmid) * sy(zmid) * 2.0 * np.pi)))
        a, b = float(um(zmid)), float(us(zmid))
        avg_uz += lw[s] * a
        avg_uz_sq += lw[s] * (a * a + b * b)
        integral += lw[s]
    assert integral > 0.0
    total = density * integral / max_density if total_charge is None else total_charge / deck["beam_charge"]
    if not deck.get("si_units", 0):
        h = cell_size(deck)
        total *= (1.0 / h[0]) * (1.0 / h[1]) * (1.0 / h[2])
    cum = np.concatenate([[0.0], np.cumsum(lw)])      # (sequential, upward)
    return dict(ns=ns, zs=zs, lw=lw, integral=float(integral), max_density=max_density, weight=abs(total / num_particles),
                uz_mean=avg_uz / integral, uz_std=float(np.sqrt(max(avg_uz_sq / integral - (avg_uz / integral) * (avg_uz / integral), 0.0))),
                cum=cum, last=int(np.flatnonzero(lw > 0.0)[-1]))


def z_fraction(w, lo_w, hi_w):
    """the position inside a sub-slice of the linear profile between lo_w and hi_w as a fraction of its width (:631-652)
    -> (fraction, the Taylor branch was taken)"""
    taylor = np.minimum(lo_w, hi_w) * 1.1 > np.maximum(lo_w, hi_w)
    with np.errstate(divide="ignore", invalid="ignore"):
        f_t = w - w * (w - 1.0) * (hi_w - lo_w) * (1.0 / (hi_w + lo_w))
        f_s = (np.sqrt(lo_w * lo_w + w * (hi_w * hi_w - lo_w * lo_w)) - lo_w) * (1.0 / (hi_w - lo_w))
    return np.where(taylor, f_t, f_s), taylor


def fixed_weight_pdf_beam(deck, pe, num_particles, position_mean, position_std, u_mean=(0.0, 0.0, 0.0), u_std=(0.0, 0.0, 0.0),
                          density=None, total_charge=None, radius=np.inf, z_foc=0.0, do_symmetrize=False, pdf_ref_ratio=4, seed=1,
                          constants=None, first=0, pdf=None):
    """-> dict(soa (7, m nd) x y z ux uy uz w of EVERY draw in draw order, the m = 4 (do_symmetrize) or 1 copies of draw i at
    m i + q; valid (m nd); i (m nd) the particle's draw; per draw (nd): s, t, w, taylor, z, x, y (the offsets before the shifts),
    attempt, X, Y, sx, sy, um (3, nd), us (3, nd), m (3, nd); table: table()'s dict; weight; dr: the smallest
    |x^2 + y^2 - radius^2| / radius^2 over every attempt of every draw, inf without a radius).  The draws are first .. first + nd - 1.
    pdf is not read (the cases carry it for the engine): pe holds its values."""
    m = 4 if do_symmetrize else 1
    assert num_particles % m == 0 and (density is None) != (total_charge is None)
    nd = num_particles // m
    c = decks.SI["c"] if deck.get("si_units", 0) else 1.0
    tab = table(deck, pe, num_particles, position_std, u_mean[2], u_std[2], density, total_charge, pdf_ref_ratio, constants)
    pe, cum, zs, last = np.asarray(pe, dtype=np.float64), tab["cum"], tab["zs"], tab["last"]
    i = np.arange(first, first + nd, dtype=U64)
    kz = F._key(seed, TAG_PDF_Z, i)
    t = W.coll_unit(W.coll_hash(kz, U64(0))) * cum[-1]
    s = np.searchsorted(cum[:last + 1], t, side="right") - 1      # the last index with cum[s] <= t, at most `last`
    w = W.coll_unit(W.coll_hash(kz, U64(1)))
    f, taylor = z_fraction(w, pe[s], pe[s + 1])
    z = (deck["lo"][2] + s * zs) + zs * f
    fn = [function(v, constants) for v in tuple(position_mean) + tuple(position_std) + tuple(u_mean) + tuple(u_std)]
    X, Y, sx, sy = (np.asarray(fn[k](z), dtype=np.float64) for k in range(4))
    um = np.stack([fn[4 + d](z) for d in range(3)])
    us = np.stack([fn[7 + d](z) for d in range(3)])
    kxy = F._key(seed, TAG_XY, i)
    x, y, attempt, valid = np.empty(nd), np.empty(nd), np.zeros(nd, dtype=np.int64), np.zeros(nd, dtype=bool)
    todo, dr = np.arange(nd), np.inf
    for k in range(MAX_ATTEMPTS if total_charge is not None else 1):
        n0, n1 = F._pair(kxy[todo], 2 * k)
        x[todo], y[todo], attempt[todo] = sx[todo] * n0, sy[todo] * n1, k
        r2 = x[todo] * x[todo] + y[todo] * y[todo]
        ok = r2 <= radius * radius
        if np.isfinite(radius):
            dr = min(dr, float(np.abs(r2 - radius * radius).min() / (radius * radius)))
        valid[todo[ok]] = True
        todo = todo[~ok]
        if todo.size == 0:
            break
    dev = B.normal_deviates(seed, i)
    u = [um[d] + us[d] * dev[d] for d in range(3)]
    out = dict(i=np.repeat(np.arange(first, first + nd), m), s=s, t=t, w=w, taylor=taylor, z=z, x=x.copy(), y=y.copy(), attempt=attempt,
               X=X, Y=Y, sx=sx, sy=sy, um=um, us=us, m=dev, table=tab, weight=tab["weight"], dr=dr)
    if z_foc != 0.0:
        x = x - z_foc * u[0] / u[2]
        y = y - z_foc * u[1] / u[2]
    soa = np.empty((7, m, nd))
    for q, (px, py) in enumerate(((1, 1), (-1, 1), (1, -1), (-1, -1))[:m]):
        soa[0, q] = X + x if px > 0 else X - x
        soa[1, q] = Y + y if py > 0 else Y - y
        soa[2, q] = z
        soa[3, q] = (u[0] if px > 0 else -u[0]) * c
        soa[4, q] = (u[1] if py > 0 else -u[1]) * c
        soa[5, q] = u[2] * c
        soa[6, q] = tab["weight"]
    out["soa"] = np.ascontiguousarray(soa.transpose(0, 2, 1).reshape(7, m * nd))
    out["valid"] = np.repeat(valid, m)
    return out


def margins(deck, beam):
    """the smallest distances of the draws from the cuts as fractions of each cut's scale: (|t - cum[s]| and |t - cum[s + 1]| over
    cum[ns]; |slice coordinate - integer|; |x^2 + y^2 - radius^2| over radius^2 over every attempt, inf without a radius)"""
    cum = beam["table"]["cum"]
    dt = min(np.abs(beam["t"] - cum[beam["s"]]).min(), np.abs(beam["t"] - cum[beam["s"] + 1]).min()) / cum[-1]
    q = slice_coordinate(deck, beam["z"])
    dq = np.abs(q - np.rint(q)).min()
    return dt, dq, beam["dr"]


# ---- the cases of tests/test_beam_fixed_weight_pdf_gpu.py (tests/test_beam_fixed_weight_pdf_cpu.py holds every one to the margin
# condition); the box of small_deck() is 16 x 16 x 8 cells of 0.2 about the origin: z in [-0.8, 0.8], 32 sub-slices of 0.05 ----

_GAUSSIAN = dict(num_particles=4096, pdf="exp(-0.5*((z-0.1)/0.3)^2)", position_mean=("0.11+0.2*z", "-0.07-0.1*z"),
                 position_std=("0.3+0.1*z", "0.25+0.05*z"), u_mean=(1.0, -2.0, "100+20*z"), u_std=(0.5, 0.4, 3.0), density=2.0, seed=1)
_ARITHMETIC = dict(position_mean=("slope*(z-0.1)", "if(z>0, 0.1, -0.1) + 0.05*z^2"), position_std=("0.3+0.1*z", "0.25/(1+z*z)"),
                   u_mean=("1+z", "-2*z", "100+20*z"), u_std=("0.5+0.1*z", "0.4-0.2*z", "3/(2+z)"), constants=dict(slope=0.2))


# the beam of decks.beam_evolution() in the moving-beam test
MOVING_BEAM = dict(num_particles=2000, pdf="exp(-0.5*((z-0.2)/0.8)^2)", position_mean=("0.05*z", 0.1), position_std=(0.3, "0.25+0.02*z"),
                   u_mean=(0.0, 0.0, 1.0e3), u_std=(2.0, 3.0, 10.0), density=1.0e-8, radius=1.0, seed=11)


def cases():
    """{name: (deck, arguments of set_beam_fixed_weight_pdf)}"""
    um = 10.0e-6
    out = dict(
        gaussian=(small_deck(), dict(_GAUSSIAN)),
        constant=(small_deck(), dict(_GAUSSIAN, pdf="1", seed=2)),
        windowed=(small_deck(), dict(_GAUSSIAN, pdf="(z>-0.52)*(z<0.63)*(1+0.5*z)", seed=3)),
        two_bunches=(small_deck(), dict(_GAUSSIAN, pdf="(z>-0.62)*(z<-0.23) + (z>0.18)*(z<0.57)*(2+z)", seed=4)),
        ratio_1=(small_deck(), dict(_GAUSSIAN, pdf_ref_ratio=1, seed=5)),
        ratio_3=(small_deck(), dict(_GAUSSIAN, pdf_ref_ratio=3, seed=6)),
        symmetrized=(small_deck(), dict(_GAUSSIAN, do_symmetrize=True, seed=7)),
        focus=(small_deck(), dict(_GAUSSIAN, z_foc=0.3, seed=8)),
        radius_density=(small_deck(), dict(_GAUSSIAN, radius=0.4, seed=9)),
        si_charge=(small_deck(si=True), dict(num_particles=1000, pdf="exp(-0.5*(z/sz)^2)", position_mean=(0.1 * um, "0.1*z"),
                                             position_std=(0.3 * um, "0.25e-5+0.02*z"), u_mean=(0.0, 0.0, 1000.0), u_std=(1.0, 2.0, 10.0),
                                             total_charge=1.0e-12, radius=0.35 * um, constants=dict(sz=0.3 * um), seed=10)),
        launch_4099=(small_deck(), dict(_GAUSSIAN, num_particles=4099, seed=11)),
        launch_8198=(small_deck(), dict(_GAUSSIAN, num_particles=8198, seed=11)),
        last_sub_slice=(small_deck(), dict(_GAUSSIAN, num_particles=1000, pdf="z>0.76", seed=12)),
        programs=(small_deck(), dict(_GAUSSIAN, **_ARITHMETIC, seed=13)),
        programs_unit=(small_deck(), dict(_GAUSSIAN, position_mean=(0.0, 0.0), position_std=(1.0, 1.0), u_mean=(0.0, 0.0, 0.0),
                                          u_std=(1.0, 1.0, 1.0), seed=13)),
    )
    for n in (1, 63, 64, 65, 257):
        out[f"size_{n}"] = (small_deck(), dict(_GAUSSIAN, num_particles=n, seed=14))
    return out
