"""Input decks for the slice engine (normalised units, explicit Bx/By solver).

Each deck is a plain dict mirroring the keys of the reference's input files that matter to the
per-slice hot path.  The named decks restate

* ``linear_wake``     -- /root/reference/examples/linear_wake/inputs_normalized
                         (run as tests/linear_wake.normalized.1Rank.sh:33-36: + ``rho``)
* ``blowout_wake``    -- /root/reference/examples/blowout_wake/inputs_normalized
                         (run as tests/blowout_wake_explicit.2Rank.sh:32-35: max_step=1, dt=0)
* ``beam_in_vacuum``  -- /root/reference/examples/beam_in_vacuum/inputs_normalized
                         (run as tests/beam_in_vacuum.normalized.Serial.sh:30-34: order 0)
* ``beam_in_vacuum_open_boundary`` -- the same deck as run by tests/beam_in_vacuum_open_boundary.normalized.1Rank.sh
                         (predictor-corrector Bx/By; oracle only)
* ``synthetic(n, nz)``-- the BASELINE.md section 3 benchmark deck (blowout deck scaled to n x n,
                         ppc 2x2) used by bench.py.
"""
import copy
import math

_DEFAULT = dict(
    nx=64, ny=64, nz=100,
    lo=(-8.0, -8.0, -6.0), hi=(8.0, 8.0, 6.0),
    order=2,                 # hipace.depos_order_xy
    deriv_type=2,            # hipace.depos_derivative_type (Hipace.H:78)
    plasma_ppc=(1, 1), plasma_density=1.0, plasma_radius=0.0,   # radius 0 -> infinite
    plasma_charge=-1.0, plasma_mass=1.0,                       # electron, normalised units
    max_qsa=35.0,            # plasmas.max_qsa_weighting_factor (PlasmaParticleContainer.H:161)
    n_subcycles=1,
    beam_profile=0,          # -1 none, 0 gaussian, 1 flattop
    beam_zmin=-5.9, beam_zmax=5.9, beam_radius=1.2, beam_density=3.0,
    beam_umean=(0.0, 0.0, 2000.0), beam_pos_mean=(0.0, 0.0, 0.0),
    beam_pos_std=(0.3, 0.3, 1.41), beam_ppc=(1, 1, 1), beam_charge=-1.0,
    bc=1,                    # boundary.particle: 0 Reflecting, 1 Periodic, 2 Absorbing
    mg_tol_rel=1.0e-4,       # hipace.MG_tolerance_rel (Hipace.H:246)
    mg_tol_abs=2.2250738585072014e-308,   # numeric_limits<double>::min() (Hipace.H:248)
    deposit_rho=0,
    n_steps=1,               # max_step + 1
    dt=0.0,                  # hipace.dt; 0 in every BASELINE deck: the beam never moves
    beam_n_subcycles=10,     # beam.n_subcycles (BeamParticleContainer.H:222)
    beam_mass=1.0,
    ext_E_slope=(0.0, 0.0),  # beams.external_E(x,y,z,t) = s0*x s1*y 0.
    bxby_solver=0,           # hipace.bxby_solver: 0 explicit (Hipace.H:244), 1 predictor-corrector
    predcorr_tol=4.0e-2,     # hipace.predcorr_B_error_tolerance (Hipace.H:210)
    predcorr_max_iter=30,    # hipace.predcorr_max_iterations (Hipace.H:213)
    predcorr_mix=0.05,       # hipace.predcorr_B_mixing_factor (Hipace.H:222)
    field_bc=0,              # boundary.field: 0 Dirichlet; 1 Open (multipole expansion of the sources to order 18, fields/Fields.cpp:678-735)
    laser_on=0,              # lasers.names != no_laser: a Gaussian envelope (laser/Laser.H:32-45), static (step 0 only)
    laser_a0=0.0, laser_w0=1.0, laser_L0=1.0, laser_lambda0=0.8e-6, laser_pos=(0.0, 0.0, 0.0),
    laser_zfoc=0.0,          # laser.focal_distance
    laser_solver=0,          # lasers.solver_type: 0 keep the envelope static, 1 "fft" (AdvanceSliceFFT), 2 "multigrid" (AdvanceSliceMG)
    beam_radiation_reaction=0, background_density_SI=0.0, beam_no_z_push=0,      # <beam>.do_radiation_reaction, hipace.background_density_SI, <beam>.do_z_push = 0
    laser_mg_tol_rel=1.0e-4, laser_mg_tol_abs=0.0,      # lasers.MG_tolerance_rel / MG_tolerance_abs
    laser_use_phase=1,       # lasers.use_phase (MultiLaser.H:203)
    grid_current_on=0, grid_current_peak=0.0, grid_current_mean=(0.0, 0.0, 0.0), grid_current_std=(1.0, 1.0, 1.0),   # grid_current.*
    si_units=0,              # hipace.normalized_units = 0: SI constants, charges and masses in C and kg, weights = charges
    # second plasma species "ion" with ADK field ionisation; the released electrons join the first species
    # (<ion>.ionization_product, PlasmaParticleContainer.cpp:61-90, 261-440)
    plasma_no_neutralize=0,  # <plasma>.neutralize_background = false for the first species
    ion_on=0, ion_ppc=(0, 0), ion_density=0.0, ion_mass=0.0, ion_charge=0.0, ion_init_level=0, ion_Z=0,
    ion_energies=(0.0,) * 56, ion_seed=0,
    # <beam>.do_spin_tracking, initial_spin, spin_anom (BeamParticleContainer.cpp:105-109; anomalous magnetic moment of the electron)
    beam_spin_tracking=0, beam_initial_spin=(1.0, 0.0, 0.0), beam_spin_anom=0.00115965218128,
)

# hipace.dt = adaptive and beams.external_E's z term.  Kept apart from _DEFAULT (whose decks the full-size fixtures record
# key by key); a deck without these keys has them at 0, which is what every value below is.  0 = the reference's default
# (utils/AdaptiveTimeStep.H:25-42): nt_per_betatron (20), dt_max (inf), adaptive_threshold_uz (2), adaptive_phase_tolerance
# (4e-4), adaptive_predict_step / adaptive_control_phase_advance (inverted: 0 keeps them on), adaptive_phase_substeps (2000),
# plasmas.adaptive_density, hipace.max_time (0: none), the initial estimate's <beam>.u_std[2]; ext_Ez_slope: external Ez = s*z
ADAPTIVE_DEFAULT = dict(
    dt_adaptive=0, nt_per_betatron=0.0, dt_max=0.0, adaptive_threshold_uz=0.0, adaptive_phase_tolerance=0.0,
    adaptive_no_predict_step=0, adaptive_no_phase_control=0, adaptive_phase_substeps=0,
    adaptive_density=0.0, max_time=0.0, beam_uz_std=0.0, ext_Ez_slope=0.0,
)

# <beam>.do_salame (salame/Salame.cpp).  Kept apart from _DEFAULT like ADAPTIVE_DEFAULT; 0 = off / the reference's default:
# hipace.salame_n_iter (5), salame_relative_tolerance (1e-4), salame_do_advance (inverted: 0 keeps it on), and the slope of
# the linear target Ez_initial + slope (zeta - zeta_initial) that stands in for the parsed hipace.salame_Ez_target
SALAME_DEFAULT = dict(beam_do_salame=0, salame_n_iter=0, salame_relative_tolerance=0.0, salame_no_advance=0,
                      salame_Ez_target_slope=0.0)
# SALAME on a witness species of a moving-beam engine: beam_do_salame is the one beam of a static-beam engine; with
# hipace.dt != 0 the SALAME beam is an entry of beam_species that carries do_salame (BEAM_SPECIES_DEFAULT).  beam_species_salame
# announces such a species -- the engine then allocates the SALAME slice ahead of every species.  Like "collisions" it is no
# member of hps_deck (nor of SALAME_DEFAULT, which mirrors the deck's members): SliceEngine applies it through
# hps_engine_set_beam_species_salame, and sets it itself when an entry of the deck's beam_species carries do_salame.
SALAME_SPECIES_DEFAULT = dict(beam_species_salame=0)

# <plasma>.fine_ppc, <ion>.fine_ppc and <plasma>.hollow_core_radius (PlasmaParticleContainer.cpp:123-169).  Kept apart from
# _DEFAULT like ADAPTIVE_DEFAULT; 0 = off.  Like "collisions" they are not members of hps_deck: SliceEngine applies them
# through hps_engine_set_plasma_init.  The patch itself (plasmas.fine_patch(x,y)) and fine_transition_cells are arguments
# of SliceEngine; a deck may carry them as "fine_patch" (a callable f(x, y) or a (ny, nx) mask) and "fine_transition_cells".
PLASMA_INIT_DEFAULT = dict(plasma_fine_ppc=(0, 0), ion_fine_ppc=(0, 0), plasma_hollow_core_radius=0.0)

# Warm plasmas: <plasma>.u_mean, u_std, temperature_in_ev of the species "plasma" and "ion", plasmas.do_symmetrize and
# prevent_centered_particle (PlasmaParticleContainer.cpp:125-145, 170).  Kept apart from _DEFAULT like PLASMA_INIT_DEFAULT and
# applied by SliceEngine through hps_engine_set_plasma_momentum / hps_engine_set_plasma_symmetry; None / 0 = not given.
# u_mean and u_std are three numbers in units of c (the input parser is out of scope); a temperature stands for an isotropic
# u_std (thermal_u_std) and excludes u_std; plasma_seed is the seed of both species' momentum draws.
PLASMA_THERMAL_DEFAULT = dict(plasma_u_mean=(0.0, 0.0, 0.0), plasma_u_std=None, plasma_temperature_in_ev=None,
                              ion_u_mean=(0.0, 0.0, 0.0), ion_u_std=None, ion_temperature_in_ev=None, plasma_seed=0,
                              plasmas_do_symmetrize=0, plasmas_prevent_centered_particle=0)


# Parsed plasma densities: <plasma>.density(x,y,z), min_density and density_table_file of the species "plasma" and "ion", and
# plasmas.density(x,y,z) for both (PlasmaParticleContainer.cpp:90-119).  Kept apart from _DEFAULT like
# PLASMA_INIT_DEFAULT and applied by SliceEngine through hps_engine_set_density_expr; None = not given.  An expression is a string
# in the input file's syntax (or a number) over x, y, z whose value is the density itself; a species' own key wins over the
# shared one; a table is a path (read_density_table) or a list of (position, expression) pairs; density_constants is
# my_constants.  A species with an expression or a table does not use the tables of set_density_profile.
DENSITY_EXPR_DEFAULT = dict(plasma_density_expr=None, ion_density_expr=None, plasmas_density_expr=None,
                            plasma_min_density=None, ion_min_density=None, plasma_density_table=None, ion_density_table=None,
                            density_constants=None)


# The general fixed_ppc beam: <beam>.density(x,y,z), min_density, u_std, random_ppc (BeamParticleContainer.cpp; InitBeamFixedPPCSlice,
# BeamParticleContainerInit.cpp:198-346).  Kept apart from _DEFAULT like PLASMA_INIT_DEFAULT and applied by SliceEngine
# through hps_engine_set_beam_fixed_ppc, which generates the beam on the device; a deck without beam_density_expr keeps the beam
# of its beam_profile.  The expression is a string in the input file's syntax (or a number) over x, y, z whose value is the density
# itself (beam_profile, beam_density and beam_pos_std are then ignored; the window beam_zmin / beam_zmax / beam_radius around
# beam_pos_mean holds); beam_u_std in units of c; beam_random_ppc per direction; beam_seed keys the position and momentum draws;
# beam_density_constants is my_constants.  beam_profile_expr(deck) writes the deck's own profile as such an expression.
BEAM_INIT_DEFAULT = dict(beam_density_expr=None, beam_min_density=0.0, beam_u_std=(0, 0, 0), beam_random_ppc=(0, 0, 0), beam_seed=1,
                         beam_density_constants=None)


def beam_profile_expr(deck):
    """(expression, constants) of the deck's own beam_profile -- 0 gaussian, 1 flattop -- in the operation order of the engine's
    host generator, for a deck that only wants beam_u_std or beam_random_ppc: dict(deck, beam_density_expr=..., beam_density_constants=...)."""
    prof = deck.get("beam_profile", 0)
    if prof == 1:
        return "n0", dict(n0=float(deck["beam_density"]))
    if prof != 0:
        raise ValueError(f"beam_profile_expr: the deck has no beam profile to write as an expression (beam_profile = {prof})")
    m, s = deck["beam_pos_mean"], deck["beam_pos_std"]
    consts = dict(n0=float(deck["beam_density"]), x0=float(m[0]), y0=float(m[1]), z0=float(m[2]), sx=float(s[0]), sy=float(s[1]), sz=float(s[2]))
    return ("n0*exp(-0.5*((x-x0)/sx)*((x-x0)/sx))*exp(-0.5*((y-y0)/sy)*((y-y0)/sy))*exp(-0.5*((z-z0)/sz)*((z-z0)/sz))", consts)


def beam_init(deck):
    """The deck's BEAM_INIT_DEFAULT keys as the arguments of SliceEngine.set_beam_fixed_ppc -- dict(expr, constants, min_density,
    u_std, random_ppc, seed) -- or None for a deck without beam_density_expr.  ValueError: beam_min_density, beam_u_std or
    beam_random_ppc without beam_density_expr (they belong to the device generator; beam_profile_expr gives the expression of
    the deck's own profile)."""
    text = deck.get("beam_density_expr")
    mind = float(deck.get("beam_min_density", 0.0) or 0.0)
    u_std = tuple(float(v) for v in (deck.get("beam_u_std") or (0, 0, 0)))
    rnd = tuple(int(bool(v)) for v in (deck.get("beam_random_ppc") or (0, 0, 0)))
    if len(u_std) != 3 or len(rnd) != 3:
        raise ValueError("beam_u_std and beam_random_ppc have three entries each")
    if text is None:
        given = [k for k, on in (("beam_min_density", mind != 0.0), ("beam_u_std", any(u_std)), ("beam_random_ppc", any(rnd))) if on]
        if given:
            raise ValueError(f"{', '.join(given)}: needs beam_density_expr (decks.beam_profile_expr(deck) writes the deck's own "
                             "beam_profile as one)")
        return None
    return dict(expr=text, constants=deck.get("beam_density_constants"), min_density=mind, u_std=u_std, random_ppc=rnd,
                seed=int(deck.get("beam_seed", 1)))


# The fixed_weight beam on the device: injection_type = fixed_weight, profile = gaussian | can (BeamParticleContainer.cpp:137-198;
# InitBeamFixedWeight3D / InitBeamFixedWeightSlice, BeamParticleContainerInit.cpp:348-475).  A deck's optional entry
# "beam_fixed_weight" is a dict of these keys -- the arguments of SliceEngine.set_beam_fixed_weight, which SliceEngine applies
# through hps_engine_set_beam_fixed_weight in place of the beam of beam_profile; the deck itself gives the grid, the units,
# beam_charge and beam_mass.  No deck function sets the entry, and it is no member of _DEFAULT, BEAM_INIT_DEFAULT or hps_deck.
# position_mean = (X(z), Y(z), z mean): X and Y numbers or strings in the input file's syntax over z with `constants`
# (my_constants); exactly one of density and total_charge (SI units only); u_mean, u_std in units of c.
BEAM_FIXED_WEIGHT_DEFAULT = dict(num_particles=0, position_mean=(0.0, 0.0, 0.0), position_std=None, u_mean=(0.0, 0.0, 0.0),
                                 u_std=(0.0, 0.0, 0.0), density=None, total_charge=None, profile="gaussian", zmin=-math.inf,
                                 zmax=math.inf, radius=math.inf, do_symmetrize=False, z_foc=0.0, duz_per_uz0_dzeta=0.0, seed=1,
                                 constants=None)


def beam_fixed_weight(deck):
    """The deck's entry beam_fixed_weight over BEAM_FIXED_WEIGHT_DEFAULT as the arguments of SliceEngine.set_beam_fixed_weight, or
    None for a deck without the entry.  ValueError: unknown keys, or the entry beside beam_density_expr (two beams for one deck)."""
    entry = deck.get("beam_fixed_weight")
    if entry is None:
        return None
    unknown = set(entry) - set(BEAM_FIXED_WEIGHT_DEFAULT)
    if unknown:
        raise ValueError(f"beam_fixed_weight: unknown entries {sorted(unknown)}")
    if deck.get("beam_density_expr") is not None:
        raise ValueError("beam_fixed_weight and beam_density_expr: a deck has one beam, from fixed_weight or from fixed_ppc")
    return dict(BEAM_FIXED_WEIGHT_DEFAULT, **entry)


# Further beam species of a moving-beam engine (beams.names = driver witness).  A deck's optional entry "beam_species"
# is a list of dicts of these keys -- the arguments of SliceEngine.add_beam_species, which SliceEngine applies, in order, behind the
# deck's own beam (species 0).  charge and mass default to the deck's beam_charge and beam_mass, the other constants to the
# deck's.  Exactly one source: fixed_weight (the keys of BEAM_FIXED_WEIGHT_DEFAULT), fixed_weight_pdf (those of
# BEAM_FIXED_WEIGHT_PDF_DEFAULT), density_expr (with the keys of BEAM_INIT_DEFAULT but the expression: constants, min_density,
# u_std, random_ppc, seed) or particles (a (7, n) array x y z ux uy uz w).  It is no member of _DEFAULT or hps_deck.
# do_salame (<beam>.do_salame of that species): it takes part in SALAME during step 0; it enters the species' record only where
# the entry sets it (hps_beam_species.do_salame stays 0 otherwise), and needs the deck's beam_species_salame (SALAME_SPECIES_DEFAULT).
BEAM_SPECIES_DEFAULT = dict(name=None, charge=None, mass=None, n_subcycles=None, do_z_push=None, radiation_reaction=None,
                            spin_anom=None, do_spin_tracking=None, uz_mean=0.0, uz_std=0.0, do_salame=None)
BEAM_SPECIES_SOURCES = ("fixed_weight", "fixed_weight_pdf", "density_expr", "particles")
BEAM_SPECIES_EXPR_KEYS = ("constants", "min_density", "u_std", "random_ppc", "seed")
MAX_BEAM_SPECIES = 4


def beam_species_spec(deck, spec, where="beam_species"):
    """One beam species over BEAM_SPECIES_DEFAULT and the deck's own beam constants -> dict(name, record, source, args):
    record = the fields of hps_beam_species, source one of BEAM_SPECIES_SOURCES, args its setter's arguments.  ValueError:
    unknown keys, no source or several, unknown keys inside the source's dict."""
    allowed = set(BEAM_SPECIES_DEFAULT) | set(BEAM_SPECIES_SOURCES) | set(BEAM_SPECIES_EXPR_KEYS)
    unknown = set(spec) - allowed
    if unknown:
        raise ValueError(f"{where}: unknown entries {sorted(unknown)}")
    given = [k for k in BEAM_SPECIES_SOURCES if spec.get(k) is not None]
    if len(given) != 1:
        raise ValueError(f"{where}: exactly one source of {', '.join(BEAM_SPECIES_SOURCES)} is needed, got {given or 'none'}")
    source = given[0]
    stray = [k for k in BEAM_SPECIES_EXPR_KEYS if k in spec and source != "density_expr"]
    if stray:
        raise ValueError(f"{where}: {', '.join(stray)} go with density_expr, not with {source}")

    def pick(key, deck_key, default):
        v = spec.get(key)
        return deck.get(deck_key, default) if v is None else v
    do_z_push = spec.get("do_z_push")
    record = dict(charge=float(pick("charge", "beam_charge", -1.0)), mass=float(pick("mass", "beam_mass", 1.0)),
                  n_subcycles=int(pick("n_subcycles", "beam_n_subcycles", 10)),
                  no_z_push=int(deck.get("beam_no_z_push", 0)) if do_z_push is None else int(not do_z_push),
                  radiation_reaction=int(bool(pick("radiation_reaction", "beam_radiation_reaction", 0))),
                  do_spin_tracking=int(bool(pick("do_spin_tracking", "beam_spin_tracking", 0))),
                  spin_anom=float(pick("spin_anom", "beam_spin_anom", 0.0)),
                  uz_mean=float(spec.get("uz_mean", 0.0) or 0.0), uz_std=float(spec.get("uz_std", 0.0) or 0.0))
    if spec.get("do_salame") is not None:
        record["do_salame"] = int(bool(spec["do_salame"]))
    if source == "fixed_weight":
        bad = set(spec[source]) - set(BEAM_FIXED_WEIGHT_DEFAULT)
        args = dict(BEAM_FIXED_WEIGHT_DEFAULT, **spec[source])
    elif source == "fixed_weight_pdf":
        bad = set(spec[source]) - set(BEAM_FIXED_WEIGHT_PDF_DEFAULT)
        args = dict(BEAM_FIXED_WEIGHT_PDF_DEFAULT, **spec[source])
    elif source == "density_expr":
        bad = set()
        args = dict(expr=spec[source], constants=spec.get("constants"), min_density=float(spec.get("min_density", 0.0) or 0.0),
                    u_std=tuple(spec.get("u_std") or (0.0, 0.0, 0.0)), random_ppc=tuple(spec.get("random_ppc") or (0, 0, 0)),
                    seed=int(spec.get("seed", 1)))
    else:
        bad = set()
        shape = getattr(spec[source], "shape", None)
        if shape is None or len(shape) != 2 or shape[0] != 7:
            raise ValueError(f"{where}: particles is a (7, n) array x y z ux uy uz w")
        args = dict(soa=spec[source])
    if bad:
        raise ValueError(f"{where}: {source}: unknown entries {sorted(bad)}")
    if source == "fixed_weight" and "uz_mean" not in spec and "uz_std" not in spec:
        record["uz_mean"], record["uz_std"] = float(args["u_mean"][2]), float(args["u_std"][2])      # the source's own u_z
    # (fixed_weight_pdf: u_z may be a function of z; SliceEngine takes the pdf-weighted moments its setter returns)
    return dict(name=spec.get("name"), record=record, source=source, args=args)


def beam_species(deck):
    """The deck's entry beam_species as a list of beam_species_spec results ([] for a deck without it).  ValueError: what
    beam_species_spec refuses, more species than the engine holds beside the deck's beam, a name given twice."""
    entry = deck.get("beam_species")
    if entry is None:
        return []
    if isinstance(entry, dict) or not hasattr(entry, "__len__"):
        raise ValueError("beam_species: a list of dicts, one per species")
    if len(entry) > MAX_BEAM_SPECIES - 1:
        raise ValueError(f"beam_species: at most {MAX_BEAM_SPECIES - 1} species beside the deck's own beam")
    out = [beam_species_spec(deck, s, f"beam_species[{k}]") for k, s in enumerate(entry)]
    names = [s["name"] for s in out if s["name"] is not None]
    if len(set(names)) != len(names):
        raise ValueError(f"beam_species: a name is given twice ({names})")
    return out


def beam_species_salame(deck):
    """-> 1 if the deck announces a do_salame beam species: its own beam_species_salame, or an entry of beam_species that carries
    do_salame (SALAME_SPECIES_DEFAULT); 0 otherwise"""
    if deck.get("beam_species_salame", 0):
        return 1
    entry = deck.get("beam_species") or ()
    if isinstance(entry, dict):
        return 0
    return int(any(isinstance(s, dict) and s.get("do_salame") for s in entry))


def with_fixed_weight_beam(deck, beam=None, **more):
    """A copy of deck with the entry beam_fixed_weight, from the keyword names of fixed_weight_beam (num_particles, density,
    total_charge, pos_mean, pos_std, u_mean, u_std, zmin, zmax, radius, seed, do_symmetrize, duz_per_uz0_dzeta): the (deck, beam)
    pairs of gaussian_weight_SI(), radiation_reaction_SI(), ... pass as with_fixed_weight_beam(*gaussian_weight_SI()), and
    single parameters as keywords, which win over the dict's.  The names of BEAM_FIXED_WEIGHT_DEFAULT pass as they are.
    A mean that is a Python callable cannot run on the device: write it as a string over z."""
    rename = dict(pos_mean="position_mean", pos_std="position_std")
    entry = {}
    for k, v in dict(beam or {}, **more).items():
        k = rename.get(k, k)
        if k not in BEAM_FIXED_WEIGHT_DEFAULT:
            raise ValueError(f"with_fixed_weight_beam: unknown beam parameter {k!r}")
        entry[k] = v
    if any(callable(m) for m in entry.get("position_mean", ())):
        raise ValueError("with_fixed_weight_beam: a position mean that is a Python callable cannot run on the device; "
                         "write it as a string over z, such as '0.2*z'")
    d = copy.deepcopy(deck)
    d["beam_fixed_weight"] = entry
    return d


# The fixed_weight_pdf beam on the device: injection_type = fixed_weight_pdf (BeamParticleContainer.cpp:200-240;
# InitBeamFixedWeightPDF3D / InitBeamFixedWeightPDFSlice, BeamParticleContainerInit.cpp:477-695).  A deck's optional
# entry "beam_fixed_weight_pdf" is a dict of these keys -- the arguments of SliceEngine.set_beam_fixed_weight_pdf, which
# SliceEngine applies through hps_engine_set_beam_fixed_weight_pdf in place of the beam of beam_profile; the deck itself gives the
# grid, the units, beam_charge and beam_mass.  No deck function sets the entry, and it is no member of _DEFAULT,
# BEAM_INIT_DEFAULT, BEAM_FIXED_WEIGHT_DEFAULT or hps_deck.  pdf, position_mean (2), position_std (2), u_mean (3), u_std (3):
# numbers or strings in the input file's syntax over z with `constants` (my_constants); exactly one of density (the peak
# density) and total_charge (SI units only); u_mean, u_std in units of c.
BEAM_FIXED_WEIGHT_PDF_DEFAULT = dict(num_particles=0, pdf=None, position_mean=(0.0, 0.0), position_std=None, u_mean=(0.0, 0.0, 0.0),
                                     u_std=(0.0, 0.0, 0.0), density=None, total_charge=None, radius=math.inf, z_foc=0.0,
                                     do_symmetrize=False, pdf_ref_ratio=4, seed=1, constants=None)


def beam_fixed_weight_pdf(deck):
    """The deck's entry beam_fixed_weight_pdf over BEAM_FIXED_WEIGHT_PDF_DEFAULT as the arguments of
    SliceEngine.set_beam_fixed_weight_pdf, or None for a deck without the entry.  ValueError: unknown keys, or the entry beside
    beam_fixed_weight or beam_density_expr (two beams for one deck)."""
    entry = deck.get("beam_fixed_weight_pdf")
    if entry is None:
        return None
    unknown = set(entry) - set(BEAM_FIXED_WEIGHT_PDF_DEFAULT)
    if unknown:
        raise ValueError(f"beam_fixed_weight_pdf: unknown entries {sorted(unknown)}")
    for other in ("beam_fixed_weight", "beam_density_expr"):
        if deck.get(other) is not None:
            raise ValueError(f"beam_fixed_weight_pdf and {other}: a deck has one beam")
    return dict(BEAM_FIXED_WEIGHT_PDF_DEFAULT, **entry)


def with_fixed_weight_pdf_beam(deck, **beam):
    """A copy of deck with the entry beam_fixed_weight_pdf from the names of BEAM_FIXED_WEIGHT_PDF_DEFAULT; pos_mean and pos_std,
    the names of fixed_weight_pdf_beam, pass too.  A function that is a Python callable cannot run on the device: write it as
    a string over z."""
    rename = dict(pos_mean="position_mean", pos_std="position_std")
    entry = {}
    for k, v in beam.items():
        k = rename.get(k, k)
        if k not in BEAM_FIXED_WEIGHT_PDF_DEFAULT:
            raise ValueError(f"with_fixed_weight_pdf_beam: unknown beam parameter {k!r}")
        entry[k] = v
    funcs = [entry.get("pdf")] + [m for k in ("position_mean", "position_std", "u_mean", "u_std") for m in entry.get(k) or ()]
    if any(callable(f) for f in funcs):
        raise ValueError("with_fixed_weight_pdf_beam: a Python callable cannot run on the device; write it as a string over z, "
                         "such as 'exp(-0.5*(z/1.41)^2)'")
    d = copy.deepcopy(deck)
    d["beam_fixed_weight_pdf"] = entry
    return d


def read_density_table(path):
    """<plasma>.density_table_file: one `position expression` per line, the expression being the rest of the line
    (PlasmaParticleContainer.cpp:107-116); a line that does not start with a number, or has nothing behind it, is skipped.
    -> [(position, expression)] in ascending order of position; of two lines with one position the first stays (std::map)."""
    table = {}
    with open(path) as f:
        for line in f:
            parts = line.split(None, 1)
            if len(parts) < 2 or not parts[1].strip():
                continue
            try:
                pos = float(parts[0])
            except ValueError:
                continue
            table.setdefault(pos, parts[1].strip())
    if not table:
        raise ValueError(f"unable to get any data out of the density table file {path!r}")
    return sorted(table.items())


def density_exprs(deck):
    """{species index: (expression or table, constants, min_density)} of the deck's DENSITY_EXPR_DEFAULT keys; a species without
    them is absent.  ValueError: an expression and a table for one species (the reference asserts "Can only use one plasma
    density from either 'density(x,y,z)' or 'density_table_file', not both"), a min_density without either, or keys for the
    ion species of a deck without one."""
    out = {}
    for sp, name in enumerate(("plasma", "ion")):
        own, table, mind = deck.get(name + "_density_expr"), deck.get(name + "_density_table"), deck.get(name + "_min_density")
        if sp == 1 and not deck.get("ion_on", 0):
            if own is not None or table is not None or mind is not None:
                raise ValueError("ion_density_expr / ion_density_table / ion_min_density: the deck has no ion species")
            continue
        text = own if own is not None else deck.get("plasmas_density_expr")
        if sp == 0 and not deck.get("plasma_density", 0.0) > 0.0 and own is None and table is None:
            continue      # (plasmas.density(x,y,z) of a deck without the species "plasma" is for the ions alone)
        if text is not None and table is not None:
            raise ValueError(f"{name}: can only use one plasma density from either '{name}_density_expr' (or plasmas_density_expr) "
                             f"or '{name}_density_table', not both")
        if table is not None:
            text = read_density_table(table) if isinstance(table, (str, bytes)) or hasattr(table, "__fspath__") else list(table)
        if text is None:
            if mind is not None:
                raise ValueError(f"{name}_min_density needs {name}_density_expr, plasmas_density_expr or {name}_density_table")
            continue
        out[sp] = (text, deck.get("density_constants"), 0.0 if mind is None else float(mind))
    return out


def thermal_u_std(deck, species="plasma"):
    """u_std of species "plasma" / "ion" from the deck's <species>_u_std or <species>_temperature_in_ev:
    u_std = sqrt(T q_e / (M c^2)) in every direction with the species' mass M in kg (PlasmaParticleContainer.cpp:138-145; a
    normalised deck's masses are in electron masses).  Both given: ValueError, as the reference asserts."""
    u_std, T = deck.get(species + "_u_std"), deck.get(species + "_temperature_in_ev")
    if u_std is not None and T is not None:
        raise ValueError(f"{species}: please specify exclusively either a temperature or the thermal momentum")
    if T is None:
        return tuple(float(v) for v in (u_std if u_std is not None else (0.0, 0.0, 0.0)))
    q_e_SI, m_e_SI, c_SI = 1.602176634e-19, 9.1093837015e-31, 299792458.0
    mass = float(deck[species + "_mass"]) * (1.0 if deck.get("si_units", 0) else m_e_SI)
    return (((float(T) * q_e_SI) / (mass * c_SI * c_SI)) ** 0.5,) * 3


# Further plasma species (plasmas.names beyond the two; MultiPlasma.cpp): the deck's optional entry plasma_species is a
# list of dicts over PLASMA_SPECIES_DEFAULT, one per fixed-charge species behind "plasma" (0) and "ion" (1).  Like "collisions" it
# is no member of hps_deck: SliceEngine applies it through hps_engine_add_plasma_species and the per-species setters.  charge and
# mass in the deck's units (default: the opposite of the plasma's charge; no default mass), density required; u_std and
# temperature_in_ev exclude each other (thermal_u_std's rule); density_expr and density_table likewise (density_exprs' rule).
PLASMA_SPECIES_DEFAULT = dict(name=None, charge=None, mass=None, density=None, ppc=(1, 1), fine_ppc=(0, 0), neutralize_background=True,
                              u_mean=(0.0, 0.0, 0.0), u_std=None, temperature_in_ev=None, seed=0,
                              density_expr=None, density_table=None, density_constants=None, min_density=None)
MAX_PLASMA_SPECIES = 6
PLASMA_SPECIES_NAMES = ("plasma", "ion")      # the names of species 0 and 1


def plasma_species_spec(deck, spec, where="plasma_species"):
    """One further plasma species over PLASMA_SPECIES_DEFAULT -> dict(name, record, u_mean, u_std, seed, density): record = the
    fields of hps_plasma_species, u_std from u_std or temperature_in_ev, density = None or (expression or table, constants,
    min_density) as density_exprs gives it.  ValueError: unknown keys, a missing density or mass, a name of the deck's own
    species, both a temperature and a u_std, both an expression and a table, a min_density without either."""
    if not isinstance(spec, dict):
        raise ValueError(f"{where}: a dict over decks.PLASMA_SPECIES_DEFAULT")
    unknown = set(spec) - set(PLASMA_SPECIES_DEFAULT)
    if unknown:
        raise ValueError(f"{where}: unknown entries {sorted(unknown)}")
    s = dict(PLASMA_SPECIES_DEFAULT, **spec)
    if s["density"] is None:
        raise ValueError(f"{where}: density is required")
    if s["mass"] is None:
        raise ValueError(f"{where}: mass is required")
    if s["name"] in PLASMA_SPECIES_NAMES:
        raise ValueError(f"{where}: the name {s['name']!r} belongs to species {PLASMA_SPECIES_NAMES.index(s['name'])} of the deck")
    charge = -float(deck.get("plasma_charge", -1.0)) if s["charge"] is None else float(s["charge"])
    record = dict(charge=charge, mass=float(s["mass"]), density=float(s["density"]), ppc=tuple(int(v) for v in s["ppc"]),
                  fine_ppc=tuple(int(v) for v in s["fine_ppc"]), neutralize_background=int(bool(s["neutralize_background"])))
    u_std = thermal_u_std(dict(q_u_std=s["u_std"], q_temperature_in_ev=s["temperature_in_ev"], q_mass=record["mass"],
                               si_units=deck.get("si_units", 0)), "q")
    text, table, mind = s["density_expr"], s["density_table"], s["min_density"]
    if text is not None and table is not None:
        raise ValueError(f"{where}: can only use one plasma density from either 'density_expr' or 'density_table', not both")
    if table is not None:
        text = read_density_table(table) if isinstance(table, (str, bytes)) or hasattr(table, "__fspath__") else list(table)
    if text is None and mind is not None:
        raise ValueError(f"{where}: min_density needs density_expr or density_table")
    density = None if text is None else (text, s["density_constants"], 0.0 if mind is None else float(mind))
    return dict(name=s["name"], record=record, u_mean=tuple(float(v) for v in s["u_mean"]), u_std=u_std, seed=int(s["seed"]),
                density=density)


def plasma_species(deck):
    """The deck's entry plasma_species as a list of plasma_species_spec results ([] for a deck without it).  ValueError: what
    plasma_species_spec refuses, more species than the engine holds behind the deck's two, a name given twice."""
    entry = deck.get("plasma_species")
    if entry is None:
        return []
    if isinstance(entry, dict) or not hasattr(entry, "__len__"):
        raise ValueError("plasma_species: a list of dicts, one per species")
    if len(entry) > MAX_PLASMA_SPECIES - 2:
        raise ValueError(f"plasma_species: at most {MAX_PLASMA_SPECIES - 2} species behind the deck's plasma and ion")
    out = [plasma_species_spec(deck, s, f"plasma_species[{k}]") for k, s in enumerate(entry)]
    names = [s["name"] for s in out if s["name"] is not None]
    if len(set(names)) != len(names):
        raise ValueError(f"plasma_species: a name is given twice ({names})")
    return out


def plasma_species_names(deck):
    """The names of the deck's plasma species in index order: "plasma", "ion", then the further species' (species<k> unnamed)"""
    return list(PLASMA_SPECIES_NAMES) + [s["name"] or f"species{2 + k}" for k, s in enumerate(plasma_species(deck))]


def plasma_species_index(names, species):
    """A species given as an index or a name of `names` -> its index.  ValueError: an unknown name, an index out of range."""
    if isinstance(species, str):
        if species not in names:
            raise ValueError(f"no plasma species named {species!r} (have {list(names)})")
        return list(names).index(species)
    k = int(species)
    if not 0 <= k < len(names):
        raise ValueError(f"no plasma species {k} (the engine holds {len(names)})")
    return k


# Ionisation energies in eV of a few elements: NIST Atomic Spectra Database (Kramida, Ralchenko, Reader and NIST ASD
# Team, ver. 5.2), the values the reference tabulates in utils/IonizationEnergiesTable.H.
IONIZATION_ENERGIES_EV = {
    "H": (13.59843449,),
    "He": (24.58738880, 54.4177650),
    "Li": (5.39171495, 75.6400964, 122.4543581),
    "N": (14.53413, 29.60125, 47.4453, 77.4735, 97.8901, 552.06732, 667.046116),
    "Ar": (15.7596117, 27.62967, 40.735, 59.58, 74.84, 91.290, 124.41, 143.4567, 422.60, 479.76, 540.4, 619.0, 685.5,
           755.13, 855.5, 918.375, 4120.6656, 4426.2228),
}
M_P_DA = 1.007276466621      # proton mass in Da; <plasma>.mass_Da is converted with m_p / 1.007276466621 (PlasmaParticleContainer.cpp:118-122)


def with_ion_species(d, element, density, ppc=(1, 1), mass_Da=None, initial_level=0, seed=0):
    """Add the species "ion" of `element` to deck d (in place): <ion>.element / mass_Da / initial_ion_level / ppc /
    density, ionization_product = the first species.  Charge +e per level, mass in units of the deck (kg in SI, electron
    masses in normalised units)."""
    en = IONIZATION_ENERGIES_EV[element]
    m_p_SI, m_e_SI, q_e_SI = 1.67262192369e-27, 9.1093837015e-31, 1.602176634e-19
    mass_Da = mass_Da if mass_Da is not None else {"H": 1.008, "He": 4.002602, "Li": 6.94, "N": 14.007, "Ar": 39.948}[element]
    mass_SI = m_p_SI * mass_Da / M_P_DA
    si = bool(d.get("si_units", 0))
    d.update(ion_on=1, ion_ppc=tuple(ppc), ion_density=density, ion_mass=mass_SI if si else mass_SI / m_e_SI,
             ion_charge=q_e_SI if si else 1.0, ion_init_level=initial_level, ion_Z=len(en),
             ion_energies=tuple(en) + (0.0,) * (56 - len(en)), ion_seed=seed)
    return d


def blowout_wake():
    d = copy.deepcopy(_DEFAULT)
    d["n_steps"] = 2
    return d


HOLLOW_BEAM_DENSITY = "if(sqrt(x^2+y^2) >= r_in and sqrt(x^2+y^2) < r_out, n_ring*exp(-0.5*(z/sigma_z)^2), 0)"


def blowout_wake_hollow_beam(r_in=0.6, r_out=1.0, density=1.0, sigma_z=1.41):
    """The 64 x 64 blowout deck driven by a ring-shaped (hollow) driver: <beam>.density(x,y,z) as a parsed function with the
    file's my_constants (BEAM_INIT_DEFAULT), evaluated on the device per lattice point; nothing of it on the axis."""
    d = blowout_wake()
    d.update(BEAM_INIT_DEFAULT)
    d.update(beam_density_expr=HOLLOW_BEAM_DENSITY,
             beam_density_constants=dict(r_in=float(r_in), r_out=float(r_out), n_ring=float(density), sigma_z=float(sigma_z)),
             beam_radius=max(float(r_out), d["beam_radius"]))
    return d


class fine_patch_disc:
    """plasmas.fine_patch(x,y) = "sqrt(x^2+y^2) < radius" (a class, so that a deck that carries it can be pickled)"""

    def __init__(self, radius):
        self.radius = float(radius)

    def __call__(self, x, y):
        return x * x + y * y < self.radius * self.radius

    def __eq__(self, other):
        return isinstance(other, fine_patch_disc) and other.radius == self.radius

    def __hash__(self):
        return hash(self.radius)


def blowout_wake_fine_patch(radius=2.0, transition_cells=2):
    """The 64 x 64 blowout deck with 1 x 1 particles per cell, 4 x 4 inside the disc r < radius around the axis and
    `transition_cells` cells of transition around it (<plasma>.fine_ppc, plasmas.fine_patch, fine_transition_cells)."""
    d = blowout_wake()
    d.update(PLASMA_INIT_DEFAULT)
    d.update(plasma_ppc=(1, 1), plasma_fine_ppc=(4, 4), fine_patch=fine_patch_disc(radius), fine_transition_cells=transition_cells)
    return d


def blowout_wake_warm(temperature_in_ev=50.0, do_symmetrize=True, seed=1, ppc=(1, 1)):
    """The 64 x 64 blowout deck with a warm plasma: <plasma>.temperature_in_ev, and plasmas.do_symmetrize (four mirrored
    copies of every particle, so that the thermal noise does not seed hosing: the reference recommends it with a temperature)."""
    d = blowout_wake()
    d.update(PLASMA_INIT_DEFAULT)
    d.update(PLASMA_THERMAL_DEFAULT)
    d.update(plasma_ppc=tuple(ppc), plasma_temperature_in_ev=float(temperature_in_ev), plasma_seed=int(seed),
             plasmas_do_symmetrize=int(bool(do_symmetrize)))
    return d


def linear_wake():
    d = copy.deepcopy(_DEFAULT)
    d.update(nx=32, ny=32, nz=200, lo=(-10.0, -10.0, -7.5), hi=(10.0, 10.0, 2.0),
             beam_profile=1, beam_zmin=-1.0, beam_zmax=1.0, beam_radius=3.0, beam_density=0.01,
             deposit_rho=1)
    return d


def linear_wake_gaussian():
    """linear_wake grid and plasma with a Gaussian driver (smooth in zeta) -- the deck of the predictor-corrector
    tests; the reference's own such test (tests/ion_motion.SI.1Rank.sh) also drives with a Gaussian beam."""
    d = linear_wake()
    d.update(beam_profile=0, beam_pos_std=(1.5, 1.5, 0.7), beam_pos_mean=(0.0, 0.0, 0.0), beam_zmin=-7.4, beam_zmax=1.9,
             beam_radius=6.0, beam_density=0.05)
    return d


def beam_in_vacuum():
    d = copy.deepcopy(_DEFAULT)
    d.update(nx=512, ny=768, nz=4, lo=(-200.0, -200.0, -2.0), hi=(200.0, 200.0, 2.0), order=0,
             plasma_ppc=(0, 0), plasma_density=0.0,
             beam_profile=1, beam_zmin=-10.0, beam_zmax=10.0, beam_radius=1.0, beam_density=1.0,
             beam_umean=(0.0, 0.0, 1.0e3), beam_ppc=(2, 2, 1), deposit_rho=1)
    return d


def synthetic(n=1024, nz=1024, ppc=2):
    """BASELINE.md section 3 / SURVEY 8(d) benchmark deck: blowout deck on n x n x nz, ppc x ppc."""
    d = copy.deepcopy(_DEFAULT)
    d.update(nx=n, ny=n, nz=nz, plasma_ppc=(ppc, ppc))
    return d


def beam_evolution():
    """tests/beam_evolution.1Rank.sh: beam_in_vacuum deck, 32x32x10, 21 steps of dt = 3 in a linear focusing field."""
    d = copy.deepcopy(_DEFAULT)
    d.update(nx=32, ny=32, nz=10, lo=(-2.0, -2.0, -2.0), hi=(2.0, 2.0, 2.0), order=2,
             plasma_ppc=(0, 0), plasma_density=0.0,
             beam_profile=1, beam_zmin=-10.0, beam_zmax=10.0, beam_radius=1.0, beam_density=1.0e-8,
             beam_umean=(0.0, 0.0, 1.0e3), beam_ppc=(4, 4, 1), n_steps=21, dt=3.0, ext_E_slope=(0.5, 0.5))
    return d


def beam_evolution_parsed():
    """tests/beam_evolution.1Rank.sh as the script writes it: beams.external_E(x,y,z,t) = .5*x .5*y 0. as parsed expressions
    (the optional entry "beam_external_fields", applied by SliceEngine through hps_engine_set_beam_external_fields -- not a
    member of hps_deck) in place of beam_evolution()'s slopes."""
    d = beam_evolution()
    d.update(ext_E_slope=(0.0, 0.0), beam_external_fields=dict(E=(".5*x", ".5*y", "0.")))
    return d


def adaptive_time_step(sign=1):
    """tests/adaptive_time_step.1Rank.sh: the beam_in_vacuum deck on 32 x 32 x 32 cells in [-2, 2]^3, a flattop beam of
    u_z = 1000 (ppc 4 4 1, four sub-cycles) in beams.external_E = (0, 0, sign * 0.5 z), no plasma, hipace.dt = adaptive with
    nt_per_betatron = 89.7597901025655 and plasmas.adaptive_density = 1, max_step = 20 (21 steps), tile size 8.
    sign = -1 is the script's first run (negative_gradient.txt), +1 its second, whose output the checksums record."""
    d = copy.deepcopy(_DEFAULT)
    d.update(ADAPTIVE_DEFAULT)
    d.update(nx=32, ny=32, nz=32, lo=(-2.0, -2.0, -2.0), hi=(2.0, 2.0, 2.0), order=2,
             plasma_ppc=(0, 0), plasma_density=0.0,
             beam_profile=1, beam_zmin=-10.0, beam_zmax=10.0, beam_radius=1.0, beam_density=1.0,
             beam_umean=(0.0, 0.0, 1.0e3), beam_ppc=(4, 4, 1), beam_n_subcycles=4, n_steps=21, dt=0.0,
             dt_adaptive=1, nt_per_betatron=89.7597901025655, adaptive_density=1.0, ext_Ez_slope=0.5 * sign)
    return d


def beam_in_vacuum_open_boundary():
    """tests/beam_in_vacuum_open_boundary.normalized.1Rank.sh:31-43 -- the reference's only checksum fixture of the
    predictor-corrector Bx/By solver: beam_in_vacuum deck, order 0, off-centre beam, boundary.field = Open."""
    d = beam_in_vacuum()
    d.update(lo=(-4.0, -4.0, -2.0), hi=(4.0, 4.0, 2.0), beam_pos_mean=(2.0, -1.0, 0.0), bc=2, deposit_rho=1,
             bxby_solver=1, predcorr_mix=0.95, predcorr_max_iter=5, predcorr_tol=4.0e-2, field_bc=1)
    return d


def laser_blowout_wake():
    """tests/laser_blowout_wake_explicit.1Rank.sh:32-45: blowout_wake deck without a beam, driven by a Gaussian laser
    pulse (a0 = 4.5, w0 = 4, L0 = 2) on 128 x 128 x 100 cells, max_step = 0."""
    d = copy.deepcopy(_DEFAULT)
    d.update(nx=128, ny=128, nz=100, lo=(-20.0, -20.0, -7.5), hi=(20.0, 20.0, 6.0), beam_profile=-1, n_steps=1,
             laser_on=1, laser_a0=4.5, laser_w0=4.0, laser_L0=2.0, laser_lambda0=0.8e-6, laser_pos=(0.0, 0.0, 0.0))
    return d


def laser_evolution():
    """tests/laser_evolution.SI.2Rank.sh with lasers.solver_type = fft (examples/laser/inputs_SI): a Gaussian pulse in
    vacuum, 128 x 128 x 50 cells, 31 steps of c dt = 70 um.  The reference runs it in SI units with kp_inv = 10 um;
    here lengths are in units of kp_inv (the envelope equation has no other scale in vacuum)."""
    d = copy.deepcopy(_DEFAULT)
    d.update(nx=128, ny=128, nz=50, lo=(-6.0, -6.0, -8.0), hi=(6.0, 6.0, 6.0), order=0, plasma_ppc=(0, 0), plasma_density=0.0,
             beam_profile=-1, n_steps=31, dt=7.0,
             laser_on=1, laser_a0=1.0, laser_w0=2.0, laser_L0=2.0, laser_lambda0=0.08, laser_pos=(0.0, 0.0, 0.0),
             laser_zfoc=100.0, laser_solver=1, laser_use_phase=1)
    return d


# 2018 CODATA values of utils/Constants.H:15-24
SI = dict(c=299792458.0, ep0=8.8541878128e-12, mu0=1.25663706212e-06, q_e=1.602176634e-19, m_e=9.1093837015e-31)


def laser_blowout_wake_SI():
    """tests/laser_blowout_wake_explicit.SI.1Rank.sh (examples/blowout_wake/inputs_SI): the laser-driven wake in SI
    units, kp_inv = 10 um, n_e = wp^2 m_e eps0 / q_e^2 with wp = c kp -- the deck of BASELINE config 5 at test size."""
    kp_inv = 10.0e-6
    wp = SI["c"] / kp_inv
    ne = wp ** 2 * SI["m_e"] * SI["ep0"] / SI["q_e"] ** 2
    d = laser_blowout_wake()
    d.update(si_units=1, lo=(-20.0 * kp_inv, -20.0 * kp_inv, -7.5 * kp_inv), hi=(20.0 * kp_inv, 20.0 * kp_inv, 6.0 * kp_inv),
             plasma_density=ne, plasma_charge=-SI["q_e"], plasma_mass=SI["m_e"],
             laser_w0=4.0 * kp_inv, laser_L0=2.0 * kp_inv, laser_lambda0=0.8e-6)
    return d


def config5(n=1024, nz=2048, solver=1, si=False, ionize=True):
    """BASELINE configs[4]: laser_blowout_wake on n x n x nz cells, 4 ppc, a Gaussian pulse (a0 = 4.5, w0 = 4 kp^-1, L0 = 2 kp^-1,
    lambda0 = 0.8 um) that drives the wake and is advanced by the envelope solver on every slice (solver 1 = fft, 2 = multigrid),
    c dt = 5 kp^-1, neutral nitrogen at a fifth of the electron density (one macro-atom per cell) field-ionised by the wake.
    si = True: the deck as BASELINE names it (tests/laser_blowout_wake_explicit.SI.1Rank.sh, examples/blowout_wake/inputs_SI:
    hipace.normalized_units = 0, kp_inv = 10 um); si = False: its normalised twin (same kernels, other constants)."""
    if si:
        kp_inv = 10.0e-6
        d = laser_blowout_wake_SI()
        d.update(nx=n, ny=n, nz=nz, plasma_ppc=(2, 2), lo=(-20.0 * kp_inv, -20.0 * kp_inv, -15.0 * kp_inv),
                 hi=(20.0 * kp_inv, 20.0 * kp_inv, 6.0 * kp_inv), laser_solver=solver, dt=5.0 * kp_inv / SI["c"])
        if ionize:
            with_ion_species(d, "N", 0.2 * d["plasma_density"], ppc=(1, 1), initial_level=0, seed=5)
        return d
    d = synthetic(n, nz, 2)
    d.update(beam_profile=-1, lo=(-20.0, -20.0, -15.0), hi=(20.0, 20.0, 6.0), laser_on=1, laser_a0=4.5, laser_w0=4.0,
             laser_L0=2.0, laser_lambda0=0.08, laser_solver=solver, dt=5.0)
    if ionize:
        with_ion_species(d, "N", 0.2, ppc=(1, 1), initial_level=0, seed=5)
        d["background_density_SI"] = 2.8239587008591567e23      # kp_inv = 10 um (hipace.background_density_SI)
    return d


def config5_laser_patch(n=1024, nz=2048, n_laser=256, solver=1, si=False, ionize=True):
    """config5 with the envelope on a centred n_laser x n_laser patch whose cells are the field's (lasers.n_cell, patch_lo,
    patch_hi; all slices): the pulse (w0 = 4 kp^-1 of a 40 kp^-1 box) needs no more."""
    d = config5(n, nz, solver, si, ionize)
    dx, dy = (d["hi"][0] - d["lo"][0]) / n, (d["hi"][1] - d["lo"][1]) / n
    cx, cy = 0.5 * (d["lo"][0] + d["hi"][0]), 0.5 * (d["lo"][1] + d["hi"][1])
    d.update(laser_n_cell=(n_laser, n_laser), laser_patch_lo=(cx - 0.5 * n_laser * dx, cy - 0.5 * n_laser * dy, d["lo"][2]),
             laser_patch_hi=(cx + 0.5 * n_laser * dx, cy + 0.5 * n_laser * dy, d["hi"][2]), laser_interp_order=1)
    return d


# lasers.n_cell, patch_lo, patch_hi, interp_order (MultiLaser::MakeLaserGeometry, laser/MultiLaser.cpp:58-115): the envelope on a
# grid of its own.  Kept apart from _DEFAULT like PLASMA_INIT_DEFAULT and applied by SliceEngine through
# hps_engine_set_laser_grid; None = the field grid's cells / the field box.  A deck without any of the four keys makes no call.
LASER_GRID_DEFAULT = dict(laser_n_cell=None, laser_patch_lo=None, laser_patch_hi=None, laser_interp_order=1)


def has_laser_grid(deck):
    return any(deck.get(k) is not None for k in ("laser_n_cell", "laser_patch_lo", "laser_patch_hi")) or "laser_interp_order" in deck


# One Gaussian pulse of the deck key "lasers" (a list of such dicts; Laser.H:32-45, Laser.cpp:33-47): the reference's names and
# defaults.  Exactly one of L0 and tau is given (L0 = tau c); PFT_yz = pi/2 is no pulse-front tilt.  CEP enters the reference's
# exponent as a real number (MultiLaser.cpp:912): it scales the pulse by e^CEP, and so it does here.  "lasers" replaces the
# deck's own pulse (laser_a0 ...; laser_lambda0 stays shared); "laser_profiles" is a list of callables f(x, y, z) -> complex
# (init_type = parser) added on top; "laser_insitu" switches the in-situ reductions on.  A deck without these keys makes no call.
LASER_PULSE_DEFAULT = dict(a0=0.0, w0=0.0, L0=None, tau=None, position_mean=(0.0, 0.0, 0.0), focal_distance=0.0, CEP=0.0,
                           propagation_angle_yz=0.0, PFT_yz=math.pi / 2.0)


def laser_pulse(pulse, c=1.0):
    """A pulse dict with the defaults filled in and tau turned into L0 -> (a0, w0, L0, position_mean, focal_distance, CEP,
    propagation_angle_yz, PFT_yz).  ValueError: an unknown key, both or neither of L0 and tau, w0 or L0 not positive."""
    unknown = set(pulse) - set(LASER_PULSE_DEFAULT)
    if unknown:
        raise ValueError(f"unknown laser pulse keys {sorted(unknown)}")
    p = dict(LASER_PULSE_DEFAULT, **pulse)
    if (p["L0"] is None) == (p["tau"] is None):
        raise ValueError("a laser pulse needs one of L0 (its length) and tau (its duration), not both and not neither")
    L0 = float(p["L0"]) if p["L0"] is not None else float(p["tau"]) * c
    pos = tuple(float(v) for v in p["position_mean"])
    if len(pos) != 3:
        raise ValueError("position_mean needs three values")
    if not (float(p["w0"]) > 0.0 and L0 > 0.0):
        raise ValueError("laser w0 and L0 must be positive")
    return (float(p["a0"]), float(p["w0"]), L0, pos, float(p["focal_distance"]), float(p["CEP"]), float(p["propagation_angle_yz"]),
            float(p["PFT_yz"]))


def laser_cell_centres(deck):
    """x (nxl), y (nyl), z (nzl) of the laser grid's cells, as the kernels compute them (i dx + xoff; slice k at the z of field slice k)"""
    import numpy as np
    nxl, nyl, zlo, zhi, lo3, hi3, dxl, dyl, xoffl, yoffl = laser_geometry(deck)
    nz, lo, hi = deck["nz"], deck["lo"], deck["hi"]
    dz = (hi[2] - lo[2]) / nz
    zoff = 0.5 * (lo[2] + hi[2] - dz * (nz - 1)) + zlo * dz
    return np.arange(nxl) * dxl + xoffl, np.arange(nyl) * dyl + yoffl, np.arange(zhi - zlo + 1) * dz + zoff


def laser_two_pulses(n=64, nz=40):
    """laser_evolution's box with the envelope on a patch of its own, a driver pulse and a weaker, tilted, off-axis second pulse
    behind it (two entries of lasers.names), in-situ reductions on."""
    d = laser_evolution()
    d.update(nx=n, ny=n, nz=nz, n_steps=2,
             laser_n_cell=(3 * n // 4, 3 * n // 4), laser_patch_lo=(-4.5, -4.5, -7.0), laser_patch_hi=(4.5, 4.5, 5.0), laser_interp_order=1,
             lasers=[dict(a0=1.0, w0=1.5, L0=1.5, position_mean=(0.0, 0.0, 1.5), focal_distance=100.0),
                     dict(a0=0.4, w0=1.2, L0=1.0, position_mean=(0.0, 0.8, -3.5), focal_distance=50.0, CEP=0.2,
                          propagation_angle_yz=0.01, PFT_yz=math.pi / 2.0 + 0.05)],
             laser_insitu=1)
    return d


def _round_half_away(v):
    return math.copysign(math.floor(abs(v) + 0.5), v)        # std::round


def laser_geometry(deck):
    """The laser grid of `deck` as the engine makes it (hps_engine_set_laser_grid): -> (nxl, nyl, zeta_lo, zeta_hi, lo3, hi3, dxl,
    dyl, xoffl, yoffl).  n_cell and the patch default to the field grid and box; zeta is snapped to whole field cells, so laser
    slice k sits at the z of field slice k; xoffl, yoffl: GetPosOffset of the laser box (position of laser cell 0).
    ValueError: an empty zeta range, a box without volume, interp_order outside 0 .. 3, odd n_cell with the multigrid solver."""
    nx, ny, nz, lo, hi = deck["nx"], deck["ny"], deck["nz"], deck["lo"], deck["hi"]
    order = deck.get("laser_interp_order", 1)
    if order is None or int(order) != order or not 0 <= order <= 3:
        raise ValueError("lasers.interp_order must be 0, 1, 2 or 3")
    n_cell = deck.get("laser_n_cell")
    nxl, nyl = (int(n_cell[0]), int(n_cell[1])) if n_cell is not None else (nx, ny)
    if nxl < 1 or nyl < 1:
        raise ValueError("lasers.n_cell must be positive")
    plo = [float(v) for v in (deck.get("laser_patch_lo") if deck.get("laser_patch_lo") is not None else lo)]
    phi = [float(v) for v in (deck.get("laser_patch_hi") if deck.get("laser_patch_hi") is not None else hi)]
    dz = (hi[2] - lo[2]) / nz
    poff_z, dz_inv = 0.5 * (lo[2] + hi[2] - dz * (nz - 1)), 1.0 / dz
    zl = max(0.0, _round_half_away((plo[2] - poff_z) * dz_inv))
    zh = min(float(nz - 1), _round_half_away((phi[2] - poff_z) * dz_inv))
    if not zl <= zh:
        raise ValueError("the laser patch holds no field slice (empty zeta range)")
    zeta_lo, zeta_hi = int(zl), int(zh)
    plo[2], phi[2] = (zeta_lo - 0.5) * dz + poff_z, (zeta_hi + 0.5) * dz + poff_z
    if not (phi[0] > plo[0] and phi[1] > plo[1] and phi[2] > plo[2]):
        raise ValueError("Laser box must have positive volume")
    dxl, dyl = (phi[0] - plo[0]) / nxl, (phi[1] - plo[1]) / nyl
    xoffl = 0.5 * (plo[0] + phi[0] - dxl * (nxl - 1))
    yoffl = 0.5 * (plo[1] + phi[1] - dyl * (nyl - 1))
    if deck.get("laser_solver", 0) == 2 and deck.get("dt", 0.0) != 0.0 and (nxl % 2 or nyl % 2):
        raise ValueError("the multigrid envelope solver needs even lasers.n_cell (cell-centred hpmg box)")
    return nxl, nyl, zeta_lo, zeta_hi, tuple(plo), tuple(phi), dxl, dyl, xoffl, yoffl


def _ne_SI(kp_inv=10.0e-6):
    wp = SI["c"] / kp_inv
    return wp ** 2 * SI["m_e"] * SI["ep0"] / SI["q_e"] ** 2


def blowout_wake_SI():
    """examples/blowout_wake/inputs_SI (run next to the normalised deck by tests/blowout_wake.2Rank.sh): the same physics
    with kp_inv = 10 um."""
    kp_inv = 10.0e-6
    ne = _ne_SI(kp_inv)
    d = blowout_wake()
    d.update(si_units=1, lo=(-8.0 * kp_inv, -8.0 * kp_inv, -6.0 * kp_inv), hi=(8.0 * kp_inv, 8.0 * kp_inv, 6.0 * kp_inv),
             beam_zmin=-59.0e-6, beam_zmax=59.0e-6, beam_radius=12.0e-6, beam_density=3.0 * ne,
             beam_pos_std=(3.0e-6, 3.0e-6, 14.1e-6), beam_charge=-SI["q_e"], beam_mass=SI["m_e"],
             plasma_density=ne, plasma_charge=-SI["q_e"], plasma_mass=SI["m_e"])
    return d


def collisions_SI(coulomb_log=-1.0, seed=0):
    """tests/collisions.SI.1Rank.sh: examples/blowout_wake/inputs_SI with hipace.collisions = collision1, collision1.species =
    plasma plasma (CoulombLog not given: computed per pair).  `collisions` is no member of hps_deck: SliceEngine turns the
    entry (species_a, species_b, CoulombLog, seed) into hps_engine_add_collision calls."""
    d = blowout_wake_SI()
    d["collisions"] = [(0, 0, coulomb_log, seed)]
    return d


def collisions_beam_SI(coulomb_log=-1.0, seed=0):
    """tests/collisions_beam.SI.1Rank.sh: examples/blowout_wake/inputs_SI with hipace.collisions = collision1, collision1.species =
    beam plasma, max_step = 0 and no hipace.dt: the beam is static, the collision's dt is 0 and no pair scatters.  The entry
    ("beam", plasma species, CoulombLog, seed) reaches hps_engine_add_beam_collision through the SliceEngine constructor."""
    d = blowout_wake_SI()
    d["n_steps"] = 1
    d["collisions"] = [("beam", 0, coulomb_log, seed)]
    return d


def linear_wake_SI():
    """tests/linear_wake.SI.1Rank.sh (examples/linear_wake/inputs_SI + rho)."""
    d = linear_wake()
    ne = _ne_SI()
    d.update(si_units=1, lo=(-100.0e-6, -100.0e-6, -75.0e-6), hi=(100.0e-6, 100.0e-6, 20.0e-6),
             beam_zmin=-10.0e-6, beam_zmax=10.0e-6, beam_radius=30.0e-6, beam_density=0.01 * ne,
             beam_charge=-SI["q_e"], beam_mass=SI["m_e"], plasma_density=ne, plasma_charge=-SI["q_e"], plasma_mass=SI["m_e"])
    return d


def gaussian_linear_wake():
    """tests/gaussian_linear_wake.normalized.1Rank.sh: the linear_wake deck with a wide Gaussian beam (+ rho)"""
    d = linear_wake()
    d.update(beam_profile=0, beam_zmin=-5.9, beam_zmax=5.9, beam_radius=10.0, beam_pos_mean=(0.0, 0.0, 0.0), beam_pos_std=(2.0, 2.0, 1.41),
             lo=(-10.0, -10.0, -6.0), hi=(10.0, 10.0, 6.0), deposit_rho=1)
    return d


def gaussian_linear_wake_SI():
    """tests/gaussian_linear_wake.SI.1Rank.sh: the same in SI units (examples/linear_wake/inputs_SI)"""
    d = linear_wake_SI()
    d.update(beam_profile=0, beam_zmin=-59.0e-6, beam_zmax=59.0e-6, beam_radius=100.0e-6, beam_pos_mean=(0.0, 0.0, 0.0),
             beam_pos_std=(20.0e-6, 20.0e-6, 14.1e-6), lo=(-100.0e-6, -100.0e-6, -60.0e-6), hi=(100.0e-6, 100.0e-6, 60.0e-6), deposit_rho=1)
    return d


def radiation_reaction():
    """examples/beam_in_vacuum/inputs_RR (tests/radiation_reaction.1Rank.sh) in normalised units (n0 = 5e24 m^-3): a
    gamma = 2000 beam in the linear focusing field E = (x/2, y/2, 0) of a blowout, no z push, 50 sub-cycles, steps of
    30 / omega_beta; the beam comes from fixed_ppc (flat top of radius 2.5 / kp, at rest transversely) instead of the
    reference's random Gaussian."""
    d = beam_evolution()
    w_beta = 1.0 / (2.0 * 2000.0) ** 0.5
    d.update(nx=32, ny=32, nz=10, lo=(-12.6, -12.6, -4.2), hi=(12.6, 12.6, 4.2), beam_profile=1, beam_zmin=-2.0, beam_zmax=2.0,
             beam_radius=2.5, beam_density=1.0e-10, beam_umean=(0.0, 0.0, 2000.0), beam_ppc=(2, 2, 1), ext_E_slope=(0.5, 0.5),
             dt=30.0 / w_beta, n_steps=6, beam_n_subcycles=50, beam_radiation_reaction=1, background_density_SI=5.0e24,
             beam_no_z_push=1)
    return d


def beam_in_vacuum_1Rank():
    """tests/beam_in_vacuum.normalized.1Rank.sh: as the Serial run with hipace.MG_tolerance_rel = 1e-5."""
    d = beam_in_vacuum()
    d.update(mg_tol_rel=1.0e-5)
    return d


def beam_in_vacuum_SI():
    """tests/beam_in_vacuum.SI.1Rank.sh (examples/beam_in_vacuum/inputs_SI, order 0, MG_tolerance_rel = 1e-5).  The deck
    has two identical beams on top of each other; one beam of twice the density deposits the same currents."""
    d = beam_in_vacuum()
    d.update(si_units=1, lo=(-2000.0e-6, -2000.0e-6, -20.0e-6), hi=(2000.0e-6, 2000.0e-6, 20.0e-6),
             beam_zmin=-100.0e-6, beam_zmax=100.0e-6, beam_radius=10.0e-6, beam_density=2 * 1.4119793504295784e23,
             beam_charge=-SI["q_e"], beam_mass=SI["m_e"], mg_tol_rel=1.0e-5, order=0)
    return d


def grid_current():
    """tests/grid_current.1Rank.sh: the beam_in_vacuum deck at 32^3, order 0, a Gaussian beam of density 0.2 and a grid
    current (grid_current.*, utils/GridCurrent.cpp) of the same shape, which cancels most of the beam's current"""
    d = beam_in_vacuum()
    d.update(nx=32, ny=32, nz=32, lo=(-8.0, -8.0, -6.0), hi=(8.0, 8.0, 6.0), n_steps=2, order=0, beam_profile=0, beam_density=0.2,
             beam_radius=1.0, beam_pos_mean=(0.0, 0.0, 0.0), beam_pos_std=(0.3, 0.3, 1.41), beam_ppc=(1, 1, 1),
             grid_current_on=1, grid_current_peak=0.2, grid_current_mean=(0.0, 0.0, 0.0), grid_current_std=(0.3, 0.3, 1.41))
    return d


def salame_grid_current(zmin=-1.4, zmax=0.78, density=0.5):
    """The SALAME test deck (<beam>.do_salame behind a grid_current.* driver; salame/Salame.cpp): explicit solver, order 2,
    64 x 64 cells over +-8, 100 slices over z in [-8, 6] (dz = 0.14), plasma 2 x 2 ppc, MG_tolerance_rel = 1e-10.  Driver: a
    Gaussian grid current of peak -0.5 (electron-like) at z = 3, sigma (0.5, 0.5, 1).  Witness: a flat-top fixed_ppc electron
    beam of radius 0.3 with u = (0, 0, 2000) exactly (jx_beam = jy_beam = 0), 4 x 4 x 1 ppc, z in [zmin, zmax) = slices 47 .. 62 (length 2.2).

    Placement, from the CPU oracle's run of the deck without the witness (on-axis Ez, mean of the four central cells):
        z      5.23   3.83   2.43   1.31   0.75   0.47   0.19  -0.37  -0.65  -0.93  -1.49  -1.77  -2.05  -2.61  -3.17
        Ez    0.003  0.045  0.084  0.001 -0.061 -0.092 -0.120 -0.162 -0.171 -0.167 -0.110 -0.056  0.009  0.123  0.171
    The head (slice 62, z = 0.75) sits where Ez = -0.061 < 0; over the witness the unloaded Ez goes to -0.171 and back to
    -0.13, a change of 180 % of the head value.  Ez changes sign at z = -2.0: `salame_grid_current_overload` reaches past it.
    On the MI355X SALAME scales the slices' weights by 3.2 (head), 4.3 (third slice), then almost linearly down to 0.83 (slice
    47): W > 0 everywhere.  The same witness would run out of wake at slice 44; a head at z = 0.47 does so 12 slices in.
    """
    d = copy.deepcopy(_DEFAULT)
    d.update(SALAME_DEFAULT)
    d.update(nx=64, ny=64, nz=100, lo=(-8.0, -8.0, -8.0), hi=(8.0, 8.0, 6.0), order=2, plasma_ppc=(2, 2), mg_tol_rel=1.0e-10, n_steps=1,
             grid_current_on=1, grid_current_peak=-0.5, grid_current_mean=(0.0, 0.0, 3.0), grid_current_std=(0.5, 0.5, 1.0),
             beam_profile=1, beam_zmin=zmin, beam_zmax=zmax, beam_radius=0.3, beam_density=density, beam_umean=(0.0, 0.0, 2000.0),
             beam_pos_mean=(0.0, 0.0, 0.0), beam_ppc=(4, 4, 1), beam_charge=-1.0, beam_do_salame=1)
    return d


def salame_grid_current_overload():
    """`salame_grid_current` with the witness reaching to z = -3.0 (slice 36), past the point (z = -2.0) where the unloaded Ez changes
    sign: no positive weight holds the target there, W < 0 must occur and the rest of the witness is dropped."""
    return salame_grid_current(zmin=-3.0)


def salame_grid_current_moving(zmin=-1.4, zmax=0.78, density=0.5, dt=0.1):
    """`salame_grid_current` in a moving-beam engine (hipace.dt = dt != 0): the deck's own beam is empty (beam_profile
    = -1) behind the same grid current, and the same witness -- the flat top written as <beam>.density(x,y,z) = n0 for the device's
    fixed_ppc generator, which takes the deck's window beam_zmin / beam_zmax / beam_radius, beam_ppc and beam_umean -- is species 1
    with do_salame.  beam_do_salame = 0, beam_species_salame = 1 (SALAME_SPECIES_DEFAULT)."""
    d = salame_grid_current(zmin=zmin, zmax=zmax, density=density)
    d.update(SALAME_SPECIES_DEFAULT)
    d.update(beam_profile=-1, beam_do_salame=0, beam_species_salame=1, dt=dt)
    d["beam_name"] = "driver"
    d["beam_species"] = [dict(name="witness", do_salame=1, density_expr="n0", constants=dict(n0=float(density)))]
    return d


def salame_grid_current_moving_overload():
    """the moving twin of `salame_grid_current_overload`"""
    return salame_grid_current_moving(zmin=-3.0)


SALAME_WITNESS_DENSITY = "if(z < zw, 1, 0)*if(x*x + y*y < rw*rw, n0, 0)"


def salame_driver_witness(zmin=-1.4, zmax=0.78, density=0.5, dt=0.1, driver_zmax=5.94, driver_radius=2.0):
    """A particle driver and a do_salame witness in one moving-beam engine, the case SALAME was written for: the box,
    the plasma and the witness of `salame_grid_current_moving`, the grid current off.  The driver is the deck's own Gaussian beam
    with the grid current's shape -- electrons, peak density 0.5, centre z = 3, sigma (0.5, 0.5, 1), u = (0, 0, 2000) -- cut at
    driver_radius = 2 (four sigma) and at z in [zmin, driver_zmax): finite beam_zmin / beam_zmax.  The fixed_ppc generators of both
    species share the deck's window and beam_ppc, so the window spans both and the witness's flat top (radius 0.3, z in [zmin,
    zmax)) is written into its density: SALAME_WITNESS_DENSITY with min_density = n0 / 2.  At the witness head (z = 0.78) the
    driver's own density is 0.5 exp(-2.46) = 0.043, at its tail 3e-5: the driver's tail overlaps the witness, as a grid current's.

    Placement, from the CPU oracle's run of the driver alone (static, no witness; on-axis Ez, mean of the four central cells):
        z      5.23   3.83   2.43   1.31   0.75   0.47   0.19  -0.37  -0.65  -0.93  -1.35  -1.77  -2.05  -2.61  -3.17
        Ez    0.003  0.040  0.083  0.008 -0.053 -0.084 -0.113 -0.156 -0.166 -0.165 -0.135 -0.066 -0.005  0.111  0.165
    The head (slice 62, z = 0.75) sits where Ez = -0.053 < 0; over the witness (down to slice 47, z = -1.35) the unloaded Ez goes
    to -0.167 (z = -0.79) and back to -0.135 without changing sign -- that happens at z = -2.07, past the witness: the table of
    `salame_grid_current` to a tenth, so the witness stays where it is.
    """
    d = salame_grid_current_moving(zmin=zmin, zmax=zmax, density=density, dt=dt)
    d.update(grid_current_on=0, grid_current_peak=0.0, beam_profile=0, beam_density=0.5, beam_pos_mean=(0.0, 0.0, 3.0),
             beam_pos_std=(0.5, 0.5, 1.0), beam_zmin=zmin, beam_zmax=driver_zmax, beam_radius=driver_radius, beam_charge=-1.0,
             beam_umean=(0.0, 0.0, 2000.0))
    d["beam_species"] = [dict(name="witness", do_salame=1, density_expr=SALAME_WITNESS_DENSITY, min_density=0.5 * float(density),
                              constants=dict(n0=float(density), zw=float(zmax), rw=0.3))]
    return d


def salame_grid_current_SI(**kw):
    """`salame_grid_current` scaled to SI units with kp_inv = 10 um, as the project's other SI twins are."""
    kp_inv = 10.0e-6
    ne = _ne_SI(kp_inv)
    E0 = SI["m_e"] * SI["c"] ** 2 / (SI["q_e"] * kp_inv)        # cold wave-breaking field m c wp / e
    d = salame_grid_current(**kw)
    sc = lambda v: tuple(x * kp_inv for x in v)
    d.update(si_units=1, lo=sc(d["lo"]), hi=sc(d["hi"]), plasma_density=ne, plasma_charge=-SI["q_e"], plasma_mass=SI["m_e"],
             beam_zmin=d["beam_zmin"] * kp_inv, beam_zmax=d["beam_zmax"] * kp_inv, beam_radius=d["beam_radius"] * kp_inv,
             beam_density=d["beam_density"] * ne, beam_charge=-SI["q_e"], beam_mass=SI["m_e"],
             grid_current_peak=d["grid_current_peak"] * ne * SI["q_e"] * SI["c"], grid_current_mean=sc(d["grid_current_mean"]),
             grid_current_std=sc(d["grid_current_std"]), salame_Ez_target_slope=d["salame_Ez_target_slope"] * E0 / kp_inv)
    return d


def beam_in_vacuum_SI_Serial():
    """tests/beam_in_vacuum.SI.Serial.sh: the SI deck with the multigrid solver's default tolerance."""
    d = beam_in_vacuum_SI()
    d.update(mg_tol_rel=beam_in_vacuum()["mg_tol_rel"])
    return d


def reset():
    """tests/reset.2Rank.sh: the blowout deck for three time steps (max_step = 2, dt = 0) with MG_tolerance_rel = 1e-5"""
    d = blowout_wake()
    d.update(n_steps=3, mg_tol_rel=1.0e-5)
    return d


def blowout_wake_step0():
    """tests/blowout_wake.Serial.sh: examples/blowout_wake/inputs_normalized as it stands (max_step = 0: one time step)."""
    d = blowout_wake()
    d["n_steps"] = 1
    return d


def predictor_corrector(base, tol=1.0e-4, max_iter=7, mix=0.0635):
    """`base` with hipace.bxby_solver = predictor-corrector; the defaults are the settings of the reference's own
    predictor-corrector-vs-explicit test (tests/ion_motion.SI.1Rank.sh:30-34)."""
    d = copy.deepcopy(base)
    d.update(bxby_solver=1, predcorr_tol=tol, predcorr_max_iter=max_iter, predcorr_mix=mix)
    return d


NAMED = dict(radiation_reaction=radiation_reaction, gaussian_linear_wake=gaussian_linear_wake, gaussian_linear_wake_SI=gaussian_linear_wake_SI, reset=reset, grid_current=grid_current, beam_in_vacuum_SI_Serial=beam_in_vacuum_SI_Serial, blowout_wake_step0=blowout_wake_step0, linear_wake_gaussian=linear_wake_gaussian, laser_blowout_wake=laser_blowout_wake, laser_blowout_wake_SI=laser_blowout_wake_SI, linear_wake_SI=linear_wake_SI, blowout_wake_SI=blowout_wake_SI, beam_in_vacuum_SI=beam_in_vacuum_SI, beam_in_vacuum_1Rank=beam_in_vacuum_1Rank, blowout_wake=blowout_wake, linear_wake=linear_wake, beam_in_vacuum=beam_in_vacuum,
             beam_evolution=beam_evolution, beam_in_vacuum_open_boundary=beam_in_vacuum_open_boundary)


def ionization_SI():
    """examples/blowout_wake/inputs_ionization_SI as tests/ionization.2Rank.sh runs it (hipace.dt = 1e-12, max_step = 2):
    neutral hydrogen (one macro-atom per cell), no electrons to begin with (elec.ppc = 0 0), a flat-top driver whose field
    ionises the gas; the released electrons form the wake."""
    ne = 1.25e24
    c, ep0, q_e, m_e = 299792458.0, 8.8541878128e-12, 1.602176634e-19, 9.1093837015e-31
    kp_inv = c / (ne * q_e * q_e / (ep0 * m_e)) ** 0.5
    d = copy.deepcopy(_DEFAULT)
    d.update(nx=64, ny=64, nz=100, lo=(-20.0e-6, -20.0e-6, -30.0e-6), hi=(20.0e-6, 20.0e-6, 30.0e-6), order=2, si_units=1,
             plasma_ppc=(0, 0), plasma_density=ne, plasma_charge=-q_e, plasma_mass=m_e, plasma_no_neutralize=1,
             beam_profile=1, beam_zmin=25.0e-6 - 2.0 * kp_inv, beam_zmax=25.0e-6, beam_radius=kp_inv / 2.0, beam_density=4.0 * ne,
             beam_umean=(0.0, 0.0, 2000.0), beam_ppc=(1, 1, 1), beam_charge=-q_e, beam_mass=m_e,
             n_steps=3, dt=1.0e-12, bc=1)
    return with_ion_species(d, "H", ne, ppc=(1, 1), mass_Da=1.008, initial_level=0)


def ion_motion_SI(nz=200):
    """examples/linear_wake/inputs_ion_motion_SI (tests/ion_motion.SI.1Rank.sh): electrons and MOBILE ions (mass 5 m_e "for
    testing", one particle per cell each, no neutralising background for either) behind an off-axis driver.  The ions are
    the second species at its top level (hydrogen, level 1 of 1: nothing left to ionise).  The reference's driver is a
    fixed_weight Gaussian drawn from amrex::Random; here a flat-top of the same peak density, length and offset (the
    deck pins the two-species push and deposition, not the beam's random positions)."""
    c, ep0, q_e, m_e = 299792458.0, 8.8541878128e-12, 1.602176634e-19, 9.1093837015e-31
    kp_inv = 10.0e-6
    ne = (c / kp_inv) ** 2 * m_e * ep0 / (q_e * q_e)
    d = copy.deepcopy(_DEFAULT)
    d.update(nx=64, ny=64, nz=nz, lo=(-8 * kp_inv, -8 * kp_inv, -6 * kp_inv), hi=(8 * kp_inv, 8 * kp_inv, 6 * kp_inv), order=2, si_units=1,
             plasma_ppc=(1, 1), plasma_density=ne, plasma_charge=-q_e, plasma_mass=m_e, plasma_no_neutralize=1,
             beam_profile=1, beam_zmin=0.6 * kp_inv, beam_zmax=3.4 * kp_inv, beam_radius=0.8 * kp_inv, beam_density=ne,
             beam_pos_mean=(0.25 * kp_inv, 0.0, 2.0 * kp_inv), beam_umean=(10.0, 20.0, 100.0), beam_ppc=(1, 1, 1), beam_charge=-q_e, beam_mass=m_e,
             n_steps=1, dt=0.0, bc=1)
    with_ion_species(d, "H", ne, ppc=(1, 1), initial_level=1)
    d["ion_mass"] = 5.0 * m_e
    return d


def blowout_wake_three_species(nz=24, dopant="N", dopant_density=0.1, background_density_SI=1.0e24):
    """Three plasma species in one engine: the blowout wake's electrons (species 0, no neutralising background),
    a neutral dopant that the wake's field ionises (species 1, "ion": ADK, its electrons join species 0) and mobile hydrogen
    ions in the electrons' place of a background (species 2, "H_ion": fixed charge +1, 1836.15 electron masses, one particle
    per cell on the electrons' lattice, so that the two cancel ahead of the driver).  A flat-top driver that leaves the head
    of the box empty; rho is deposited."""
    d = copy.deepcopy(_DEFAULT)
    d.update(nz=nz, lo=(-8.0, -8.0, -6.0), hi=(8.0, 8.0, 6.0), plasma_no_neutralize=1, deposit_rho=1, n_steps=1,
             beam_profile=1, beam_zmin=-4.0, beam_zmax=4.0, beam_radius=1.2, beam_density=3.0,
             background_density_SI=background_density_SI)
    with_ion_species(d, dopant, dopant_density, ppc=(1, 1), initial_level=0, seed=7)
    d["plasma_species"] = [dict(name="H_ion", charge=1.0, mass=1836.15267343, density=d["plasma_density"], ppc=(1, 1),
                                neutralize_background=False)]
    return d


def laser_ionization_SI():
    """BASELINE config 5 at test size: the laser-driven wake of tests/laser_blowout_wake_explicit.SI.1Rank.sh in a gas that
    also holds neutral nitrogen (a fifth of the electron density, one macro-atom per cell) -- the wake's field ionises the
    atoms it reaches (ADK), the released electrons join the plasma electrons.  Neutral atoms and electron + ion pairs
    carry no net charge, so the pre-formed plasma stays neutralised by its own background."""
    d = laser_blowout_wake_SI()
    return with_ion_species(d, "N", 0.2 * d["plasma_density"], ppc=(1, 1), initial_level=0, seed=5)


def transverse_benchmark(nxy=1023, nz=1000):
    """examples/benchmarks/inputs_transverse_benchmark as tests/transverse_benchmark.1Rank.sh runs it (my_constants.nxy = 1023):
    the reference's own transverse scaling benchmark -- 2^N - 1 cells per side, 1000 slices, one plasma electron per cell,
    absorbing particle boundary, explicit solver.  Its driver is a fixed_weight_pdf beam of 10 nxy^2 particles drawn from
    amrex::Random: the deck carries no beam (beam_profile = -1), the host hands one in with
    SliceEngine.set_beam_particles(fixed_weight_pdf_beam(deck, **TRANSVERSE_BENCHMARK_BEAM(nxy)))."""
    d = copy.deepcopy(_DEFAULT)
    d.update(nx=nxy, ny=nxy, nz=nz, lo=(-6.0, -6.0, -12.0), hi=(6.0, 6.0, 6.0), order=2, plasma_ppc=(1, 1), plasma_density=1.0,
             beam_profile=-1, bc=2, n_steps=1, dt=0.0)
    return d


def TRANSVERSE_BENCHMARK_BEAM(nxy=1023):
    import numpy as np
    return dict(num_particles=nxy * nxy * 10, density=2.0, pdf=lambda z: np.exp(-0.5 * (z / 1.41) ** 2), pos_std=(0.3, 0.3),
                u_mean=(0.0, 0.0, 2000.0))


def TRANSVERSE_BENCHMARK_BEAM_PARSED(nxy=1023):
    """The same driver as the file writes it, for the device: with_fixed_weight_pdf_beam(transverse_benchmark(nxy),
    **TRANSVERSE_BENCHMARK_BEAM_PARSED(nxy)) or SliceEngine.set_beam_fixed_weight_pdf(**...)."""
    return dict(num_particles=nxy * nxy * 10, density=2.0, pdf="exp(-0.5*(z/1.41)^2)", position_mean=(0.0, 0.0), position_std=(0.3, 0.3),
                u_mean=(0.0, 0.0, 2000.0), u_std=(0.0, 0.0, 0.0))


def timestep_benchmark_beam(num_particles=268_000_000_000):
    """examples/benchmarks/inputs_timestep_benchmark's proton driver (normalised units, beam1.element = proton: the deck's
    beam_charge and beam_mass) as the arguments of SliceEngine.set_beam_fixed_weight_pdf: the Gaussian current profile cut at
    4 sigma_z by two comparisons, widths and momentum spreads from my_constants.  The file's 268e9 particles are more draws than
    one engine takes (2^32): a run gives its own num_particles.  The file's box in z ends where the window does, at
    -+4 sigma_z kp, so both end edges carry no weight."""
    constants = dict(n0=9.38e20, wp="sqrt( n0 * q_e^2 / (m_e *epsilon0) )", kp="wp/clight",
                     nb="43e-9 /q_e / ( (2*pi)^(3/2) *sigma_x * sigma_y * sigma_z * n0 )", sigma_x=0.45e-3, sigma_y=0.54e-3,
                     sigma_z=0.049, emittance=2.5e-6)
    return dict(num_particles=int(num_particles), density="nb",
                pdf="exp(-0.5*(z/(sigma_z*kp))^2)*(z > -4*sigma_z*kp)*(z < 4*sigma_z*kp)", position_mean=(0.0, 0.0),
                position_std=("sigma_x*kp", "sigma_y*kp"), u_mean=(0.0, 0.0, "400/0.938+1"),
                u_std=("emittance/sigma_x", "emittance/sigma_y", 0.003499), constants=constants)


def fixed_weight_pdf_beam(deck, num_particles, density, pdf, pos_mean=(0.0, 0.0), pos_std=(1.0, 1.0), u_mean=(0.0, 0.0, 0.0),
                          u_std=(0.0, 0.0, 0.0), seed=0, pdf_ref_ratio=4):
    """beam.injection_type = fixed_weight_pdf with a peak density (InitBeamFixedWeightPDF3D / ...PDFSlice,
    particles/beam/BeamParticleContainerInit.cpp:479-695), on the host: the longitudinal profile `pdf(z)` (vectorised
    callable) is integrated by the trapezoidal rule on nz * pdf_ref_ratio sub-slices (:502-528), the total weight is
    density * integral / max_density with max_density = max local_weight / (dz_sub * sigma_x * sigma_y * 2 pi) (:514-531), in
    normalised units over the cell volume (:540-542); every particle carries total / num_particles (:618).  The particle
    count of a sub-slice is drawn in proportion to its share of the integral (the reference iterates Poisson draws until
    the total is num_particles, :546-579 -- a multinomial draw here), z inside a sub-slice follows the linear profile
    between its two ends (:645-652), x, y and u are normal (:663-670).  numpy's generator stands in for amrex::Random: the
    beam is the reference's in distribution, not particle by particle.
    -> (7, num_particles) array x y z ux uy uz w in the engine's units (u times c; AddOneBeamParticleSlice, :86-116)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    nz = deck["nz"]
    lo, hi = deck["lo"], deck["hi"]
    dx, dy, dz = (hi[0] - lo[0]) / deck["nx"], (hi[1] - lo[1]) / deck["ny"], (hi[2] - lo[2]) / nz
    c = 299792458.0 if deck.get("si_units", 0) else 1.0
    ns = nz * pdf_ref_ratio
    zs = dz / pdf_ref_ratio
    edges = lo[2] + zs * np.arange(ns + 1)
    pe = np.asarray(pdf(edges), dtype=np.float64)
    assert (pe >= 0.0).all(), "PDF must be >= 0 everywhere"
    lw = 0.5 * (pe[:-1] + pe[1:])
    integral = lw.sum()
    max_density = (lw / (zs * pos_std[0] * pos_std[1] * 2.0 * np.pi)).max()
    total_weight = density * integral / max_density
    if not deck.get("si_units", 0):
        total_weight /= dx * dy * dz
    counts = rng.multinomial(num_particles, lw / integral)
    sub = np.repeat(np.arange(ns), counts)
    w01 = rng.random(num_particles)
    lo_w, hi_w = pe[:-1][sub], pe[1:][sub]
    taylor = np.minimum(lo_w, hi_w) * 1.1 > np.maximum(lo_w, hi_w)
    with np.errstate(divide="ignore", invalid="ignore"):
        z_t = w01 - w01 * (w01 - 1.0) * (hi_w - lo_w) / (hi_w + lo_w)
        z_s = (np.sqrt(lo_w * lo_w + w01 * (hi_w * hi_w - lo_w * lo_w)) - lo_w) / (hi_w - lo_w)
    z = edges[:-1][sub] + zs * np.where(taylor, z_t, z_s)
    out = np.empty((7, num_particles))
    out[0] = pos_mean[0] + rng.normal(0.0, pos_std[0], num_particles)
    out[1] = pos_mean[1] + rng.normal(0.0, pos_std[1], num_particles)
    out[2] = z
    for k in range(3):
        out[3 + k] = (u_mean[k] + (rng.normal(0.0, u_std[k], num_particles) if u_std[k] else 0.0)) * c
    out[6] = abs(total_weight / num_particles)
    return out


def fixed_weight_beam(deck, num_particles, density, pos_mean, pos_std, u_mean=(0.0, 0.0, 0.0), u_std=(0.0, 0.0, 0.0),
                      zmin=-float("inf"), zmax=float("inf"), radius=float("inf"), seed=0, total_charge=None, do_symmetrize=False,
                      duz_per_uz0_dzeta=0.0):
    """beam.injection_type = fixed_weight, profile = gaussian, with a peak density (BeamParticleContainer.cpp:137-198,
    InitBeamFixedWeight3D / InitBeamFixedWeightSlice, BeamParticleContainerInit.cpp:350-477), on the host: z is normal about
    pos_mean[2] (:375-377), x and y are normal about pos_mean[0](z), pos_mean[1](z) -- numbers or vectorised callables of z
    (:435-454) --, every particle carries density (2 pi)^(3/2) sigma_x sigma_y sigma_z / num_particles, in normalised units
    over the cell volume (BeamParticleContainer.cpp:179-190, :420).  Particles outside [zmin, zmax] or the radius are invalid
    in the reference (:443-446): left out here; particles outside the box are left out by set_beam_particles.  numpy's
    generator stands in for amrex::Random.  -> (7, n <= num_particles) array x y z ux uy uz w, u times c.
    do_symmetrize: num_particles / 4 draws, each placed four times at (+-x, +-y) about the mean with (+-ux, +-uy) (:457-470);
    duz_per_uz0_dzeta: uz += (z - z_mean) duz_per_uz0_dzeta u_mean[2] (GetInitialMomentum.H:47)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    lo, hi = deck["lo"], deck["hi"]
    dx, dy, dz = (hi[0] - lo[0]) / deck["nx"], (hi[1] - lo[1]) / deck["ny"], (hi[2] - lo[2]) / deck["nz"]
    c = 299792458.0 if deck.get("si_units", 0) else 1.0
    if total_charge is not None:          # <beam>.total_charge (SI units only, BeamParticleContainer.cpp:167-172): density is not read
        assert deck.get("si_units", 0) and density is None
        weight = abs(total_charge / deck["beam_charge"]) / num_particles
    else:
        weight = density * (2.0 * np.pi) ** 1.5 * pos_std[0] * pos_std[1] * pos_std[2] / num_particles
    if not deck.get("si_units", 0):
        weight /= dx * dy * dz
    nd = num_particles // 4 if do_symmetrize else num_particles
    assert not do_symmetrize or num_particles % 4 == 0, "to symmetrize the beam its particle number must be divisible by 4"
    z = rng.normal(pos_mean[2], pos_std[2], nd)
    x = rng.normal(0.0, pos_std[0], nd)
    y = rng.normal(0.0, pos_std[1], nd)
    ok = (z >= zmin) & (z <= zmax) & (x * x + y * y <= radius * radius)
    mx = pos_mean[0](z) if callable(pos_mean[0]) else pos_mean[0]
    my = pos_mean[1](z) if callable(pos_mean[1]) else pos_mean[1]
    u = [u_mean[k] + (rng.normal(0.0, u_std[k], nd) if u_std[k] else np.zeros(nd)) for k in range(3)]
    u[2] = u[2] + (z - pos_mean[2]) * duz_per_uz0_dzeta * u_mean[2]
    parts = []
    for sx, sy in (((1, 1), (-1, 1), (1, -1), (-1, -1)) if do_symmetrize else ((1, 1),)):
        o = np.empty((7, nd))
        o[0], o[1], o[2] = mx + sx * x, my + sy * y, z
        o[3], o[4], o[5] = sx * u[0] * c, sy * u[1] * c, u[2] * c
        o[6] = abs(weight)
        parts.append(o[:, ok])
    return np.ascontiguousarray(np.concatenate(parts, axis=1))


def ion_motion_SI_reference_beam(deck, seed=1):
    """the driver of examples/linear_wake/inputs_ion_motion_SI: fixed_weight, 10^6 particles, peak density ne, a Gaussian of
    (0.4, 0.4, 1.41) kp^-1 about (0.25 kp^-1, 0.2 (z - 2 kp^-1), 2 kp^-1), u = (10, 20, 100)"""
    kp_inv = 10.0e-6
    return fixed_weight_beam(deck, 1000000, deck["plasma_density"], (0.25 * kp_inv, lambda z: (z - 2.0 * kp_inv) * 0.2, 2.0 * kp_inv),
                             (0.4 * kp_inv, 0.4 * kp_inv, 1.41 * kp_inv), u_mean=(10.0, 20.0, 100.0), seed=seed)


def production_lwfa(n=64, nz=100, max_step=10):
    """examples/get_started/inputs_lwfa as tests/production.SI.2Rank.sh runs it (amr.n_cell = 64 64 100, max_step = 10): a laser
    pulse (a0 = 1.9, w0 = 3 kp^-1, L0 = 0.5 kp^-1, multigrid envelope solver, MG_tolerance_rel = 1e-5) enters a parabolic plasma
    channel of radius 23 kp^-1 through a cosine up-ramp of 6 mm, steps of c dt = 10 kp^-1, SI units, ne = 1.0505e23 m^-3.
    The density function n_e (1 + 4 r^2 / (kp^2 Rm^4)) ramp(c t) [c t > 0] is the engine's tabulated form f_r(r) f_t(c t):
    -> (deck with plasma_radius, (r, fr, ct, ft)) for SliceEngine.set_density_profile -- the radial table on the lattice's own
    radii (exact at every particle), the time table on the steps' own times."""
    import numpy as np
    ne = 1.0505e23
    wp = (ne * SI["q_e"] ** 2 / (SI["m_e"] * SI["ep0"])) ** 0.5
    kp_inv = SI["c"] / wp
    kp = wp / SI["c"]
    Rm, Lramp = 3.0 * kp_inv, 6.0e-3
    d = copy.deepcopy(_DEFAULT)
    d.update(nx=n, ny=n, nz=nz, lo=(-18.0 * kp_inv, -18.0 * kp_inv, -7.5 * kp_inv), hi=(18.0 * kp_inv, 18.0 * kp_inv, 1.5 * kp_inv),
             order=2, si_units=1, plasma_ppc=(1, 1), plasma_density=ne, plasma_charge=-SI["q_e"], plasma_mass=SI["m_e"],
             beam_profile=-1, bc=1, n_steps=max_step + 1, dt=10.0 * kp_inv / SI["c"],
             laser_on=1, laser_a0=1.9, laser_w0=3.0 * kp_inv, laser_L0=0.5 * kp_inv, laser_lambda0=800.0e-9, laser_pos=(0.0, 0.0, 0.0),
             laser_solver=2, laser_mg_tol_rel=1.0e-5)
    dx = (d["hi"][0] - d["lo"][0]) / n
    xs = d["lo"][0] + (np.arange(n) + 0.5) * dx
    r2 = np.unique(np.add.outer(xs * xs, xs * xs).round(decimals=22))
    r = np.sqrt(r2)
    d["plasma_radius"] = 23.0 * kp_inv                   # plasma.radius: no particles in the box's corners
    r_tab = r
    fr = 1.0 + 4.0 * r_tab ** 2 / (kp ** 2 * Rm ** 4)
    if r_tab[0] > 0.0:
        r_tab = np.concatenate([[0.0], r_tab]); fr = np.concatenate([[1.0], fr])
    ct = np.array([SI["c"] * d["dt"] * k for k in range(max_step + 2)])
    ft = np.where(ct > 0.0, np.where(ct > Lramp, 1.0, 0.5 * (1.0 - np.cos(np.pi * ct / Lramp))), 0.0)
    return d, (r_tab, fr, ct, ft)


# examples/get_started/inputs_lwfa: my_constants as the file writes them (they resolve through one another), and
# plasma.density(x,y,z) with the line breaks of the file's quoted value
LWFA_CONSTANTS = dict(kp_inv="clight/wp", kp="wp/clight", wp="sqrt( ne * q_e^2/(m_e *epsilon0) )", ne=1.0505e23, Rm="3*kp_inv",
                      Lramp=6.e-3)
LWFA_DENSITY = ("ne*(1+4*(x^2+y^2)/(kp^2 * Rm^4 ) ) *\n"
                "                         if (z > Lramp, 1, .5*(1-cos(pi*z/Lramp))) *\n"
                "                         if (z>0,1,0)")


def production_pwfa(nxy=64, nz=100, n_steps=11, seed=1):
    """examples/get_started/inputs_pwfa as tests/production.SI.2Rank.sh runs it (amr.n_cell = 64 64 100, max_step = 10): SI units,
    electrons and mobile hydrogen ions of 2e22 m^-3 (one particle per cell each, neither with a neutralising background), two
    fixed_weight electron beams of 10^6 particles with do_symmetrize -- the driver (0.6 nC, sigma 2, 2, 30 um about z = 0) as the
    deck's beam, the witness (0.2 nC, sigma 2, 2, 5 um about z = -160 um) as the one entry of beam_species --, hipace.dt =
    adaptive with nt_per_betatron = 30 and max_time = 0.3 / c.  seed: the driver's draws; the witness takes seed + 1000."""
    um = 1.0e-6
    d = copy.deepcopy(_DEFAULT)
    d.update(ADAPTIVE_DEFAULT)
    ne = 2.0e22
    d.update(nx=nxy, ny=nxy, nz=nz, lo=(-250.0 * um, -250.0 * um, -250.0 * um), hi=(250.0 * um, 250.0 * um, 110.0 * um), order=2,
             si_units=1, plasma_ppc=(1, 1), plasma_density=ne, plasma_charge=-SI["q_e"], plasma_mass=SI["m_e"], plasma_no_neutralize=1,
             beam_profile=-1, beam_charge=-SI["q_e"], beam_mass=SI["m_e"], beam_umean=(0.0, 0.0, 1000.0), beam_uz_std=10.0,
             bc=1, n_steps=n_steps, dt=0.0, dt_adaptive=1, nt_per_betatron=30.0, max_time=0.3 / SI["c"])
    with_ion_species(d, "H", ne, ppc=(1, 1), initial_level=1)
    beam = dict(num_particles=1000000, position_std=(2.0 * um, 2.0 * um, 30.0 * um), position_mean=(0.0, 0.0, 0.0),
                u_mean=(0.0, 0.0, 1000.0), u_std=(2.0, 2.0, 10.0), total_charge=0.6e-9, do_symmetrize=True, seed=int(seed))
    d["beam_name"] = "driver"
    d["beam_fixed_weight"] = beam
    d["beam_species"] = [dict(name="witness", fixed_weight=dict(beam, position_mean=(0.0, 0.0, -160.0 * um),
                                                                 position_std=(2.0 * um, 2.0 * um, 5.0 * um), total_charge=0.2e-9,
                                                                 seed=int(seed) + 1000))]
    return d


def production_lwfa_parsed(n=64, nz=100, max_step=10):
    """production_lwfa() with the density as examples/get_started/inputs_lwfa writes it: plasma.density(x,y,z) as one parsed
    function with the file's my_constants (DENSITY_EXPR_DEFAULT), evaluated on the device per lattice point; no tables.
    -> deck"""
    d, _ = production_lwfa(n, nz, max_step)
    d.update(DENSITY_EXPR_DEFAULT)
    d.update(plasma_density_expr=LWFA_DENSITY, density_constants=dict(LWFA_CONSTANTS))
    return d


def gaussian_weight_SI():
    """examples/gaussian_weight/inputs_SI as the last run of tests/gaussian_weight.1Rank.sh (the one its checksum file holds): a
    fixed_weight beam of 10^5 particles and 1 nC, a Gaussian of (30, 40, 50) um about (0, 10, 20) um, in vacuum on 64^3 cells,
    absorbing particle boundary.  -> (deck without a beam, the beam's parameters for fixed_weight_beam)"""
    d = copy.deepcopy(_DEFAULT)
    d.update(nx=64, ny=64, nz=64, lo=(-200.0e-6, -200.0e-6, -200.0e-6), hi=(200.0e-6, 200.0e-6, 200.0e-6), order=2, si_units=1,
             plasma_ppc=(0, 0), plasma_density=0.0, plasma_charge=-SI["q_e"], plasma_mass=SI["m_e"],
             beam_profile=-1, beam_charge=-SI["q_e"], beam_mass=SI["m_e"], bc=2, n_steps=1, dt=0.0)
    beam = dict(num_particles=100000, density=None, total_charge=1.0e-9, pos_mean=(0.0, 10.0e-6, 20.0e-6),
                pos_std=(30.0e-6, 40.0e-6, 50.0e-6), u_mean=(0.0, 0.0, 1.0e3), zmin=-1.0, zmax=1.0, radius=1.0)
    return d, beam


def radiation_reaction_SI():
    """examples/beam_in_vacuum/inputs_RR as tests/radiation_reaction.1Rank.sh runs it: a matched gamma = 2000 beam sheet
    (sigma_y = 1e-12 m) of 10^5 fixed_weight particles in the linear focusing field E = (kp E0 / 2)(x, y, 0) of a blowout at
    n0 = 5e24 m^-3, SI units, 16 x 16 x 4 cells, six steps of 30 / omega_beta with 50 sub-cycles, radiation reaction on, no z push.
    -> (deck without a beam, the beam's parameters for fixed_weight_beam)"""
    ne = 5.0e24
    wp = (ne * SI["q_e"] ** 2 / (SI["ep0"] * SI["m_e"])) ** 0.5
    E0 = wp * SI["m_e"] * SI["c"] / SI["q_e"]
    kp = wp / SI["c"]
    K, gamma0, emit = kp / 2.0 ** 0.5, 2000.0, 313.0e-6
    sigma_x = (emit / kp / (gamma0 / 2.0) ** 0.5) ** 0.5
    sigma_ux = emit / sigma_x
    uz = (gamma0 ** 2 - 1.0 - sigma_ux ** 2) ** 0.5
    w_beta = K * SI["c"] / gamma0 ** 0.5
    d = copy.deepcopy(_DEFAULT)
    d.update(nx=16, ny=16, nz=4, lo=(-30.0e-6, -30.0e-6, -10.0e-6), hi=(30.0e-6, 30.0e-6, 10.0e-6), order=2, si_units=1,
             plasma_ppc=(0, 0), plasma_density=0.0, plasma_charge=-SI["q_e"], plasma_mass=SI["m_e"],
             beam_profile=-1, beam_charge=-SI["q_e"], beam_mass=SI["m_e"], bc=1, n_steps=6, dt=30.0 / w_beta,
             ext_E_slope=(0.5 * kp * E0, 0.5 * kp * E0), beam_n_subcycles=50, beam_radiation_reaction=1, beam_no_z_push=1)
    beam = dict(num_particles=100000, density=ne / 1.0e10, pos_mean=(0.0, 0.0, 0.0), pos_std=(sigma_x, 1.0e-12, 1.0e-6),
                u_mean=(0.0, 0.0, uz), u_std=(sigma_ux, 0.0, uz * 0.01))
    return d, beam


def hosing():
    """tests/hosing.2Rank.sh: the blowout deck with hipace.dt = 20, mobile ions (charge 1, mass 1836, one per cell, neither species
    with a neutralising background) and a tilted fixed_weight driver (beam.dx_per_dzeta = 0.2, density 200, sigma 0.1, 0.1, 1.41) --
    the deck of the hosing instability.  (Its checksum file predates the explicit solver's field set: parity is with the oracle.)
    -> (deck without a beam, the beam's parameters for fixed_weight_beam; the reference draws 10^6 particles)"""
    d = blowout_wake()
    d.update(n_steps=11, dt=20.0, beam_profile=-1, plasma_no_neutralize=1, background_density_SI=1.0e23)
    with_ion_species(d, "H", 1.0, ppc=(1, 1), initial_level=1)
    d["ion_mass"] = 1836.0
    beam = dict(num_particles=1000000, density=200.0, pos_mean=(lambda z: 0.2 * z, 0.0, 0.0), pos_std=(0.1, 0.1, 1.41),
                u_mean=(0.0, 0.0, 2000.0))
    return d, beam
