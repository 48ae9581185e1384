"""ctypes binding of libhpslice.so (include/hpslice.h).  Fails loudly when the HIP library is
missing: there is no CPU fallback for any product path."""
import ctypes as C
import os
import subprocess


def hip_already_started():
    """True if this process has (or may have) touched HIP: torch has initialised the device, or libhpslice.so has been
    loaded and used (an engine, a solver: hipSetDevice) -- GPU_MAX_HW_QUEUES set now would come too late."""
    import sys
    if _LIB is not None:
        return True
    t = sys.modules.get("torch")
    try:
        return bool(t is not None and t.cuda.is_initialized())
    except Exception:      # noqa: BLE001
        return False


_LIB = None
_HWQ_PRESET = "GPU_MAX_HW_QUEUES" in os.environ     # set by the host's environment, before this process started
_HIP_STARTED_AT_IMPORT = hip_already_started()
_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO = os.environ.get("HPS_LIB") or os.path.join(CSRC, "libhpslice.so")      # HPS_LIB: a diagnostic build (make stamps)


class Slab(C.Structure):
    _fields_ = [("p", C.c_void_p), ("nx", C.c_int), ("ny", C.c_int), ("ng", C.c_int), ("ncomp", C.c_int),
                ("jstride", C.c_long), ("nstride", C.c_long)]


PL_REAL = ["x", "y", "w", "ux", "uy", "psi", "x_prev", "y_prev", "ux_half", "uy_half", "psi_half"]


class Plasma(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in PL_REAL] + [("idcpu", C.c_void_p), ("ion_lev", C.c_void_p), ("n", C.c_long)]


class BeamSlice(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("x", "y", "z", "ux", "uy", "uz", "w")] + [("nsub", C.c_void_p), ("n", C.c_long)]


class Geom(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("dx", "dy", "dz", "xoff", "yoff", "c", "ep0", "mu0", "q_e", "m_e")] + \
               [("plo", C.c_double * 2), ("phi", C.c_double * 2), ("bc", C.c_int), ("normalized", C.c_int)]


class LaserPulse(C.Structure):      # hps_laser_pulse
    _fields_ = [("a0", C.c_double), ("w0", C.c_double), ("L0", C.c_double), ("pos", C.c_double * 3), ("zfoc", C.c_double),
                ("cep", C.c_double), ("propagation_angle_yz", C.c_double), ("pft_yz", C.c_double)]


class ExprIns(C.Structure):         # hps_expr_ins
    _fields_ = [("op", C.c_int), ("arg", C.c_int)]


class Expr(C.Structure):            # hps_expr
    _fields_ = [("n_ins", C.c_int), ("n_const", C.c_int), ("ins", C.POINTER(ExprIns)), ("consts", C.POINTER(C.c_double))]


class BeamFixedWeight(C.Structure):     # hps_beam_fixed_weight
    _fields_ = [("num_particles", C.c_long), ("profile", C.c_int), ("do_symmetrize", C.c_int), ("pos_mean_z", C.c_double),
                ("pos_std", C.c_double * 3), ("u_mean", C.c_double * 3), ("u_std", C.c_double * 3),
                ("zmin", C.c_double), ("zmax", C.c_double), ("radius", C.c_double), ("z_foc", C.c_double),
                ("duz_per_uz0_dzeta", C.c_double), ("density", C.c_double), ("total_charge", C.c_double),
                ("charge_is_specified", C.c_int)]


class BeamFixedWeightPdf(C.Structure):  # hps_beam_fixed_weight_pdf
    _fields_ = [("num_particles", C.c_long), ("do_symmetrize", C.c_int), ("pdf_ref_ratio", C.c_int), ("radius", C.c_double),
                ("z_foc", C.c_double), ("density", C.c_double), ("total_charge", C.c_double), ("charge_is_specified", C.c_int)]


class BeamSpecies(C.Structure):         # hps_beam_species
    _fields_ = [("charge", C.c_double), ("mass", C.c_double), ("n_subcycles", C.c_int), ("no_z_push", C.c_int),
                ("radiation_reaction", C.c_int), ("do_spin_tracking", C.c_int), ("spin_anom", C.c_double),
                ("uz_mean", C.c_double), ("uz_std", C.c_double), ("do_salame", C.c_int)]


class PlasmaSpecies(C.Structure):       # hps_plasma_species
    _fields_ = [("charge", C.c_double), ("mass", C.c_double), ("density", C.c_double), ("ppc", C.c_int * 2),
                ("fine_ppc", C.c_int * 2), ("neutralize_background", C.c_int)]


class Deck(C.Structure):
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("lo", C.c_double * 3), ("hi", C.c_double * 3),
                ("order", C.c_int), ("deriv_type", C.c_int),
                ("plasma_ppc", C.c_int * 2), ("plasma_density", C.c_double), ("plasma_radius", C.c_double),
                ("plasma_charge", C.c_double), ("plasma_mass", C.c_double), ("max_qsa", C.c_double),
                ("n_subcycles", C.c_int),
                ("beam_profile", C.c_int), ("beam_zmin", C.c_double), ("beam_zmax", C.c_double),
                ("beam_radius", C.c_double), ("beam_density", C.c_double),
                ("beam_umean", C.c_double * 3), ("beam_pos_mean", C.c_double * 3),
                ("beam_pos_std", C.c_double * 3), ("beam_ppc", C.c_int * 3), ("beam_charge", C.c_double),
                ("bc", C.c_int), ("mg_tol_rel", C.c_double), ("mg_tol_abs", C.c_double),
                ("deposit_rho", C.c_int), ("n_steps", C.c_int),
                ("dt", C.c_double), ("beam_n_subcycles", C.c_int), ("beam_mass", C.c_double), ("ext_E_slope", C.c_double * 2),
                ("bxby_solver", C.c_int), ("predcorr_tol", C.c_double), ("predcorr_max_iter", C.c_int),
                ("predcorr_mix", C.c_double), ("field_bc", C.c_int),
                ("laser_on", C.c_int), ("laser_a0", C.c_double), ("laser_w0", C.c_double), ("laser_L0", C.c_double),
                ("laser_lambda0", C.c_double), ("laser_pos", C.c_double * 3),
                ("laser_zfoc", C.c_double), ("laser_solver", C.c_int), ("laser_use_phase", C.c_int), ("si_units", C.c_int),
                ("grid_current_on", C.c_int), ("grid_current_peak", C.c_double), ("grid_current_mean", C.c_double * 3),
                ("grid_current_std", C.c_double * 3), ("laser_mg_tol_rel", C.c_double), ("laser_mg_tol_abs", C.c_double),
                ("beam_radiation_reaction", C.c_int), ("background_density_SI", C.c_double), ("beam_no_z_push", C.c_int),
                ("plasma_no_neutralize", C.c_int), ("ion_on", C.c_int), ("ion_ppc", C.c_int * 2), ("ion_density", C.c_double),
                ("ion_mass", C.c_double), ("ion_charge", C.c_double), ("ion_init_level", C.c_int), ("ion_Z", C.c_int),
                ("ion_energies", C.c_double * 56), ("ion_seed", C.c_ulonglong),
                ("beam_spin_tracking", C.c_int), ("beam_initial_spin", C.c_double * 3), ("beam_spin_anom", C.c_double),
                ("dt_adaptive", C.c_int), ("nt_per_betatron", C.c_double), ("dt_max", C.c_double),
                ("adaptive_threshold_uz", C.c_double), ("adaptive_phase_tolerance", C.c_double),
                ("adaptive_no_predict_step", C.c_int), ("adaptive_no_phase_control", C.c_int), ("adaptive_phase_substeps", C.c_int),
                ("adaptive_density", C.c_double), ("max_time", C.c_double), ("beam_uz_std", C.c_double),
                ("ext_Ez_slope", C.c_double),
                ("beam_do_salame", C.c_int), ("salame_n_iter", C.c_int), ("salame_relative_tolerance", C.c_double),
                ("salame_no_advance", C.c_int), ("salame_Ez_target_slope", C.c_double)]


# engine component names, index = value of the HPS_C_* enum in include/hpslice.h
COMPS = ["N_jx_beam", "N_jy_beam", "chi", "Sy", "Sx", "ExmBy", "EypBx", "Ez", "Bx", "By", "Bz",
         "Psi", "jx_beam", "jy_beam", "jz_beam", "jx", "jy", "rhomjz", "P_jx_beam", "P_jy_beam",
         "Ion_rhomjz", "rho"]
CIDX = {n: i for i, n in enumerate(COMPS)}
# predictor-corrector layout, index = value of the HPS_PC_* enum
COMPS_PC = ["N_jx", "N_jy", "ExmBy", "EypBx", "Ez", "Bx", "By", "Bz", "Psi", "jx", "jy", "jz", "rhomjz",
            "P_Bx", "P_By", "P_jx", "P_jy", "Ion_rhomjz", "It_Bx", "It_By", "PIt_Bx", "PIt_By", "rho"]
CIDX_PC = {n: i for i, n in enumerate(COMPS_PC)}
# the SALAME slice, index = value of the HPS_SAL_* enum; appended behind the engine's own components in a beam_do_salame deck
# and in a moving-beam engine whose deck carries beam_species_salame (hps_engine_set_beam_species_salame)
COMPS_SALAME = ["Ez_target", "Ez_no_salame", "Ez", "jx", "jy", "jz_beam", "Bx", "By", "Sy", "Sx", "Sy_back", "Sx_back"]
ID_VALID = 1 << 63

_SIGS = {
    "hps_last_error": (C.c_char_p, []),
    "hps_version": (C.c_char_p, []),
    "hps_deposit_current": (C.c_int, [Slab, Plasma, Geom, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_double,
                                      C.c_int, C.c_void_p, C.c_void_p]),
    "hps_explicit_deposit": (C.c_int, [Slab, Plasma, Geom, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int,
                                       C.c_int, C.c_int, C.c_void_p]),
    "hps_advance_plasma": (C.c_int, [Slab, Plasma, Geom, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_void_p]),
    "hps_tiling_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_long, C.POINTER(C.c_void_p)]),
    "hps_reorder_particles": (C.c_int, [C.c_void_p, Plasma, Plasma, Geom, C.c_void_p]),
    "hps_tiling_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "hps_tiling_destroy": (C.c_int, [C.c_void_p]),
    "hps_deposit_current_tiled": (C.c_int, [Slab, Plasma, Geom, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_double,
                                            C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hps_explicit_deposit_tiled": (C.c_int, [Slab, Plasma, Geom, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int,
                                             C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hps_advance_plasma_tiled": (C.c_int, [Slab, Plasma, Geom, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hps_deposit_current_tiled_laser": (C.c_int, [Slab, Plasma, Geom, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int,
                                                  C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hps_explicit_deposit_tiled_laser": (C.c_int, [Slab, Plasma, Geom, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double,
                                                   C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hps_advance_plasma_tiled_laser": (C.c_int, [Slab, Plasma, Geom, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int,
                                                 C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hps_tiling_set_validity": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "hps_particles_record": (C.c_int, [C.c_int]),
    "hps_particles_recorded": (C.c_int, [C.c_char_p, C.c_long, C.POINTER(C.c_long)]),
    "hps_poisson_create": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_void_p)]),
    "hps_poisson_solve": (C.c_int, [C.c_void_p, C.c_void_p, Slab, C.c_int, C.c_void_p]),
    "hps_poisson_solve_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, Slab, C.c_void_p, C.c_void_p]),
    "hps_poisson_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hps_poisson_destroy": (C.c_int, [C.c_void_p]),
    "hps_mg_create": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_void_p)]),
    "hps_mg_solve1": (C.c_int, [C.c_void_p, Slab, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_void_p]),
    "hps_mg_solve1_fabs": (C.c_int, [C.c_void_p, Slab, Slab, Slab, C.c_double, C.c_double, C.c_int,
                                     C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_void_p]),
    "hps_mg_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                              C.POINTER(C.c_long), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hps_mg_info_schedule": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "hps_mg_info_upleg": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "hps_mg_destroy": (C.c_int, [C.c_void_p]),
    "hps_mg2_create": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_void_p)]),
    "hps_mg2_solve2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int,
                                 C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_void_p]),
    "hps_mg2_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hps_mg2_destroy": (C.c_int, [C.c_void_p]),
    "hps_engine_laser_vcycles": (C.c_int, [C.c_void_p, C.POINTER(C.c_long)]),
    "hps_engine_create": (C.c_int, [C.POINTER(Deck), C.c_int, C.POINTER(C.c_void_p)]),
    "hps_engine_destroy": (C.c_int, [C.c_void_p]),
    "hps_engine_begin_step": (C.c_int, [C.c_void_p]),
    "hps_engine_solve_slice": (C.c_int, [C.c_void_p, C.c_int]),
    "hps_engine_solve_slice_begin": (C.c_int, [C.c_void_p, C.c_int]),
    "hps_engine_solve_slice_finish": (C.c_int, [C.c_void_p, C.c_int]),
    "hps_engine_slice_ready": (C.c_int, [C.c_void_p]),
    "hps_engine_run_step": (C.c_int, [C.c_void_p]),
    "hps_engine_sync": (C.c_int, [C.c_void_p]),
    "hps_engine_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_long)]),
    "hps_engine_slab": (Slab, [C.c_void_p]),
    "hps_engine_plasma": (Plasma, [C.c_void_p]),
    "hps_engine_stream": (C.c_void_p, [C.c_void_p]),
    "hps_engine_ions": (Plasma, [C.c_void_p]),
    "hps_engine_ion_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "hps_engine_checksums": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_beam_sort_by_box": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "hps_engine_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "hps_engine_early_init_slices": (C.c_int, [C.c_void_p, C.POINTER(C.c_long)]),
    "hps_engine_schedule": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hps_engine_qsa_drops": (C.c_int, [C.c_void_p, C.POINTER(C.c_long)]),
    "hps_engine_set_insitu_plasma": (C.c_int, [C.c_void_p, C.c_double]),
    "hps_engine_set_insitu_beam": (C.c_int, [C.c_void_p, C.c_double]),
    "hps_engine_insitu_beam": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_engine_insitu_plasma": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_engine_set_insitu_fields": (C.c_int, [C.c_void_p, C.c_int]),
    "hps_engine_insitu_fields": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_engine_set_field_diagnostic": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hps_engine_field_diagnostic": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_engine_set_field_diagnostic_box": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hps_engine_field_diagnostic_geometry": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hps_engine_record_event": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "hps_engine_wait_event": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_stream_pool_shared_pairs": (C.c_int, [C.c_int]),
    "hps_engine_copy_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]),
    "hps_engine_set_profiling_stride": (C.c_int, [C.c_void_p, C.c_int]),
    "hps_engine_set_laser_import": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "hps_engine_set_step": (C.c_int, [C.c_void_p, C.c_int]),
    "hps_engine_set_time": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "hps_engine_beam_moments": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_adaptive_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "hps_adaptive_set_density_profile": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hps_adaptive_initial_dt": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_double)]),
    "hps_adaptive_before_step": (C.c_int, [C.c_void_p, C.c_double, C.POINTER(C.c_double)]),
    "hps_adaptive_next_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "hps_adaptive_after_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_double)]),
    "hps_adaptive_destroy": (C.c_int, [C.c_void_p]),
    "hps_engine_export_laser_slice": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "hps_engine_import_laser_slice": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "hps_engine_import_laser_from": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "hps_engine_laser_envelope": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_engine_laser_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "hps_engine_set_laser_grid": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]),
    "hps_engine_laser_grid": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hps_engine_laser_chi": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_engine_set_laser_pulses": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(LaserPulse)]),
    "hps_engine_add_laser_samples": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_double),
                                               C.POINTER(C.c_double), C.c_double]),
    "hps_engine_set_insitu_laser": (C.c_int, [C.c_void_p, C.c_int]),
    "hps_engine_insitu_laser": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_laser_interp_aabs": (C.c_int, [Slab, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                        Geom, C.c_int, C.c_void_p]),
    "hps_laser_interp_chi": (C.c_int, [Slab, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                       C.c_double, Geom, C.c_int, C.c_int, C.c_void_p]),
    "hps_deposit_current_laser": (C.c_int, [Slab, Plasma, Geom, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double,
                                            C.c_int, C.c_void_p, C.c_void_p]),
    "hps_explicit_deposit_laser": (C.c_int, [Slab, Plasma, Geom, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_int,
                                             C.c_int, C.c_int, C.c_void_p]),
    "hps_advance_plasma_laser": (C.c_int, [Slab, Plasma, Geom, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_void_p]),
    "hps_engine_pc_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_double)]),
    "hps_engine_pc_zero_b_slices": (C.c_int, [C.c_void_p, C.POINTER(C.c_long)]),
    "hps_engine_set_diagnostics": (C.c_int, [C.c_void_p, C.c_int]),
    "hps_engine_set_tiling": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "hps_engine_fallbacks": (C.c_int, [C.c_void_p, C.POINTER(C.c_long)]),
    "hps_engine_set_fusion": (C.c_int, [C.c_void_p, C.c_int]),
    "hps_engine_set_density_profile": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hps_engine_set_plasma_init": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_double]),
    "hps_engine_set_fine_patch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "hps_engine_set_plasma_momentum": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_ulonglong]),
    "hps_engine_set_plasma_symmetry": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "hps_engine_sorts": (C.c_int, [C.c_void_p, C.POINTER(C.c_long)]),
    "hps_engine_assume_initial_beam_support": (C.c_int, [C.c_void_p]),
    "hps_engine_beam_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hps_engine_beam_capacity": (C.c_int, [C.c_void_p, C.POINTER(C.c_long)]),
    "hps_engine_set_beam_capacity": (C.c_int, [C.c_void_p, C.c_long]),
    "hps_engine_beam_message_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "hps_engine_beam_spin": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_engine_set_beam_import": (C.c_int, [C.c_void_p, C.c_int]),
    "hps_engine_export_beam_slice": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "hps_engine_import_beam_slice": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "hps_engine_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "hps_engine_phase_times": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hps_engine_beam_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_long), C.c_void_p]),
    "hps_engine_set_beam_particles": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.POINTER(C.c_long)]),
    "hps_engine_set_beam_storage": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_engine_initial_beam": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_ring_unique_id": (C.c_int, [C.c_char_p]),
    "hps_ring_init": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "hps_ring_send_slice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "hps_ring_recv_slice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "hps_ring_sendrecv_self": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "hps_ring_stream_wait": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "hps_ring_sync_sends": (C.c_int, [C.c_void_p]),
    "hps_ring_sync": (C.c_int, [C.c_void_p]),
    "hps_ring_sync_timeout": (C.c_int, [C.c_void_p, C.c_double]),
    "hps_ring_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "hps_engine_tiling": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "hps_ring_info": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int)] * 5),
    "hps_ring_destroy": (C.c_int, [C.c_void_p]),
    "hps_ring_edge_kind": (C.c_int, [C.c_void_p]),
    "hps_ring_can_send": (C.c_int, [C.c_void_p]),
    "hps_ring_recv_landed": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_ring_engine_wait": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hps_engine_salame_stats": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_salame_only_advance": (C.c_int, [Slab, Plasma, Geom, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p]),
    "hps_salame_jxjy_from_bxby": (C.c_int, [Slab, Geom, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "hps_salame_sxsy_from_jz": (C.c_int, [Slab, Geom, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "hps_salame_get_w": (C.c_int, [Slab, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hps_salame_scale_beam_slice": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_void_p]),
    "hps_engine_set_beam_species_salame": (C.c_int, [C.c_void_p, C.c_int]),
    "hps_engine_deposit_beam_species": (C.c_int, [C.c_void_p, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int]),
    "hps_engine_salame_scale_slice": (C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    "hps_open_boundary": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint,
                                    C.c_void_p]),
    "hps_collide_plasma": (C.c_int, [Plasma, C.c_void_p, Plasma, C.c_void_p, Geom, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                     C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_ulonglong, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(C.c_long), C.POINTER(C.c_long), C.c_void_p]),
    "hps_engine_add_collision": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_ulonglong]),
    "hps_engine_collision_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "hps_collide_beam_plasma": (C.c_int, [BeamSlice, Plasma, Geom, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                          C.c_int, C.c_double, C.c_double, C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_double,
                                          C.POINTER(C.c_long), C.POINTER(C.c_long), C.c_void_p]),
    "hps_engine_add_beam_collision": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_ulonglong]),
    "hps_expr_check": (C.c_int, [C.POINTER(Expr), C.c_int, C.POINTER(C.c_int)]),
    "hps_expr_eval_host": (C.c_int, [C.POINTER(Expr), C.c_int, C.c_long, C.POINTER(C.c_void_p), C.c_void_p]),
    "hps_expr_eval": (C.c_int, [C.POINTER(Expr), C.c_int, C.c_long, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]),
    "hps_engine_set_beam_external_fields": (C.c_int, [C.c_void_p, C.POINTER(Expr), C.POINTER(Expr)]),
    "hps_engine_set_density_expr": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Expr), C.c_void_p, C.c_double]),
    "hps_engine_set_beam_fixed_ppc": (C.c_int, [C.c_void_p, C.POINTER(Expr), C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_ulonglong]),
    "hps_engine_set_beam_fixed_weight": (C.c_int, [C.c_void_p, C.POINTER(BeamFixedWeight), C.POINTER(Expr), C.POINTER(Expr), C.c_ulonglong,
                                                   C.POINTER(C.c_long)]),
    "hps_engine_set_beam_fixed_weight_pdf": (C.c_int, [C.c_void_p, C.POINTER(BeamFixedWeightPdf), C.POINTER(Expr), C.POINTER(Expr),
                                                       C.c_ulonglong, C.POINTER(C.c_long), C.POINTER(C.c_double)]),
    "hps_adaptive_set_density_expr": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Expr), C.c_void_p]),
    "hps_adaptive_rho_max": (C.c_int, [C.c_void_p, C.c_double, C.POINTER(C.c_double)]),
    "hps_engine_add_beam_species": (C.c_int, [C.c_void_p, C.POINTER(BeamSpecies), C.POINTER(C.c_int)]),
    "hps_engine_select_beam_species": (C.c_int, [C.c_void_p, C.c_int]),
    "hps_engine_beam_species_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_long)]),
    "hps_engine_beam_state_species": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_long), C.c_void_p, C.c_void_p]),
    "hps_engine_insitu_beam_species": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "hps_engine_beam_tags": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_engine_beam_moments_species": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hps_engine_beam_kernels": (C.c_int, [C.c_void_p, C.c_char_p, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_int)]),
    "hps_engine_add_plasma_species": (C.c_int, [C.c_void_p, C.POINTER(PlasmaSpecies), C.POINTER(C.c_int)]),
    "hps_engine_plasma_species_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_long)]),
    "hps_engine_plasma_species": (Plasma, [C.c_void_p, C.c_int]),
    "hps_engine_insitu_plasma_species": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "hps_adaptive_add_species": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "hps_adaptive_initial_dt_beams": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                C.POINTER(C.c_double)]),
    "hps_adaptive_after_step_beams": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int,
                                                C.POINTER(C.c_double)]),
    "hps_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long]),
    "hps_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long]),
    "hps_device_count": (C.c_int, [C.POINTER(C.c_int)]),
}


def build(force=False):
    """Compile libhpslice.so for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC, "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args + ["libhpslice.so"], stdout=subprocess.DEVNULL)
    return SO


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO):
            raise RuntimeError(
                f"{SO} is missing: the HIP extension was not built (run __graft_entry__.build()); "
                "hipace_amd has no CPU fallback")
        L = C.CDLL(SO)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)      # AttributeError here = the library does not export the ABI
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


class HpsError(RuntimeError):
    pass


def check(status):
    if status != 0:
        raise HpsError(f"hpslice status {status}: {lib().hps_last_error().decode()}")


def fill_struct(st, d):
    for name, typ in st._fields_:
        if name not in d:
            continue
        v = d[name]
        if hasattr(typ, "_length_"):
            setattr(st, name, typ(*v))
        else:
            setattr(st, name, v)
    return st
