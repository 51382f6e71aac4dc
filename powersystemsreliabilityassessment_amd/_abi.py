"""ctypes mirror of the plain-C structs in include/relmc.h (data layout only, no code path).

Both the product loader (``_lib.py``) and the test-only oracle binding
(``oracle/coracle.py``) describe their arguments with these classes.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

RELMC_MAX_BUS = 128
RELMC_MAX_COMP = 256

RELMC_REFERENCE_EMULATE = 0
RELMC_PHYSICAL = 1

ST_CONVERGED, ST_MAXIT, ST_NUMFAIL, ST_SINGULAR = 0, 1, 2, 3

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_uint8_p = C.POINTER(C.c_uint8)
c_uint32_p = C.POINTER(C.c_uint32)
c_int64_p = C.POINTER(C.c_int64)


class CaseDesc(C.Structure):
    _fields_ = [
        ("base_mva", C.c_double),
        ("nb", C.c_int32), ("ng", C.c_int32), ("nl", C.c_int32), ("nd", C.c_int32),
        ("ref_bus", C.c_int32),
        ("bus_pd", c_double_p),
        ("inj_bus", c_int32_p),
        ("inj_pmin", c_double_p), ("inj_pmax", c_double_p), ("inj_cost", c_double_p),
        ("br_from", c_int32_p), ("br_to", c_int32_p),
        ("br_b", c_double_p), ("br_rate", c_double_p),
        ("unavail", c_double_p),
        ("always_up", c_uint8_p),
        ("total_load", C.c_double),
    ]


class SolverOpts(C.Structure):
    _fields_ = [
        ("singular_policy", C.c_int32), ("max_it", C.c_int32),
        ("feastol", C.c_double), ("gradtol", C.c_double), ("comptol", C.c_double),
        ("costtol", C.c_double), ("xi", C.c_double), ("sigma", C.c_double), ("z0", C.c_double),
        ("alpha_min", C.c_double), ("max_stepsize", C.c_double),
        ("screen", C.c_int32), ("reserved", C.c_int32),
    ]


class Acc(C.Structure):
    _fields_ = [
        ("n", C.c_int64), ("n_fail", C.c_int64), ("n_singular", C.c_int64),
        ("n_infeasible", C.c_int64), ("n_nonconverged", C.c_int64), ("sum_iters", C.c_int64),
        ("comp_fail", C.c_int64 * RELMC_MAX_COMP),
        ("n_screened", C.c_int64),
        ("sum_dns", C.c_double), ("sum_dns2", C.c_double),
        ("sum_nodal", C.c_double * RELMC_MAX_BUS),
    ]

    N_INT = 6 + RELMC_MAX_COMP + 1
    N_DBL = 2 + RELMC_MAX_BUS

    def to_arrays(self):
        """(int64[N_INT], float64[N_DBL]) views copied out — the all-reduce payload."""
        raw = np.frombuffer(bytes(self), dtype=np.uint8)
        ints = raw[: self.N_INT * 8].view(np.int64).copy()
        dbls = raw[self.N_INT * 8:].view(np.float64).copy()
        return ints, dbls

    @classmethod
    def from_arrays(cls, ints, dbls):
        ints = np.ascontiguousarray(ints, dtype=np.int64)
        dbls = np.ascontiguousarray(dbls, dtype=np.float64)
        assert ints.size == cls.N_INT and dbls.size == cls.N_DBL
        return cls.from_buffer_copy(ints.tobytes() + dbls.tobytes())


# relmc_allreduce_fn: int32 fn(void* user, relmc_acc* acc_inout)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(Acc))
# relmc_allreduce_f64_fn: int32 fn(void* user, double* buf_inout, int64 count)
ALLREDUCE_F64_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, c_double_p, C.c_int64)


class Indices(C.Structure):
    _fields_ = [
        ("n", C.c_int64),
        ("edns", C.c_double), ("lole", C.c_double), ("plc", C.c_double), ("beta", C.c_double),
        ("eens", C.c_double), ("mean_iters", C.c_double),
        ("nodal_eens", C.c_double * RELMC_MAX_BUS),
        ("comp_importance", C.c_double * RELMC_MAX_COMP),
    ]


class NsqOpts(C.Structure):
    _fields_ = [
        ("beta_limit", C.c_double), ("max_samples", C.c_int64), ("batch", C.c_int64),
        ("seed", C.c_uint64), ("hours_per_year", C.c_double),
        ("solver", SolverOpts),
        ("history_cap", C.c_int64),
        ("beta_history", c_double_p), ("edns_history", c_double_p),
        ("lole_history", c_double_p), ("plc_history", c_double_p),
        ("distinct_states", C.c_int32),
    ]


class NsqResult(C.Structure):
    _fields_ = [
        ("acc", Acc), ("idx", Indices),
        ("checkpoints", C.c_int64), ("converged", C.c_int32),
        ("wall_seconds", C.c_double), ("kernel_seconds", C.c_double),
        ("batches", C.c_int64),
    ]


class SeqYear(C.Structure):
    _fields_ = [("ens", C.c_double), ("dlc", C.c_double), ("nlc", C.c_double), ("n_contingency", C.c_int64)]


class SeqEvent(C.Structure):              # relmc_seq_event
    _fields_ = [("year", C.c_int32), ("start_hour", C.c_int32), ("duration", C.c_int32), ("censored", C.c_int32),
                ("energy_mwh", C.c_double), ("peak_mw", C.c_double),
                ("onset", C.c_uint32 * (RELMC_MAX_COMP // 32)), ("involved", C.c_uint32 * (RELMC_MAX_COMP // 32))]


class SeqEventAcc(C.Structure):           # relmc_seq_event_acc
    _fields_ = [("years", C.c_int64), ("events", C.c_int64), ("censored", C.c_int64), ("load_onset_events", C.c_int64),
                ("sum_dur", C.c_int64), ("sum_dur2", C.c_int64), ("max_dur", C.c_int64),
                ("sum_energy", C.c_double), ("sum_energy2", C.c_double), ("max_energy", C.c_double), ("max_peak", C.c_double),
                ("onset_events", C.c_int64 * RELMC_MAX_COMP), ("involved_events", C.c_int64 * RELMC_MAX_COMP),
                ("onset_energy", C.c_double * RELMC_MAX_COMP), ("involved_energy", C.c_double * RELMC_MAX_COMP)]


class Hl1SeqYear(C.Structure):            # relmc_hl1_seq_year
    _fields_ = [("lole", C.c_double), ("eue", C.c_double), ("lolf", C.c_double)]


class Hl1SeqAcc(C.Structure):             # relmc_hl1_seq_acc
    _fields_ = [("years", C.c_int64), ("sum_lole", C.c_double), ("sum_eue", C.c_double), ("sum_lolf", C.c_double),
                ("sum_lole2", C.c_double), ("sum_eue2", C.c_double), ("sum_lolf2", C.c_double)]


class Hl1Event(C.Structure):              # relmc_hl1_event
    _fields_ = [("chain", C.c_int64), ("start_step", C.c_int64), ("duration", C.c_int64), ("energy_mwh", C.c_double), ("peak_mw", C.c_double)]


class Hl1SweepLevel(C.Structure):         # relmc_hl1_sweep_level (24 bytes)
    _fields_ = [("scale", C.c_double), ("shift", C.c_double), ("fleet", C.c_int32), ("reserved", C.c_int32)]


HL1_SWEEP_MAX_LEVELS = 16                 # RELMC_HL1_SWEEP_MAX_LEVELS


class Hl1MaintWindow(C.Structure):        # relmc_hl1_maint_window (16 bytes)
    _fields_ = [("schedule", C.c_int32), ("unit", C.c_int32), ("start_hour", C.c_int32), ("hours", C.c_int32)]


HL1_MAINT_MAX_SCHEDULES = 8               # RELMC_HL1_MAINT_MAX_SCHEDULES


class Hl1AttrUnit(C.Structure):           # relmc_hl1_attr_unit (32 bytes): one chain's loss steps with the unit DOWN
    _fields_ = [("down_hours", C.c_double), ("down_mwh", C.c_double), ("critical_hours", C.c_double), ("relief_mwh", C.c_double)]


class Hl1AttrAcc(C.Structure):            # relmc_hl1_attr_acc (64 bytes): sums of x and x * x over the chains, x in Hl1AttrUnit's field order
    _fields_ = [("sum", C.c_double * 4), ("sum2", C.c_double * 4)]


HL1_MAX_STORAGE = 8                       # RELMC_HL1_MAX_STORAGE


class Hl1Storage(C.Structure):            # relmc_hl1_storage (48 bytes)
    _fields_ = [("charge_mw", C.c_double), ("discharge_mw", C.c_double), ("energy_mwh", C.c_double), ("eta_charge", C.c_double),
                ("eta_discharge", C.c_double), ("soc0_mwh", C.c_double)]


class Hl1StorageYear(C.Structure):        # relmc_hl1_storage_year
    _fields_ = [("served_hours", C.c_double), ("discharged_mwh", C.c_double), ("charged_mwh", C.c_double)]


class Hl1StorageAcc(C.Structure):         # relmc_hl1_storage_acc
    _fields_ = [("years", C.c_int64), ("sum_lole", C.c_double), ("sum_eue", C.c_double), ("sum_lolf", C.c_double),
                ("sum_lole2", C.c_double), ("sum_eue2", C.c_double), ("sum_lolf2", C.c_double),
                ("sum_served", C.c_double), ("sum_discharged", C.c_double), ("sum_charged", C.c_double),
                ("sum_served2", C.c_double), ("sum_discharged2", C.c_double), ("sum_charged2", C.c_double)]


HL1_VAR_MAX_RESOURCES = 8                 # RELMC_HL1_VAR_MAX_RESOURCES
HL1_VAR_MAX_WEATHER = 256                 # RELMC_HL1_VAR_MAX_WEATHER
HL1_VAR_TAG = 0x60000000                  # RELMC_HL1_VAR_TAG
HL1_VAR_PICK_RANDOM, HL1_VAR_PICK_CYCLE = 0, 1     # RELMC_HL1_VAR_PICK_*
HL1_STRESS_MAX_CLASSES = 8                # RELMC_HL1_STRESS_MAX_CLASSES


class Hl1VarOpts(C.Structure):            # relmc_hl1_var_opts (88 bytes)
    _fields_ = [("resource_scale", C.c_double * HL1_VAR_MAX_RESOURCES), ("scale", C.c_double), ("shift", C.c_double),
                ("pick", C.c_int32), ("reserved", C.c_int32)]


HL1_MS_BRANCH_TAG = 0x50000000            # RELMC_HL1_MS_BRANCH_TAG
HL1_MS_MAX_HOURS = 1 << 30                # RELMC_HL1_MS_MAX_HOURS


class Hl1MsUnit(C.Structure):             # relmc_hl1_ms_unit (64 bytes)
    _fields_ = [("capacity_mw", C.c_double), ("derated_mw", C.c_double), ("mean_h", C.c_double * 3), ("first_p", C.c_double * 3)]


class Hl1MsYear(C.Structure):             # relmc_hl1_ms_year
    _fields_ = [("derated_unit_h", C.c_double), ("down_unit_h", C.c_double)]


class Hl1MsAcc(C.Structure):              # relmc_hl1_ms_acc
    _fields_ = [("years", C.c_int64), ("sum_lole", C.c_double), ("sum_eue", C.c_double), ("sum_lolf", C.c_double),
                ("sum_lole2", C.c_double), ("sum_eue2", C.c_double), ("sum_lolf2", C.c_double),
                ("sum_derated", C.c_double), ("sum_down", C.c_double), ("sum_derated2", C.c_double), ("sum_down2", C.c_double)]


class Hl1EventAcc(C.Structure):           # relmc_hl1_event_acc
    _fields_ = [("years", C.c_int64), ("events", C.c_int64), ("censored", C.c_int64), ("sum_dur", C.c_int64), ("sum_dur2", C.c_int64),
                ("max_dur", C.c_int64), ("sum_energy", C.c_double), ("sum_energy2", C.c_double), ("max_energy", C.c_double),
                ("max_peak", C.c_double)]


HL1_START_ALL_UP, HL1_START_STATIONARY = 0, 1     # RELMC_HL1_START_*
AREA_MAX = 8                                       # RELMC_AREA_MAX
HL1_AREA_ISOLATED, HL1_AREA_INTERCONNECTED = 0, 1  # RELMC_HL1_AREA_*
HL1_AREA_FLOW_REFERENCE, HL1_AREA_FLOW_MAX_FLOW = 0, 1   # RELMC_HL1_AREA_FLOW_*
HL1_TIE_MAX, HL1_TIE_DRAW_BASE = 32, 128           # RELMC_HL1_TIE_MAX, RELMC_HL1_TIE_DRAW_BASE
HL1_AREA_SWEEP_MAX_LEVELS = 8                      # RELMC_HL1_AREA_SWEEP_MAX_LEVELS


class Hl1AreaLevel(C.Structure):                   # relmc_hl1_area_level (144 bytes)
    _fields_ = [("load_scale", C.c_double * AREA_MAX), ("load_shift", C.c_double * AREA_MAX), ("tie_scale", C.c_double),
                ("fleet", C.c_int32), ("reserved", C.c_int32)]


class Hl1AreaVarOpts(C.Structure):                 # relmc_hl1_area_var_opts (208 bytes)
    _fields_ = [("resource_scale", C.c_double * HL1_VAR_MAX_RESOURCES), ("load_scale", C.c_double * AREA_MAX),
                ("load_shift", C.c_double * AREA_MAX), ("policy", C.c_int32), ("flow", C.c_int32), ("pick", C.c_int32),
                ("reserved", C.c_int32)]


class Hl1AreaStorage(C.Structure):                 # relmc_hl1_area_storage (56 bytes): `area` is 0-based
    _fields_ = [("s", Hl1Storage), ("area", C.c_int32), ("reserved", C.c_int32)]


class SeqOpts(C.Structure):
    _fields_ = [
        ("cov_threshold", C.c_double), ("max_years", C.c_int32), ("batch_years", C.c_int32), ("seed", C.c_uint64),
        ("curtail_threshold", C.c_double), ("solver", SolverOpts),
        ("years_cap", C.c_int64), ("results_year", C.POINTER(SeqYear)), ("cum_eens", c_double_p), ("cum_cov", c_double_p),
    ]


class SeqResult(C.Structure):
    _fields_ = [
        ("final_year", C.c_int32), ("converged", C.c_int32),
        ("eens", C.c_double), ("cov", C.c_double), ("lole", C.c_double), ("lolf", C.c_double), ("plc", C.c_double),
        ("n_contingency", C.c_int64), ("acc", Acc),
        ("nodal_eens_avg", C.c_double * RELMC_MAX_BUS), ("comp_importance", C.c_double * RELMC_MAX_COMP),
        ("wall_seconds", C.c_double), ("kernel_seconds", C.c_double),
    ]


class DbStats(C.Structure):
    _fields_ = [("rows", C.c_int64), ("samples", C.c_int64), ("new_rows", C.c_int64), ("batch_distinct", C.c_int64)]


IS_TUNE_MAX_PASSES = 32                   # RELMC_IS_TUNE_MAX_PASSES


class IsAcc(C.Structure):                 # relmc_is_acc
    _fields_ = [
        ("n", C.c_int64), ("n_fail", C.c_int64), ("n_singular", C.c_int64),
        ("n_infeasible", C.c_int64), ("n_nonconverged", C.c_int64), ("sum_iters", C.c_int64),
        ("sum_w", C.c_double), ("sum_w2", C.c_double), ("sum_wfail", C.c_double), ("sum_w2fail", C.c_double),
        ("sum_wdns", C.c_double), ("sum_w2dns2", C.c_double),
        ("comp_wfail", C.c_double * RELMC_MAX_COMP), ("comp_wdns", C.c_double * RELMC_MAX_COMP),
        ("sum_wnodal", C.c_double * RELMC_MAX_BUS),
    ]


class IsIndices(C.Structure):             # relmc_is_indices
    _fields_ = [
        ("n", C.c_int64),
        ("edns", C.c_double), ("lole", C.c_double), ("plc", C.c_double), ("beta", C.c_double),
        ("eens", C.c_double), ("mean_iters", C.c_double),
        ("beta_plc", C.c_double), ("mean_w", C.c_double), ("ess", C.c_double),
        ("nodal_eens", C.c_double * RELMC_MAX_BUS),
        ("comp_importance", C.c_double * RELMC_MAX_COMP),
    ]


class IsTuneOpts(C.Structure):            # relmc_is_tune_opts
    _fields_ = [
        ("seed", C.c_uint64), ("n_pilot", C.c_int64), ("max_iters", C.c_int32), ("final_iters", C.c_int32),
        ("min_elite", C.c_int64), ("rho", C.c_double), ("objective", C.c_int32), ("reserved", C.c_int32),
        ("alpha", C.c_double), ("q_max", C.c_double), ("solver", SolverOpts),
    ]


class IsTuneReport(C.Structure):          # relmc_is_tune_report
    _fields_ = [
        ("passes", C.c_int32), ("final_passes", C.c_int32),
        ("n_fail", C.c_int64 * IS_TUNE_MAX_PASSES), ("n_elite", C.c_int64 * IS_TUNE_MAX_PASSES),
        ("sum_e", C.c_double * IS_TUNE_MAX_PASSES), ("level", C.c_double * IS_TUNE_MAX_PASSES),
        ("kernel_seconds", C.c_double), ("wall_seconds", C.c_double),
    ]


class IsRunOpts(C.Structure):             # relmc_is_run_opts
    _fields_ = [
        ("beta_limit", C.c_double), ("max_samples", C.c_int64), ("batch", C.c_int64),
        ("seed", C.c_uint64), ("hours_per_year", C.c_double),
        ("solver", SolverOpts),
        ("unavail_is", c_double_p),
        ("history_cap", C.c_int64),
        ("beta_history", c_double_p), ("edns_history", c_double_p), ("plc_history", c_double_p),
    ]


class IsRunResult(C.Structure):           # relmc_is_run_result
    _fields_ = [
        ("acc", IsAcc), ("idx", IsIndices),
        ("checkpoints", C.c_int64), ("batches", C.c_int64), ("converged", C.c_int32), ("reserved", C.c_int32),
        ("wall_seconds", C.c_double), ("kernel_seconds", C.c_double),
    ]


assert C.sizeof(Acc) == (Acc.N_INT + Acc.N_DBL) * 8


def default_solver_opts(policy: int = RELMC_REFERENCE_EMULATE) -> SolverOpts:
    """MIPS defaults MATPOWER uses for OPF_ALG_DC=200 (nsqMain.m:185-186)."""
    return SolverOpts(singular_policy=policy, max_it=150, feastol=5e-6, gradtol=1e-6,
                      comptol=1e-6, costtol=1e-6, xi=0.99995, sigma=0.1, z0=1.0,
                      alpha_min=1e-8, max_stepsize=1e10, screen=0, reserved=0)


class CaseHolder:
    """Keeps the numpy arrays a CaseDesc points into alive."""

    def __init__(self, case):
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        self.case = case
        self._keep = dict(
            bus_pd=f64(case.bus_pd), inj_bus=i32(case.inj_bus), inj_pmin=f64(case.inj_pmin),
            inj_pmax=f64(case.inj_pmax), inj_cost=f64(case.inj_cost), br_from=i32(case.br_from),
            br_to=i32(case.br_to), br_b=f64(case.br_b), br_rate=f64(case.br_rate),
            unavail=f64(case.unavail),
            always_up=np.ascontiguousarray(case.always_up, dtype=np.uint8))
        k = self._keep
        self.desc = CaseDesc(
            base_mva=case.base_mva, nb=case.nb, ng=case.ng, nl=case.nl, nd=case.nd,
            ref_bus=case.ref_bus,
            bus_pd=k["bus_pd"].ctypes.data_as(c_double_p),
            inj_bus=k["inj_bus"].ctypes.data_as(c_int32_p),
            inj_pmin=k["inj_pmin"].ctypes.data_as(c_double_p),
            inj_pmax=k["inj_pmax"].ctypes.data_as(c_double_p),
            inj_cost=k["inj_cost"].ctypes.data_as(c_double_p),
            br_from=k["br_from"].ctypes.data_as(c_int32_p),
            br_to=k["br_to"].ctypes.data_as(c_int32_p),
            br_b=k["br_b"].ctypes.data_as(c_double_p),
            br_rate=k["br_rate"].ctypes.data_as(c_double_p),
            unavail=k["unavail"].ctypes.data_as(c_double_p),
            always_up=k["always_up"].ctypes.data_as(c_uint8_p),
            total_load=case.total_load)
