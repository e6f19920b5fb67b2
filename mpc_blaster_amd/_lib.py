"""ctypes binding of libmpcblaster.so (the C ABI declared in include/mpcb.h).

The HIP library is the product: there is no CPU fallback.  If the shared object is missing
the import of any compute entry point raises, loudly.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = 'libmpcblaster.so'
LIB_PATH = os.path.join(_HERE, LIB_NAME)

ABI_VERSION = 5
MPCB_F64, MPCB_F32 = 0, 1
MPCB_MAX_NX, MPCB_MAX_NU = 17, 6
MODEL_REC = 14   # MPCB_MODEL_REC: elements of one instance's vehicle record
STATUS_OK, STATUS_NAN, STATUS_MAXITER, STATUS_MINSTEP, STATUS_QP_FAIL = 0, 1, 2, 3, 4

EXPORTS = ('mpcb_create', 'mpcb_destroy', 'mpcb_last_error', 'mpcb_abi_version',
           'mpcb_workspace_bytes', 'mpcb_path', 'mpcb_solve', 'mpcb_solve_iterate', 'mpcb_linearize',
           'mpcb_sim_step', 'mpcb_gen_inputs', 'mpcb_histogram', 'mpcb_set_timing',
           'mpcb_last_timing', 'mpcb_set_params', 'mpcb_set_t_blast', 'mpcb_qp_stats', 'mpcb_poc_jacobians',
           'mpcb_quat_ops', 'mpcb_plan_kernels', 'mpcb_last_kernels', 'mpcb_eval', 'mpcb_solve_vjp',
           'mpcb_solve_vjp_w', 'mpcb_set_weights', 'mpcb_solve_gains', 'mpcb_solve_iterate_pw',
           'mpcb_solve_vjp_pw', 'mpcb_sim_step_pm', 'mpcb_solve_iterate_pm', 'mpcb_solve_gains_pm',
           'mpcb_sim_step_vjp')
# the per-instance-model entry points among them (typed after the version check, like the others
# that joined ABI version 5 without a new number)
EXPORTS_PM = ('mpcb_sim_step_pm', 'mpcb_solve_iterate_pm', 'mpcb_solve_gains_pm')
# ... and the entry points named after the 17/6 model's dimensions (the list above is held to the
# header's names by a letters-only pattern; tests/test_gpu_vjp17.py checks these)
EXPORTS_17 = ('mpcb_solve_vjp17', 'mpcb_sim_step_p17', 'mpcb_sim_step_vjp17', 'mpcb_solve_iterate_pw17',
              'mpcb_solve_vjp_pw17', 'mpcb_solve_vjp17_sx')
# the timing / launch-log slots of the split path (mpcb_last_timing, mpcb_plan_kernels) and of the
# 17/6 model
PHASES_12 = ('nominal', 'riccati', 'forward', 'linearise')
PHASES_17 = ('nominal', 'riccati', 'linearise', '')


class MpcbConfig(ctypes.Structure):
    """Mirror of ``mpcb_config`` (include/mpcb.h)."""

    _fields_ = [
        ('nx', ctypes.c_int32), ('nu', ctypes.c_int32), ('N', ctypes.c_int32),
        ('dtype', ctypes.c_int32), ('box_u', ctypes.c_int32), ('max_as_iter', ctypes.c_int32),
        ('box_x', ctypes.c_int32), ('reserved', ctypes.c_int32),
        ('dt', ctypes.c_double), ('cost_scale', ctypes.c_double),
        ('mass', ctypes.c_double), ('lx', ctypes.c_double), ('ly', ctypes.c_double),
        ('c', ctypes.c_double), ('g', ctypes.c_double), ('t_blast', ctypes.c_double),
        ('J', ctypes.c_double * 9),
        ('Q', ctypes.c_double * (MPCB_MAX_NX * MPCB_MAX_NX)),
        ('R', ctypes.c_double * (MPCB_MAX_NU * MPCB_MAX_NU)),
        ('QN', ctypes.c_double * (MPCB_MAX_NX * MPCB_MAX_NX)),
        ('lbu', ctypes.c_double * MPCB_MAX_NU), ('ubu', ctypes.c_double * MPCB_MAX_NU),
        ('lbx', ctypes.c_double * MPCB_MAX_NX), ('ubx', ctypes.c_double * MPCB_MAX_NX),
    ]


_lib = None


class LibraryMissing(ImportError):
    pass


def load(path: str | None = None):
    """Load (once) and type the shared library; raises LibraryMissing if it is absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get('MPCB_LIB') or LIB_PATH
    if not os.path.exists(p):
        raise LibraryMissing(
            f'{p} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(hipcc --offload-arch=gfx950).  There is no CPU fallback.')
    lib = ctypes.CDLL(p)
    vp, i64, i32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    u64 = ctypes.c_uint64
    lib.mpcb_create.argtypes = [ctypes.POINTER(MpcbConfig), i32, i64, ctypes.POINTER(vp)]
    lib.mpcb_destroy.argtypes = [vp]
    lib.mpcb_last_error.restype = ctypes.c_char_p
    lib.mpcb_last_error.argtypes = []
    lib.mpcb_abi_version.argtypes = []
    lib.mpcb_workspace_bytes.argtypes = [vp]
    lib.mpcb_workspace_bytes.restype = i64
    lib.mpcb_path.argtypes = [vp]
    lib.mpcb_solve.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp]
    lib.mpcb_solve_iterate.argtypes = [vp, i64, vp, i64, vp, vp, vp, i64, vp, i64, vp, i64,
                                       vp, vp, vp, vp, vp]
    lib.mpcb_linearize.argtypes = [vp, i64, vp, vp, vp, i64, vp, vp, vp, vp]
    lib.mpcb_eval.argtypes = [vp, i64, vp, i64, vp, vp, vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp]
    lib.mpcb_solve_vjp.argtypes = [vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    lib.mpcb_solve_vjp_w.argtypes = [vp, i64, vp, vp, vp, vp, vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp,
                                     vp, vp, vp, vp, vp]
    lib.mpcb_set_weights.argtypes = [vp, ctypes.POINTER(dbl), ctypes.POINTER(dbl), ctypes.POINTER(dbl)]
    lib.mpcb_sim_step.argtypes =[vp, i64, vp, vp, vp, i64, dbl, vp, vp]
    lib.mpcb_gen_inputs.argtypes = [vp, i64, u64, u64, i32, vp, vp, i64, vp, i64, vp, vp]
    lib.mpcb_histogram.argtypes = [vp, i64, vp, dbl, dbl, i32, vp, vp]
    lib.mpcb_set_timing.argtypes = [vp, i32]
    lib.mpcb_last_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    lib.mpcb_set_params.argtypes = [vp, i64, vp, i64, i64]
    lib.mpcb_set_t_blast.argtypes = [vp, dbl]
    lib.mpcb_qp_stats.argtypes = [vp, i64, vp, vp]
    lib.mpcb_poc_jacobians.argtypes = [i64, vp, dbl, ctypes.POINTER(dbl), i32, dbl, vp, vp, vp, vp, vp,
                                       vp, vp]
    lib.mpcb_quat_ops.argtypes = [i64, vp, vp, vp, vp, vp, vp]
    lib.mpcb_plan_kernels.argtypes = [ctypes.POINTER(MpcbConfig), i64, i64, i32, i32, ctypes.c_char_p, i64]
    lib.mpcb_last_kernels.argtypes = [vp, ctypes.c_char_p, i64]
    for name in EXPORTS:
        if name not in ('mpcb_last_error', 'mpcb_workspace_bytes', 'mpcb_solve_gains', 'mpcb_solve_iterate_pw',
                        'mpcb_solve_vjp_pw', 'mpcb_sim_step_vjp') + EXPORTS_PM:
            getattr(lib, name).restype = i32
    got = int(lib.mpcb_abi_version())
    if got != ABI_VERSION:
        # a stale library would read arguments of a changed signature as the wrong types
        # (mpcb_set_params gained two arguments in v4), so refuse it before any call
        raise LibraryMissing(f'{p} has C ABI version {got}, this binding expects {ABI_VERSION}: '
                             'rebuild it (__graft_entry__.build())')
    # (typed after the version check: the entry point joined ABI version 5 without a new number, so
    # a library of that version from before it is told apart by the missing symbol)
    if not hasattr(lib, 'mpcb_solve_vjp17'):
        raise LibraryMissing(f'{p} has no mpcb_solve_vjp17: rebuild it (__graft_entry__.build())')
    lib.mpcb_solve_vjp17.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp,
                                     vp, vp, vp]
    lib.mpcb_solve_vjp17.restype = i32
    # (likewise: the gains joined version 5 after it)
    if not hasattr(lib, 'mpcb_solve_gains'):
        raise LibraryMissing(f'{p} has no mpcb_solve_gains: rebuild it (__graft_entry__.build())')
    lib.mpcb_solve_gains.argtypes = [vp, i64, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp]
    lib.mpcb_solve_gains.restype = i32
    # (likewise: the per-instance-weight solve and its product)
    for name in ('mpcb_solve_iterate_pw', 'mpcb_solve_vjp_pw'):
        if not hasattr(lib, name):
            raise LibraryMissing(f'{p} has no {name}: rebuild it (__graft_entry__.build())')
    lib.mpcb_solve_iterate_pw.argtypes = [vp, i64, vp, i64, vp, vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64,
                                          vp, i64, vp, vp, vp, vp, vp]
    lib.mpcb_solve_iterate_pw.restype = i32
    lib.mpcb_solve_vjp_pw.argtypes = [vp, i64, vp, vp, vp, vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64,
                                      vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mpcb_solve_vjp_pw.restype = i32
    # (likewise: the per-instance-model plant step, solve and gains)
    for name in EXPORTS_PM:
        if not hasattr(lib, name):
            raise LibraryMissing(f'{p} has no {name}: rebuild it (__graft_entry__.build())')
        getattr(lib, name).restype = i32
    lib.mpcb_sim_step_pm.argtypes = [vp, i64, vp, vp, vp, i64, vp, i64, dbl, vp, vp]
    lib.mpcb_solve_iterate_pm.argtypes = [vp, i64, vp, i64, vp, vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64,
                                          vp, i64, vp, i64, vp, vp, vp, vp, vp]
    lib.mpcb_solve_gains_pm.argtypes = [vp, i64, vp, vp, vp, vp, vp, i64, vp, i64, vp, vp, vp, vp]
    # (likewise: the reverse mode of the plant step)
    if not hasattr(lib, 'mpcb_sim_step_vjp'):
        raise LibraryMissing(f'{p} has no mpcb_sim_step_vjp: rebuild it (__graft_entry__.build())')
    lib.mpcb_sim_step_vjp.argtypes = [vp, i64, vp, vp, vp, i64, vp, i64, dbl, vp, vp, vp, vp, vp, vp]
    lib.mpcb_sim_step_vjp.restype = i32
    # (likewise: the 17/6 plant step with its parameters as an argument, and its reverse mode)
    for name in ('mpcb_sim_step_p17', 'mpcb_sim_step_vjp17'):
        if not hasattr(lib, name):
            raise LibraryMissing(f'{p} has no {name}: rebuild it (__graft_entry__.build())')
        getattr(lib, name).restype = i32
    lib.mpcb_sim_step_p17.argtypes = [vp, i64, vp, vp, vp, i64, dbl, vp, vp]
    lib.mpcb_sim_step_vjp17.argtypes = [vp, i64, vp, vp, vp, i64, dbl, vp, vp, vp, vp, vp]
    # (likewise: the per-instance-weight solve and its product on the 17/6 model)
    for name in ('mpcb_solve_iterate_pw17', 'mpcb_solve_vjp_pw17'):
        if not hasattr(lib, name):
            raise LibraryMissing(f'{p} has no {name}: rebuild it (__graft_entry__.build())')
        getattr(lib, name).restype = i32
    lib.mpcb_solve_iterate_pw17.argtypes = [vp, i64, vp, i64, vp, vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64,
                                            vp, vp, vp, vp, vp]
    lib.mpcb_solve_vjp_pw17.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64,
                                        vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    # (likewise: the product with active state rows; mpcb_solve_vjp_pw17's arguments and fixed_x)
    if not hasattr(lib, 'mpcb_solve_vjp17_sx'):
        raise LibraryMissing(f'{p} has no mpcb_solve_vjp17_sx: rebuild it (__graft_entry__.build())')
    lib.mpcb_solve_vjp17_sx.restype = i32
    lib.mpcb_solve_vjp17_sx.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64,
                                        vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    if path is None:
        _lib = lib
    return lib


class MpcbError(RuntimeError):
    pass


def kernel_names(fill, full: bool) -> dict:
    """{phase: rocprof kernel name} from mpcb_plan_kernels / mpcb_last_kernels (``fill(buf, len)``
    calls one of them), phases without a launch omitted."""
    buf = ctypes.create_string_buffer(4096)
    check(fill(buf, len(buf)))
    names = buf.value.decode().split('\n')
    keys = PHASES_17 if full else PHASES_12
    return {k: n for k, n in zip(keys, names) if k and n}


def plan_kernels(cfg: MpcbConfig, max_batch: int, B: int, iterate: bool = False, want_traj: bool = True) -> dict:
    """The kernels a handle of (cfg, max_batch) launches for a solve of B instances, without a
    device (include/mpcb.h mpcb_plan_kernels)."""
    lib = load()
    return kernel_names(lambda b, n: lib.mpcb_plan_kernels(ctypes.byref(cfg), int(max_batch), int(B),
                                                           1 if iterate else 0, 1 if want_traj else 0, b, n),
                        cfg.nx == 17)


def check(rc: int):
    if rc != 0:
        msg = load().mpcb_last_error()
        raise MpcbError(f'mpcb error {rc}: {msg.decode() if msg else ""}')
