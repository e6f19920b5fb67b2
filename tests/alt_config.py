"""The alternative problem definition ALT shared by tests/test_gpu_config.py and the CPU oracle
tests; a helper, not a test.  Every ``mpcb_config`` field differs from its default and no two
channels or matrix entries are alike, so a transposed weight table, ``dt`` used for ``cost_scale``,
one channel's bound used for all, or two model constants swapped cannot cancel out.
"""
import numpy as np

from oracle.model import Params

SB_LO = np.array([-1.5, -1.5, 0, -0.174532925, -0.174532925, -0.349066, -1.0, -1.0, -1.0, -0.0872665, -0.0872665,
                  -0.0872665, -0.174532925, -0.523599, -1.5, -1.5, -2.5])
SB_HI = np.array([1.5, 1.5, 5.0, 0.174532925, 0.174532925, 0.349066, 1.0, 1.0, 1.0, 0.0872665, 0.0872665,
                  0.0872665, 1.22173, 0.523599, 1.5, 1.5, 2.5])


def spd(rng, n, scale):
    m = rng.normal(size=(n, n))
    return scale * (m @ m.T / n + np.eye(n))


def _dense(seed, nx, nu):
    rng = np.random.default_rng(seed)
    return {'Q': spd(rng, nx, 5.0), 'R': spd(rng, nu, 0.1), 'QN': spd(rng, nx, 50.0)}


def weights12():
    """Dense SPD weights, as _weights('dense') of tests/test_gpu_c2_trim.py; QN is no multiple of Q."""
    return _dense(7, 12, 4)


def weights17():
    return _dense(11, 17, 6)


def model():
    J = np.diag([0.31, 0.58, 0.66])
    J[0, 1] = J[1, 0] = 0.02
    J[1, 2] = J[2, 1] = -0.015
    return dict(mass=6.5, J=J, lx=0.21, ly=0.40, c=0.05, g=9.5, t_blast=4.0)


# ALT-a leaves cost_scale at its default (= dt); only ALT-b tells the two fields apart
TIME = {'a': dict(dt=0.02), 'b': dict(dt=0.05, cost_scale=1.0)}

LBU12, UBU12 = np.array([2.0, 0.0, 5.0, 1.0]), np.array([40.0, 65.0, 22.0, 50.0])
LBU17 = np.array([2.0, 0.0, 5.0, 1.0, -0.05, -0.12])
UBU17 = np.array([40.0, 65.0, 22.0, 50.0, 0.09, 0.03])
LBX17, UBX17 = 1.1 * SB_LO - 0.01, 0.9 * SB_HI + 0.02

GROUPS = ('weights', 'model', 'time', 'box')


def _r32(v):
    """A config value as an fp32 handle holds it."""
    if isinstance(v, np.ndarray):
        return v.astype(np.float32).astype(np.float64)
    return float(np.float32(v))


def fields(full=False, alt='a', groups=GROUPS, box='input', dtype='f64'):
    """The MPCConfig keyword fields of ALT restricted to ``groups`` (the others keep their
    defaults); ``box``: 'none' | 'input' | 'all' (the group 'box' swaps the default box for
    ALT's; without it a boxed case keeps [0, 65] / the reference's 17/6 box).  fp32 handles hold
    their values in fp32, so for ``dtype='f32'`` the fields are rounded first: the oracle sees
    what the device sees."""
    kw = {}
    if 'weights' in groups:
        kw.update(weights17() if full else weights12())
    if 'model' in groups:
        kw.update(model())
    if 'time' in groups:
        kw.update(TIME[alt])
    if box != 'none':
        if 'box' in groups:
            kw.update(lbu=LBU17 if full else LBU12, ubu=UBU17 if full else UBU12)
        else:
            kw.update(lbu=np.r_[np.zeros(4), [-0.0872665] * 2] if full else np.zeros(4),
                      ubu=np.r_[np.full(4, 65.0), [0.0872665] * 2] if full else np.full(4, 65.0))
        if box == 'all':
            kw.update(lbx=LBX17 if 'box' in groups else SB_LO, ubx=UBX17 if 'box' in groups else SB_HI)
    if dtype == 'f32':
        kw = {k: _r32(v) for k, v in kw.items()}
    return kw


_MODEL_KEYS = ('mass', 'J', 'lx', 'ly', 'c', 'g', 't_blast')


def spec_kwargs(kw):
    """MPCConfig fields -> OcpSpec / FullSpec fields (the model constants go into Params)."""
    out = {k: v for k, v in kw.items() if k not in _MODEL_KEYS}
    mk = {k: v for k, v in kw.items() if k in _MODEL_KEYS}
    if mk:
        out['params'] = Params(**mk)
    return out
