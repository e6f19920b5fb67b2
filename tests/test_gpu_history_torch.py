"""The torch layer (mpc_blaster_amd/autograd.py) on a handle with a history: forward and backward
passes interleaved with one another and with other calls, and handle state changed between a forward
pass and its backward pass.

Interleaving.  Several forward passes on one handle, their backward passes in either order, other
entry points in between: each gradient equals, bit for bit, the gradient of the same forward and
backward pass run alone on a fresh handle, and lies within BOUND['f64'] of tests/test_gpu_vjp.py
(1e-9, its metric ``relerr``) of the NumPy reference of the product tests (vjp_ref, simvjp_ref,
vjp17_ref; closed_loop_diff: the quotients and the bound of tests/test_gpu_simvjp.py).

State changed in between.  Every gradient of the step reads the handle's weights and vehicle again
in the backward pass.  ``_either`` states the contract: the backward pass returns the gradient of the
problem the forward pass solved (within the bound of the reference computed with the forward's
weights and model) or raises ``RuntimeError``, never anything else.  The layer's rule is to raise
(module docstring of autograd.py), which each case asserts as well; where the backward pass does not
read the state (a ``model`` record in the plant step, all three per-instance weights) it must go
through.  tests/test_autograd_versions_cpu.py holds the same table without a GPU.

Cases: 12/4 fp64 with and without the input box, B = 7 and 5, N = 8 (the draws of
tests/test_gpu_vjp_weights.py), and the boxed 17/6 fp64 case of tests/vjp17_ref.py.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_call as ab   # noqa: E402
import simvjp_ref as sr   # noqa: E402
import vjp17_ref as vr   # noqa: E402
from pm_ref import pack_params, pm_models   # noqa: E402
from pw_ref import pw_vjp_ref   # noqa: E402
from vjp_ref import vjp_ref   # noqa: E402

from oracle.ocp import OcpSpec   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from test_gpu_vjp import BOUND, LB, UB, _mpc, relerr   # noqa: E402
from test_gpu_vjp_weights import _case, _vec_weights   # noqa: E402

N, BA, BB = 8, 7, 5
KEYS = ('gx0', 'gxref', 'guref')
BOXES = [False, True]


def _t(a, grad=False):
    return None if a is None else torch.tensor(np.asarray(a), dtype=torch.float64, device='cuda', requires_grad=grad)


def _kw(box):
    return dict(lbu=LB, ubu=UB) if box else {}


def _spec(box, **kw):
    """The handle's definition; a changed Q leaves QN at the default the handle keeps."""
    return OcpSpec(N=N, lbu=LB if box else None, ubu=UB if box else None, **dict(dict(QN=OcpSpec(N=N).QN), **kw))


def _cases(box):
    """Two forward passes with different inputs and different B."""
    return _case(BA, N, 'hover', False, box), _case(BB, N, 'sine', True, box)


class Pass:
    """One forward pass of ``solve_iterate_diff`` on ``m`` and its loss sum w0 u0 + sum wX X."""

    def __init__(self, m, c, seed, **kw):
        B = c['x0'].shape[0]
        rng = np.random.default_rng(seed)
        self.c, self.m = c, m
        self.w0, self.wX = rng.standard_normal((B, m.nu)), rng.standard_normal((B, m.cfg.N + 1, m.nx))
        self.leaves = [_t(c[k], True) for k in ('x0', 'xref', 'uref')]
        self.u0, self.X, self.U = m.solve_iterate_diff(self.leaves[0], c['xbar'], c['ubar'], self.leaves[1], self.leaves[2],
                                                       wind=c.get('wind'), **kw)
        self.status = m.get_status().clone()
        self.gU = np.zeros(c['ubar'].shape)
        self.gU[:, 0] = self.w0

    def backward(self):
        ((_t(self.w0) * self.u0).sum() + (_t(self.wX) * self.X).sum()).backward()
        return [t.grad for t in self.leaves]

    def check(self, ref, tag):
        """The leaves' gradients against a reference; an instance whose forward status is not 0 has
        zero gradients (module docstring of autograd.py)."""
        st = self.status.cpu().numpy()
        for t, k in zip(self.leaves, KEYS):
            want = np.where((st == 0).reshape(-1, *([1] * (ref[k].ndim - 1))), ref[k], 0.0)
            e = relerr(t.grad.cpu().numpy(), want).max()
            print(f'{tag}: {k} {e:.2e}/{BOUND["f64"]:.0e} (status != 0: {int((st != 0).sum())})')
            assert e <= BOUND['f64'], (tag, k, e)

    def ref(self, spec):
        c = self.c
        return vjp_ref(c['xbar'], c['ubar'], self.U.detach().cpu().numpy(), self.wX, self.gU, spec, c.get('wind'))


def _alone(box, c, seed):
    """The same forward and backward pass alone on a fresh handle."""
    m = _mpc(N, BA, **_kw(box))
    p = Pass(m, c, seed)
    return p.backward()


# ------------------------------------------------------------------------------ interleaved
@pytest.mark.parametrize('first', ['a', 'b'])
@pytest.mark.parametrize('box', BOXES)
def test_two_solve_forwards_backward_in_either_order(box, first):
    ca, cb = _cases(box)
    m = _mpc(N, BA, **_kw(box))
    pa, pb = Pass(m, ca, 31), Pass(m, cb, 32)
    for p in ((pa, pb) if first == 'a' else (pb, pa)):
        p.backward()
    for p, c, seed, tag in ((pa, ca, 31, 'a'), (pb, cb, 32, 'b')):
        for g, want, k in zip([t.grad for t in p.leaves], _alone(box, c, seed), KEYS):
            assert ab.same_bits(g, want), f'forward {tag}, {k}: not the bits of the pass run alone (box={box}, first={first})'
        p.check(p.ref(_spec(box)), f'interleaved box={box} first={first} forward {tag}')
    if box:
        assert bool(((pa.U <= LB[0]) | (pa.U >= UB[0])).any())   # the active set is not empty


SIM_SPEC = OcpSpec(N=3)


def _sim_case(B, seed):
    rng = np.random.default_rng(seed)
    return dict(x=rng.uniform(-0.5, 0.5, (B, 12)), u=rng.uniform(0, 65, (B, 4)), wind=rng.uniform(-2, 2, (B, 3)),
                M=pm_models(B, SIM_SPEC), g=rng.standard_normal((B, 12)))


class SimPass:
    def __init__(self, m, c, model):
        self.c, self.model = c, model
        self.leaves = [_t(c['x'], True), _t(c['u'], True), _t(c['wind'], True)]
        self.M = _t(c['M'], True) if model else None
        self.xo = m.sim_step_diff(self.leaves[0], self.leaves[1], wind=self.leaves[2], model=self.M)

    def backward(self):
        (_t(self.c['g']) * self.xo).sum().backward()
        return [t.grad for t in self.leaves] + ([self.M.grad] if self.model else [])

    def check(self, tag):
        c = self.c
        M = c['M'] if self.model else pack_params(SIM_SPEC.params)[None]
        ref = sr.simvjp_ref(c['x'], c['u'], c['g'], SIM_SPEC.dt, SIM_SPEC, M, c['wind'])
        for g, k in zip(self.backward_grads(), ('gx', 'gu', 'gwind', 'gmodel')):
            e = relerr(g.cpu().numpy(), ref[k]).max()
            print(f'{tag}: {k} {e:.2e}/{BOUND["f64"]:.0e}')
            assert e <= BOUND['f64'], (tag, k, e)

    def backward_grads(self):
        return [t.grad for t in self.leaves] + ([self.M.grad] if self.model else [])


@pytest.mark.parametrize('first', ['a', 'b'])
def test_two_sim_step_forwards_backward_in_either_order(first):
    """One with vehicle records at B = 7, one with the handle's own vehicle at B = 5."""
    ca, cb = _sim_case(BA, 4), _sim_case(BB, 5)
    m = _mpc(3, BA)
    pa, pb = SimPass(m, ca, True), SimPass(m, cb, False)
    for p in ((pa, pb) if first == 'a' else (pb, pa)):
        p.backward()
    for p, c, model, tag in ((pa, ca, True, 'a'), (pb, cb, False, 'b')):
        alone = SimPass(_mpc(3, BA), c, model).backward()
        for g, want in zip(p.backward_grads(), alone):
            assert ab.same_bits(g, want), f'plant step {tag}: not the bits of the pass run alone (first={first})'
        p.check(f'interleaved plant steps first={first} forward {tag}')


@pytest.mark.parametrize('box', BOXES)
def test_closed_loop_diff_backward_after_other_calls(box):
    """closed_loop_diff (nsim = 3, the frozen case of tests/test_gpu_simvjp.py), then an unrelated
    closed_loop, solve_iterate_gains and evaluate on the same handle, then the backward pass: the
    bits of the run alone on a fresh handle, and the reference's quotients within that test's bound."""
    from mpc_blaster_amd.closed_loop import closed_loop, closed_loop_diff
    case = sr.loop_case(box)
    B, Nl, nsim = sr.LOOP_B, sr.LOOP_N, sr.LOOP_NSIM
    assert nsim == 3
    kw = dict(lbu=sr.LOOP_LB, ubu=sr.LOOP_UB) if box else {}
    th = {k: _t(v) for k, v in case['theta'].items()}
    xbar, ubar, w = (_t(case[k]) for k in ('xbar', 'ubar', 'w'))

    def forward(m):
        leaves = {k: v.clone().requires_grad_(True) for k, v in th.items()}
        X, U, st = closed_loop_diff(m, leaves['x0'], leaves['xref'], leaves['uref'], nsim, xbar, ubar,
                                    weights=dict(Q=leaves['Q'], R=leaves['R'], QN=leaves['QN']),
                                    plant_model=leaves['plant_model'], warm_start=False)
        assert int(st.max()) == 0
        return leaves, X

    m = _mpc(Nl, B, **kw)
    leaves, X = forward(m)
    Xs, Us, _ = closed_loop(m, th['x0'] + 0.01, th['xref'], th['uref'], 2, xbar=xbar, ubar=ubar)
    m.solve_iterate_gains(xbar, ubar, U=ubar)
    m.evaluate(xbar, ubar, th['xref'], th['uref'])
    (w * X).sum().backward()
    alone, Xa = forward(_mpc(Nl, B, **kw))
    (w * Xa).sum().backward()
    for k in sr.LOOP_KEYS:
        assert ab.same_bits(leaves[k].grad, alone[k].grad), f'{k}: not the bits of the loop run alone (box={box})'
    quot, same = sr.loop_quotients(case)
    assert same
    bound = max(1e-9, 10.0 * sr.LOOP_SELF[box])
    for d, q in zip(case['dirs'], quot):
        ip = sum(float((leaves[k].grad.cpu().numpy() * d[k]).sum()) for k in sr.LOOP_KEYS)
        e = abs(ip - q) / max(abs(q), 1.0)
        print(f'closed_loop_diff after other calls box={box}: <grad, d> {ip:.10g}  quotient {q:.10g}  error {e:.2e}/{bound:.1e}')
        assert e <= bound


# ------------------------------------------------------------------------------ state changed in between
def _either(backward, check, must_raise, tag):
    """The contract: the gradient of the problem the forward pass solved (``check`` asserts the bound
    against the reference computed with the forward's weights and model) or ``RuntimeError``, never
    anything else; and the layer's own rule, which of the two."""
    try:
        backward()
    except RuntimeError as e:
        print(f'{tag}: raised: {str(e)[:70]}')
        raised = True
    else:
        check()
        raised = False
    assert raised == must_raise, f'{tag}: the backward pass {"went through" if must_raise else "raised"}'


@pytest.mark.parametrize('box', BOXES)
def test_set_weights_after_a_forward_without_weight_arguments(box):
    c = _cases(box)[0]
    m = _mpc(N, BA, **_kw(box))
    p = Pass(m, c, 33)
    m.set_weights(Q=2.0 * _vec_weights(OcpSpec(N=N))[0])
    _either(p.backward, lambda: p.check(p.ref(_spec(box)), 'stale Q'), True, f'set_weights after forward, box={box}')
    assert all(t.grad is None for t in p.leaves)
    # the control: a new forward pass sees the handle as it is now
    p = Pass(m, c, 33)
    p.backward()
    p.check(p.ref(_spec(box, Q=np.diag(2.0 * _vec_weights(OcpSpec(N=N))[0]))), f'control, box={box}')


@pytest.mark.parametrize('box', BOXES)
def test_second_forward_with_other_weight_tensors(box):
    """Only x0 (and the references) require a gradient; the weight tensors do not."""
    c = _cases(box)[0]
    q = _vec_weights(OcpSpec(N=N))[0]
    m = _mpc(N, BA, **_kw(box))
    p1 = Pass(m, c, 34, Q=_t(1.5 * q))
    p2 = Pass(m, c, 35, Q=_t(0.5 * q))
    _either(p1.backward, lambda: p1.check(p1.ref(_spec(box, Q=np.diag(1.5 * q))), 'first'), True,
            f'second forward with other weights, box={box}')
    p2.backward()
    p2.check(p2.ref(_spec(box, Q=np.diag(0.5 * q))), f'the second forward itself, box={box}')


@pytest.mark.parametrize('omit', ['Q', 'R', 'QN', None])
@pytest.mark.parametrize('box', BOXES)
def test_per_instance_weights_with_one_omitted(box, omit):
    """An omitted per-instance weight falls back to the handle's, so set_weights in between makes
    the backward pass stale; with all three given it reads no weight of the handle."""
    c = _cases(box)[0]
    spec = _spec(box)
    rng = np.random.default_rng(36)
    dflt = dict(zip(('Q', 'R', 'QN'), _vec_weights(spec)))
    wts = {k: v * rng.uniform(0.7, 1.3, (BA, v.size)) for k, v in dflt.items()}
    given = {k: _t(v) for k, v in wts.items() if k != omit}
    m = _mpc(N, BA, **_kw(box))
    p = Pass(m, c, 37, per_instance_weights=True, **given)
    m.set_weights(**{(omit or 'Q'): 2.0 * dflt[omit or 'Q']})

    def check():
        full = {k: np.stack([np.diag(r) for r in (wts[k] if k != omit else np.tile(dflt[k], (BA, 1)))]) for k in dflt}
        U = p.U.detach().cpu().numpy()
        ref = pw_vjp_ref(c['xbar'], c['ubar'], p.X.detach().cpu().numpy(), U, c['xref'], c['uref'], p.wX, p.gU, spec,
                         full['Q'], full['R'], full['QN'], c.get('wind'))
        p.check(ref, f'per-instance weights, {omit} omitted, box={box}')

    _either(p.backward, check, omit is not None, f'per-instance weights, {omit} omitted, box={box}')


@pytest.mark.parametrize('box', BOXES)
def test_set_t_blast_between_forward_and_backward_of_the_solve(box):
    c = _cases(box)[0]
    m = _mpc(N, BA, **_kw(box))
    p = Pass(m, c, 38)
    m.set_t_blast(2.5)
    _either(p.backward, lambda: p.check(p.ref(_spec(box)), 'stale T_blast'), True, f'set_t_blast after forward, box={box}')


def test_set_t_blast_between_forward_and_backward_of_the_plant_step():
    c = _sim_case(BA, 6)
    m = _mpc(3, BA)
    own, rec = SimPass(m, c, False), SimPass(m, c, True)
    m.set_t_blast(2.5)
    _either(own.backward, lambda: own.check('stale T_blast, own vehicle'), True, 'plant step, model=None')
    # a record carries the whole vehicle: the step does not depend on the handle's and goes through
    _either(rec.backward, lambda: rec.check('records given'), False, 'plant step, records given')


# ------------------------------------------------------------------------------ 17/6
def _mpc17(Nf, B):
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    return BatchedMPC(MPCConfig.full(N=Nf, lbu=vr.LBU17, ubu=vr.UBU17), max_batch=B)


def _case17():
    spec, c = vr.boxed_case()
    c = {k: np.array(v) for k, v in c.items()}
    B2 = 5
    c2 = {k: v[:B2].copy() for k, v in c.items()}
    c2['x0'] = c2['x0'] + 0.01   # other inputs, the parameter rows of the same instances
    return spec, c, c2


def _ref17(p, spec):
    fixed = p.m.active_mask17(p.U.detach()).cpu().numpy().astype(bool)
    c = p.c
    return vr.vjp17_ref(c['xbar'], c['ubar'], c['p'], fixed, p.wX, p.gU, spec), fixed


@pytest.mark.parametrize('first', ['a', 'b'])
def test_full17_two_forwards_backward_in_either_order(first):
    spec, ca, cb = _case17()
    B, Nf = ca['ubar'].shape[:2]
    m = _mpc17(Nf, B)
    m.set_params(ca['p'])
    pa, pb = Pass(m, ca, 41), Pass(m, cb, 42)
    assert (pa.status == 0).all() and (pb.status == 0).all()
    for p in ((pa, pb) if first == 'a' else (pb, pa)):
        p.backward()
    for p, c, seed, tag in ((pa, ca, 41, 'a'), (pb, cb, 42, 'b')):
        m2 = _mpc17(Nf, B)
        m2.set_params(ca['p'])
        alone = Pass(m2, c, seed).backward()
        for g, want, k in zip([t.grad for t in p.leaves], alone, KEYS):
            assert ab.same_bits(g, want), f'17/6 forward {tag}, {k}: not the bits of the pass run alone (first={first})'
        ref, fixed = _ref17(p, spec)
        assert fixed.any()
        p.check(ref, f'17/6 interleaved first={first} forward {tag}')


def test_full17_set_params_between_forward_and_backward():
    spec, c, _ = _case17()
    B, Nf = c['ubar'].shape[:2]
    m = _mpc17(Nf, B)
    m.set_params(c['p'])
    p = Pass(m, c, 43)
    p2 = 1.05 * c['p']
    m.set_params(p2)
    _either(p.backward, lambda: p.check(_ref17(p, spec)[0], 'stale parameters'), True, '17/6 set_params after forward')
    p = Pass(m, dict(c, p=p2), 43)   # the control: forward and backward under the new parameters
    p.backward()
    p.check(_ref17(p, spec)[0], '17/6 control under the new parameters')
