"""The version logic of mpc_blaster_amd/autograd.py without a GPU: which sequences of forward pass,
setter and backward pass raise, and which go through.

``solve_iterate_diff`` and ``sim_step_diff`` run on CPU tensors against a stub that has the attributes
and methods the layer calls on a ``BatchedMPC`` and returns fixed tensors; its setters bump the
versions exactly as ``BatchedMPC``'s do (tests/test_gpu_history_torch.py holds the real handle to the
same table).  The rule under test (module docstring of autograd.py): every gradient of the step reads
the handle's weights and vehicle again in the backward pass, so a backward pass after ``set_weights``,
``set_t_blast`` or ``set_params`` raises ``RuntimeError`` naming the setter, except where it reads
none of that state: per-instance weights with all of Q, R, QN given (weights), the plant step with a
``model`` record (vehicle).
"""
import types

import pytest

torch = pytest.importorskip('torch')

from mpc_blaster_amd.autograd import sim_step_diff, solve_iterate_diff   # noqa: E402

B, N = 3, 2


class Stub:
    """The surface of ``BatchedMPC`` that the layer touches; every result is a constant tensor."""

    def __init__(self, nx=12, nu=4, boxed=False):
        self.nx, self.nu, self.dtype, self._tdev = nx, nu, torch.float64, torch.device('cpu')
        self.cfg = types.SimpleNamespace(N=N, lbx=None, boxed=boxed, dtype='f64', dt=0.05)
        self._weights_version = self._model_version = 0
        self._model_setter = None
        self.calls = []

    def _dev(self, t, shape_tail, name, batch=None, allow_broadcast=False):
        t = torch.as_tensor(t, dtype=self.dtype)
        if t.dim() == len(shape_tail):
            t = t.unsqueeze(0)
        return t.contiguous(), (0 if batch is not None and t.shape[0] != batch else 1)

    def _model_arg(self, model, Bn):
        t = torch.as_tensor(model, dtype=self.dtype)
        return (t if t.dim() == 2 else t.unsqueeze(0)), 14

    def set_weights(self, Q=None, R=None, QN=None):
        self._weights_version += 1

    def set_t_blast(self, v):
        self._model_version += 1
        self._model_setter = 'set_t_blast'

    def set_params(self, p):
        self._model_version += 1
        self._model_setter = 'set_params'

    def solve_iterate(self, x0, xbar, ubar, x_ref, u_ref, wind=None, Q=None, R=None, QN=None):
        self.calls.append('solve_iterate')
        return torch.ones(B, self.nu, dtype=self.dtype)

    def get_state_trajectory(self):
        return torch.ones(B, N + 1, self.nx, dtype=self.dtype)

    def get_input_trajectory(self):
        return torch.ones(B, N, self.nu, dtype=self.dtype)

    def get_status(self):
        return torch.zeros(B, dtype=torch.int32)

    def active_mask17(self, U, active_tol=None):
        return None

    def solve_iterate_vjp(self, xbar, ubar, gX=None, gU=None, U=None, weights=False, **kw):
        self.calls.append('vjp')
        out = dict(gx0=torch.full((B, self.nx), 2.0, dtype=self.dtype),
                   gxref=torch.full((B, N + 1, self.nx), 3.0, dtype=self.dtype),
                   guref=torch.full((B, N, self.nu), 4.0, dtype=self.dtype))
        if weights:
            out.update(gQ=torch.ones(B, self.nx, self.nx, dtype=self.dtype), gR=torch.ones(B, self.nu, self.nu, dtype=self.dtype),
                       gQN=torch.ones(B, self.nx, self.nx, dtype=self.dtype))
        return out

    def sim_step(self, x, u, T=None, wind=None, model=None):
        return torch.ones(B, self.nx, dtype=self.dtype)

    def sim_step_vjp(self, x, u, gxn, T=None, wind=None, model=None, want=('gx', 'gu')):
        self.calls.append('sim_vjp')
        cols = dict(gx=self.nx, gu=self.nu, gwind=3, gmodel=14)
        return {k: torch.full((B, cols[k]), 5.0, dtype=self.dtype) for k in want}


def _z(*shape, grad=False):
    return torch.zeros(*shape, dtype=torch.float64, requires_grad=grad)


def _forward(m, **kw):
    x0 = _z(B, m.nx, grad=True)
    u0, X, U = solve_iterate_diff(m, x0, _z(B, N + 1, m.nx), _z(B, N, m.nu), _z(B, N + 1, m.nx), _z(B, N, m.nu), **kw)
    return x0, X


def _pw(nx=12, nu=4, grad=False):
    return dict(Q=torch.ones(B, nx, dtype=torch.float64, requires_grad=grad), R=torch.ones(B, nu, dtype=torch.float64),
                QN=torch.ones(B, nx, dtype=torch.float64))


def _goes_through(x0, X, m):
    X.sum().backward()
    assert torch.equal(x0.grad, torch.full((B, m.nx), 2.0, dtype=torch.float64))
    assert m.calls[-1] == 'vjp'


def _raises(x0, X, m, match):
    before = m.calls.count('vjp')
    with pytest.raises(RuntimeError, match=match):
        X.sum().backward()
    assert x0.grad is None and m.calls.count('vjp') == before   # refused before the product is called


# ------------------------------------------------------------------------------ weights
def test_nothing_in_between_goes_through():
    m = Stub()
    _goes_through(*_forward(m), m)
    _goes_through(*_forward(m, Q=torch.ones(12, dtype=torch.float64, requires_grad=True)), m)
    _goes_through(*_forward(m, per_instance_weights=True, **_pw()), m)


def test_set_weights_after_a_forward_without_weight_arguments_raises():
    m = Stub()
    x0, X = _forward(m)
    m.set_weights(Q=torch.ones(12))
    _raises(x0, X, m, 'set_weights')


def test_set_weights_after_a_forward_with_weight_arguments_raises():
    m = Stub()
    q = torch.ones(12, dtype=torch.float64, requires_grad=True)
    x0, X = _forward(m, Q=q)
    m.set_weights(Q=torch.ones(12))
    _raises(x0, X, m, 'set_weights')
    assert q.grad is None


def test_second_forward_with_other_weight_tensors_raises_for_the_first_only():
    """Only x0 requires a gradient; the second forward installs its own weights."""
    m = Stub()
    x0a, Xa = _forward(m, Q=torch.ones(12, dtype=torch.float64))
    x0b, Xb = _forward(m, Q=2.0 * torch.ones(12, dtype=torch.float64))
    _raises(x0a, Xa, m, 'another forward pass with weight tensors')
    _goes_through(x0b, Xb, m)


def test_second_forward_without_weight_arguments_leaves_the_first_valid():
    m = Stub()
    x0a, Xa = _forward(m)
    x0b, Xb = _forward(m)
    _goes_through(x0b, Xb, m)
    _goes_through(x0a, Xa, m)


@pytest.mark.parametrize('omit', ['Q', 'R', 'QN'])
def test_per_instance_weights_with_one_omitted_fall_back_to_the_handle_and_raise(omit):
    m = Stub()
    w = _pw()
    w.pop(omit)
    x0, X = _forward(m, per_instance_weights=True, **w)
    m.set_weights(Q=torch.ones(12))
    _raises(x0, X, m, 'set_weights')


@pytest.mark.parametrize('grad', [False, True])
def test_per_instance_weights_all_given_do_not_read_the_handle(grad):
    m = Stub()
    w = _pw(grad=grad)
    x0, X = _forward(m, per_instance_weights=True, **w)
    m.set_weights(Q=torch.ones(12))
    _goes_through(x0, X, m)
    assert (w['Q'].grad is not None) == grad


# ------------------------------------------------------------------------------ model
@pytest.mark.parametrize('kw', [{}, dict(Q=torch.ones(12, dtype=torch.float64)), 'pw'])
def test_set_t_blast_between_forward_and_backward_raises(kw):
    m = Stub()
    x0, X = _forward(m, **(dict(per_instance_weights=True, **_pw()) if kw == 'pw' else kw))
    m.set_t_blast(2.5)
    _raises(x0, X, m, 'set_t_blast')


def test_set_params_between_forward_and_backward_raises_on_17_6():
    m = Stub(17, 6)
    x0, X = _forward(m)
    m.set_params(torch.zeros(25))
    _raises(x0, X, m, 'set_params')
    x0, X = _forward(m)
    _goes_through(x0, X, m)   # a forward after the setter is valid again
    x0, X = _forward(m)
    m.set_params(None)
    _raises(x0, X, m, 'set_params')


def test_setter_before_the_forward_is_no_refusal():
    m = Stub()
    m.set_weights(Q=torch.ones(12))
    m.set_t_blast(1.0)
    _goes_through(*_forward(m), m)


# ------------------------------------------------------------------------------ plant step
def _sim(m, model=None):
    x, u = _z(B, 12, grad=True), _z(B, 4, grad=True)
    return x, u, sim_step_diff(m, x, u, model=model)


def test_sim_step_without_a_record_reads_the_handles_vehicle():
    m = Stub()
    x, u, xo = _sim(m)
    xo.sum().backward()
    assert torch.equal(x.grad, torch.full((B, 12), 5.0, dtype=torch.float64)) and u.grad is not None
    x, u, xo = _sim(m)
    m.set_t_blast(2.5)
    with pytest.raises(RuntimeError, match='set_t_blast'):
        xo.sum().backward()
    assert x.grad is None and m.calls.count('sim_vjp') == 1


def test_sim_step_with_a_record_goes_through():
    m = Stub()
    rec = torch.ones(B, 14, dtype=torch.float64, requires_grad=True)
    x, u, xo = _sim(m, rec)
    m.set_t_blast(2.5)
    xo.sum().backward()
    assert x.grad is not None and rec.grad is not None


def test_sim_step_does_not_read_the_weights():
    m = Stub()
    x, u, xo = _sim(m)
    m.set_weights(Q=torch.ones(12))
    xo.sum().backward()
    assert x.grad is not None


def test_two_interleaved_forwards_keep_their_own_versions():
    m = Stub()
    xa, ua, xoa = _sim(m)
    m.set_t_blast(2.5)
    xb, ub, xob = _sim(m)
    xob.sum().backward()
    assert xb.grad is not None
    with pytest.raises(RuntimeError, match='set_t_blast'):
        xoa.sum().backward()
