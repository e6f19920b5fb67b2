"""The C ABI's calling conventions (include/mpcb.h) on every kernel path.

The rest of the GPU suite reaches the library through ``BatchedMPC``: contiguous tensors, packed
strides or 0, fresh 256-byte aligned outputs, torch's default stream.  It checks what the kernels
compute and nothing about where they read and write.  Here tests/abi_call.py calls the ABI as a
plain C consumer may: padded odd strides, element-aligned bases, broadcast arrays, outputs that
alias the iterate, one of X / U alone, a stream of the caller's own, and every output inside a
guard band of sentinels.

Every path of tests/test_gpu_config.py's PATHS table and the 17/6 model with bounds none / input /
all, at that file's horizons, under the DEFAULT problem definition, with wind on every 12/4 case.
Per case one baseline: a contiguous, default-stream, separate-output raw call, held once to the CPU
oracle by the acceptance functions of tests/test_gpu_config.py (test_baseline_matches_oracle).
Every variant must then reproduce the baseline's u0, X, U and status BIT FOR BIT: per-instance
arithmetic depends on no address, stride, stream or neighbour.  (Reading the code found no stride
that selects other arithmetic: the ``uref_sb == 0`` LDS staging of mpcb_split.hip only moves loads.)

Shapes: B = 7 on the 16-lane paths (a full quad and a ragged one of 3), B = 70 on the thread-per-
instance and single-kernel paths (a full wave and 6), every handle with max_batch > B, and one
chunked case per model (MPCB_CHUNK=64, B = 70: the second chunk starts at b0 = 64).

Header argument -> variant that passes it a non-packed value
    mpcb_solve / mpcb_solve_iterate  x0_sb, xref_sb, uref_sb, wind_sb   padded (b), broadcast (c)
      u0, status element-aligned; X, U exactly 16-byte aligned          guards (a), padded (b)
      X / U alias xbar / ubar                                            in place (d)
      X or U NULL                                                        partial (e)
      hip_stream                                                         stream (f)
    mpcb_eval            x0_sb, xref_sb, uref_sb, wind_sb               test_eval_strides
    mpcb_solve_vjp_w     xref_sb, uref_sb, wind_sb                      test_vjp_w_strides
    mpcb_solve_vjp17     xref_sb, uref_sb                               test_vjp17_strides_and_params
    mpcb_set_params      params_sb, params_kb                           test_vjp17_strides_and_params,
                                                                        test_set_params_strides
    mpcb_linearize, mpcb_sim_step   wind_sb                             test_linearize_and_sim_step_strides
    mpcb_gen_inputs      xref_sb, uref_sb                               test_gen_inputs_strides
    mpcb_qp_stats, mpcb_histogram   (outputs only)                      test_stats_and_histogram_outputs
    every stride above, negative                                         test_refusals, test_negative_strides_*
Nothing here faults by design: every access a test provokes lies inside an allocation it owns.
"""
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_call as ab   # noqa: E402
import alt_config as ac   # noqa: E402
import test_gpu_config as gc   # noqa: E402

from oracle.full import FullSpec, mpc_solve17   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

E_INVALID = -1
MARGIN = 9   # handle rows beyond the batch, which a call must not touch


# ------------------------------------------------------------------------------ cases
class K:
    """One (path, dtype, horizon, batch) of a model; ``chunk``: MPCB_CHUNK=64."""

    def __init__(self, model, path, dtype, N, B, chunk=False, modes=gc.MODES):
        self.model, self.path, self.dtype, self.N, self.B, self.chunk, self.modes = model, path, dtype, N, B, chunk, modes
        self.id = f'{model}-{path}-{dtype}-N{N}-B{B}' + ('-chunk64' if chunk else '')


KS = [K(12, 'fused', 'f64', 6, 7), K(12, 'two', 'f64', 6, 7), K(12, 'notan', 'f64', 6, 7), K(12, 'row32', 'f32', 6, 7),
      K(12, 'small', 'f64', 6, 7), K(12, 'small', 'f32', 6, 7), K(12, 'single', 'f64', 6, 70),
      K(12, 'single', 'f32', 6, 70), K(12, 'thread', 'f64', 6, 70), K(12, 'thread', 'f32', 6, 70),
      K(12, 'lanequad', 'f64', 130, 7), K(12, 'lanequad', 'f32', 260, 7, modes=('iterate',)),
      K(12, 'box', 'f64', 6, 7), K(12, 'box_ipm', 'f64', 6, 7), K(12, 'box_v1', 'f64', 6, 7),
      # fp32 box, iterate mode at N = 2: at N = 6 the oracle's own fp32 sensitivity of instance 2 is
      # 4.2e-5, above the 1e-5 that test_gpu_config's acceptance calls ill-conditioned, and its
      # allowance of 5 % of a case is no instance of seven (rollout: 8.1e-6 at most; N = 2: 1.4e-6)
      K(12, 'box', 'f32', 6, 7, modes=('rollout',)), K(12, 'box', 'f32', 2, 7),
      K(12, 'fused', 'f64', 6, 70, chunk=True),
      K(17, 'none', 'f64', 7, 7), K(17, 'none', 'f32', 7, 7), K(17, 'input', 'f64', 7, 7), K(17, 'input', 'f32', 7, 7),
      K(17, 'all', 'f64', 7, 7), K(17, 'input', 'f64', 7, 70, chunk=True),
      # N = 2 for the padded parameter strides (_padded_params)
      K(17, 'input', 'f64', 2, 7), K(17, 'input', 'f64', 2, 70, chunk=True)]
CASES = [(k, mode) for k in KS for mode in k.modes]
IDS = [f'{k.id}-{mode}' for k, mode in CASES]
ITER_KS = [k for k in KS if 'iterate' in k.modes]
ITER_CASES = [(k, 'iterate') for k in ITER_KS]
ITER_IDS = [f'{k.id}-iterate' for k in ITER_KS]
BOXED12 = ('box', 'box_ipm', 'box_v1')


def _alt(mode):
    """The default definition has no ALT-a / ALT-b; the letter only picks test_gpu_config's wind
    rule (_use_wind), here so that every 12/4 case has wind."""
    return 'a' if mode == 'iterate' else 'b'


def _np_inputs(k):
    """{name: [B, ...] float64 array as the handle's dtype holds it} of a case, both modes."""
    if k.model == 12:
        return dict(gc._inputs(k.N, k.B, k.dtype))
    return dict(_inputs17(k.N, k.B, k.dtype))


@functools.lru_cache(maxsize=None)
def _inputs17(N, B, dtype):
    """test_gpu_config._inputs17 for B instances."""
    from test_gpu_fuzz17 import inputs
    rng = np.random.default_rng(17)
    x0, xref, uref, p = inputs(B, N, rng, True)
    p[..., 24] = 4.0
    xb = x0[:, None, :] + rng.normal(0, 0.03, (B, N + 1, 17))
    ub = uref + rng.normal(0, 0.5, (B, N, 6))
    c = gc._cast(dtype)
    return dict(x0=c(x0), xref=c(xref), uref=c(uref), p=c(p), xbar=c(xb), ubar=c(ub))


def _cfg_fields(k):
    if k.model == 12:
        kw = ac.fields(groups=(), box='input' if k.path in BOXED12 else 'none', dtype=k.dtype)
        if k.path == 'box_ipm':
            kw['max_as_iter'] = 1
        elif k.path in BOXED12:
            kw['max_as_iter'] = 200
        return kw
    return ac.fields(full=True, groups=(), box=k.path, dtype=k.dtype)


@functools.lru_cache(maxsize=None)
def _oracle(k, mode):
    """The CPU reference of a case, computed once and never modified: (oracle output, spec)."""
    if k.model == 12:
        boxed = k.path in BOXED12
        return gc._oracle(k.N, k.B, mode, _alt(mode), k.dtype, boxed, 1 if k.path == 'box_ipm' else 200, ())
    i = _np_inputs(k)
    spec = FullSpec(N=k.N, **ac.spec_kwargs(_cfg_fields(k)))
    it = dict(mode='iterate', xbar=i['xbar'], ubar=i['ubar']) if mode == 'iterate' else {}
    return mpc_solve17(i['x0'], i['xref'], i['uref'], spec, i['p'], **it), spec


def _expected_kernels(k, mode):
    it = gc._it(mode)
    if k.model == 17:
        return {'nominal': f'mpcb::nominal17q_kernel<{gc.T[k.dtype]}>', 'riccati': gc.RIC17[k.path, k.dtype],
                'linearise': f'mpcb::lin17ws_kernel<{gc.T[k.dtype]}>'}
    exp = gc.PATHS[k.path][2](k.dtype, it)
    # PATHS names ALT's general inertia; the default diagonal one is the DJ = true instantiation of
    # the row rollout, alone and fused with the Riccati pass (test_gpu_config._check_box's rule)
    for ph, name in exp.items():
        name = re.sub(r'(row_riccati_kernel<\w+), false>', r'\1, true>', name)
        exp[ph] = re.sub(r'(nominal_row_kernel<\w+, \w+), false,', r'\1, true,', name)
    return exp


class Case:
    """A handle, its device-free facts, and the baseline of one mode (computed on first use)."""

    def __init__(self, k, mode):
        from mpc_blaster_amd import BatchedMPC, MPCConfig
        self.k, self.mode, self.B, self.N = k, mode, k.B, k.N
        self.iterate = mode == 'iterate'
        # the path switches are read when a handle is created (and by the device-free plan that
        # _kernels_are compares with), never by a solve: they are set for the construction alone
        with pytest.MonkeyPatch.context() as mp:
            if k.chunk:
                mp.setenv('MPCB_CHUNK', '64')
            if k.model == 12:
                self.m = gc._handle(k.path, k.N, k.B + MARGIN, k.dtype, mp, **_cfg_fields(k))
            else:
                self.m = BatchedMPC(MPCConfig.full(N=k.N, dtype=k.dtype, **_cfg_fields(k)), max_batch=k.B + MARGIN)
            self._baseline()

    def _baseline(self):
        k = self.k
        assert self.m.max_batch > k.B
        self.raw = ab.Raw(self.m)
        self.nx, self.nu, self.tdt = self.m.nx, self.m.nu, self.m.dtype
        self.esz = 8 if k.dtype == 'f64' else 4
        self.inp = _np_inputs(k)
        if k.model == 17:
            self.inp['wind'] = None
            p = self.inp['p']
            self.p_packed = torch.as_tensor(p.copy(), device='cuda').to(self.tdt).contiguous()
            self.set_params_packed()
        self.len = dict(x0=self.nx, xref=(k.N + 1) * self.nx, uref=k.N * self.nu, wind=3,
                        xbar=(k.N + 1) * self.nx, ubar=k.N * self.nu)
        self.base = self.solve(self.inputs(), self.plain_outputs())
        gc._kernels_are(self.m, k.B, self.mode, _expected_kernels(k, self.mode))

    def set_params_packed(self):
        p = self.p_packed
        assert self.raw.set_params(p.shape[0], p, p.shape[1] * 25, 25) == 0, self.raw.error()

    # -- buffers
    def inputs(self, layout=None, arrays=None):
        """{name: Padded} of the case's inputs; ``layout``: {name: (stride, lead)}, packed otherwise."""
        layout, arrays = layout or {}, arrays or self.inp
        out = {}
        for name in ('x0', 'xref', 'uref', 'wind') + (('xbar', 'ubar') if self.iterate else ()):
            a = arrays.get(name)
            if a is None:
                out[name] = None
                continue
            stride, lead = layout.get(name, (self.len[name], 0))
            out[name] = ab.padded(a.reshape(a.shape[0], -1), stride, lead, self.tdt)
        return out

    def plain_outputs(self):
        e = lambda *s: torch.full(s, float('nan'), dtype=self.tdt, device='cuda')   # noqa: E731
        return dict(u0=e(self.B, self.nu), X=e(self.B, self.N + 1, self.nx), U=e(self.B, self.N, self.nu),
                    status=torch.full((self.B,), ab.I_SENTINEL, dtype=torch.int32, device='cuda'))

    def guarded_outputs(self, X=True, U=True):
        return dict(u0=ab.guarded((self.B, self.nu), self.tdt),
                    X=ab.guarded((self.B, self.N + 1, self.nx), self.tdt, 16) if X else None,
                    U=ab.guarded((self.B, self.N, self.nu), self.tdt, 16) if U else None,
                    status=ab.guarded((self.B,), torch.int32))

    # -- the call
    def call(self, bufs, outs, stream=0, B=None, **over):
        """The raw solve of this case's mode; ``over`` replaces single arguments (name=value,
        name_sb=stride).  Returns the library's return code."""
        a = {}
        for name in ('x0', 'xref', 'uref', 'wind'):
            b = bufs.get(name)
            a[name], a[name + '_sb'] = b, (b.stride if b is not None else 0)
        a.update(xbar=bufs.get('xbar'), ubar=bufs.get('ubar'), **outs)
        a.update(over)
        return self.raw.solve(self.B if B is None else B, a['x0'], a['x0_sb'], a['xref'], a['xref_sb'], a['uref'],
                              a['uref_sb'], a['wind'], a['wind_sb'], a['u0'], a['X'], a['U'], a['status'], stream,
                              iterate=self.iterate, xbar=a['xbar'], ubar=a['ubar'])

    def solve(self, bufs, outs, **kw):
        rc = self.call(bufs, outs, **kw)
        assert rc == 0, self.raw.error()
        torch.cuda.synchronize()
        return results(outs)


def results(outs):
    """{name: host array} of the outputs given (tensors or Guarded views)."""
    return {n: (o.view if isinstance(o, ab.Guarded) else o).cpu().numpy().copy() for n, o in outs.items() if o is not None}


def same(got, want, names=('u0', 'X', 'U', 'status')):
    """Bitwise equality of the named outputs, with the first difference in the message."""
    for n in names:
        a, b = got[n], want[n]
        assert a.shape == b.shape and a.dtype == b.dtype, n
        if a.tobytes() != b.tobytes():
            ne = ~((a == b) | (np.isnan(a) & np.isnan(b))) if a.dtype.kind == 'f' else a != b
            idx = np.argwhere(ne)
            raise AssertionError(f'{n} differs from the baseline in {len(idx)} of {a.size} entries, first at '
                                 f'{idx[:4].tolist()}: {a[ne][:4]} against {b[ne][:4]}')


def check_guards(outs):
    for o in outs.values():
        if isinstance(o, ab.Guarded):
            o.check()


def check_inputs(bufs):
    for n, b in bufs.items():
        assert b is None or b.unchanged(), f'the call wrote into its input {n}'


_CASES = {}


def case(k, mode):
    """One handle and baseline per (case, mode) for the whole module: the variants share it."""
    if (k, mode) not in _CASES:
        _CASES[k, mode] = Case(k, mode)
    return _CASES[k, mode]


# ------------------------------------------------------------------------------ baseline
@pytest.mark.parametrize('k,mode', CASES, ids=IDS)
def test_baseline_matches_oracle(k, mode):
    """The baseline raw call against the CPU oracle at test_gpu_config's own acceptance for the
    path (_accept_free, _accept_box, _accept17; the fp32 N = 260 case by its _noise_move rule), and
    the kernels it claims (asserted when the case is built)."""
    c = case(k, mode)
    o, spec = _oracle(k, mode)
    r, i = c.base, c.inp
    assert (o['status'] == 0).all()
    if k.model == 17:
        gc._accept17(IDS[CASES.index((k, mode))], o, spec, i['x0'], i['xref'], i['uref'], r['u0'], r['X'], r['U'],
                     r['status'], k.path, k.dtype)
    elif k.path in BOXED12:
        frac = gc._on_bound(o['U'], spec.lbu, spec.ubu).mean()
        assert frac >= 0.10   # the box is active, so the box kernels' own stores are exercised
        gc._accept_box(f'{k.id} {mode}', o, spec, i, r['u0'], r['X'], r['U'], r['status'], k.dtype)
    else:
        tol = None
        if k.dtype == 'f32' and k.N > 40:
            tol = max(5e-5, 10.0 * gc._noise_move(o, i, spec))
        gc._accept_free(f'{k.id} {mode}', o, r['u0'], r['X'], r['U'], r['status'], k.dtype, tol)


# ------------------------------------------------------------------------------ (a) guards
@pytest.mark.parametrize('k,mode', CASES, ids=IDS)
def test_guard_bands_and_read_only_inputs(k, mode):
    """(a) u0, X, U and status inside sentinel bands (u0 / status at exactly their element's
    alignment, X / U at exactly 16 bytes): every guard element survives the call, every input
    buffer keeps its bits, and the outputs are the baseline's."""
    c = case(k, mode)
    bufs, outs = c.inputs(), c.guarded_outputs()
    r = c.solve(bufs, outs)
    check_guards(outs)
    check_inputs(bufs)
    same(r, c.base)


# ------------------------------------------------------------------------------ (b) padded
def _odd_layout(c):
    return dict(x0=(c.nx + 1, 1), xref=((c.N + 1) * c.nx + 3, 1), uref=(c.N * c.nu + 1, 1), wind=(5, 1))


@pytest.mark.parametrize('k,mode', CASES, ids=IDS)
def test_padded_odd_strides_and_element_aligned_bases(k, mode):
    """(b) x0_sb = nx + 1, xref_sb = (N+1) nx + 3, uref_sb = N nu + 1, wind_sb = 5, each one element
    into its allocation: every record is only element-aligned in both dtypes, and every pad is NaN,
    so a pad value that reaches an output shows as status 1 or as a bit difference."""
    c = case(k, mode)
    bufs, outs = c.inputs(_odd_layout(c)), c.guarded_outputs()
    for n in ('x0', 'xref', 'uref', 'wind'):
        if bufs[n] is not None:
            assert bufs[n].ptr % 16 != 0 and bufs[n].ptr % c.esz == 0
    r = c.solve(bufs, outs)
    check_guards(outs)
    check_inputs(bufs)
    same(r, c.base)


# ------------------------------------------------------------------------------ (c) broadcast
def _with_arrays(cases, ids, names):
    """cases x names, without wind on the 17/6 model (a 12/4-model extension)."""
    out = [(k, mode, n) for k, mode in cases for n in names if n != 'wind' or k.model == 12]
    return out, [f'{ids[cases.index((k, mode))]}-{n}' for k, mode, n in out]


BCAST, BCAST_IDS = _with_arrays(CASES, IDS, ('x0', 'xref', 'uref', 'wind'))


@pytest.mark.parametrize('k,mode,which', BCAST, ids=BCAST_IDS)
def test_broadcast(k, mode, which):
    """(c) one of x0, xref, uref, wind at stride 0 (one record for the batch), the others per
    instance, against the contiguous call on the materialised copies."""
    c = case(k, mode)
    arrays = dict(c.inp)
    arrays[which] = np.repeat(c.inp[which][2:3], c.B, axis=0)   # (instance 2's record: not the first)
    want = c.solve(c.inputs(arrays=arrays), c.plain_outputs())
    bufs, outs = c.inputs({which: (0, 1)}, dict(arrays, **{which: arrays[which][:1]})), c.guarded_outputs()
    assert bufs[which].stride == 0
    r = c.solve(bufs, outs)
    check_guards(outs)
    check_inputs(bufs)
    same(r, want)
    assert (r['status'] == 0).all()


# ------------------------------------------------------------------------------ (d) in place
@pytest.mark.parametrize('alias', ['XU', 'X', 'U'])
@pytest.mark.parametrize('k,mode', ITER_CASES, ids=ITER_IDS)
def test_in_place(k, mode, alias):
    """(d) iterate mode with X = xbar and U = ubar the same buffers, then X alone, then U alone
    ("X/U may alias xbar/ubar"): the outputs of the out-of-place baseline.  The fp32 box path
    re-reads U in its refinement kernel, the interior-point hand-over runs after the active-set
    kernel has stored U, the 17/6 kernels copy the iterate first, and the chunked cases alias past
    the first chunk."""
    c = case(k, mode)
    bufs, outs = c.inputs(), c.guarded_outputs()
    for n, src in (('X', 'xbar'), ('U', 'ubar')):
        if n in alias:
            outs[n].view.copy_(bufs[src].buf[: outs[n].n].view(outs[n].view.shape))
            bufs[src] = None
    r = c.solve(bufs, outs, xbar=outs['X'] if 'X' in alias else bufs['xbar'],
                ubar=outs['U'] if 'U' in alias else bufs['ubar'])
    check_guards(outs)
    check_inputs(bufs)
    same(r, c.base)


# ------------------------------------------------------------------------------ (e) partial
@pytest.mark.parametrize('given', ['X', 'U'])
@pytest.mark.parametrize('k,mode', CASES, ids=IDS)
def test_one_trajectory_output(k, mode, given):
    """(e) X with U = NULL, and U with X = NULL: the given output, u0 and status are the
    baseline's (the fp32 box path substitutes a buffer of its own for a missing U)."""
    c = case(k, mode)
    bufs, outs = c.inputs(), c.guarded_outputs(X=given == 'X', U=given == 'U')
    r = c.solve(bufs, outs)
    check_guards(outs)
    check_inputs(bufs)
    same(r, c.base, ('u0', given, 'status'))


# ------------------------------------------------------------------------------ (f) stream
# The delay enqueued ahead of the library call: DELAY_MATMULS products of two DELAY_N x DELAY_N fp32
# matrices.  Measured with events on the MI355X (test_stream_delay_is_long_enough prints it): 86 ms,
# against well under a millisecond of host time for the copies and the library call that are enqueued
# behind it, so ``s.query() is False`` holds with a margin of about a hundred.
DELAY_N, DELAY_MATMULS = 8192, 12


@functools.lru_cache(maxsize=None)
def _delay_operands():
    a = torch.ones((DELAY_N, DELAY_N), dtype=torch.float32, device='cuda')
    torch.mm(a, a)   # (the BLAS library's first-call set-up happens here, on the default stream)
    torch.cuda.synchronize()
    return a, torch.empty_like(a)


def _delay():
    a, out = _delay_operands()
    for _ in range(DELAY_MATMULS):
        torch.mm(a, a, out=out)


def _on_stream(tensors, launch):
    """The sequence of variant (f): ``tensors`` are the input device buffers of ``launch(stream
    handle)``.  NaN them on the default stream; on a new stream enqueue the delay, the copies of the
    real inputs, and the library call; the stream must still be busy when the call returns (else
    the test would pass vacuously).  A kernel or memset the library issued on the null stream runs
    before the inputs exist and leaves NaN status or other bits."""
    _delay_operands()
    real = [t.clone() for t in tensors]
    for t in tensors:
        t.fill_(float('nan')) if t.dtype.is_floating_point else t.fill_(0)
    # the same call on the NaN inputs first, default stream: it leaves NaN in the handle's
    # workspace, which still held the intermediates of the baseline's identical solve (a later
    # kernel of the path that ran early would otherwise read those and give the right bits)
    assert launch(0) == 0
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _delay()
        for t, r in zip(tensors, real):
            t.copy_(r)
        rc = launch(s.cuda_stream)
        busy = s.query() is False
    s.synchronize()
    torch.cuda.synchronize()
    assert rc == 0
    assert busy, 'the delay ended before the library call returned: the stream test proves nothing'


def test_stream_delay_is_long_enough():
    """The delay of variant (f) by events, printed: DELAY_MATMULS x mm(8192 x 8192, fp32), 86.1 ms
    when measured on the MI355X.  Every stream test asserts for itself that the delay sufficed
    (``s.query() is False`` right after the call); this one keeps the number honest."""
    _delay_operands()
    s = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        e0.record()
        _delay()
        e1.record()
    s.synchronize()
    ms = e0.elapsed_time(e1)
    print(f'stream delay: {DELAY_MATMULS} x mm({DELAY_N}) took {ms:.1f} ms')
    assert ms > 10.0   # a library call takes tens of microseconds of host time to enqueue


STREAM_KS = [k for k in KS if not k.chunk and (k.model, k.path, k.dtype) in {
    (12, 'fused', 'f64'), (12, 'two', 'f64'), (12, 'small', 'f64'), (12, 'thread', 'f64'), (12, 'box', 'f64'),
    (12, 'box', 'f32'), (12, 'box_ipm', 'f64'), (17, 'none', 'f64'), (17, 'all', 'f64')}]
STREAM_CASES = [(k, mode) for k in STREAM_KS for mode in k.modes]


@pytest.mark.parametrize('k,mode', STREAM_CASES, ids=[f'{k.id}-{mode}' for k, mode in STREAM_CASES])
def test_solve_on_a_stream_of_its_own(k, mode):
    """(f) one case per launch structure: every kernel and memset of the solve is ordered behind
    the copies that create its inputs on the caller's stream."""
    c = case(k, mode)
    bufs, outs = c.inputs(), c.guarded_outputs()
    _on_stream([b.buf for b in bufs.values() if b is not None], lambda st: c.call(bufs, outs, stream=st))
    check_guards(outs)
    same(results(outs), c.base)


# ------------------------------------------------------------------------------ (g) other entry points
def _dev(c, a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda').to(c.tdt)


EVAL_KS = [k for k in ITER_KS if (k.model, k.path, k.dtype, k.chunk) in {(12, 'box', 'f64', False), (12, 'box', 'f32', False),
                                                                     (17, 'input', 'f64', False), (17, 'input', 'f32', False)}]
EVAL_KEYS = ('cost', 'res_eq', 'res_ineq', 'res_stat')


def _eval(c, bufs, X, U, outs, stream=0):
    g = lambda n: bufs.get(n)   # noqa: E731
    sb = lambda n: bufs[n].stride if bufs.get(n) is not None else 0   # noqa: E731
    return c.raw.eval(c.B, g('x0'), sb('x0'), X, U, g('xref'), sb('xref'), g('uref'), sb('uref'), g('wind'), sb('wind'),
                      outs['cost'], outs['res_eq'], outs['res_ineq'], outs['res_stat'], stream)


def _eval_outs(c):
    return {n: ab.guarded((c.B,), c.tdt) for n in EVAL_KEYS}


REFS = ('x0', 'xref', 'uref', 'wind')
EVAL_CASES, EVAL_IDS = _with_arrays([(k, 'iterate') for k in EVAL_KS], [k.id for k in EVAL_KS], ('padded',) + REFS)


@pytest.mark.parametrize('k,mode,layout', EVAL_CASES, ids=EVAL_IDS)
def test_eval_strides(k, mode, layout):
    """(g) mpcb_eval of the baseline's iterate with padded, and with each broadcast, x0 / xref /
    uref / wind against its contiguous call on the materialised arrays; [B] outputs in guards."""
    c = case(k, mode)
    X, U = _dev(c, c.base['X']), _dev(c, c.base['U'])
    arrays, lay = dict(c.inp), _odd_layout(c)
    if layout != 'padded':
        arrays[layout] = np.repeat(c.inp[layout][2:3], c.B, axis=0)
        lay = {layout: (0, 1)}
    packed = _ref_bufs(c, {}, arrays, REFS)
    bufs = _ref_bufs(c, lay, arrays if layout == 'padded' else dict(arrays, **{layout: arrays[layout][:1]}), REFS)
    want, outs = _eval_outs(c), _eval_outs(c)
    assert _eval(c, packed, X, U, want) == 0, c.raw.error()
    assert _eval(c, bufs, X, U, outs) == 0, c.raw.error()
    torch.cuda.synchronize()
    check_guards(outs)
    check_inputs(bufs)
    w = results(want)
    same(results(outs), w, EVAL_KEYS)
    assert all(np.isfinite(w[n]).all() for n in EVAL_KEYS) and w['res_stat'].min() > 0


def test_eval_on_a_stream_of_its_own():
    k = EVAL_KS[0]
    c = case(k, 'iterate')
    X, U = _dev(c, c.base['X']), _dev(c, c.base['U'])
    bufs = _ref_bufs(c, {}, None, REFS)
    want, outs = _eval_outs(c), _eval_outs(c)
    assert _eval(c, bufs, X, U, want) == 0
    torch.cuda.synchronize()
    _on_stream([b.buf for b in bufs.values()] + [X, U], lambda st: _eval(c, bufs, X, U, outs, st))
    check_guards(outs)
    same(results(outs), results(want), EVAL_KEYS)


VJP_KEYS = ('gx0', 'gxref', 'guref', 'gQ', 'gR', 'gQN', 'status')


def _vjp_outs(c):
    nx, nu, N, B = c.nx, c.nu, c.N, c.B
    o = dict(gx0=(B, nx), gxref=(B, N + 1, nx), guref=(B, N, nu), gQ=(B, nx, nx), gR=(B, nu, nu), gQN=(B, nx, nx))
    out = {n: ab.guarded(s, c.tdt) for n, s in o.items()}
    out['status'] = ab.guarded((B,), torch.int32)
    return out


def _vjp_data(c):
    """The baseline's iterate and solution plus fixed random cotangents, on the device."""
    rng = np.random.default_rng(29)
    cast = gc._cast(c.k.dtype)
    gX, gU = cast(rng.standard_normal(c.base['X'].shape)), cast(rng.standard_normal(c.base['U'].shape))
    return {n: _dev(c, a) for n, a in dict(xbar=c.inp['xbar'], ubar=c.inp['ubar'], X=c.base['X'], U=c.base['U'],
                                           gX=gX, gU=gU).items()}


def _ref_bufs(c, layout, arrays=None, names=('xref', 'uref', 'wind')):
    arrays = arrays or c.inp
    out = {}
    for n in names:
        a = arrays.get(n)
        if a is None:
            out[n] = None
            continue
        stride, lead = layout.get(n, (c.len[n], 0))
        out[n] = ab.padded(a.reshape(a.shape[0], -1), stride, lead, c.tdt)
    return out


def _vjp_w(c, d, bufs, outs, stream=0):
    sb = lambda n: bufs[n].stride if bufs.get(n) is not None else 0   # noqa: E731
    return c.raw.vjp_w(c.B, d['xbar'], d['ubar'], d['X'], d['U'], bufs['xref'], sb('xref'), bufs['uref'], sb('uref'),
                       bufs['wind'], sb('wind'), d['gX'], d['gU'], outs['gx0'], outs['gxref'], outs['guref'],
                       outs['gQ'], outs['gR'], outs['gQN'], outs['status'], stream)


VJP_KS = [k for k in ITER_KS if (k.model, k.path, k.dtype, k.chunk) in {(12, 'fused', 'f64', False), (12, 'box', 'f64', False),
                                                                    (12, 'box', 'f32', False)}]


@pytest.mark.parametrize('layout', ['padded', 'xref', 'uref', 'wind'])
@pytest.mark.parametrize('k', VJP_KS, ids=[k.id for k in VJP_KS])
def test_vjp_w_strides(k, layout):
    """(g) mpcb_solve_vjp_w with weight outputs: padded, and each broadcast, xref_sb / uref_sb /
    wind_sb against the contiguous per-instance call; all six gradients and status in guards."""
    c = case(k, 'iterate')
    d = _vjp_data(c)
    arrays, lay = dict(c.inp), {n: v for n, v in _odd_layout(c).items() if n != 'x0'}
    if layout != 'padded':
        arrays[layout] = np.repeat(c.inp[layout][2:3], c.B, axis=0)
        lay = {layout: (0, 1)}
    packed = _ref_bufs(c, {}, arrays)
    bufs = _ref_bufs(c, lay, arrays if layout == 'padded' else dict(arrays, **{layout: arrays[layout][:1]}))
    want, outs = _vjp_outs(c), _vjp_outs(c)
    assert _vjp_w(c, d, packed, want) == 0, c.raw.error()
    assert _vjp_w(c, d, bufs, outs) == 0, c.raw.error()
    torch.cuda.synchronize()
    check_guards(outs)
    check_guards(want)
    check_inputs(bufs)
    w = results(want)
    same(results(outs), w, VJP_KEYS)
    assert (w['status'] == 0).all() and np.abs(w['gQ']).max() > 0


def test_vjp_w_on_a_stream_of_its_own():
    c = case(VJP_KS[1], 'iterate')
    d, bufs = _vjp_data(c), _ref_bufs(c, {})
    want, outs = _vjp_outs(c), _vjp_outs(c)
    assert _vjp_w(c, d, bufs, want) == 0   # (the first call allocates the call's workspace)
    torch.cuda.synchronize()
    _on_stream([b.buf for b in bufs.values()] + list(d.values()), lambda st: _vjp_w(c, d, bufs, outs, st))
    check_guards(outs)
    same(results(outs), results(want), VJP_KEYS)


def _vjp17(c, d, bufs, outs, stream=0):
    return c.raw.vjp17(c.B, d['xbar'], d['ubar'], d['fixed'], d['X'], d['U'], bufs['xref'], bufs['xref'].stride,
                       bufs['uref'], bufs['uref'].stride, d['gX'], d['gU'], outs['gx0'], outs['gxref'], outs['guref'],
                       outs['gQ'], outs['gR'], outs['gQN'], outs['status'], stream)


def _vjp17_data(c):
    d = _vjp_data(c)
    d['fixed'] = c.m.active_mask17(d['U'], 1e-4)
    return d


def _padded_params(c):
    """The case's parameters with params_sb = stages * 25 + 7 and params_kb = 27, one element in.
    (From five stages up these strides interleave the rows of neighbouring instances -- 7 stages:
    182 < 6 * 27 + 25 -- so the parameter cases run at N = 2, a horizon of test_gpu_config's too.)"""
    p = c.inp['p']
    B, stages = p.shape[0], p.shape[1]
    kb, sb = 27, stages * 25 + 7
    assert stages == c.N and sb >= (stages - 1) * kb + 25
    rows = np.full((B, sb), np.nan)
    for s in range(stages):
        rows[:, s * kb: s * kb + 25] = p[:, s]
    return ab.padded(rows, sb, 1, c.tdt), sb, kb


PARAM_KS = [k for k in KS if k.model == 17 and k.N == 2]   # B = 7, and chunked B = 70
VJP17_KS = PARAM_KS


@pytest.mark.parametrize('layout', ['padded', 'xref', 'uref'])
@pytest.mark.parametrize('k', VJP17_KS, ids=[k.id for k in VJP17_KS])
def test_vjp17_strides_and_params(k, layout):
    """(g) mpcb_solve_vjp17 with weight outputs: padded and broadcast xref_sb / uref_sb, and in the
    padded run also mpcb_set_params with params_sb = stages * 25 + 7, params_kb = 27, against the
    contiguous call with packed parameters (B = 7, and the chunked B = 70)."""
    c = case(k, 'iterate')
    d = _vjp17_data(c)
    arrays, lay = dict(c.inp), {n: v for n, v in _odd_layout(c).items() if n in ('xref', 'uref')}
    if layout != 'padded':
        arrays[layout] = np.repeat(c.inp[layout][2:3], c.B, axis=0)
        lay = {layout: (0, 1)}
    packed = _ref_bufs(c, {}, arrays, ('xref', 'uref'))
    bufs = _ref_bufs(c, lay, arrays if layout == 'padded' else dict(arrays, **{layout: arrays[layout][:1]}),
                     ('xref', 'uref'))
    want, outs = _vjp_outs(c), _vjp_outs(c)
    assert _vjp17(c, d, packed, want) == 0, c.raw.error()
    torch.cuda.synchronize()
    try:
        if layout == 'padded':
            pp, sb, kb = _padded_params(c)
            assert c.raw.set_params(c.B, pp, sb, kb) == 0, c.raw.error()
        assert _vjp17(c, d, bufs, outs) == 0, c.raw.error()
        torch.cuda.synchronize()
    finally:
        c.set_params_packed()
    check_guards(outs)
    check_inputs(bufs)
    if layout == 'padded':
        assert pp.unchanged()
    w = results(want)
    same(results(outs), w, VJP_KEYS)
    assert (w['status'] == 0).all() and np.abs(w['gQ']).max() > 0 and int(d['fixed'].sum()) > 0


def test_vjp17_on_a_stream_of_its_own():
    c = case(VJP17_KS[0], 'iterate')
    d, bufs = _vjp17_data(c), _ref_bufs(c, {}, None, ('xref', 'uref'))
    want, outs = _vjp_outs(c), _vjp_outs(c)
    assert _vjp17(c, d, bufs, want) == 0   # (the first call allocates the call's workspace)
    torch.cuda.synchronize()
    _on_stream([b.buf for b in bufs.values()] + list(d.values()), lambda st: _vjp17(c, d, bufs, outs, st))
    check_guards(outs)
    same(results(outs), results(want), VJP_KEYS)


@pytest.mark.parametrize('mode', gc.MODES)
@pytest.mark.parametrize('k', PARAM_KS, ids=[k.id for k in PARAM_KS])
def test_set_params_strides(k, mode):
    """(g) the 17/6 solve reading padded parameters (params_sb = stages * 25 + 7, params_kb = 27,
    NaN pads) gives the bits of the solve with packed parameters, chunked case included."""
    c = case(k, mode)
    bufs, outs = c.inputs(), c.guarded_outputs()
    pp, sb, kb = _padded_params(c)
    try:
        assert c.raw.set_params(c.B, pp, sb, kb) == 0, c.raw.error()
        r = c.solve(bufs, outs)
    finally:
        c.set_params_packed()
    check_guards(outs)
    assert pp.unchanged()
    same(r, c.base)


@pytest.mark.parametrize('layout', ['padded', 'broadcast'])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_linearize_and_sim_step_strides(dtype, layout):
    """(g) mpcb_linearize and mpcb_sim_step with wind_sb = 5 (one element in, NaN pads) and with
    wind_sb = 0, against their contiguous calls; A, B, x_next and x_out in guards."""
    k = next(k for k in KS if (k.model, k.path, k.dtype) == (12, 'row32' if dtype == 'f32' else 'fused', dtype))
    c = case(k, 'iterate')
    B, N, nx, nu = c.B, c.N, c.nx, c.nu
    xb, ub = _dev(c, c.inp['xbar']), _dev(c, c.inp['ubar'])
    x, u = xb[:, 0].contiguous(), ub[:, 0].contiguous()
    wind = c.inp['wind'] if layout == 'padded' else np.repeat(c.inp['wind'][2:3], B, axis=0)
    packed = ab.padded(wind, 3, 0, c.tdt)
    w = ab.padded(wind, 5, 1, c.tdt) if layout == 'padded' else ab.padded(wind[:1], 0, 1, c.tdt)

    def outs():
        return dict(A=ab.guarded((B, N, nx, nx), c.tdt), Bm=ab.guarded((B, N, nx, nu), c.tdt),
                    xn=ab.guarded((B, N, nx), c.tdt), xo=ab.guarded((B, nx), c.tdt))

    want, got = outs(), outs()
    for o, wb in ((want, packed), (got, w)):
        assert c.raw.linearize(B, xb, ub, wb, wb.stride, o['A'], o['Bm'], o['xn']) == 0, c.raw.error()
        assert c.raw.sim_step(B, x, u, wb, wb.stride, 0.013, o['xo']) == 0, c.raw.error()
    torch.cuda.synchronize()
    check_guards(got)
    assert w.unchanged()
    rw = results(want)
    same(results(got), rw, ('A', 'Bm', 'xn', 'xo'))
    assert all(np.isfinite(v).all() for v in rw.values())


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_gen_inputs_strides(dtype):
    """(g) mpcb_gen_inputs, ref_kind 1, writing records at xref_sb = (N+1) nx + 3 and
    uref_sb = N nu + 1 into sentinel-filled buffers: the records are the packed call's, and every
    pad and guard element keeps its sentinel."""
    k = next(k for k in KS if (k.model, k.path, k.dtype) == (12, 'row32' if dtype == 'f32' else 'fused', dtype))
    c = case(k, 'rollout')
    B, N, nx, nu = c.B, c.N, c.nx, c.nu
    nxr, nur = (N + 1) * nx, N * nu
    want = dict(x0=ab.guarded((B, nx), c.tdt), xref=ab.guarded((B, nxr), c.tdt), uref=ab.guarded((B, nur), c.tdt),
                wind=ab.guarded((B, 3), c.tdt))
    got = dict(x0=ab.guarded((B, nx), c.tdt), xref=ab.guarded((B, nxr + 3), c.tdt),
               uref=ab.guarded((B, nur + 1), c.tdt), wind=ab.guarded((B, 3), c.tdt))
    assert c.raw.gen_inputs(B, 11, 5, 1, want['x0'], want['xref'], nxr, want['uref'], nur, want['wind']) == 0
    assert c.raw.gen_inputs(B, 11, 5, 1, got['x0'], got['xref'], nxr + 3, got['uref'], nur + 1, got['wind']) == 0
    torch.cuda.synchronize()
    check_guards(want)
    check_guards(got)
    rw, rg = results(want), results(got)
    assert rg['x0'].tobytes() == rw['x0'].tobytes() and rg['wind'].tobytes() == rw['wind'].tobytes()
    for n, ln in (('xref', nxr), ('uref', nur)):
        assert rg[n][:, :ln].tobytes() == rw[n].tobytes(), n
        assert (rg[n][:, ln:] == ab.F_SENTINEL).all(), f'{n}: a pad element between two records was written'
        assert np.isfinite(rw[n]).all() and not (rw[n] == ab.F_SENTINEL).all()
    assert np.ptp(rw['xref'], axis=0).max() > 0   # per-instance references, as ref_kind 1 promises


def test_stats_and_histogram_outputs():
    """(g) mpcb_qp_stats and mpcb_histogram write [B, 2] int32 and [nu, nbins] int64 and nothing
    around them."""
    k = next(k for k in KS if (k.model, k.path, k.dtype) == (12, 'box', 'f64'))
    c = case(k, 'rollout')
    c.solve(c.inputs(), c.plain_outputs())   # (the statistics are those of the handle's last solve)
    st = ab.guarded((c.B, 2), torch.int32)
    assert c.raw.qp_stats(c.B, st) == 0, c.raw.error()
    hist = ab.guarded((c.nu, 16), torch.int64)
    hist.view.zero_()
    u0 = _dev(c, c.base['u0'])
    assert c.raw.histogram(c.B, u0, 0.0, 65.0, 16, hist) == 0, c.raw.error()
    torch.cuda.synchronize()
    st.check()
    hist.check()
    s, hcount = st.view.cpu().numpy(), hist.view.cpu().numpy()
    assert (s[:, 0] >= 1).all() and (s != ab.I_SENTINEL).all()
    assert (hcount.sum(axis=1) == c.B).all()   # (values outside [lo, hi) are counted in the end bins)


# ------------------------------------------------------------------------------ (h) refusals
REFUSAL_KS = [k for k in KS if not k.chunk and (k.model, k.path, k.dtype) in {(12, 'fused', 'f64'), (12, 'box', 'f32'),
                                                                              (17, 'input', 'f64')}]


REFUSAL_CASES = [(k, mode) for k in REFUSAL_KS for mode in k.modes]


@pytest.mark.parametrize('k,mode', REFUSAL_CASES, ids=[f'{k.id}-{mode}' for k, mode in REFUSAL_CASES])
def test_refusals(k, mode):
    """(h) a misaligned X or U, B > max_batch, each required NULL and each negative stride return
    MPCB_E_INVALID before any launch: the outputs and their guards keep every sentinel, and a
    valid call afterwards gives the baseline's bits."""
    c = case(k, mode)
    bufs, outs = c.inputs(), c.guarded_outputs()
    bad = [dict(X=outs['X'].ptr + c.esz), dict(U=outs['U'].ptr + c.esz), dict(B=c.m.max_batch + 1)]
    bad += [{n: None} for n in ('x0', 'xref', 'uref', 'u0', 'status') + (('xbar', 'ubar') if c.iterate else ())]
    bad += [{n + '_sb': -1} for n in ('x0', 'xref', 'uref')] + [dict(x0_sb=-c.nx), dict(wind_sb=-3)]
    for over in bad:
        assert c.call(bufs, outs, **over) == E_INVALID, f'{over} was accepted'
        assert c.raw.error()
    torch.cuda.synchronize()
    for n, o in outs.items():
        assert o.untouched(), f'a refused call wrote into {n}'
    check_inputs(bufs)
    r = c.solve(bufs, outs)
    check_guards(outs)
    same(r, c.base)


def test_negative_strides_of_the_other_entry_points():
    """(h) mpcb_eval, mpcb_linearize, mpcb_sim_step, mpcb_gen_inputs, mpcb_solve_vjp_w and (17/6)
    mpcb_set_params, mpcb_solve_vjp17 refuse a negative stride with MPCB_E_INVALID and write
    nothing."""
    k = next(k for k in KS if (k.model, k.path, k.dtype) == (12, 'fused', 'f64'))
    c = case(k, 'iterate')
    B, N, nx, nu = c.B, c.N, c.nx, c.nu
    X, U = _dev(c, c.base['X']), _dev(c, c.base['U'])
    refs = _ref_bufs(c, {}, None, ('x0', 'xref', 'uref', 'wind'))
    eo = _eval_outs(c)
    for n in ('x0', 'xref', 'uref', 'wind'):
        sb = {m: (refs[m].stride if m != n else -1) for m in refs}
        assert c.raw.eval(B, refs['x0'], sb['x0'], X, U, refs['xref'], sb['xref'], refs['uref'], sb['uref'],
                          refs['wind'], sb['wind'], eo['cost'], eo['res_eq'], eo['res_ineq'], eo['res_stat']) == E_INVALID, n
    lo = dict(A=ab.guarded((B, N, nx, nx), c.tdt), Bm=ab.guarded((B, N, nx, nu), c.tdt),
              xn=ab.guarded((B, N, nx), c.tdt), xo=ab.guarded((B, nx), c.tdt))
    xb, ub = _dev(c, c.inp['xbar']), _dev(c, c.inp['ubar'])
    assert c.raw.linearize(B, xb, ub, refs['wind'], -3, lo['A'], lo['Bm'], lo['xn']) == E_INVALID
    assert c.raw.sim_step(B, X[:, 0].contiguous(), U[:, 0].contiguous(), refs['wind'], -3, 0.01, lo['xo']) == E_INVALID
    go = dict(x0=ab.guarded((B, nx), c.tdt), xref=ab.guarded((B, (N + 1) * nx), c.tdt), uref=ab.guarded((B, N * nu), c.tdt))
    assert c.raw.gen_inputs(B, 1, 0, 1, go['x0'], go['xref'], -(N + 1) * nx, go['uref'], N * nu, None) == E_INVALID
    assert c.raw.gen_inputs(B, 1, 0, 1, go['x0'], go['xref'], (N + 1) * nx, go['uref'], -N * nu, None) == E_INVALID
    d, vo = _vjp_data(c), _vjp_outs(c)
    for n in ('xref', 'uref', 'wind'):
        sb = {m: (refs[m].stride if m != n else -1) for m in refs}
        assert c.raw.vjp_w(B, d['xbar'], d['ubar'], d['X'], d['U'], refs['xref'], sb['xref'], refs['uref'], sb['uref'],
                           refs['wind'], sb['wind'], d['gX'], d['gU'], vo['gx0'], vo['gxref'], vo['guref'], vo['gQ'],
                           vo['gR'], vo['gQN'], vo['status']) == E_INVALID, n
    torch.cuda.synchronize()
    for group in (eo, lo, go, vo):
        for n, o in group.items():
            assert o.untouched(), f'a refused call wrote into {n}'
    k17 = next(k for k in KS if (k.model, k.path, k.dtype, k.chunk) == (17, 'input', 'f64', False))
    c = case(k17, 'iterate')
    p = c.p_packed
    assert c.raw.set_params(p.shape[0], p, -p.shape[1] * 25, 25) == E_INVALID
    assert c.raw.set_params(p.shape[0], p, p.shape[1] * 25, -25) == E_INVALID
    d, vo, refs = _vjp17_data(c), _vjp_outs(c), _ref_bufs(c, {}, None, ('xref', 'uref'))
    for n in ('xref', 'uref'):
        sb = {m: (refs[m].stride if m != n else -1) for m in refs}
        assert c.raw.vjp17(c.B, d['xbar'], d['ubar'], d['fixed'], d['X'], d['U'], refs['xref'], sb['xref'],
                           refs['uref'], sb['uref'], d['gX'], d['gU'], vo['gx0'], vo['gxref'], vo['guref'], vo['gQ'],
                           vo['gR'], vo['gQN'], vo['status']) == E_INVALID, n
    torch.cuda.synchronize()
    assert all(o.untouched() for o in vo.values())
    # the handle still reads its packed parameters: the refused set calls changed nothing
    same(c.solve(c.inputs(), c.plain_outputs()), c.base)
