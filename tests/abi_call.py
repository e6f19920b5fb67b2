"""A raw caller of the C ABI (include/mpcb.h) for tests/test_gpu_abi.py; a helper, not a test.

``Raw`` passes pointers, strides and the stream to libmpcblaster.so exactly as given, on the handle
of an existing ``BatchedMPC`` (which is used for nothing but its handle): no tensor is made
contiguous, no stride is derived, no output is allocated.  Every call returns the library's return
code, so that a refusal can be asserted.

Two buffer builders place records where the Python layer never does.  Their index arithmetic is in
pure-numpy functions (``pack_padded`` / ``unpack_padded`` / ``guard_offset`` / ``guarded_np``),
tested without a GPU by tests/test_abi_pack_cpu.py; ``padded`` and ``guarded`` are the same layouts
on the device.
"""
import ctypes

import numpy as np

GUARD = 64          # guard elements on each side of a ``guarded`` view, at least
TAIL = 16           # NaN elements after the last record of a ``padded`` buffer
F_SENTINEL = 7.0    # a finite non-NaN float no kernel here produces as a whole band
I_SENTINEL = -77    # status / statistics sentinel (no acados status code)


# ---------------------------------------------------------------------------- numpy layouts
def padded_size(B, n, stride, lead):
    """Elements of a padded buffer: ``lead`` pad elements, then B records of n elements at
    ``lead + b * stride`` (stride >= n), or one record when stride == 0, then TAIL pad elements (so
    that no record ends where the allocation ends)."""
    if stride == 0:
        return lead + n + TAIL
    if stride < n:
        raise ValueError(f'stride {stride} < record length {n}: records would overlap')
    return lead + B * stride + TAIL


def pack_padded(a, stride, lead):
    """``a`` [B, n] (stride 0: [1, n], or [B, n] whose first record is taken) as a flat NaN-filled
    array with record b at ``lead + b * stride``."""
    a = np.asarray(a)
    a = a.reshape(a.shape[0], -1)
    B, n = (1, a.shape[1]) if stride == 0 else a.shape
    flat = np.full(padded_size(B, n, stride, lead), np.nan, dtype=a.dtype)
    for b in range(B):
        flat[lead + b * stride: lead + b * stride + n] = a[b]
    return flat


def unpack_padded(flat, B, n, stride, lead):
    """The inverse of pack_padded: [B, n] (stride 0: [1, n])."""
    rows = 1 if stride == 0 else B
    return np.stack([flat[lead + b * stride: lead + b * stride + n] for b in range(rows)])


def pad_mask(B, n, stride, lead):
    """True where a padded buffer holds pad, False where it holds a record."""
    rows = 1 if stride == 0 else B
    mask = np.ones(padded_size(rows, n, stride, lead), dtype=bool)
    for b in range(rows):
        mask[lead + b * stride: lead + b * stride + n] = False
    return mask


def guard_offset(base_addr, itemsize, align, guard=GUARD):
    """The first element offset >= guard at which a view inside an allocation starting at byte
    address ``base_addr`` is aligned to exactly ``align`` bytes: a multiple of ``align`` and no
    multiple of 2 * align, so that a 16-byte request is not served by a 256-byte aligned start and
    an element-aligned one is never 16-byte aligned by accident."""
    if align % itemsize or base_addr % itemsize:
        raise ValueError('alignment must be a multiple of the element size')
    off = guard
    while (base_addr + off * itemsize) % (2 * align) != align:
        off += 1
    return off


def guarded_size(n, itemsize, align, guard=GUARD):
    """Elements of an allocation that holds a guarded view of n elements wherever it starts."""
    return guard + 2 * align // itemsize + n + guard


def guarded_np(shape, dtype, align, sentinel):
    """(whole flat array, offset, view of ``shape``) of the guarded layout on the host."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape))
    buf = np.full(guarded_size(n, dtype.itemsize, align), sentinel, dtype=dtype)
    off = guard_offset(buf.ctypes.data, dtype.itemsize, align)
    return buf, off, buf[off: off + n].reshape(shape)


# ---------------------------------------------------------------------------- device buffers
def _bits(t):
    import torch
    return t.view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    """Bitwise equality of two tensors (NaN payloads included)."""
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a.contiguous()), _bits(b.contiguous())))


class Padded:
    """A device buffer in the pack_padded layout.  ``ptr`` is the address of element ``lead``."""

    def __init__(self, a, stride, lead, dtype, device='cuda'):
        import torch
        a = np.asarray(a)
        self.B, self.n = a.shape[0], int(np.prod(a.shape[1:]))
        self.stride, self.lead = int(stride), int(lead)
        flat = pack_padded(a.reshape(self.B, self.n), self.stride, self.lead)
        self.buf = torch.as_tensor(flat, device=device).to(dtype)
        self.ptr = self.buf.data_ptr() + self.lead * self.buf.element_size()
        self.before = self.buf.clone()

    def unchanged(self):
        return same_bits(self.buf, self.before)


def padded(a, stride, lead, dtype, device='cuda'):
    return Padded(a, stride, lead, dtype, device)


class Guarded:
    """An output view of ``shape`` inside a larger sentinel-filled allocation, at least GUARD
    elements of it before and after, starting at exactly ``align`` bytes (guard_offset).  The view
    itself starts out as sentinel too, so ``untouched()`` tells whether a call wrote anything."""

    def __init__(self, shape, dtype, align, device='cuda'):
        import torch
        self.sentinel = F_SENTINEL if dtype.is_floating_point else I_SENTINEL
        self.n = int(np.prod(shape))
        isz = torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((guarded_size(self.n, isz, align),), self.sentinel, dtype=dtype, device=device)
        self.off = guard_offset(self.buf.data_ptr(), isz, align)
        self.view = self.buf[self.off: self.off + self.n].view(*shape)
        self.ptr = self.view.data_ptr()
        assert self.ptr % (2 * align) == align and self.off >= GUARD
        assert self.buf.numel() - self.off - self.n >= GUARD

    def check(self):
        lo, hi = self.buf[: self.off], self.buf[self.off + self.n:]
        bad = int((lo != self.sentinel).sum()) + int((hi != self.sentinel).sum())
        assert bad == 0, (f'{bad} guard elements overwritten: before the view at '
                          f'{(lo != self.sentinel).nonzero().flatten().tolist()[:8]}, after it at '
                          f'{(hi != self.sentinel).nonzero().flatten().tolist()[:8]}')

    def untouched(self):
        return bool((self.buf == self.sentinel).all())

    def reset(self):
        self.buf.fill_(self.sentinel)


def guarded(shape, dtype, align=None, device='cuda'):
    """``align`` defaults to the element size (every array but X and U, which take 16)."""
    import torch
    if align is None:
        align = torch.empty((), dtype=dtype).element_size()
    return Guarded(tuple(shape), dtype, align, device)


# ---------------------------------------------------------------------------- the raw caller
def _p(v):
    """None -> NULL; an int -> that address; a tensor / Padded / Guarded -> where its data starts."""
    if v is None:
        return ctypes.c_void_p(0)
    if isinstance(v, (Padded, Guarded)):
        return ctypes.c_void_p(v.ptr)
    if hasattr(v, 'data_ptr'):
        return ctypes.c_void_p(v.data_ptr())
    return ctypes.c_void_p(int(v))


class Raw:
    def __init__(self, m):
        from mpc_blaster_amd import _lib
        self.m, self.lib, self.h = m, _lib.load(), m._h

    def error(self):
        return (self.lib.mpcb_last_error() or b'').decode()

    def solve(self, B, x0, x0_sb, xref, xref_sb, uref, uref_sb, wind, wind_sb, u0, X, U, status, stream=0,
              iterate=False, xbar=None, ubar=None, h=None):
        h = self.h if h is None else h
        if iterate:
            return self.lib.mpcb_solve_iterate(h, B, _p(x0), x0_sb, _p(xbar), _p(ubar), _p(xref), xref_sb,
                                               _p(uref), uref_sb, _p(wind), wind_sb, _p(u0), _p(X), _p(U),
                                               _p(status), _p(stream))
        return self.lib.mpcb_solve(h, B, _p(x0), x0_sb, _p(xref), xref_sb, _p(uref), uref_sb, _p(wind), wind_sb,
                                   _p(u0), _p(X), _p(U), _p(status), _p(stream))

    def eval(self, B, x0, x0_sb, X, U, xref, xref_sb, uref, uref_sb, wind, wind_sb, cost, res_eq, res_ineq,
             res_stat, stream=0):
        return self.lib.mpcb_eval(self.h, B, _p(x0), x0_sb, _p(X), _p(U), _p(xref), xref_sb, _p(uref), uref_sb,
                                  _p(wind), wind_sb, _p(cost), _p(res_eq), _p(res_ineq), _p(res_stat), _p(stream))

    def vjp_w(self, B, xbar, ubar, X, U, xref, xref_sb, uref, uref_sb, wind, wind_sb, gX, gU, gx0, gxref, guref,
              gQ, gR, gQN, status, stream=0):
        return self.lib.mpcb_solve_vjp_w(self.h, B, _p(xbar), _p(ubar), _p(X), _p(U), _p(xref), xref_sb, _p(uref),
                                         uref_sb, _p(wind), wind_sb, _p(gX), _p(gU), _p(gx0), _p(gxref), _p(guref),
                                         _p(gQ), _p(gR), _p(gQN), _p(status), _p(stream))

    def vjp17(self, B, xbar, ubar, fixed, X, U, xref, xref_sb, uref, uref_sb, gX, gU, gx0, gxref, guref, gQ, gR,
              gQN, status, stream=0):
        return self.lib.mpcb_solve_vjp17(self.h, B, _p(xbar), _p(ubar), _p(fixed), _p(X), _p(U), _p(xref), xref_sb,
                                         _p(uref), uref_sb, _p(gX), _p(gU), _p(gx0), _p(gxref), _p(guref), _p(gQ),
                                         _p(gR), _p(gQN), _p(status), _p(stream))

    def linearize(self, B, xbar, ubar, wind, wind_sb, A, Bm, xnext, stream=0):
        return self.lib.mpcb_linearize(self.h, B, _p(xbar), _p(ubar), _p(wind), wind_sb, _p(A), _p(Bm), _p(xnext),
                                       _p(stream))

    def sim_step(self, B, x, u, wind, wind_sb, T, x_out, stream=0):
        return self.lib.mpcb_sim_step(self.h, B, _p(x), _p(u), _p(wind), wind_sb, float(T), _p(x_out), _p(stream))

    def gen_inputs(self, B, seed, id_offset, ref_kind, x0, xref, xref_sb, uref, uref_sb, wind, stream=0):
        return self.lib.mpcb_gen_inputs(self.h, B, int(seed), int(id_offset), int(ref_kind), _p(x0), _p(xref),
                                        xref_sb, _p(uref), uref_sb, _p(wind), _p(stream))

    def set_params(self, count, params, params_sb, params_kb):
        return self.lib.mpcb_set_params(self.h, count, _p(params), params_sb, params_kb)

    def qp_stats(self, B, out, stream=0):
        return self.lib.mpcb_qp_stats(self.h, B, _p(out), _p(stream))

    def histogram(self, B, u0, lo, hi, nbins, counts, stream=0):
        return self.lib.mpcb_histogram(self.h, B, _p(u0), float(lo), float(hi), int(nbins), _p(counts), _p(stream))
