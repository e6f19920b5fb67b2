"""The index arithmetic of tests/abi_call.py's buffer builders, on the host: the layouts that
tests/test_gpu_abi.py hands to the C ABI are what they claim to be."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_call as ab   # noqa: E402


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('B,n,stride,lead', [(7, 12, 13, 1), (7, 84, 87, 1), (70, 24, 25, 1), (3, 3, 5, 1),
                                             (5, 12, 12, 0), (1, 12, 13, 3), (4, 25, 182, 2)])
def test_padded_round_trip(B, n, stride, lead, dtype):
    rng = np.random.default_rng(B * 1000 + n)
    a = rng.standard_normal((B, n)).astype(dtype)
    flat = ab.pack_padded(a, stride, lead)
    assert flat.dtype == a.dtype and flat.ndim == 1
    assert flat.size == ab.padded_size(B, n, stride, lead) == lead + B * stride + ab.TAIL
    for b in range(B):   # the stated offsets, spelled out
        assert (flat[lead + b * stride: lead + b * stride + n] == a[b]).all()
    assert (ab.unpack_padded(flat, B, n, stride, lead) == a).all()
    # only pad elements are NaN, and every pad element is
    mask = ab.pad_mask(B, n, stride, lead)
    assert mask.sum() == flat.size - B * n
    assert np.isnan(flat[mask]).all() and not np.isnan(flat[~mask]).any()
    # the lead, the gaps between records and the tail are pad
    assert mask[:lead].all() and mask[-ab.TAIL:].all()
    if stride > n:
        assert mask[lead + n: lead + stride].all()


def test_padded_stride_zero_is_one_record():
    a = np.arange(24.0).reshape(2, 12)
    flat = ab.pack_padded(a, 0, 1)
    assert flat.size == 1 + 12 + ab.TAIL
    assert np.isnan(flat[0]) and (flat[1:13] == a[0]).all() and np.isnan(flat[13:]).all()
    assert (ab.unpack_padded(flat, 2, 12, 0, 1) == a[:1]).all()
    assert ab.pad_mask(2, 12, 0, 1).sum() == 1 + ab.TAIL


def test_padded_refuses_overlapping_records():
    with pytest.raises(ValueError):
        ab.pack_padded(np.zeros((3, 12)), 11, 1)


@pytest.mark.parametrize('dtype,align', [(np.float64, 16), (np.float32, 16), (np.float64, 8), (np.float32, 4),
                                         (np.int32, 4), (np.int64, 8)])
@pytest.mark.parametrize('shape', [(7, 4), (7, 7, 12), (1,), (70, 6, 6)])
def test_guarded_layout(shape, dtype, align):
    sentinel = ab.F_SENTINEL if np.issubdtype(dtype, np.floating) else ab.I_SENTINEL
    buf, off, view = ab.guarded_np(shape, dtype, align, sentinel)
    n = int(np.prod(shape))
    assert view.shape == tuple(shape) and view.base is not None and np.shares_memory(view, buf)
    # exactly the requested alignment: no stricter one by accident
    assert view.ctypes.data % align == 0 and view.ctypes.data % (2 * align) == align
    assert view.ctypes.data == buf.ctypes.data + off * buf.itemsize
    assert off >= ab.GUARD and buf.size - off - n >= ab.GUARD
    assert (buf == sentinel).all() and np.isfinite(float(sentinel))
    view[...] = 1
    assert (buf[:off] == sentinel).all() and (buf[off + n:] == sentinel).all() and (buf[off: off + n] == 1).all()


@pytest.mark.parametrize('itemsize,align', [(8, 16), (4, 16), (8, 8), (4, 4)])
def test_guard_offset_for_any_base(itemsize, align):
    """Whatever the allocation's own alignment, the offset exists within the slack guarded_size
    leaves, and is the first one at or after the guard."""
    for base in range(0, 512, itemsize):
        off = ab.guard_offset(base, itemsize, align)
        assert (base + off * itemsize) % (2 * align) == align
        assert ab.GUARD <= off < ab.GUARD + 2 * align // itemsize
        assert off + 1 + ab.GUARD <= ab.guarded_size(1, itemsize, align)
        assert not any((base + o * itemsize) % (2 * align) == align for o in range(ab.GUARD, off))
