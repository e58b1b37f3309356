"""What the GPU test modules do alike, stated once: each of these was pasted, body for body, into several of them.  They keep
the names under which the tests call them.  Nothing here touches the GPU until it is called."""
import contextlib
import ctypes
import io

import numpy


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _field(*a, **kw):
    from nemoflux_amd.field import Field
    return _quiet(Field.fromArrays, *a, **kw)


def _on(a, resident):
    import torch
    return torch.from_numpy(numpy.ascontiguousarray(a)).cuda() if resident else numpy.ascontiguousarray(a)


def _rows(pair):
    """[segments | transects] rows of a (totals, segments) pair, the axes in front kept"""
    tot, seg = pair
    return numpy.concatenate([seg, tot], axis=-1)


def _resident(f):
    """the step that is resident in the handle: integrated velocity, eU, eV and the largest edge flux"""
    from nemoflux_amd import _lib
    from nemoflux_amd._lib import lib, check
    n = f.ny * f.nx
    iV, eU, eV, mx = numpy.zeros((n, 4)), numpy.zeros(n), numpy.zeros(n), ctypes.c_double()
    check(lib.nf_field_read_step(ctypes.byref(f._h), _lib.dptr(iV), _lib.dptr(eU), _lib.dptr(eV), ctypes.byref(mx)))
    return iV, eU, eV, mx.value


def _same_bits(a, b):
    a, b = numpy.ascontiguousarray(a, numpy.float64), numpy.ascontiguousarray(b, numpy.float64)
    return a.shape == b.shape and numpy.array_equal(a.view(numpy.uint64), b.view(numpy.uint64))


@contextlib.contextmanager
def _knob(name, value, default):
    """one tuning knob set to `value` inside the block, back to `default` after it"""
    from nemoflux_amd._lib import lib, check
    check(lib.nf_tuning_set(name, int(value)))
    try:
        yield
    finally:
        check(lib.nf_tuning_set(name, default))
