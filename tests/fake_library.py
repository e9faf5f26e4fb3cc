"""Stand-ins for the shared library behind a capi.Context, for the tests that run without a GPU: one that fails the test
when a wrapper reaches it, one that writes down what it was sent, and the context that carries either."""
import ctypes
import numbers

import numpy as np

from course5_amd import capi


class NoLibrary:
    """Any call into the library fails the test: the wrapper's argument checks must have raised before."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was entered ({name})")


def _normalised(arg):
    if isinstance(arg, ctypes.c_void_p):
        arg = arg.value
    if arg is None or isinstance(arg, numbers.Integral):
        return int(arg) if arg else None  # (NULL is NULL, however it was spelt)
    return float(arg) if isinstance(arg, float) else "ptr"


class RecordingLibrary:
    """Every symbol is a call that appends (symbol, arguments) to `calls` and returns C5_OK.  The arguments are normalised:
    None, a NULL c_void_p and 0 are None; other integers and c_void_p values are int; floats are float; every other ctypes
    pointer or array is the string "ptr"."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, symbol):
        def call(*args):
            self.calls.append((symbol, tuple(_normalised(a) for a in args)))
            return capi.C5_OK
        return call


class _BareContext(capi.Context):
    local_rows = property(lambda self: self.__dict__["_local_rows"])  # (the real one asks the library)


def bare_context(n_cells=7, n_pts=9, rows=5, cols=6):
    """A capi.Context that was never created (no GPU here: the argument checks come before the library) over NoLibrary;
    give it another `lib` to let calls through."""
    ctx = _BareContext.__new__(_BareContext)
    ctx.lib, ctx.handle = NoLibrary(), None
    ctx.n_cells, ctx.n_pts, ctx.res_x, ctx.res_y, ctx.device = n_cells, n_pts, cols, rows, 0
    ctx.rots = np.zeros((0, 3))
    ctx.__dict__["_local_rows"] = rows
    return ctx
