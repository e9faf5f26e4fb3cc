"""What holds a ray matrix (capi.Context.ray_matrix(with_depth=True): row_ptr, col, dz, z_exit) to the reference's segment
lists, shared by tests/test_gpu_ray_matrix.py and the geometry sweep of tests/derivative_fuzz.py.  Plain asserts: a caller
that collects mismatches catches AssertionError.

Bars (tests/derivative_fuzz.py's, none fitted to what the GPU returns).  Chords and depths: |error| <= unit x max(1, F),
unit = 16 x 2^-52 x max(1, max |view-space coordinate|) (derivative_fuzz.dz_err), F = |gx| + |gy| of the steeper of the
segment's two faces (adjoint_reference.segment_lists(with_slope=True)).  Structure - the sorted (pixel, cell) pairs - must
match exactly; the order inside a row is checked apart: z_exit never decreases."""
import numpy as np


def rows_of(row_ptr):
    return np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))


def check_csr(m, n_px, n_cells, depth_order: bool = True):
    """depth_order=False leaves out "z_exit never decreases" (tests/test_gpu_degenerate_rays.py: the one scene where it does
    not hold, by a rounding)."""
    row_ptr, col, dz, z_exit = m
    assert row_ptr.dtype == np.int64 and col.dtype == np.int32 and dz.dtype == np.float64 and z_exit.dtype == np.float64
    assert row_ptr.shape == (n_px + 1,) and row_ptr[0] == 0 and (np.diff(row_ptr) >= 0).all()
    assert len(col) == len(dz) == len(z_exit) == row_ptr[-1]
    assert ((col >= 0) & (col < n_cells)).all() and (dz > 0).all() and np.isfinite(dz).all() and np.isfinite(z_exit).all()
    pix = rows_of(row_ptr)
    assert len(np.unique(pix * np.int64(n_cells) + col)) == len(col)  # a ray crosses a cell at most once
    inside = pix[1:] == pix[:-1]
    assert not depth_order or (np.diff(z_exit)[inside] >= 0).all()  # deepest first, z ascending
    return pix


def check_against_reference(m, reference, unit, n_px, n_cells, want, what, log=print):
    """Structure exactly, nnz, dz and z_exit within the chord bar; logs and returns the worst error / bar of both.
    reference: segment_lists(with_slope=True)'s (pixel, cell, z_hi, dz, slope) of the frame's pixels; want: the number of
    segments the frame is known to have."""
    rpix, rcell, rzh, rdz, rslope = reference
    row_ptr, col, dz, z_exit = m
    pix = check_csr(m, n_px, n_cells)
    assert len(rpix) == want  # (the reference's own count: the scene is what it is said to be)
    assert row_ptr[-1] == want
    og, orf = np.lexsort((col, pix)), np.lexsort((rcell, rpix))
    assert np.array_equal(pix[og], rpix[orf]) and np.array_equal(col[og], rcell[orf])
    if want == 0:
        return 0.0, 0.0
    bar = unit * np.maximum(1.0, rslope[orf])
    e_dz, e_z = np.abs(dz[og] - rdz[orf]) / bar, np.abs(z_exit[og] - rzh[orf]) / bar
    log(f"{what}: nnz {want}, smallest chord {rdz.min():.3g}, bar {bar.min():.3g} .. {bar.max():.3g}, worst error / bar: "
        f"dz {e_dz.max():.3g}, z_exit {e_z.max():.3g}")
    assert (e_dz <= 1.0).all(), f"{what}: {int((e_dz > 1).sum())} chords over their bar, worst {e_dz.max():.3g}"
    assert (e_z <= 1.0).all(), f"{what}: {int((e_z > 1).sum())} depths over their bar, worst {e_z.max():.3g}"
    return float(e_dz.max()), float(e_z.max())


def bit_equal_rows(part, whole, global_px):
    """The rows of `part` (local pixels = global_px of the whole frame) are bit for bit those rows of `whole`."""
    (rp, col, dz, z), (wrp, wcol, wdz, wz) = part, whole
    lengths = (wrp[1:] - wrp[:-1])[global_px]
    if not np.array_equal(np.diff(rp), lengths):
        return False
    at = np.repeat(wrp[global_px] - rp[:-1], lengths) + np.arange(rp[-1])
    return (np.array_equal(col, wcol[at]) and np.array_equal(dz.view(np.uint64), wdz[at].view(np.uint64))
            and np.array_equal(z.view(np.uint64), wz[at].view(np.uint64)))
