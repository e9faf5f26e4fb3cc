"""ctypes binding of the C ABI in include/course5_hip.h (libcourse5_hip.so).

Test/bench plumbing only: the product is the shared library and the `course` CLI.  There is no
CPU fallback here — if the library is missing or no GPU is present, calls raise.

When device buffers are shared with PyTorch (render_device into a torch tensor), import torch
BEFORE the first call into this module: torch bundles its own HIP runtime, and whichever runtime is
loaded first serves the whole process.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("C5_LIB", os.path.join(PKG, "libcourse5_hip.so"))  # C5_LIB: A/B another build

C5_OK, C5_ERR_INVALID, C5_ERR_STATE, C5_ERR_HIP, C5_ERR_MESH, C5_ERR_NO_DEVICE, C5_ERR_WALK, C5_RETRY = range(8)
# the kinds of exact sums of c5_render_exact_bounds / c5_render_exact_sums
C5_EXACT_ADJOINT, C5_EXACT_GN_DIAGONAL, C5_EXACT_HVP = range(3)
# the smoothness prior's penalties and weightings (c5_prior)
C5_PRIOR_QUADRATIC, C5_PRIOR_PSEUDO_HUBER = range(2)
C5_PRIOR_UNIT, C5_PRIOR_TPFA = range(2)
# the shape prior's energies (c5_shape_prior)
C5_SHAPE_DIRICHLET, C5_SHAPE_NEO_HOOKEAN = range(2)


class Rotation(C.Structure):
    _fields_ = [("axis", C.c_int32), ("reserved", C.c_int32), ("angle", C.c_double), ("x0", C.c_double)]


class Stats(C.Structure):
    _fields_ = [("segments", C.c_int64), ("covered_pixels", C.c_int64), ("solid_pixels", C.c_int64),
                ("entries", C.c_int64), ("boundary_faces", C.c_int64), ("steps", C.c_int64),
                ("walk_overflow", C.c_int32), ("entry_overflow", C.c_int32),
                ("ms_transform", C.c_float), ("ms_records", C.c_float), ("ms_entries", C.c_float),
                ("ms_solids", C.c_float), ("ms_walk", C.c_float), ("ms_total", C.c_float),
                ("odd_pixels", C.c_int64), ("pool_entries", C.c_int64), ("pool_capacity", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Prior(C.Structure):
    """c5_prior: the smoothness prior's penalty, weighting, and per field its lambda (0: the field is left out) and the
    pseudo-Huber delta."""
    _fields_ = [("penalty", C.c_int32), ("weighting", C.c_int32), ("lambda_alpha", C.c_double), ("lambda_q", C.c_double),
                ("delta_alpha", C.c_double), ("delta_q", C.c_double)]

    def __init__(self, penalty=C5_PRIOR_QUADRATIC, weighting=C5_PRIOR_TPFA, lambda_alpha=0.0, lambda_q=0.0, delta_alpha=1.0, delta_q=1.0):
        super().__init__(int(penalty), int(weighting), float(lambda_alpha), float(lambda_q), float(delta_alpha), float(delta_q))


class ShapePrior(C.Structure):
    """c5_shape_prior: the shape prior's energy, its weight lambda and the Neo-Hookean volume term's kappa."""
    _fields_ = [("energy", C.c_int32), ("reserved", C.c_int32), ("lambda_", C.c_double), ("kappa", C.c_double)]

    def __init__(self, energy=C5_SHAPE_NEO_HOOKEAN, lambda_=0.0, kappa=1.0, reserved=0):
        super().__init__(int(energy), int(reserved), float(lambda_), float(kappa))


class C5Error(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"[c5 status {code}] {message}")
        self.code = code
        self.message = message


_vp, _dp_t, _fp_t, _ip_t, _lp_t = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
_rp_t = C.POINTER(Rotation)
_pp_t = C.POINTER(Prior)
_sp_t = C.POINTER(ShapePrior)

# every symbol include/course5_hip.h declares: its argument types, or (argument types, result type) where that is not int
SIGNATURES = {
    "c5_abi_version": None,
    "c5_device_count": [C.POINTER(C.c_int)],
    "c5_create": [C.c_int, C.POINTER(_vp)],
    "c5_destroy": ([_vp], None),
    "c5_last_error": ([_vp], C.c_char_p),
    "c5_upload_grid": [_vp, _dp_t, C.c_int64, _ip_t, C.c_int64, _dp_t, _dp_t],
    "c5_update_scalars": [_vp, _dp_t, _dp_t, C.c_int64],
    "c5_set_solid": [_vp, C.c_int, _dp_t, C.c_int64, C.c_double],
    "c5_set_image": [_vp, C.c_int, C.c_int, _dp_t],
    "c5_set_row_tiles": [_vp, C.c_int, C.c_int, C.c_int],
    "c5_local_rows": [_vp, C.POINTER(C.c_int)],
    "c5_set_view": [_vp, _rp_t, C.c_int],
    "c5_set_solid_view": [_vp, C.c_int, _rp_t, C.c_int],
    "c5_set_alpha_limit": [_vp, C.c_double],
    "c5_set_option": [_vp, C.c_char_p, C.c_double],
    "c5_render": [_vp, _fp_t],
    "c5_render_device": [_vp, _vp],
    "c5_synchronize": [_vp],
    "c5_get_stats": [_vp, C.POINTER(Stats)],
    "c5_walk_kernel_ms": [_vp, C.c_int, _dp_t, _lp_t],
    "c5_download_view_points": [_vp, _dp_t],
    "c5_face_adjacency": [_ip_t, C.c_int64, C.c_int64, _ip_t, _lp_t],
    "c5_set_stream": [_vp, _vp],
    "c5_set_row_range": [_vp, C.c_int, C.c_int],
    "c5_get_row_costs": [_vp, C.POINTER(C.c_uint32), C.c_int],
    "c5_weld_points": [_dp_t, C.c_int64, _ip_t, _lp_t],
    "c5_render_host_async": [_vp, _fp_t],
    "c5_render_host_wait": [_vp],
    "c5_host_alloc": [_vp, C.c_size_t, C.POINTER(_vp)],
    "c5_host_free": [_vp, _vp],
    "c5_render_frame_rows_async": [_vp, _fp_t],
    "c5_render_adjoint": [_vp, _fp_t, _dp_t, _dp_t],
    "c5_render_adjoint_device": [_vp, _vp, _vp, _vp],
    "c5_render_tangent": [_vp, _dp_t, _dp_t, _fp_t],
    "c5_render_tangent_device": [_vp, _vp, _vp, _vp],
    "c5_render_tangent_batch": [_vp, C.c_int, _dp_t, _dp_t, _fp_t],
    "c5_render_tangent_batch_device": [_vp, C.c_int, _vp, _vp, _vp],
    "c5_render_adjoint_batch": [_vp, C.c_int, _fp_t, _dp_t, _dp_t],
    "c5_render_adjoint_batch_device": [_vp, C.c_int, _vp, _vp, _vp],
    "c5_update_scalars_device": [_vp, _vp, _vp, C.c_int64],
    "c5_render_gn_product": [_vp, C.c_int, _dp_t, _dp_t, _fp_t, _dp_t, _dp_t, _fp_t],
    "c5_render_gn_product_device": [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp],
    "c5_render_gn_diagonal": [_vp, _fp_t, _dp_t, _dp_t],
    "c5_render_gn_diagonal_device": [_vp, _vp, _vp, _vp],
    "c5_render_hvp": [_vp, _dp_t, _dp_t, _fp_t, _dp_t, _dp_t],
    "c5_render_hvp_device": [_vp, _vp, _vp, _vp, _vp, _vp],
    "c5_render_motion_tangent": [_vp, C.c_int, _dp_t, _fp_t],
    "c5_render_motion_tangent_device": [_vp, C.c_int, _dp_t, _vp],
    "c5_rotation_motion": [_rp_t, C.c_int, C.c_int, C.c_int, _dp_t],
    "c5_render_vertex_adjoint": [_vp, _fp_t, _dp_t],
    "c5_render_vertex_adjoint_device": [_vp, _vp, _vp],
    "c5_render_vertex_adjoint_batch": [_vp, C.c_int, _fp_t, _dp_t],
    "c5_render_vertex_adjoint_batch_device": [_vp, C.c_int, _vp, _vp],
    "c5_render_vertex_exact_bounds": [_vp, _fp_t, _ip_t],
    "c5_render_vertex_exact_bounds_device": [_vp, _vp, _vp],
    "c5_render_vertex_exact_sums": [_vp, _fp_t, _ip_t, _lp_t],
    "c5_render_vertex_exact_sums_device": [_vp, _vp, _vp, _vp],
    "c5_vertex_exact_finish": [_vp, _ip_t, _lp_t, _dp_t],
    "c5_vertex_exact_finish_device": [_vp, _vp, _vp, _vp],
    "c5_update_points": [_vp, _dp_t, C.c_int64],
    "c5_render_vertex_tangent": [_vp, C.c_int, _dp_t, _fp_t],
    "c5_render_vertex_tangent_device": [_vp, C.c_int, _vp, _vp],
    "c5_render_vertex_gn_product": [_vp, C.c_int, _dp_t, _fp_t, _dp_t, _fp_t],
    "c5_render_vertex_gn_product_device": [_vp, C.c_int, _vp, _vp, _vp, _vp],
    "c5_ray_matrix_rows": [_vp, _lp_t, _lp_t],
    "c5_ray_matrix_rows_device": [_vp, _vp, _lp_t],
    "c5_ray_matrix_fill": [_vp, _lp_t, C.c_int64, _ip_t, _dp_t, _dp_t],
    "c5_ray_matrix_fill_device": [_vp, _vp, C.c_int64, _vp, _vp, _vp],
    "c5_ray_jacobian_fill": [_vp, _lp_t, C.c_int64, _ip_t, _dp_t, _dp_t, _dp_t],
    "c5_ray_jacobian_fill_device": [_vp, _vp, C.c_int64, _vp, _vp, _vp, _vp],
    "c5_ray_shape_jacobian_fill": [_vp, _lp_t, C.c_int64, _dp_t, C.POINTER(C.c_uint8), _dp_t],
    "c5_ray_shape_jacobian_fill_device": [_vp, _vp, C.c_int64, _vp, _vp, _vp],
    "c5_face_gradients": [_vp, _ip_t, _dp_t],
    "c5_face_gradients_device": [_vp, _vp, _vp],
    "c5_render_adjoint_exact_bounds": [_vp, _fp_t, _ip_t, _ip_t],
    "c5_render_adjoint_exact_bounds_device": [_vp, _vp, _vp, _vp],
    "c5_render_adjoint_exact_sums": [_vp, _fp_t, _ip_t, _ip_t, _lp_t, _lp_t],
    "c5_render_adjoint_exact_sums_device": [_vp, _vp, _vp, _vp, _vp, _vp],
    "c5_render_exact_bounds": [_vp, C.c_int, _dp_t, _dp_t, _fp_t, _ip_t, _ip_t],
    "c5_render_exact_bounds_device": [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp],
    "c5_render_exact_sums": [_vp, C.c_int, _dp_t, _dp_t, _fp_t, _ip_t, _ip_t, _lp_t, _lp_t],
    "c5_render_exact_sums_device": [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "c5_exact_sums_finish": [_ip_t, _lp_t, C.c_int64, C.c_int, C.c_int, _dp_t],
    "c5_exact_quantise": [_dp_t, C.c_int64, C.c_int32, C.c_int, C.c_int, _lp_t],
    "c5_prior_weights": [_vp, C.c_int, _dp_t, _lp_t, _lp_t],
    "c5_prior_weights_device": [_vp, C.c_int, _vp, _lp_t, _lp_t],
    "c5_prior_gradient": [_vp, _pp_t, _dp_t, _dp_t, _dp_t, _dp_t, _dp_t],
    "c5_prior_gradient_device": [_vp, _pp_t, _vp, _vp, _vp, _vp, _vp],
    "c5_prior_product": [_vp, _pp_t, _dp_t, _dp_t, _dp_t, _dp_t, _dp_t, _dp_t],
    "c5_prior_product_device": [_vp, _pp_t, _vp, _vp, _vp, _vp, _vp, _vp],
    "c5_prior_diagonal": [_vp, _pp_t, _dp_t, _dp_t, _dp_t, _dp_t],
    "c5_prior_diagonal_device": [_vp, _pp_t, _vp, _vp, _vp, _vp],
    "c5_shape_prior_rest": [_vp, _dp_t, C.c_int64, _lp_t],
    "c5_shape_prior_rest_device": [_vp, _vp, C.c_int64, _lp_t],
    "c5_shape_prior_rest_data": [_vp, _dp_t, _dp_t, _ip_t],
    "c5_shape_prior_rest_data_device": [_vp, _vp, _vp, _vp],
    "c5_shape_prior_gradient": [_vp, _sp_t, _dp_t, _dp_t, _lp_t, _dp_t],
    "c5_shape_prior_gradient_device": [_vp, _sp_t, _vp, _vp, _vp, _vp],
    "c5_shape_prior_product": [_vp, _sp_t, _dp_t, _dp_t, _dp_t],
    "c5_shape_prior_product_device": [_vp, _sp_t, _vp, _vp, _vp],
    "c5_shape_prior_diagonal": [_vp, _sp_t, _dp_t, _dp_t],
    "c5_shape_prior_diagonal_device": [_vp, _sp_t, _vp, _vp],
    "c5_shape_prior_quality": [_vp, _dp_t, _dp_t, _lp_t],
    "c5_shape_prior_quality_device": [_vp, _vp, _vp, _vp],
}
EXPORTS = list(SIGNATURES)

_lib = None


def load_library() -> C.CDLL:
    """dlopen the in-tree library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} is missing: run `python -m course5_amd.build` (or __graft_entry__.build())")
    lib = C.CDLL(LIB_PATH)
    for name, signature in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = signature if isinstance(signature, tuple) else (signature, C.c_int)
    _lib = lib
    return lib


def _rot_array(rots) -> tuple:
    rots = np.asarray(rots, dtype=np.float64).reshape(-1, 3)
    arr = (Rotation * max(len(rots), 1))()
    for k, (axis, angle, x0) in enumerate(rots):
        arr[k].axis = int(axis)
        arr[k].angle = float(angle)
        arr[k].x0 = float(x0)
    return arr, len(rots)


def _dp(a):
    """The pointer of a float64 array, or NULL for None."""
    return None if a is None else a.ctypes.data_as(_dp_t)


def _fp(a):
    """The pointer of a float32 array, or NULL for None."""
    return None if a is None else a.ctypes.data_as(_fp_t)


def _device_ptr(t, dtype, shape) -> int:
    """A raw device pointer as it is (None: 0), or the data pointer of a contiguous torch tensor of that dtype and shape
    on the GPU."""
    if t is None or isinstance(t, int):
        return t or 0
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or not t.is_cuda:
        raise ValueError(f"expected a contiguous {dtype} tensor of shape {tuple(shape)} on the GPU")
    return t.data_ptr()


class Context:
    """One GPU render context (c5_context)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        self.handle = C.c_void_p()
        rc = self.lib.c5_create(device, C.byref(self.handle))
        if rc != C5_OK:
            raise C5Error(rc, self.lib.c5_last_error(None).decode())
        self.device = device
        self.res_x = self.res_y = 0
        self.n_cells = 0
        self.n_pts = 0
        self.points = np.zeros((0, 3))  # the points as upload_grid / update_points last had them (course5_amd.autograd.render_mesh)
        # bumped by everything that changes which frame a render produces apart from the cells' scalars (grid, view, image,
        # rows, solids, alpha limit): course5_amd.autograd refuses to differentiate a frame other than the one it rendered
        self.frame_state = 0
        # which set of scalars the context holds (course5_amd.autograd; None: the caller's own)
        self.scalars_owner = None
        self.stream_ptr = 0
        self.rots = np.zeros((0, 3))  # the view as set_view last had it: rows (axis, angle, x0)
        # the library's instruments are off by default (they cost 5 % of a frame); tests and scripts read stats()["ms_*"] and
        # walk_kernel_ms() everywhere, so this wrapper switches them on - bench.py switches the stage events off again
        self.set_option("stage_timing", 1)
        self.set_option("walk_timing", 1)

    def close(self):
        if getattr(self, "handle", None) and self.handle.value:
            self.lib.c5_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int, allow=()):
        if rc != C5_OK and rc not in allow:
            raise C5Error(rc, self.lib.c5_last_error(self.handle).decode())
        return rc

    def set_stream(self, stream_ptr: int):
        """Run on a caller-owned HIP stream (e.g. torch.cuda.current_stream().cuda_stream); 0 = own."""
        rc = self._check(self.lib.c5_set_stream(self.handle, C.c_void_p(stream_ptr)), allow=(C5_RETRY,))
        self.stream_ptr = stream_ptr
        return rc

    # -- scene ---------------------------------------------------------------------------------
    def upload_grid(self, xyz, cells, alpha, q):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 4)
        alpha = np.ascontiguousarray(alpha, dtype=np.float64)
        q = np.ascontiguousarray(q, dtype=np.float64)
        if alpha.shape[0] != cells.shape[0] or q.shape[0] != cells.shape[0]:
            raise ValueError("one alpha and one q per cell")
        self._check(self.lib.c5_upload_grid(self.handle, _dp(xyz), xyz.shape[0],
                                            cells.ctypes.data_as(C.POINTER(C.c_int32)), cells.shape[0],
                                            _dp(alpha), _dp(q)))
        self.n_cells = cells.shape[0]
        self.n_pts = xyz.shape[0]
        self.frame_state += 1
        self.scalars_owner = None
        self.points = xyz.copy()

    def update_points(self, xyz):
        """Replace the coordinates of the uploaded grid's points (float64 [n_pts, 3], the order of upload_grid);
        connectivity, weld groups, cell order and scalars stay.  A render after it is bit for bit that of a fresh context
        uploaded with these coordinates, as long as they create no new coincident points.  Waits for the stream."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        if xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError(f"xyz must be [n_pts, 3], not {list(xyz.shape)}")
        self._check(self.lib.c5_update_points(self.handle, _dp(xyz), xyz.shape[0]))
        self.frame_state += 1
        self.points = xyz.copy()

    def update_scalars(self, alpha, q):
        alpha = np.ascontiguousarray(alpha, dtype=np.float64)
        q = np.ascontiguousarray(q, dtype=np.float64)
        self._check(self.lib.c5_update_scalars(self.handle, _dp(alpha), _dp(q), alpha.shape[0]))
        self.scalars_owner = None

    def update_scalars_device(self, alpha, q):
        """update_scalars from device memory: torch tensors on this context's GPU (float64 [n_cells] contiguous) or raw
        device pointers, read on the context's stream.  Waits for the stream (the host needs the largest and smallest
        alpha back)."""
        import torch
        n = self.n_cells
        self._check(self.lib.c5_update_scalars_device(
            self.handle, C.c_void_p(_device_ptr(alpha, torch.float64, (n,))), C.c_void_p(_device_ptr(q, torch.float64, (n,))), n))
        self.scalars_owner = None

    def set_solid(self, slot: int, tets, colour: float = float("nan")):
        tets = np.ascontiguousarray(tets, dtype=np.float64).reshape(-1, 12)
        self._check(self.lib.c5_set_solid(self.handle, slot, _dp(tets), tets.shape[0], colour))
        self.frame_state += 1

    # -- per frame -----------------------------------------------------------------------------
    def set_image(self, res_x: int, res_y: int, bounds):
        b = np.ascontiguousarray(bounds, dtype=np.float64)
        self._check(self.lib.c5_set_image(self.handle, res_x, res_y, _dp(b)))
        self.res_x, self.res_y = res_x, res_y
        self.frame_state += 1

    def set_row_tiles(self, tile_rows: int, rank: int, world: int):
        self._check(self.lib.c5_set_row_tiles(self.handle, tile_rows, rank, world))
        self.frame_state += 1

    def set_row_range(self, row_begin: int, row_count: int = -1):
        self._check(self.lib.c5_set_row_range(self.handle, row_begin, row_count))
        self.frame_state += 1

    def row_costs(self) -> np.ndarray:
        """Segments per local row of the last frame (option "row_costs" must be on)."""
        out = np.zeros(self.local_rows, dtype=np.uint32)
        self._check(self.lib.c5_get_row_costs(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size))
        return out

    @property
    def local_rows(self) -> int:
        n = C.c_int()
        self._check(self.lib.c5_local_rows(self.handle, C.byref(n)))
        return n.value

    def set_view(self, rots):
        arr, n = _rot_array(rots)
        self._check(self.lib.c5_set_view(self.handle, arr, n))
        self.rots = np.array(rots, dtype=np.float64).reshape(-1, 3)
        self.frame_state += 1

    def set_solid_view(self, slot: int, rots):
        arr, n = _rot_array(rots)
        self._check(self.lib.c5_set_solid_view(self.handle, slot, arr, n))
        self.frame_state += 1

    def set_alpha_limit(self, v: float):
        self._check(self.lib.c5_set_alpha_limit(self.handle, v))
        self.frame_state += 1

    def set_option(self, name: str, value: float):
        self._check(self.lib.c5_set_option(self.handle, name.encode(), float(value)))

    # -- render --------------------------------------------------------------------------------
    def render(self) -> np.ndarray:
        """Synchronous render of the local rows -> float32 [rows, res_x, 2] on the host."""
        out = np.empty((self.local_rows, self.res_x, 2), dtype=np.float32)
        self._check(self.lib.c5_render(self.handle, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def render_device(self, device_ptr: int):
        """Asynchronous render into device memory (e.g. a torch tensor's data_ptr())."""
        self._check(self.lib.c5_render_device(self.handle, C.c_void_p(device_ptr)))

    # -- the derivative renders' arguments -------------------------------------------------------------
    # host forms: numpy arrays, checked here (the messages name the argument); device forms: _device_ptr
    def _image(self, a, name: str, batch: bool = False) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.float32)
        shape = (self.local_rows, self.res_x, 2)
        if (a.shape[1:] if batch else a.shape) != shape:
            raise ValueError(f"{name} must be [{'K, ' if batch else ''}{shape[0]}, {shape[1]}, 2], not {list(a.shape)}")
        return a

    def _direction(self, d):
        if d is None:
            return None
        d = np.ascontiguousarray(d, dtype=np.float64)
        if d.shape != (self.n_cells,):
            raise ValueError(f"a direction must hold one value per cell ({self.n_cells}), not {list(d.shape)}")
        return d

    @staticmethod
    def _fit(fit, once: bool = False) -> tuple:
        fit = tuple(fit)
        if not fit or any(f not in ("alpha", "q") for f in fit) or (once and len(set(fit)) != len(fit)):
            raise ValueError(f"fit must name 'alpha', 'q' or both, not {fit!r}")
        return fit

    def _images(self, k: int) -> np.ndarray:
        return np.zeros((k, self.local_rows, self.res_x, 2), dtype=np.float32)

    def _cells_dev(self, t, k: int | None = None) -> int:
        import torch
        return _device_ptr(t, torch.float64, (self.n_cells,) if k is None else (k, self.n_cells))

    def _image_dev(self, t, k: int | None = None) -> int:
        import torch
        shape = (self.local_rows, self.res_x, 2)
        return _device_ptr(t, torch.float32, shape if k is None else (k,) + shape)

    # -- adjoint render ----------------------------------------------------------------------------
    def render_adjoint(self, grad_out) -> tuple:
        """Gradients of the frame render() would produce now, weighted by grad_out ([local_rows, res_x, 2]: the weights
        of tau and of I per pixel): (grad_alpha, grad_q), float64 [n_cells] each in the order of upload_grid.
        Synchronous; retries by itself.  fp64 atomics, not bit-reproducible - unless set_option("adjoint_exact", 1): then
        the exact sums, the same bits every run and for any split of the rows (as for the _device and batch forms)."""
        g = self._image(grad_out, "grad_out")
        ga, gq = np.zeros(self.n_cells), np.zeros(self.n_cells)
        self._check(self.lib.c5_render_adjoint(self.handle, _fp(g), _dp(ga), _dp(gq)))
        return ga, gq

    def render_adjoint_device(self, grad_out, grad_alpha, grad_q):
        """Asynchronous form on the context's stream, into device memory: torch tensors on this context's GPU (grad_out
        float32 [local_rows, res_x, 2] contiguous, grad_alpha / grad_q float64 [n_cells] contiguous) or raw device
        pointers.  The status comes with the next synchronize() (C5_RETRY: run it again)."""
        self._check(self.lib.c5_render_adjoint_device(self.handle, self._image_dev(grad_out), self._cells_dev(grad_alpha),
                                                      self._cells_dev(grad_q)))

    # -- exact adjoint sums ------------------------------------------------------------------------
    # (set_option("adjoint_exact", 1) makes render_adjoint* return them finished; these are the two intermediate results,
    # for callers who split an image: sharding.combine_exact, then exact_sums_finish)
    def _exponents(self, e, name: str) -> np.ndarray:
        e = np.asarray(e)
        if e.dtype != np.int32 or e.shape != (self.n_cells,) or not e.flags.c_contiguous:
            raise ValueError(f"{name} must be a contiguous int32 array of one exponent per cell ({self.n_cells}), "
                             f"not {e.dtype} {list(e.shape)}")
        return e

    def render_adjoint_exact_bounds(self, grad_out) -> tuple:
        """The exponents of the exact adjoint sums over the context's rows for the upstream image grad_out ([local_rows,
        res_x, 2]): (exp_alpha, exp_q), int32 [n_cells] each in the order of upload_grid (INT32_MIN: no contribution,
        INT32_MAX: one that is not finite).  Parts of an image combine by elementwise max.  Synchronous; retries by itself."""
        g = self._image(grad_out, "grad_out")
        ea, eq = np.zeros(self.n_cells, np.int32), np.zeros(self.n_cells, np.int32)
        self._check(self.lib.c5_render_adjoint_exact_bounds(self.handle, _fp(g), ea.ctypes.data_as(_ip_t), eq.ctypes.data_as(_ip_t)))
        return ea, eq

    def render_adjoint_exact_sums(self, grad_out, exp_alpha, exp_q) -> tuple:
        """The words of the exact adjoint sums over the context's rows against the given exponents (int32 [n_cells] each:
        those of render_adjoint_exact_bounds, combined over every part of the image): (sums_alpha, sums_q), int64
        [n_cells, 2] each.  Parts of an image combine by elementwise integer add.  C5_ERR_INVALID if a contribution lies
        beyond its cell's exponent.  Synchronous; retries by itself."""
        g = self._image(grad_out, "grad_out")
        ea, eq = self._exponents(exp_alpha, "exp_alpha"), self._exponents(exp_q, "exp_q")
        sa, sq = np.zeros((self.n_cells, 2), np.int64), np.zeros((self.n_cells, 2), np.int64)
        self._check(self.lib.c5_render_adjoint_exact_sums(self.handle, _fp(g), ea.ctypes.data_as(_ip_t), eq.ctypes.data_as(_ip_t),
                                                          sa.ctypes.data_as(_lp_t), sq.ctypes.data_as(_lp_t)))
        return sa, sq

    def render_adjoint_exact_bounds_device(self, grad_out, exp_alpha, exp_q):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (grad_out float32 [local_rows,
        res_x, 2], exp_alpha / exp_q int32 [n_cells], contiguous) or raw device pointers.  The status comes with the next
        synchronize()."""
        import torch
        n = (self.n_cells,)
        self._check(self.lib.c5_render_adjoint_exact_bounds_device(self.handle, self._image_dev(grad_out), _device_ptr(exp_alpha, torch.int32, n),
                                                                   _device_ptr(exp_q, torch.int32, n)))

    def render_adjoint_exact_sums_device(self, grad_out, exp_alpha, exp_q, sums_alpha, sums_q):
        """Asynchronous form on the context's stream: as render_adjoint_exact_bounds_device, and sums_alpha / sums_q int64
        [n_cells, 2].  The status (C5_ERR_INVALID for exponents that are too small included) comes with the next
        synchronize()."""
        import torch
        n, n2 = (self.n_cells,), (self.n_cells, 2)
        self._check(self.lib.c5_render_adjoint_exact_sums_device(
            self.handle, self._image_dev(grad_out), _device_ptr(exp_alpha, torch.int32, n), _device_ptr(exp_q, torch.int32, n),
            _device_ptr(sums_alpha, torch.int64, n2), _device_ptr(sums_q, torch.int64, n2)))

    # -- exact sums of every operator of a fit (set_option("exact_sums", 1) makes render_adjoint*, render_gn_diagonal*,
    # render_gn_product* and render_hvp* return them finished; these are the two intermediate results of one kind of sum -
    # C5_EXACT_ADJOINT, C5_EXACT_GN_DIAGONAL or C5_EXACT_HVP - for callers who split an image: fit.RowShards)
    def _exact_inputs(self, what, image, d_alpha, d_q) -> tuple:
        g = None if image is None else self._image(image, "image")
        return g, self._direction(d_alpha), self._direction(d_q)

    def render_exact_bounds(self, what: int, image=None, d_alpha=None, d_q=None) -> tuple:
        """The exponents of one kind of exact sum over the context's rows: (exp_alpha, exp_q), int32 [n_cells] each in the
        order of upload_grid (INT32_MIN: no contribution, INT32_MAX: one that is not finite).  image [local_rows, res_x, 2]:
        the upstream image (C5_EXACT_ADJOINT, C5_EXACT_HVP: required) or the weights (C5_EXACT_GN_DIAGONAL; None: ones);
        d_alpha / d_q [n_cells]: the direction, for C5_EXACT_HVP alone (either may be None, not both).  Parts of an image
        combine by elementwise max.  Synchronous; retries by itself."""
        g, da, dq = self._exact_inputs(what, image, d_alpha, d_q)
        ea, eq = np.zeros(self.n_cells, np.int32), np.zeros(self.n_cells, np.int32)
        self._check(self.lib.c5_render_exact_bounds(self.handle, what, _dp(da), _dp(dq), _fp(g), ea.ctypes.data_as(_ip_t),
                                                    eq.ctypes.data_as(_ip_t)))
        return ea, eq

    def render_exact_sums(self, what: int, exp_alpha, exp_q, image=None, d_alpha=None, d_q=None) -> tuple:
        """The words of one kind of exact sum over the context's rows against the given exponents (int32 [n_cells] each:
        those of render_exact_bounds, combined over every part of the image): (sums_alpha, sums_q), int64 [n_cells, 2]
        each.  Parts of an image combine by elementwise integer add (sharding.combine_exact), and exact_sums_finish then
        gives the bits of the single call under set_option("exact_sums", 1) over the whole image.  C5_ERR_INVALID if a
        contribution lies beyond its cell's exponent.  Synchronous; retries by itself."""
        g, da, dq = self._exact_inputs(what, image, d_alpha, d_q)
        ea, eq = self._exponents(exp_alpha, "exp_alpha"), self._exponents(exp_q, "exp_q")
        sa, sq = np.zeros((self.n_cells, 2), np.int64), np.zeros((self.n_cells, 2), np.int64)
        self._check(self.lib.c5_render_exact_sums(self.handle, what, _dp(da), _dp(dq), _fp(g), ea.ctypes.data_as(_ip_t),
                                                  eq.ctypes.data_as(_ip_t), sa.ctypes.data_as(_lp_t), sq.ctypes.data_as(_lp_t)))
        return sa, sq

    def render_exact_bounds_device(self, what: int, exp_alpha, exp_q, image=None, d_alpha=None, d_q=None):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (image float32 [local_rows, res_x,
        2], d_alpha / d_q float64 [n_cells], exp_alpha / exp_q int32 [n_cells], contiguous; None where render_exact_bounds
        allows it) or raw device pointers.  The status comes with the next synchronize()."""
        import torch
        n = (self.n_cells,)
        self._check(self.lib.c5_render_exact_bounds_device(self.handle, what, self._cells_dev(d_alpha), self._cells_dev(d_q),
                                                           self._image_dev(image), _device_ptr(exp_alpha, torch.int32, n),
                                                           _device_ptr(exp_q, torch.int32, n)))

    def render_exact_sums_device(self, what: int, exp_alpha, exp_q, sums_alpha, sums_q, image=None, d_alpha=None, d_q=None):
        """Asynchronous form on the context's stream: as render_exact_bounds_device, and sums_alpha / sums_q int64
        [n_cells, 2].  The status (C5_ERR_INVALID for exponents that are too small included) comes with the next
        synchronize()."""
        import torch
        n, n2 = (self.n_cells,), (self.n_cells, 2)
        self._check(self.lib.c5_render_exact_sums_device(
            self.handle, what, self._cells_dev(d_alpha), self._cells_dev(d_q), self._image_dev(image),
            _device_ptr(exp_alpha, torch.int32, n), _device_ptr(exp_q, torch.int32, n), _device_ptr(sums_alpha, torch.int64, n2),
            _device_ptr(sums_q, torch.int64, n2)))

    # -- vertex adjoint render ---------------------------------------------------------------------
    def render_vertex_adjoint(self, grad_out) -> np.ndarray:
        """The gradient of the frame render() would produce now with respect to the grid's points, weighted by grad_out
        ([local_rows, res_x, 2]: the weights of tau and of I per pixel): float64 [n_pts, 3] in the order and the coordinates
        of upload_grid.  A point welded to another at upload gets 0, its representative the group's sum.  Synchronous;
        retries by itself.  Not bit-reproducible from run to run (fp64 atomics), like render_adjoint - unless
        set_option("vertex_exact", 1): then the exact vertex adjoint sums, the same bits every run, under either cell order
        and for any split of the rows (as for the _device and batch forms)."""
        g = self._image(grad_out, "grad_out")
        out = np.zeros((self.n_pts, 3))
        self._check(self.lib.c5_render_vertex_adjoint(self.handle, _fp(g), _dp(out)))
        return out

    def render_vertex_adjoint_device(self, grad_out, grad_xyz):
        """Asynchronous form on the context's stream, in device memory: torch tensors on this context's GPU (grad_out
        float32 [local_rows, res_x, 2], grad_xyz float64 [n_pts, 3]; contiguous) or raw device pointers.  The status comes
        with the next synchronize() (C5_RETRY: run it again)."""
        import torch
        self._check(self.lib.c5_render_vertex_adjoint_device(self.handle, self._image_dev(grad_out),
                                                             _device_ptr(grad_xyz, torch.float64, (self.n_pts, 3))))

    def render_vertex_adjoint_batch(self, grad_out) -> np.ndarray:
        """render_vertex_adjoint for K upstream images at once (grad_out [K, local_rows, res_x, 2], or one image
        [local_rows, res_x, 2]): float64 [K, n_pts, 3], every slice render_vertex_adjoint's for that image alone up to the
        order of the fp64 additions.  One walk per ray for up to "batch_width" images.  Synchronous; retries by itself."""
        g = np.ascontiguousarray(grad_out, dtype=np.float32)
        shape = (self.local_rows, self.res_x, 2)
        if g.ndim not in (3, 4) or g.shape[-3:] != shape or g.shape[0] == 0:
            raise ValueError(f"grad_out must be [{shape[0]}, {shape[1]}, 2] or [K, {shape[0]}, {shape[1]}, 2], not {list(g.shape)}")
        k = 1 if g.ndim == 3 else g.shape[0]
        out = np.zeros((k, self.n_pts, 3))
        self._check(self.lib.c5_render_vertex_adjoint_batch(self.handle, k, _fp(g), _dp(out)))
        return out

    def render_vertex_adjoint_batch_device(self, grad_out, grad_xyz, n: int | None = None):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (grad_out float32 [K, local_rows,
        res_x, 2], grad_xyz float64 [K, n_pts, 3], contiguous) or raw device pointers (then give n = K).  The status comes
        with the next synchronize() (C5_RETRY: run it again)."""
        import torch
        k = n if n is not None else (grad_xyz.shape[0] if hasattr(grad_xyz, "shape") and len(grad_xyz.shape) == 3 else -1)
        if k < 1:
            raise ValueError("grad_xyz must be [K, n_pts, 3] with K >= 1 (or give n = K with raw device pointers)")
        ptrs = self._image_dev(grad_out, k), _device_ptr(grad_xyz, torch.float64, (k, self.n_pts, 3))
        self._check(self.lib.c5_render_vertex_adjoint_batch_device(self.handle, k, *ptrs))

    # -- exact vertex adjoint sums -----------------------------------------------------------------
    # (set_option("vertex_exact", 1) makes render_vertex_adjoint* return them finished; these are the intermediate results,
    # for callers who split an image: elementwise max of the exponents, elementwise add of the words - sharding.
    # combine_vertex_exact - then vertex_exact_finish on any one of the contexts: fit.RowShards.shape_operators)
    def _slot_exponents(self, e) -> np.ndarray:
        e = np.asarray(e)
        if e.dtype != np.int32 or e.shape != (self.n_cells, 12) or not e.flags.c_contiguous:
            raise ValueError(f"exps must be a contiguous int32 array [{self.n_cells}, 12] (one exponent per cell and slot), "
                             f"not {e.dtype} {list(e.shape)}")
        return e

    def _slot_words(self, s) -> np.ndarray:
        s = np.asarray(s)
        if s.dtype != np.int64 or s.shape != (self.n_cells, 12, 2) or not s.flags.c_contiguous:
            raise ValueError(f"sums must be a contiguous int64 array [{self.n_cells}, 12, 2] (two words per cell and slot), "
                             f"not {s.dtype} {list(s.shape)}")
        return s

    def render_vertex_exact_bounds(self, grad_out) -> np.ndarray:
        """The exponents of the exact vertex adjoint sums over the context's rows for the upstream image grad_out
        ([local_rows, res_x, 2]): int32 [n_cells, 12] in the cell order of upload_grid, a cell's slots [4 faces][3 vertices
        of the face] (INT32_MIN: no contribution, INT32_MAX: one that is not finite).  Parts of an image combine by
        elementwise max.  Synchronous; retries by itself."""
        g = self._image(grad_out, "grad_out")
        exps = np.zeros((self.n_cells, 12), np.int32)
        self._check(self.lib.c5_render_vertex_exact_bounds(self.handle, _fp(g), exps.ctypes.data_as(_ip_t)))
        return exps

    def render_vertex_exact_sums(self, grad_out, exps) -> np.ndarray:
        """The words of the exact vertex adjoint sums over the context's rows against the given exponents (int32 [n_cells,
        12]: those of render_vertex_exact_bounds, combined over every part of the image): int64 [n_cells, 12, 2].  Parts
        of an image combine by elementwise integer add.  C5_ERR_INVALID if a contribution lies beyond its slot's
        exponent.  Synchronous; retries by itself."""
        g = self._image(grad_out, "grad_out")
        e = self._slot_exponents(exps)
        sums = np.zeros((self.n_cells, 12, 2), np.int64)
        self._check(self.lib.c5_render_vertex_exact_sums(self.handle, _fp(g), e.ctypes.data_as(_ip_t), sums.ctypes.data_as(_lp_t)))
        return sums

    def vertex_exact_finish(self, exps, sums) -> np.ndarray:
        """The gradient the exponents and words stand for (int32 [n_cells, 12], int64 [n_cells, 12, 2]: combined over every
        part of the image): float64 [n_pts, 3], bit for bit render_vertex_adjoint's under set_option("vertex_exact", 1)
        over the whole image.  Uses the context's grid, points and view, none of its rows.  Synchronous; retries by itself."""
        e, s = self._slot_exponents(exps), self._slot_words(sums)
        out = np.zeros((self.n_pts, 3))
        self._check(self.lib.c5_vertex_exact_finish(self.handle, e.ctypes.data_as(_ip_t), s.ctypes.data_as(_lp_t), _dp(out)))
        return out

    def render_vertex_exact_bounds_device(self, grad_out, exps):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (grad_out float32 [local_rows,
        res_x, 2], exps int32 [n_cells, 12], contiguous) or raw device pointers.  The status comes with the next
        synchronize()."""
        import torch
        ptrs = self._image_dev(grad_out), _device_ptr(exps, torch.int32, (self.n_cells, 12))
        self._check(self.lib.c5_render_vertex_exact_bounds_device(self.handle, *ptrs))

    def render_vertex_exact_sums_device(self, grad_out, exps, sums):
        """Asynchronous form on the context's stream: as render_vertex_exact_bounds_device, and sums int64 [n_cells, 12, 2].
        The status (C5_ERR_INVALID for exponents that are too small included) comes with the next synchronize()."""
        import torch
        ptrs = (self._image_dev(grad_out), _device_ptr(exps, torch.int32, (self.n_cells, 12)),
                _device_ptr(sums, torch.int64, (self.n_cells, 12, 2)))
        self._check(self.lib.c5_render_vertex_exact_sums_device(self.handle, *ptrs))

    def vertex_exact_finish_device(self, exps, sums, grad_xyz):
        """Asynchronous form on the context's stream: exps int32 [n_cells, 12], sums int64 [n_cells, 12, 2], grad_xyz float64
        [n_pts, 3]; torch tensors on this context's GPU, contiguous, or raw device pointers.  The status comes with the next
        synchronize()."""
        import torch
        ptrs = (_device_ptr(exps, torch.int32, (self.n_cells, 12)), _device_ptr(sums, torch.int64, (self.n_cells, 12, 2)),
                _device_ptr(grad_xyz, torch.float64, (self.n_pts, 3)))
        self._check(self.lib.c5_vertex_exact_finish_device(self.handle, *ptrs))

    # -- vertex tangent render ---------------------------------------------------------------------
    def render_vertex_tangent(self, d_xyz) -> np.ndarray:
        """The change of the frame render() would produce now when every grid point moves with the velocity d_xyz (float64
        [n_pts, 3] in the order and the coordinates of upload_grid): float32 [local_rows, res_x, 2] (tau_dot, I_dot); K
        fields [K, n_pts, 3] give [K, local_rows, res_x, 2], every slice bit for bit the call for that field alone.  The
        rows of points welded to another at upload are not read (the group moves with its representative).  The operator
        render_vertex_adjoint is the transpose of.  Synchronous; retries by itself.  Bit-reproducible."""
        d = np.ascontiguousarray(d_xyz, dtype=np.float64)
        if d.ndim not in (2, 3) or d.shape[-2:] != (self.n_pts, 3) or d.shape[0] == 0:
            raise ValueError(f"d_xyz must be [{self.n_pts}, 3] or [K, {self.n_pts}, 3], not {list(d.shape)}")
        k = 1 if d.ndim == 2 else d.shape[0]
        out = self._images(k)
        self._check(self.lib.c5_render_vertex_tangent(self.handle, k, _dp(d), _fp(out)))
        return out[0] if d.ndim == 2 else out

    def render_vertex_tangent_device(self, d_xyz, out, n: int | None = None):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (d_xyz float64 [K, n_pts, 3], out
        float32 [K, local_rows, res_x, 2], contiguous) or raw device pointers (then give n = K).  The status comes with the
        next synchronize() (C5_RETRY: run it again)."""
        import torch
        k = n if n is not None else (out.shape[0] if hasattr(out, "shape") and len(out.shape) == 4 else -1)
        if k < 0:
            raise ValueError("out must be [K, local_rows, res_x, 2] (or give n = K with raw device pointers)")
        ptrs = _device_ptr(d_xyz, torch.float64, (k, self.n_pts, 3)), self._image_dev(out, k)
        self._check(self.lib.c5_render_vertex_tangent_device(self.handle, k, *ptrs))

    # -- vertex Gauss-Newton product -----------------------------------------------------------------
    def render_vertex_gn_product(self, d_xyz, weight=None, want_jv: bool = False):
        """H v = J^T W J v for per-point fields v (d_xyz float64 [n_pts, 3] or [K, n_pts, 3], render_vertex_tangent's
        conventions), J the Jacobian of the frame render() would produce now with respect to the grid's points, W =
        diag(weight) ([local_rows, res_x, 2] float32 >= 0; None: ones): float64 [n_pts, 3] or [K, n_pts, 3] with
        render_vertex_adjoint's conventions (0 on points welded to another); with want_jv the pair (h, J v), J v float32
        [local_rows, res_x, 2] or [K, ...], bit for bit render_vertex_tangent's.  One call for
        render_vertex_adjoint_batch(weight * render_vertex_tangent(v)): the same up to the order of the fp64 additions,
        bit for bit under set_option("vertex_exact", 1).  Synchronous; retries by itself."""
        d = np.ascontiguousarray(d_xyz, dtype=np.float64)
        if d.ndim not in (2, 3) or d.shape[-2:] != (self.n_pts, 3) or d.shape[0] == 0:
            raise ValueError(f"d_xyz must be [{self.n_pts}, 3] or [K, {self.n_pts}, 3], not {list(d.shape)}")
        w = None if weight is None else self._image(weight, "weight")
        k = 1 if d.ndim == 2 else d.shape[0]
        h = np.zeros((k, self.n_pts, 3))
        jv = self._images(k) if want_jv else None
        self._check(self.lib.c5_render_vertex_gn_product(self.handle, k, _dp(d), _fp(w), _dp(h), _fp(jv)))
        if d.ndim == 2:
            h, jv = h[0], (jv[0] if want_jv else None)
        return (h, jv) if want_jv else h

    def render_vertex_gn_product_device(self, d_xyz, weight, h_xyz, jv_out=None, n: int | None = None):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (d_xyz and h_xyz float64 [K, n_pts,
        3], weight float32 [local_rows, res_x, 2] or None, jv_out float32 [K, local_rows, res_x, 2] or None; contiguous) or
        raw device pointers (then give n = K).  The status comes with the next synchronize() (C5_RETRY: run it again)."""
        import torch
        k = n if n is not None else (h_xyz.shape[0] if hasattr(h_xyz, "shape") and len(h_xyz.shape) == 3 else -1)
        if k < 1:
            raise ValueError("h_xyz must be [K, n_pts, 3] with K >= 1 (or give n = K with raw device pointers)")
        if d_xyz is None or h_xyz is None:
            raise ValueError("give d_xyz and h_xyz")
        shape = (k, self.n_pts, 3)
        ptrs = (_device_ptr(d_xyz, torch.float64, shape), self._image_dev(weight), _device_ptr(h_xyz, torch.float64, shape),
                self._image_dev(jv_out, k))
        self._check(self.lib.c5_render_vertex_gn_product_device(self.handle, k, *ptrs))

    # -- ray matrix --------------------------------------------------------------------------------
    def ray_matrix_rows(self) -> np.ndarray:
        """row_ptr of the ray matrix of the frame render() would produce now: int64 [local_rows * res_x + 1], the exclusive
        prefix sums of the pixels' segment counts (row_ptr[-1]: all of them).  Synchronous; retries by itself."""
        row_ptr = np.zeros(self.local_rows * self.res_x + 1, dtype=np.int64)
        nnz = C.c_int64()  # (row_ptr[-1] says the same)
        self._check(self.lib.c5_ray_matrix_rows(self.handle, row_ptr.ctypes.data_as(_lp_t), C.byref(nnz)))
        return row_ptr

    def ray_matrix_rows_device(self, row_ptr) -> int:
        """The same into device memory: a contiguous int64 [local_rows * res_x + 1] torch tensor on this context's GPU or a
        raw device pointer.  Waits for the stream and returns the number of segments; runs the call again on C5_RETRY."""
        import torch
        nnz = C.c_int64()
        ptr = _device_ptr(row_ptr, torch.int64, (self.local_rows * self.res_x + 1,))
        for _ in range(3):
            if self._check(self.lib.c5_ray_matrix_rows_device(self.handle, ptr, C.byref(nnz)), allow=(C5_RETRY,)) == C5_OK:
                return nnz.value
        raise C5Error(C5_RETRY, "ray_matrix_rows_device: the entry buffer kept overflowing")

    def _fill_rows(self, row_ptr, capacity) -> tuple:
        """What the host forms of the three fills take first: (row_ptr checked and contiguous, n = the capacity asked for or
        row_ptr's total, the length to allocate: an empty array has no pointer to hand over)."""
        if not isinstance(row_ptr, np.ndarray) or row_ptr.dtype != np.int64:
            raise ValueError("row_ptr must be the int64 array ray_matrix_rows returned")
        if row_ptr.shape != (self.local_rows * self.res_x + 1,):
            raise ValueError(f"row_ptr must be [{self.local_rows * self.res_x + 1}], not {list(row_ptr.shape)}")
        n = int(row_ptr[-1]) if capacity is None else int(capacity)
        if n < 0:
            raise ValueError(f"capacity must not be negative ({n})")
        return np.ascontiguousarray(row_ptr), n, max(n, 1)

    @staticmethod
    def _fill_capacity(capacity, *arrays):
        """What the device forms of the three fills take for the capacity: the one given, else the length of the first array
        that is there - which a raw device pointer does not say."""
        if capacity is None:
            first = next((t for t in arrays if t is not None), None)
            if first is None or isinstance(first, int):
                raise ValueError("give capacity with raw device pointers")
            capacity = first.shape[0]
        return capacity

    def ray_matrix_fill(self, row_ptr, with_depth: bool = False, capacity: int | None = None) -> tuple:
        """The ray matrix's arrays for ray_matrix_rows' row_ptr of this frame: (col int32, dz float64[, z_exit float64]),
        [capacity] each (default: row_ptr[-1]).  col: cells in the order of upload_grid; within a row deepest segment first;
        z_exit: the segment's far end in view space.  Raises C5_ERR_STATE if the frame changed since ray_matrix_rows.
        Synchronous; retries by itself.  Bit-reproducible."""
        row_ptr, n, room = self._fill_rows(row_ptr, capacity)
        col = np.zeros(room, dtype=np.int32)
        dz = np.zeros(room)
        z_exit = np.zeros(room) if with_depth else None
        self._check(self.lib.c5_ray_matrix_fill(self.handle, row_ptr.ctypes.data_as(_lp_t), n, col.ctypes.data_as(_ip_t), _dp(dz),
                                                _dp(z_exit)))
        return (col[:n], dz[:n], z_exit[:n]) if with_depth else (col[:n], dz[:n])

    def ray_matrix_fill_device(self, row_ptr, col, dz, z_exit=None, capacity: int | None = None):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (row_ptr int64 [local_rows * res_x
        + 1], col int32 / dz float64 / z_exit float64 or None, [capacity] each, contiguous) or raw device pointers (then
        give capacity).  Nothing beyond capacity is written; a frame that changed since ray_matrix_rows, or a capacity
        below row_ptr's total, makes the next synchronize() raise C5_ERR_STATE."""
        import torch
        capacity = self._fill_capacity(capacity, col)
        shape = (capacity,)
        ptrs = (_device_ptr(row_ptr, torch.int64, (self.local_rows * self.res_x + 1,)), _device_ptr(col, torch.int32, shape),
                _device_ptr(dz, torch.float64, shape), _device_ptr(z_exit, torch.float64, shape))
        self._check(self.lib.c5_ray_matrix_fill_device(self.handle, ptrs[0], capacity, *ptrs[1:]))

    def ray_matrix(self, with_depth: bool = False) -> tuple:
        """The ray matrix A of the frame render() would produce now as CSR arrays (row_ptr, col, dz[, z_exit]): rows are the
        local pixels lrow * res_x + col, columns the cells in the order of upload_grid, A[pixel, cell] = the chord of the
        pixel's ray through the cell.  A @ alpha is channel 0 of render() in fp64."""
        row_ptr = self.ray_matrix_rows()
        return (row_ptr,) + self.ray_matrix_fill(row_ptr, with_depth)

    # -- ray Jacobian ------------------------------------------------------------------------------
    def ray_jacobian_fill(self, row_ptr, capacity: int | None = None, with_structure: bool = True) -> tuple:
        """The ray Jacobian's arrays for ray_matrix_rows' row_ptr of this frame: (col int32, dz, dI_dalpha, dI_dq), float64,
        [capacity] each (default: row_ptr[-1]), or (dI_dalpha, dI_dq) alone without the structure.  col and dz are
        ray_matrix_fill's, bit for bit; dI_dalpha / dI_dq: the derivative of the pixel's I with respect to the crossed
        cell's alpha / Q at the scalars and the alpha limit the context holds now (0 where the cell is inactive; dI_dalpha
        0 where its alpha is clamped).  Raises C5_ERR_STATE if the frame changed since ray_matrix_rows.  Synchronous;
        retries by itself.  Bit-reproducible."""
        row_ptr, n, room = self._fill_rows(row_ptr, capacity)
        col = np.zeros(room, dtype=np.int32) if with_structure else None
        dz = np.zeros(room) if with_structure else None
        da, dq = np.zeros(room), np.zeros(room)
        self._check(self.lib.c5_ray_jacobian_fill(self.handle, row_ptr.ctypes.data_as(_lp_t), n,
                                                  None if col is None else col.ctypes.data_as(_ip_t), _dp(dz), _dp(da), _dp(dq)))
        return (col[:n], dz[:n], da[:n], dq[:n]) if with_structure else (da[:n], dq[:n])

    def ray_jacobian_fill_device(self, row_ptr, col, dz, dI_dalpha, dI_dq, capacity: int | None = None):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (row_ptr int64 [local_rows * res_x
        + 1]; col int32, dz / dI_dalpha / dI_dq float64, [capacity] each, contiguous) or raw device pointers (then give
        capacity).  col and dz may be None, and one of dI_dalpha and dI_dq.  Nothing beyond capacity is written; a frame
        that changed since ray_matrix_rows, or a capacity below row_ptr's total, makes the next synchronize() raise
        C5_ERR_STATE."""
        import torch
        if dI_dalpha is None and dI_dq is None:
            raise ValueError("give dI_dalpha or dI_dq")
        if row_ptr is None:
            raise ValueError("give row_ptr")
        capacity = self._fill_capacity(capacity, dI_dalpha, dI_dq)
        if capacity < 0:
            raise ValueError(f"capacity must not be negative ({capacity})")
        shape = (capacity,)
        ptrs = (_device_ptr(row_ptr, torch.int64, (self.local_rows * self.res_x + 1,)), _device_ptr(col, torch.int32, shape),
                _device_ptr(dz, torch.float64, shape), _device_ptr(dI_dalpha, torch.float64, shape),
                _device_ptr(dI_dq, torch.float64, shape))
        self._check(self.lib.c5_ray_jacobian_fill_device(self.handle, ptrs[0], capacity, *ptrs[1:]))

    def ray_jacobian(self) -> tuple:
        """The Jacobian of the frame render() would produce now with respect to the cells' scalars, per segment, as CSR
        arrays (row_ptr, col, dz, dI_dalpha, dI_dq) over the ray matrix's structure: d tau[pixel] / d alpha[cell] = dz,
        d I[pixel] / d alpha[cell] = dI_dalpha, d I[pixel] / d Q[cell] = dI_dq."""
        row_ptr = self.ray_matrix_rows()
        return (row_ptr,) + self.ray_jacobian_fill(row_ptr)

    # -- ray shape Jacobian ------------------------------------------------------------------------
    def ray_shape_jacobian_fill(self, row_ptr, capacity: int | None = None) -> tuple:
        """The shape Jacobian's per-segment arrays for ray_matrix_rows' row_ptr of this frame: (dI_ddz float64 [capacity],
        faces uint8 [capacity], bary float64 [capacity, 2, 3]) (default capacity: row_ptr[-1]), over ray_matrix_fill's
        structure.  dI_ddz: d I[pixel] / d (the chord of the crossed cell), 0 where the cell is inactive; faces: exit face |
        entry face << 2 | 16 (the exit face contributes) | 32 (the entry face does); bary: the pixel's barycentric
        coordinates in the exit and the entry face, zeros where the face does not contribute.  Raises C5_ERR_STATE if the
        frame changed since ray_matrix_rows.  Synchronous; retries by itself.  Bit-reproducible."""
        row_ptr, n, room = self._fill_rows(row_ptr, capacity)
        dI = np.zeros(room)
        faces = np.zeros(room, dtype=np.uint8)
        bary = np.zeros((room, 2, 3))
        self._check(self.lib.c5_ray_shape_jacobian_fill(self.handle, row_ptr.ctypes.data_as(_lp_t), n, _dp(dI),
                                                        faces.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(bary)))
        return dI[:n], faces[:n], bary[:n]

    def ray_shape_jacobian_device(self, row_ptr, dI_ddz, faces, bary, capacity: int | None = None):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (row_ptr int64 [local_rows * res_x
        + 1]; dI_ddz float64 [capacity], faces uint8 [capacity], bary float64 [capacity, 2, 3], contiguous) or raw device
        pointers (then give capacity).  Any one of the three may be None, not all.  Nothing beyond capacity is written; a
        frame that changed since ray_matrix_rows, or a capacity below row_ptr's total, makes the next synchronize() raise
        C5_ERR_STATE."""
        import torch
        if dI_ddz is None and faces is None and bary is None:
            raise ValueError("give dI_ddz, faces or bary")
        if row_ptr is None:
            raise ValueError("give row_ptr")
        capacity = self._fill_capacity(capacity, dI_ddz, faces, bary)
        if capacity < 0:
            raise ValueError(f"capacity must not be negative ({capacity})")
        ptrs = (_device_ptr(row_ptr, torch.int64, (self.local_rows * self.res_x + 1,)), _device_ptr(dI_ddz, torch.float64, (capacity,)),
                _device_ptr(faces, torch.uint8, (capacity,)), _device_ptr(bary, torch.float64, (capacity, 2, 3)))
        self._check(self.lib.c5_ray_shape_jacobian_fill_device(self.handle, ptrs[0], capacity, *ptrs[1:]))

    def face_gradients(self) -> tuple:
        """Per cell (the order of upload_grid) and face, for the grid, points and view the context holds: (face_points int32
        [n_cells, 4, 3]: the points of the face's three vertices, representatives where points were welded; dw_dxyz float64
        [n_cells, 4, 3]: the change of the face's depth per unit of barycentric weight and unit motion of a vertex, zeros
        for a face edge-on to the rays).  Synchronous; retries by itself."""
        fp = np.zeros((max(self.n_cells, 1), 4, 3), dtype=np.int32)
        dw = np.zeros((max(self.n_cells, 1), 4, 3))
        self._check(self.lib.c5_face_gradients(self.handle, fp.ctypes.data_as(_ip_t), _dp(dw)))
        return fp[:self.n_cells], dw[:self.n_cells]

    def face_gradients_device(self, face_points, dw_dxyz):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (face_points int32, dw_dxyz float64,
        [n_cells, 4, 3] each, contiguous) or raw device pointers."""
        import torch
        if face_points is None or dw_dxyz is None:
            raise ValueError("give face_points and dw_dxyz")
        shape = (self.n_cells, 4, 3)
        self._check(self.lib.c5_face_gradients_device(self.handle, _device_ptr(face_points, torch.int32, shape),
                                                      _device_ptr(dw_dxyz, torch.float64, shape)))

    def ray_shape_jacobian(self) -> tuple:
        """The Jacobian of the frame render() would produce now with respect to the grid's points, per segment:
        (row_ptr, col, dz, dI_ddz, faces, bary, face_points, dw_dxyz) - ray_matrix's structure, ray_shape_jacobian_fill's
        arrays and face_gradients' (the formula: include/course5_hip.h, "ray shape Jacobian")."""
        row_ptr = self.ray_matrix_rows()
        return (row_ptr,) + self.ray_matrix_fill(row_ptr) + self.ray_shape_jacobian_fill(row_ptr) + self.face_gradients()

    # -- tangent render ----------------------------------------------------------------------------
    def render_tangent(self, d_alpha=None, d_q=None) -> np.ndarray:
        """The change of the frame render() would produce now for a change (d_alpha, d_q) of the cells' scalars ([n_cells]
        each in the order of upload_grid; None: zero): float32 [local_rows, res_x, 2] (tau_dot, I_dot).  Synchronous;
        retries by itself.  Bit-reproducible."""
        da, dq = self._direction(d_alpha), self._direction(d_q)
        out = np.zeros((self.local_rows, self.res_x, 2), dtype=np.float32)
        self._check(self.lib.c5_render_tangent(self.handle, _dp(da), _dp(dq), _fp(out)))
        return out

    def render_tangent_device(self, d_alpha, d_q, out):
        """Asynchronous form on the context's stream, in device memory: torch tensors on this context's GPU (d_alpha / d_q
        float64 [n_cells] contiguous or None for zero, out float32 [local_rows, res_x, 2] contiguous) or raw device
        pointers (0: zero).  The status comes with the next synchronize() (C5_RETRY: run it again)."""
        self._check(self.lib.c5_render_tangent_device(self.handle, self._cells_dev(d_alpha), self._cells_dev(d_q), self._image_dev(out)))

    # -- batched derivative renders ---------------------------------------------------------------
    def _batch_directions(self, d_alpha, d_q) -> tuple:
        def direction(d):
            if d is None:
                return None
            d = np.ascontiguousarray(d, dtype=np.float64)
            if d.ndim != 2 or d.shape[1] != self.n_cells:
                raise ValueError(f"directions must be [K, {self.n_cells}], not {list(d.shape)}")
            return d

        da, dq = direction(d_alpha), direction(d_q)
        ks = {d.shape[0] for d in (da, dq) if d is not None}
        if len(ks) != 1:
            raise ValueError("give d_alpha and / or d_q, with the same number of directions")
        return da, dq, ks.pop()

    def render_tangent_batch(self, d_alpha=None, d_q=None) -> np.ndarray:
        """render_tangent for K directions at once (d_alpha / d_q: [K, n_cells], either may be None: zero): float32
        [K, local_rows, res_x, 2], every slice bit for bit render_tangent's for that direction alone."""
        da, dq, k = self._batch_directions(d_alpha, d_q)
        out = self._images(k)
        self._check(self.lib.c5_render_tangent_batch(self.handle, k, _dp(da), _dp(dq), _fp(out)))
        return out

    def render_tangent_batch_device(self, d_alpha, d_q, out, n: int | None = None):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (d_alpha / d_q float64 [K,
        n_cells] contiguous or None, out float32 [K, local_rows, res_x, 2] contiguous) or raw device pointers (then give
        n = K).  The status comes with the next synchronize() (C5_RETRY: run it again)."""
        k = n if n is not None else out.shape[0]
        self._check(self.lib.c5_render_tangent_batch_device(self.handle, k, self._cells_dev(d_alpha, k), self._cells_dev(d_q, k),
                                                            self._image_dev(out, k)))

    def render_adjoint_batch(self, grad_out) -> tuple:
        """render_adjoint for K upstream images at once (grad_out [K, local_rows, res_x, 2]): (grad_alpha, grad_q), float64
        [K, n_cells] each; every slice render_adjoint's for that image to rounding.  Synchronous; retries by itself."""
        g = self._image(grad_out, "grad_out", batch=True)
        k = g.shape[0]
        ga, gq = np.zeros((k, self.n_cells)), np.zeros((k, self.n_cells))
        self._check(self.lib.c5_render_adjoint_batch(self.handle, k, _fp(g), _dp(ga), _dp(gq)))
        return ga, gq

    def render_adjoint_batch_device(self, grad_out, grad_alpha, grad_q, n: int | None = None):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (grad_out float32 [K, local_rows,
        res_x, 2], grad_alpha / grad_q float64 [K, n_cells], contiguous) or raw device pointers (then give n = K).  The
        status comes with the next synchronize() (C5_RETRY: run it again)."""
        k = n if n is not None else grad_out.shape[0]
        self._check(self.lib.c5_render_adjoint_batch_device(self.handle, k, self._image_dev(grad_out, k), self._cells_dev(grad_alpha, k),
                                                            self._cells_dev(grad_q, k)))

    # -- motion tangent render -----------------------------------------------------------------------
    @staticmethod
    def _motion_fields(fields) -> np.ndarray:
        f = np.ascontiguousarray(fields, dtype=np.float64)
        if f.ndim not in (1, 2) or f.shape[-1] != 12 or f.size == 0:
            raise ValueError(f"fields must be [12] or [K, 12] (A row-major, then b), not {list(f.shape)}")
        return f

    def render_motion_tangent(self, fields) -> np.ndarray:
        """The change of the frame render() would produce now when the grid moves in view space with the velocity field
        u(p) = A p + b (fields [K, 12]: A row-major then b; rotation_motion gives a view angle's): float32 [K, local_rows,
        res_x, 2] (tau_dot, I_dot); a single [12] field gives [local_rows, res_x, 2].  Synchronous; retries by itself.
        Bit-reproducible, and every slice is bit for bit the call for that field alone."""
        f = self._motion_fields(fields)
        k = f.size // 12
        out = self._images(k)
        self._check(self.lib.c5_render_motion_tangent(self.handle, k, _dp(f), _fp(out)))
        return out[0] if f.ndim == 1 else out

    def render_motion_tangent_device(self, fields, out):
        """Asynchronous form on the context's stream: fields as above (host memory: they travel as kernel arguments), out a
        float32 [K, local_rows, res_x, 2] contiguous torch tensor on this context's GPU or a raw device pointer.  The
        status comes with the next synchronize() (C5_RETRY: run it again)."""
        f = self._motion_fields(fields)
        k = f.size // 12
        self._check(self.lib.c5_render_motion_tangent_device(self.handle, k, _dp(f), self._image_dev(out, k)))

    def view_fields(self) -> np.ndarray:
        """[n_rots, 12]: the velocity field of every angle of the current view (rotation_motion)."""
        return np.array([rotation_motion(self.rots, i) for i in range(len(self.rots))]).reshape(-1, 12)

    def render_view_tangent(self) -> np.ndarray:
        """d image / d angle for every rotation of the current view (set_view): float32 [n_rots, local_rows, res_x, 2], per
        radian."""
        if len(self.rots) == 0:
            return self._images(0)
        return self.render_motion_tangent(self.view_fields())

    # -- Gauss-Newton renders -----------------------------------------------------------------------
    def render_gn_product(self, d_alpha=None, d_q=None, weight=None, want_jv: bool = False, fit=("alpha", "q")):
        """H v = J^T W J v for K directions (d_alpha / d_q: [K, n_cells], either may be None: zero), J the Jacobian of the
        frame render() would produce now, W = diag(weight) ([local_rows, res_x, 2] float32 >= 0; None: ones):
        (h_alpha, h_q), float64 [K, n_cells] each; with want_jv also J v, float32 [K, local_rows, res_x, 2], bit for bit
        render_tangent_batch's.  fit names the blocks wanted (the other comes back as None).  One call for
        render_adjoint_batch(weight * render_tangent_batch(v)); synchronous, retries by itself."""
        da, dq, k = self._batch_directions(d_alpha, d_q)
        w = None if weight is None else self._image(weight, "weight")
        fit = self._fit(fit)
        ha = np.zeros((k, self.n_cells)) if "alpha" in fit else None
        hq = np.zeros((k, self.n_cells)) if "q" in fit else None
        jv = self._images(k) if want_jv else None
        self._check(self.lib.c5_render_gn_product(self.handle, k, _dp(da), _dp(dq), _fp(w), _dp(ha), _dp(hq), _fp(jv)))
        return (ha, hq, jv) if want_jv else (ha, hq)

    def render_gn_product_device(self, d_alpha, d_q, weight, h_alpha, h_q, jv_out=None, n: int | None = None):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (d_alpha / d_q float64 [K,
        n_cells] or None, weight float32 [local_rows, res_x, 2] or None, h_alpha / h_q float64 [K, n_cells], one of them
        may be None, jv_out float32 [K, local_rows, res_x, 2] or None; contiguous) or raw device pointers (then give
        n = K).  The status comes with the next synchronize() (C5_RETRY: run it again)."""
        if n is None:
            shaped = [t for t in (h_alpha, h_q, d_alpha, d_q) if t is not None and not isinstance(t, int)]
            if not shaped:
                raise ValueError("give n with raw device pointers")
            n = shaped[0].shape[0]
        if d_alpha is None and d_q is None:
            raise ValueError("give d_alpha and / or d_q")
        if h_alpha is None and h_q is None:
            raise ValueError("give h_alpha and / or h_q")
        self._check(self.lib.c5_render_gn_product_device(
            self.handle, n, self._cells_dev(d_alpha, n), self._cells_dev(d_q, n), self._image_dev(weight),
            self._cells_dev(h_alpha, n), self._cells_dev(h_q, n), self._image_dev(jv_out, n)))

    def render_gn_diagonal(self, weight=None) -> tuple:
        """diag(J^T W J) as (diag_alpha, diag_q), float64 [n_cells] each in the order of upload_grid (weight: as
        render_gn_product).  Synchronous; retries by itself."""
        w = None if weight is None else self._image(weight, "weight")
        da, dq = np.zeros(self.n_cells), np.zeros(self.n_cells)
        self._check(self.lib.c5_render_gn_diagonal(self.handle, _fp(w), _dp(da), _dp(dq)))
        return da, dq

    def render_gn_diagonal_device(self, weight, diag_alpha, diag_q):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (weight float32 [local_rows,
        res_x, 2] or None, diag_alpha / diag_q float64 [n_cells]; contiguous) or raw device pointers.  The status comes
        with the next synchronize() (C5_RETRY: run it again)."""
        self._check(self.lib.c5_render_gn_diagonal_device(self.handle, self._image_dev(weight), self._cells_dev(diag_alpha),
                                                          self._cells_dev(diag_q)))

    # -- smoothness prior -----------------------------------------------------------------------------
    def _cells_host(self, a, name: str):
        """A per-cell float64 array of the caller's, or None."""
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (self.n_cells,):
            raise ValueError(f"{name} must be [n_cells] = [{self.n_cells}], not {list(a.shape)}")
        return a

    def _prior_out(self, prior):
        """The two output arrays of an operator of `prior` (None for a field whose lambda is 0)."""
        return (np.zeros(self.n_cells) if prior.lambda_alpha != 0.0 else None, np.zeros(self.n_cells) if prior.lambda_q != 0.0 else None)

    def prior_weights(self, weighting: int = C5_PRIOR_TPFA) -> tuple:
        """(w, n_interior_faces, n_degenerate): the prior's face weights, float64 [n_cells, 4] in the order of upload_grid
        and its face numbering (0 on a face without a neighbour), the number of interior faces, and of those whose TPFA
        weight was not finite and positive and is stored as 0.  Needs a grid and nothing else."""
        w = np.zeros((self.n_cells, 4))
        n_int, n_deg = C.c_int64(), C.c_int64()
        self._check(self.lib.c5_prior_weights(self.handle, int(weighting), _dp(w), C.byref(n_int), C.byref(n_deg)))
        return w, n_int.value, n_deg.value

    def prior_weights_device(self, weighting: int, w) -> tuple:
        """The weights into device memory (a torch tensor float64 [n_cells, 4] on this context's GPU, or a raw device
        pointer, or None) on the context's stream: (n_interior_faces, n_degenerate)."""
        import torch
        n_int, n_deg = C.c_int64(), C.c_int64()
        self._check(self.lib.c5_prior_weights_device(self.handle, int(weighting), _device_ptr(w, torch.float64, (self.n_cells, 4)),
                                                     C.byref(n_int), C.byref(n_deg)))
        return n_int.value, n_deg.value

    def prior_gradient(self, prior: Prior, alpha=None, q=None) -> tuple:
        """(value, grad_alpha, grad_q) of the smoothness prior at the fields alpha / q (float64 [n_cells] in the order of
        upload_grid; the context's own scalars play no part): value = float64 [2], (R(alpha), R(q)); a field whose lambda
        is 0 may be None and comes back as None.  Synchronous; bit-reproducible."""
        a, qq = self._cells_host(alpha, "alpha"), self._cells_host(q, "q")
        value = np.zeros(2)
        ga, gq = self._prior_out(prior)
        self._check(self.lib.c5_prior_gradient(self.handle, C.byref(prior), _dp(a), _dp(qq), _dp(value), _dp(ga), _dp(gq)))
        return value, ga, gq

    def prior_gradient_device(self, prior: Prior, alpha, q, value, grad_alpha, grad_q):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (float64 [n_cells]; value
        float64 [2] or None) or raw device pointers."""
        import torch
        self._check(self.lib.c5_prior_gradient_device(self.handle, C.byref(prior), self._cells_dev(alpha), self._cells_dev(q),
                                                      _device_ptr(value, torch.float64, (2,)), self._cells_dev(grad_alpha),
                                                      self._cells_dev(grad_q)))

    def prior_product(self, prior: Prior, alpha=None, q=None, v_alpha=None, v_q=None) -> tuple:
        """(h_alpha, h_q) = Hess R(alpha, q) (v_alpha, v_q); the point may be None where the penalty is quadratic."""
        a, qq = self._cells_host(alpha, "alpha"), self._cells_host(q, "q")
        va, vq = self._cells_host(v_alpha, "v_alpha"), self._cells_host(v_q, "v_q")
        ha, hq = self._prior_out(prior)
        self._check(self.lib.c5_prior_product(self.handle, C.byref(prior), _dp(a), _dp(qq), _dp(va), _dp(vq), _dp(ha), _dp(hq)))
        return ha, hq

    def prior_product_device(self, prior: Prior, alpha, q, v_alpha, v_q, h_alpha, h_q):
        """Asynchronous form on the context's stream (tensors or raw device pointers as prior_gradient_device)."""
        self._check(self.lib.c5_prior_product_device(self.handle, C.byref(prior), self._cells_dev(alpha), self._cells_dev(q),
                                                     self._cells_dev(v_alpha), self._cells_dev(v_q), self._cells_dev(h_alpha),
                                                     self._cells_dev(h_q)))

    def prior_diagonal(self, prior: Prior, alpha=None, q=None) -> tuple:
        """(diag_alpha, diag_q): the diagonal of Hess R(alpha, q); the point may be None where the penalty is quadratic."""
        a, qq = self._cells_host(alpha, "alpha"), self._cells_host(q, "q")
        da, dq = self._prior_out(prior)
        self._check(self.lib.c5_prior_diagonal(self.handle, C.byref(prior), _dp(a), _dp(qq), _dp(da), _dp(dq)))
        return da, dq

    def prior_diagonal_device(self, prior: Prior, alpha, q, diag_alpha, diag_q):
        """Asynchronous form on the context's stream (tensors or raw device pointers as prior_gradient_device)."""
        self._check(self.lib.c5_prior_diagonal_device(self.handle, C.byref(prior), self._cells_dev(alpha), self._cells_dev(q),
                                                      self._cells_dev(diag_alpha), self._cells_dev(diag_q)))

    # -- shape prior ------------------------------------------------------------------------------------
    def _points_host(self, a, name: str):
        """A per-point float64 [n_pts, 3] array of the caller's, or None."""
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (self.n_pts, 3):
            raise ValueError(f"{name} must be [n_pts, 3] = [{self.n_pts}, 3], not {list(a.shape)}")
        return a

    def _points_dev(self, t) -> int:
        import torch
        return _device_ptr(t, torch.float64, (self.n_pts, 3))

    def shape_prior_rest(self, xyz=None) -> int:
        """Take the shape prior's rest shape: xyz float64 [n_pts, 3] in the order of upload_grid, or None for the points
        the context holds now.  Returns the number of degenerate rest cells (stored with volume 0: they contribute nothing).
        The rest data stay until the next upload_grid; update_points does not touch them.  Waits for the stream."""
        x = self._points_host(xyz, "xyz")
        n_deg = C.c_int64()
        self._check(self.lib.c5_shape_prior_rest(self.handle, _dp(x), self.n_pts, C.byref(n_deg)))
        return n_deg.value

    def shape_prior_rest_device(self, xyz) -> int:
        """shape_prior_rest from device memory (a torch tensor float64 [n_pts, 3] on this context's GPU, a raw device
        pointer, or None: the context's points), read on the context's stream and waited for."""
        n_deg = C.c_int64()
        self._check(self.lib.c5_shape_prior_rest_device(self.handle, self._points_dev(xyz), self.n_pts, C.byref(n_deg)))
        return n_deg.value

    def shape_prior_rest_data(self) -> tuple:
        """(binv, vol, vert): the rest data in the order of upload_grid's cells - B = Dm^-1 float64 [n_cells, 3, 3], V0
        float64 [n_cells] (0: a degenerate cell) and int32 [n_cells, 4], the four points (weld representatives) in the
        order the arithmetic uses."""
        n = self.n_cells
        binv, vol, vert = np.zeros((n, 3, 3)), np.zeros(n), np.zeros((n, 4), dtype=np.int32)
        self._check(self.lib.c5_shape_prior_rest_data(self.handle, _dp(binv), _dp(vol), vert.ctypes.data_as(_ip_t)))
        return binv, vol, vert

    def shape_prior_rest_data_device(self, binv, vol, vert):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (float64 [n_cells, 3, 3], float64
        [n_cells], int32 [n_cells, 4]; any may be None) or raw device pointers."""
        import torch
        n = self.n_cells
        self._check(self.lib.c5_shape_prior_rest_data_device(self.handle, _device_ptr(binv, torch.float64, (n, 3, 3)),
                                                             _device_ptr(vol, torch.float64, (n,)), _device_ptr(vert, torch.int32, (n, 4))))

    def shape_prior_gradient(self, prior: ShapePrior, xyz) -> tuple:
        """(value, n_inverted, grad_xyz) of the shape prior at the coordinates xyz (float64 [n_pts, 3] in the order of
        upload_grid; the context's own points play no part): a float (+inf under the Neo-Hookean energy where a cell is
        inverted), the number of inverted cells and float64 [n_pts, 3].  Synchronous; bit-reproducible."""
        x = self._points_host(xyz, "xyz")
        value, n_inv, grad = np.zeros(1), C.c_int64(), np.zeros((self.n_pts, 3))
        self._check(self.lib.c5_shape_prior_gradient(self.handle, C.byref(prior), _dp(x), _dp(value), C.byref(n_inv), _dp(grad)))
        return float(value[0]), n_inv.value, grad

    def shape_prior_gradient_device(self, prior: ShapePrior, xyz, value, n_inverted, grad_xyz):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (xyz, grad_xyz float64 [n_pts, 3];
        value float64 [1] or None; n_inverted int64 [1] or None) or raw device pointers."""
        import torch
        self._check(self.lib.c5_shape_prior_gradient_device(self.handle, C.byref(prior), self._points_dev(xyz),
                                                            _device_ptr(value, torch.float64, (1,)), _device_ptr(n_inverted, torch.int64, (1,)),
                                                            self._points_dev(grad_xyz)))

    def shape_prior_product(self, prior: ShapePrior, xyz, v_xyz) -> np.ndarray:
        """Hess R(xyz) v_xyz, float64 [n_pts, 3]; xyz may be None under the Dirichlet energy (it is ignored there)."""
        x, v = self._points_host(xyz, "xyz"), self._points_host(v_xyz, "v_xyz")
        h = np.zeros((self.n_pts, 3))
        self._check(self.lib.c5_shape_prior_product(self.handle, C.byref(prior), _dp(x), _dp(v), _dp(h)))
        return h

    def shape_prior_product_device(self, prior: ShapePrior, xyz, v_xyz, h_xyz):
        """Asynchronous form on the context's stream (tensors or raw device pointers as shape_prior_gradient_device)."""
        self._check(self.lib.c5_shape_prior_product_device(self.handle, C.byref(prior), self._points_dev(xyz), self._points_dev(v_xyz),
                                                           self._points_dev(h_xyz)))

    def shape_prior_diagonal(self, prior: ShapePrior, xyz=None) -> np.ndarray:
        """The diagonal of Hess R(xyz), float64 [n_pts, 3]: the product applied to unit vectors."""
        x = self._points_host(xyz, "xyz")
        d = np.zeros((self.n_pts, 3))
        self._check(self.lib.c5_shape_prior_diagonal(self.handle, C.byref(prior), _dp(x), _dp(d)))
        return d

    def shape_prior_diagonal_device(self, prior: ShapePrior, xyz, diag_xyz):
        """Asynchronous form on the context's stream (tensors or raw device pointers as shape_prior_gradient_device)."""
        self._check(self.lib.c5_shape_prior_diagonal_device(self.handle, C.byref(prior), self._points_dev(xyz), self._points_dev(diag_xyz)))

    def shape_prior_quality(self, xyz) -> tuple:
        """(ratio, n_inverted): J = det F of every cell at xyz against the rest shape, float64 [n_cells] in the order of
        upload_grid (0 for a degenerate rest cell), and the number of cells with J <= 0 or not finite."""
        x = self._points_host(xyz, "xyz")
        ratio, n_inv = np.zeros(self.n_cells), C.c_int64()
        self._check(self.lib.c5_shape_prior_quality(self.handle, _dp(x), _dp(ratio), C.byref(n_inv)))
        return ratio, n_inv.value

    def shape_prior_quality_device(self, xyz, ratio, n_inverted):
        """Asynchronous form on the context's stream: xyz float64 [n_pts, 3], ratio float64 [n_cells] or None, n_inverted
        int64 [1] or None (torch tensors on this context's GPU, or raw device pointers)."""
        import torch
        self._check(self.lib.c5_shape_prior_quality_device(self.handle, self._points_dev(xyz), _device_ptr(ratio, torch.float64, (self.n_cells,)),
                                                           _device_ptr(n_inverted, torch.int64, (1,))))

    # -- Hessian-vector render ------------------------------------------------------------------------
    def render_hvp(self, d_alpha=None, d_q=None, grad_out=None, fit=("alpha", "q")) -> tuple:
        """(h_alpha, h_q) = Hess(sum_p g_I I_p) (d_alpha, d_q) of the frame render() would produce now: the exact second
        derivative in the cells' scalars applied to one direction (d_alpha / d_q: [n_cells], either may be None: zero),
        grad_out [local_rows, res_x, 2] the upstream image (channel 0 has no effect: tau is linear in alpha).  float64
        [n_cells] each in the order of upload_grid; fit names the blocks wanted (the other comes back as None).
        Synchronous; retries by itself.  Not bit-reproducible (fp64 atomics), as render_adjoint - unless
        set_option("exact_sums", 1): then exact sums, as render_gn_product's and render_gn_diagonal's."""
        da, dq = self._direction(d_alpha), self._direction(d_q)
        if da is None and dq is None:
            raise ValueError("give d_alpha and / or d_q")
        if grad_out is None:
            raise ValueError("grad_out is required")
        g = self._image(grad_out, "grad_out")
        fit = self._fit(fit)
        ha = np.zeros(self.n_cells) if "alpha" in fit else None
        hq = np.zeros(self.n_cells) if "q" in fit else None
        self._check(self.lib.c5_render_hvp(self.handle, _dp(da), _dp(dq), _fp(g), _dp(ha), _dp(hq)))
        return ha, hq

    def render_hvp_device(self, d_alpha, d_q, grad_out, h_alpha, h_q):
        """Asynchronous form on the context's stream: torch tensors on this context's GPU (d_alpha / d_q float64 [n_cells],
        one of them may be None; grad_out float32 [local_rows, res_x, 2]; h_alpha / h_q float64 [n_cells], one of them may
        be None; contiguous) or raw device pointers.  The status comes with the next synchronize() (C5_RETRY: run it
        again)."""
        if d_alpha is None and d_q is None:
            raise ValueError("give d_alpha and / or d_q")
        if h_alpha is None and h_q is None:
            raise ValueError("give h_alpha and / or h_q")
        if grad_out is None:
            raise ValueError("grad_out is required")
        ptrs = (self._cells_dev(d_alpha), self._cells_dev(d_q), self._image_dev(grad_out), self._cells_dev(h_alpha),
                self._cells_dev(h_q))
        self._check(self.lib.c5_render_hvp_device(self.handle, *ptrs))
    # -- frames delivered to host memory, pipelined -------------------------------------------------
    def host_image(self, full: bool = False) -> np.ndarray:
        """A pinned float32 [local_rows (or res_y), res_x, 2] image (c5_host_alloc); release with free_host_image."""
        rows = self.res_y if full else self.local_rows
        n = rows * self.res_x * 2
        p = C.c_void_p()
        self._check(self.lib.c5_host_alloc(self.handle, n * 4, C.byref(p)))
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n,)).reshape(rows, self.res_x, 2)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def free_host_image(self, arr: np.ndarray):
        p = self._pinned.pop(arr.ctypes.data)
        self._check(self.lib.c5_host_free(self.handle, p))

    def render_host_async(self, out: np.ndarray):
        self._check(self.lib.c5_render_host_async(self.handle, out.ctypes.data_as(C.POINTER(C.c_float))))

    def render_frame_rows_async(self, frame: np.ndarray):
        """This context's rows straight into their places of the full [res_y, res_x, 2] host image."""
        self._check(self.lib.c5_render_frame_rows_async(self.handle, frame.ctypes.data_as(C.POINTER(C.c_float))))

    def render_host_wait(self) -> int:
        return self._check(self.lib.c5_render_host_wait(self.handle), allow=(C5_RETRY,))

    def bench_host_frames(self, frames: int, ring: int = 3) -> dict:
        """Throughput of frames DELIVERED TO HOST MEMORY (what plane::trace_rays returns, plane.cpp:144-172):
        c5_render_host_async / _wait with `ring` frames in flight into pinned images, plus the plain
        synchronous c5_render into a pinned and into a pageable image."""
        import time
        bufs = [self.host_image() for _ in range(ring)]
        rays = self.local_rows * self.res_x
        out = {}
        try:
            def burst(n):
                bad = False
                for k in range(n):
                    if k >= ring:
                        bad |= self.render_host_wait() != C5_OK
                    self.render_host_async(bufs[k % ring])
                for k in range(min(ring, n)):
                    bad |= self.render_host_wait() != C5_OK
                return bad

            for attempt in range(3):
                # warm: the ring's device images and pinned pages are touched, the copy stream exists, the clocks are up
                # (BENCH_r02: 1.18 ms per frame over 20 cold frames against 0.78 sustained)
                burst(max(40, ring))
                t0 = time.perf_counter()
                redo = burst(frames)
                dt = time.perf_counter() - t0
                if dt < 0.2 and not redo:  # at least 0.2 s of frames
                    frames = int(frames * 0.25 / max(dt, 1e-3)) + 1
                    t0 = time.perf_counter()
                    redo = burst(frames)
                    dt = time.perf_counter() - t0
                if not redo:
                    break
            out["pipelined"] = {"ms_per_frame": round(dt * 1e3 / frames, 4), "value": round(rays * frames / dt / 1e6, 1),
                                "frames": frames, "in_flight": ring, "destination": "pinned"}
            for name, dst in (("sync_pinned", bufs[0]), ("sync_pageable", np.empty_like(bufs[0]))):
                self._check(self.lib.c5_render(self.handle, dst.ctypes.data_as(C.POINTER(C.c_float))))
                n = max(5, frames // 5)
                t0 = time.perf_counter()
                for _ in range(n):
                    self._check(self.lib.c5_render(self.handle, dst.ctypes.data_as(C.POINTER(C.c_float))))
                dt = time.perf_counter() - t0
                out[name] = {"ms_per_frame": round(dt * 1e3 / n, 4), "value": round(rays * n / dt / 1e6, 1), "frames": n}
            out["unit"] = "Mrays/s"
            out["what"] = ("the same frames delivered to HOST memory (the image plane::trace_rays returns): PCIe-inclusive, "
                           "never the headline value")
        finally:
            for b in bufs:
                self.free_host_image(b)
        return out

    def synchronize(self) -> int:
        """Waits for the stream; returns C5_OK or C5_RETRY (frame must be rendered again)."""
        return self._check(self.lib.c5_synchronize(self.handle), allow=(C5_RETRY,))

    def stats(self) -> dict:
        st = Stats()
        self._check(self.lib.c5_get_stats(self.handle, C.byref(st)))
        return st.as_dict()

    def walk_kernel_ms(self, reset: bool = True):
        avg, n = C.c_double(), C.c_int64()
        self._check(self.lib.c5_walk_kernel_ms(self.handle, int(reset), C.byref(avg), C.byref(n)))
        return avg.value, n.value

    def view_points(self, n_pts: int) -> np.ndarray:
        out = np.empty((n_pts, 3), dtype=np.float64)
        self._check(self.lib.c5_download_view_points(self.handle, _dp(out)), allow=(C5_RETRY,))
        return out


def _host_check(lib, rc: int) -> None:
    """The status of a call that takes no context."""
    if rc != C5_OK:
        raise C5Error(rc, lib.c5_last_error(None).decode())


def exact_sums_finish(exp, sums, res_x: int, res_y: int) -> np.ndarray:
    """Host-only: the fp64 values of exact adjoint sums - exp int32 [n], sums int64 [n, 2], contiguous, for an image of
    res_x x res_y pixels (the whole image, not a rank's rows) - rounded once, via c5_exact_sums_finish."""
    exp, sums = np.asarray(exp), np.asarray(sums)
    if exp.dtype != np.int32 or exp.ndim != 1 or not exp.flags.c_contiguous:
        raise ValueError(f"exp must be a contiguous int32 array [n], not {exp.dtype} {list(exp.shape)}")
    if sums.dtype != np.int64 or sums.shape != (exp.shape[0], 2) or not sums.flags.c_contiguous:
        raise ValueError(f"sums must be a contiguous int64 array [{exp.shape[0]}, 2], not {sums.dtype} {list(sums.shape)}")
    if int(res_x) < 1 or int(res_y) < 1:
        raise ValueError(f"an image of {res_x} x {res_y} pixels")
    lib = load_library()
    out = np.zeros(exp.shape[0], dtype=np.float64)
    _host_check(lib, lib.c5_exact_sums_finish(exp.ctypes.data_as(_ip_t), sums.ctypes.data_as(_lp_t), exp.shape[0], int(res_x), int(res_y),
                                              _dp(out)))
    return out


def face_adjacency(cells, n_pts: int):
    """Host-only: (adj[n,4], n_boundary_faces) via c5_face_adjacency."""
    lib = load_library()
    cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 4)
    adj = np.empty_like(cells)
    nb = C.c_int64()
    _host_check(lib, lib.c5_face_adjacency(cells.ctypes.data_as(_ip_t), cells.shape[0], n_pts, adj.ctypes.data_as(_ip_t), C.byref(nb)))
    return adj, nb.value


def rotation_motion(rots, index: int, what: int = 0) -> np.ndarray:
    """Host-only: the view-space velocity field [12] (A row-major, then b) of d / d(angle) (what 0) or d / d(x0) (what 1)
    of rotation `index` of the view `rots` (rows (axis, angle, x0)), via c5_rotation_motion."""
    lib = load_library()
    arr, n = _rot_array(rots)
    field = np.zeros(12, dtype=np.float64)
    _host_check(lib, lib.c5_rotation_motion(arr, n, index, what, _dp(field)))
    return field


def weld_points(xyz):
    """Host-only: (rep[n_pts], n_merged) via c5_weld_points."""
    lib = load_library()
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    rep = np.empty(xyz.shape[0], dtype=np.int32)
    m = C.c_int64()
    _host_check(lib, lib.c5_weld_points(_dp(xyz), xyz.shape[0], rep.ctypes.data_as(_ip_t), C.byref(m)))
    return rep, m.value


def device_count() -> int:
    lib = load_library()
    n = C.c_int()
    lib.c5_device_count(C.byref(n))
    return n.value
