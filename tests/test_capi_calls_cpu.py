"""What every derivative method of capi.Context sends to the library, no GPU: each is called once per distinct pattern of
its arguments on a bare context over a recording library (tests/fake_library.py), and the recorded (symbol, arguments) and
the dtype and shape of what the method returns are compared with a literal table.

The table was written down once from the wrappers as they stood before their argument handling was folded into shared
helpers, by running this very body with the recorder printing; it is the record of what the library is sent and is not
regenerated from the code it checks.  A new render adds rows; a change to a row is a change of the ABI's use.

7 cells, 9 points, a 5 x 6 image and K = 3 tell every argument apart.  Device forms take raw device pointers (integers),
which the wrappers pass through unchecked."""
import numpy as np
import pytest

from tests.fake_library import RecordingLibrary, bare_context

K = 3
P1, P2, P3, P4, P5, P6 = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
D = np.zeros(7)                        # a direction per cell
DK = np.zeros((K, 7))
G = np.zeros((5, 6, 2), np.float32)    # an upstream image, a weight
GK = np.zeros((K, 5, 6, 2), np.float32)
X = np.zeros((9, 3))                   # a displacement per point
XK = np.zeros((K, 9, 3))
F = np.zeros(12)                       # an affine motion field
FK = np.zeros((K, 12))
ROWS = np.arange(31, dtype=np.int64) // 8   # a row_ptr of 5 x 6 + 1 entries that ends at 3

IMG, IMGS = ("float32", (5, 6, 2)), ("float32", (K, 5, 6, 2))
CELLS, CELLSK = ("float64", (7,)), ("float64", (K, 7))

# (method, args, kwargs, the calls recorded, what came back)
CASES = [
    ("render_adjoint", (G,), {},
     [("c5_render_adjoint", (None, "ptr", "ptr", "ptr"))], (CELLS, CELLS)),
    ("render_adjoint", (G.astype(np.float64),), {},
     [("c5_render_adjoint", (None, "ptr", "ptr", "ptr"))], (CELLS, CELLS)),
    ("render_adjoint_device", (P1, P2, P3), {},
     [("c5_render_adjoint_device", (None, P1, P2, P3))], None),
    ("render_vertex_adjoint", (G,), {},
     [("c5_render_vertex_adjoint", (None, "ptr", "ptr"))], ("float64", (9, 3))),
    ("render_vertex_adjoint_device", (P1, P2), {},
     [("c5_render_vertex_adjoint_device", (None, P1, P2))], None),
    ("render_vertex_adjoint_device", (None, P2), {},
     [("c5_render_vertex_adjoint_device", (None, None, P2))], None),
    ("render_vertex_adjoint_device", (P1, None), {},
     [("c5_render_vertex_adjoint_device", (None, P1, None))], None),
    ("render_vertex_tangent", (X,), {},
     [("c5_render_vertex_tangent", (None, 1, "ptr", "ptr"))], IMG),
    ("render_vertex_tangent", (XK,), {},
     [("c5_render_vertex_tangent", (None, 3, "ptr", "ptr"))], IMGS),
    ("render_vertex_tangent_device", (P1, P2), {"n": K},
     [("c5_render_vertex_tangent_device", (None, 3, P1, P2))], None),
    ("render_vertex_tangent_device", (None, P2), {"n": K},
     [("c5_render_vertex_tangent_device", (None, 3, None, P2))], None),
    ("render_vertex_tangent_device", (P1, None), {"n": K},
     [("c5_render_vertex_tangent_device", (None, 3, P1, None))], None),
    ("ray_matrix_rows", (), {},
     [("c5_ray_matrix_rows", (None, "ptr", "ptr"))], ("int64", (31,))),
    ("ray_matrix_rows_device", (P1,), {},
     [("c5_ray_matrix_rows_device", (None, P1, "ptr"))], 0),
    ("ray_matrix_rows_device", (None,), {},
     [("c5_ray_matrix_rows_device", (None, None, "ptr"))], 0),
    ("ray_matrix_fill", (ROWS,), {},
     [("c5_ray_matrix_fill", (None, "ptr", 3, "ptr", "ptr", None))], (("int32", (3,)), ("float64", (3,)))),
    ("ray_matrix_fill", (ROWS,), {"with_depth": True},
     [("c5_ray_matrix_fill", (None, "ptr", 3, "ptr", "ptr", "ptr"))], (("int32", (3,)), ("float64", (3,)), ("float64", (3,)))),
    ("ray_matrix_fill", (ROWS,), {"capacity": 10},
     [("c5_ray_matrix_fill", (None, "ptr", 10, "ptr", "ptr", None))], (("int32", (10,)), ("float64", (10,)))),
    ("ray_matrix_fill", (ROWS, True, 0), {},
     [("c5_ray_matrix_fill", (None, "ptr", None, "ptr", "ptr", "ptr"))],
     (("int32", (0,)), ("float64", (0,)), ("float64", (0,)))),
    ("ray_matrix_fill_device", (P1, P2, P3), {"capacity": 4},
     [("c5_ray_matrix_fill_device", (None, P1, 4, P2, P3, None))], None),
    ("ray_matrix_fill_device", (P1, P2, P3, P4), {"capacity": 4},
     [("c5_ray_matrix_fill_device", (None, P1, 4, P2, P3, P4))], None),
    ("ray_matrix_fill_device", (None, None, None, None), {"capacity": 4},
     [("c5_ray_matrix_fill_device", (None, None, 4, None, None, None))], None),
    ("ray_matrix", (), {},
     [("c5_ray_matrix_rows", (None, "ptr", "ptr")), ("c5_ray_matrix_fill", (None, "ptr", None, "ptr", "ptr", None))],
     (("int64", (31,)), ("int32", (0,)), ("float64", (0,)))),
    ("ray_matrix", (), {"with_depth": True},
     [("c5_ray_matrix_rows", (None, "ptr", "ptr")), ("c5_ray_matrix_fill", (None, "ptr", None, "ptr", "ptr", "ptr"))],
     (("int64", (31,)), ("int32", (0,)), ("float64", (0,)), ("float64", (0,)))),
    ("render_tangent", (D, D), {},
     [("c5_render_tangent", (None, "ptr", "ptr", "ptr"))], IMG),
    ("render_tangent", (D, None), {},
     [("c5_render_tangent", (None, "ptr", None, "ptr"))], IMG),
    ("render_tangent", (None, D), {},
     [("c5_render_tangent", (None, None, "ptr", "ptr"))], IMG),
    ("render_tangent", (), {},
     [("c5_render_tangent", (None, None, None, "ptr"))], IMG),
    ("render_tangent_device", (P1, P2, P3), {},
     [("c5_render_tangent_device", (None, P1, P2, P3))], None),
    ("render_tangent_device", (None, P2, P3), {},
     [("c5_render_tangent_device", (None, None, P2, P3))], None),
    ("render_tangent_device", (P1, None, P3), {},
     [("c5_render_tangent_device", (None, P1, None, P3))], None),
    ("render_tangent_device", (0, 0, P3), {},
     [("c5_render_tangent_device", (None, None, None, P3))], None),
    ("render_tangent_device", (P1, P2, None), {},
     [("c5_render_tangent_device", (None, P1, P2, None))], None),
    ("render_tangent_batch", (DK, DK), {},
     [("c5_render_tangent_batch", (None, 3, "ptr", "ptr", "ptr"))], IMGS),
    ("render_tangent_batch", (DK, None), {},
     [("c5_render_tangent_batch", (None, 3, "ptr", None, "ptr"))], IMGS),
    ("render_tangent_batch", (None, DK), {},
     [("c5_render_tangent_batch", (None, 3, None, "ptr", "ptr"))], IMGS),
    ("render_tangent_batch_device", (P1, P2, P3), {"n": K},
     [("c5_render_tangent_batch_device", (None, 3, P1, P2, P3))], None),
    ("render_tangent_batch_device", (None, P2, P3), {"n": K},
     [("c5_render_tangent_batch_device", (None, 3, None, P2, P3))], None),
    ("render_tangent_batch_device", (P1, None, P3), {"n": K},
     [("c5_render_tangent_batch_device", (None, 3, P1, None, P3))], None),
    ("render_adjoint_batch", (GK,), {},
     [("c5_render_adjoint_batch", (None, 3, "ptr", "ptr", "ptr"))], (CELLSK, CELLSK)),
    ("render_adjoint_batch_device", (P1, P2, P3), {"n": K},
     [("c5_render_adjoint_batch_device", (None, 3, P1, P2, P3))], None),
    ("render_motion_tangent", (F,), {},
     [("c5_render_motion_tangent", (None, 1, "ptr", "ptr"))], IMG),
    ("render_motion_tangent", (FK,), {},
     [("c5_render_motion_tangent", (None, 3, "ptr", "ptr"))], IMGS),
    ("render_motion_tangent_device", (F, P1), {},
     [("c5_render_motion_tangent_device", (None, 1, "ptr", P1))], None),
    ("render_motion_tangent_device", (FK, P1), {},
     [("c5_render_motion_tangent_device", (None, 3, "ptr", P1))], None),
    ("render_view_tangent", (), {},
     [], ("float32", (0, 5, 6, 2))),
    ("render_gn_product", (DK, DK), {},
     [("c5_render_gn_product", (None, 3, "ptr", "ptr", None, "ptr", "ptr", None))], (CELLSK, CELLSK)),
    ("render_gn_product", (DK, None, G), {},
     [("c5_render_gn_product", (None, 3, "ptr", None, "ptr", "ptr", "ptr", None))], (CELLSK, CELLSK)),
    ("render_gn_product", (None, DK), {"want_jv": True},
     [("c5_render_gn_product", (None, 3, None, "ptr", None, "ptr", "ptr", "ptr"))], (CELLSK, CELLSK, IMGS)),
    ("render_gn_product", (DK, DK, G, True), {"fit": ("alpha",)},
     [("c5_render_gn_product", (None, 3, "ptr", "ptr", "ptr", "ptr", None, "ptr"))], (CELLSK, None, IMGS)),
    ("render_gn_product", (DK, DK), {"fit": ("q",)},
     [("c5_render_gn_product", (None, 3, "ptr", "ptr", None, None, "ptr", None))], (None, CELLSK)),
    ("render_gn_product_device", (P1, P2, P3, P4, P5, P6), {"n": K},
     [("c5_render_gn_product_device", (None, 3, P1, P2, P3, P4, P5, P6))], None),
    ("render_gn_product_device", (P1, None, None, P4, None), {"n": K},
     [("c5_render_gn_product_device", (None, 3, P1, None, None, P4, None, None))], None),
    ("render_gn_product_device", (None, P2, P3, None, P5, None), {"n": K},
     [("c5_render_gn_product_device", (None, 3, None, P2, P3, None, P5, None))], None),
    ("render_gn_diagonal", (), {},
     [("c5_render_gn_diagonal", (None, None, "ptr", "ptr"))], (CELLS, CELLS)),
    ("render_gn_diagonal", (G,), {},
     [("c5_render_gn_diagonal", (None, "ptr", "ptr", "ptr"))], (CELLS, CELLS)),
    ("render_gn_diagonal_device", (P1, P2, P3), {},
     [("c5_render_gn_diagonal_device", (None, P1, P2, P3))], None),
    ("render_gn_diagonal_device", (None, P2, P3), {},
     [("c5_render_gn_diagonal_device", (None, None, P2, P3))], None),
    ("render_hvp", (D, D, G), {},
     [("c5_render_hvp", (None, "ptr", "ptr", "ptr", "ptr", "ptr"))], (CELLS, CELLS)),
    ("render_hvp", (D, None, G), {"fit": ("alpha",)},
     [("c5_render_hvp", (None, "ptr", None, "ptr", "ptr", None))], (CELLS, None)),
    ("render_hvp", (None, D, G), {"fit": ("q",)},
     [("c5_render_hvp", (None, None, "ptr", "ptr", None, "ptr"))], (None, CELLS)),
    ("render_hvp_device", (P1, P2, P3, P4, P5), {},
     [("c5_render_hvp_device", (None, P1, P2, P3, P4, P5))], None),
    ("render_hvp_device", (None, P2, P3, None, P5), {},
     [("c5_render_hvp_device", (None, None, P2, P3, None, P5))], None),
    ("render_hvp_device", (P1, None, P3, P4, None), {},
     [("c5_render_hvp_device", (None, P1, None, P3, P4, None))], None),
]


def described(out):
    if isinstance(out, tuple):
        return tuple(described(o) for o in out)
    return (out.dtype.name, out.shape) if isinstance(out, np.ndarray) else out


def transcript(method, args, kwargs):
    ctx = bare_context()
    ctx.lib = RecordingLibrary()
    out = getattr(ctx, method)(*args, **kwargs)
    return ctx.lib.calls, described(out)


@pytest.mark.parametrize("method,args,kwargs,calls,returned", CASES, ids=[f"{i}-{c[0]}" for i, c in enumerate(CASES)])
def test_the_library_is_sent(method, args, kwargs, calls, returned):
    assert transcript(method, args, kwargs) == (calls, returned)
