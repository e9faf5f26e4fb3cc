"""`course --view_tangent PREFIX`: one two-channel .vti per rotation of the grid's view, equal to
capi.Context.render_view_tangent."""
import os
import subprocess

import numpy as np
import pytest

from course5_amd import capi, meshgen as mg, vtkio
from tests import motion_reference as mr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COURSE = os.path.join(ROOT, "course5_amd", "course")


def test_view_tangent_files_equal_the_library_call(tmp_path):
    xyz, cells = mg.kuhn_box(4, jitter=0.1)
    alpha, q = mr.scalars(len(cells), 12)
    q = q.astype(np.float32).astype(np.float64)  # the binary writer stores Q as float
    src = tmp_path / "g.vtk"
    mg.write_vtk_binary(str(src), xyz, cells, alpha, q)
    rx, ry, ax, ay, ai = 96, 72, 0.1, 0.07, 0.02
    r = subprocess.run([COURSE, "-f", str(src), "-d", str(tmp_path / "a.vti"), "-x", str(rx), "-y", str(ry), "-X", str(ax), "-Y", str(ay),
                        "-I", str(ai), "--no_solids", "-j", "4", "--view_tangent", str(tmp_path / "t")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rots = mg.view_rotations(ax, ay, ai)
    with capi.Context(0) as ctx:
        ctx.upload_grid(xyz, cells, alpha, q)
        ctx.set_image(rx, ry, mg.REFERENCE_BOUNDS)
        ctx.set_view(rots)
        want = ctx.render_view_tangent()
        frame = ctx.render()
    assert np.array_equal(vtkio.read_vti(str(tmp_path / "a.vti"))[0].astype(np.float32), frame)
    for i, name in enumerate(("I", "Y", "X")):  # the list's order: the system's turn about x (-I), about y (-Y), about x (-X)
        img, info = vtkio.read_vti(str(tmp_path / f"t_{name}.vti"))
        assert info["components"] == 2 and img.shape == (ry, rx, 2)
        assert np.abs(want[i]).max() > 0
        assert np.array_equal(img.astype(np.float32), want[i]), name

