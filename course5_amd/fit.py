"""One Gauss-Newton step of a fit of the cell field (alpha, Q) to observed images (and, at the end, of a shape fit: its
gradient, shape_gradient, and its Gauss-Newton step over the grid's points, shape_step, whose CG takes one
autograd.vertex_gn_product per iteration).

    delta, models = course5_amd.fit.gn_step(ctx, alpha, q, residual, fit=("q",))

With J the Jacobian of the frame of `ctx` at (alpha, q), r = render(alpha, q) - target the residual image and W the
per-pixel weights, the step minimises the quadratic model  m(d) = 1/2 d^T H d + d^T J^T W r,  H = J^T W J, by
preconditioned conjugate gradients on

    (H + damping * diag(H)) d = -J^T W r

with one adjoint render for the right-hand side, one gn_diagonal (the Jacobi preconditioner and Levenberg-Marquardt's
scaling) and one gn_product per iteration (course5_amd.autograd).  No line search and no outer loop: the caller owns
both.  Everything is float64 on the context's GPU.

A context may bring its own operators: if it has a method gn_operators(alpha, q, weight) returning an object with
rhs(residual) -> (J^T W r)_alpha, (..)_q, diagonal() -> (diag_alpha, diag_q) and product(v_alpha, v_q) -> (h_alpha, h_q)
(torch float64 tensors; v_alpha / v_q None: zero), gn_step uses those - a set of row shards that sums its parts
(RowShards below), a dense model, or the Jacobian itself: ExplicitJacobian(ctx) exports it once per linearisation
(autograd.ray_jacobian's arrays), and every CG iteration is then sparse products in float64 with no walk.

newton_product and newton_step are the same with the EXACT Hessian of 1/2 sum w r^2: H + sum_p w_p r_p Hess(img_p), the
second term from autograd.hvp (c5_render_hvp) on grad_img = W r.  The frame is exponential in alpha, so a fit of alpha is
not a linear least-squares problem and the two differ by the residual-weighted curvature; in q alone they coincide.  A
context's own operators then also need hvp(v_alpha, v_q, grad_img) -> (h_alpha, h_q).

Where rays say nothing - a cell no ray crosses, the null space along every ray of one view - the system above is singular:
SmoothnessPrior(ctx, lambda_q=...) is the library's face-neighbour penalty (include/course5_hip.h: c5_prior_*), and
gn_step(..., prior=P) / newton_step(WithPrior(ctx, P), ...) add its gradient, Hessian and diagonal to the system.

The shape fit has the same gap - a point none of whose cells a ray crosses - and one more: nothing keeps a step from turning
a cell inside out.  ShapePrior(ctx, lam) is the library's elastic energy of the points against a rest shape
(include/course5_hip.h: c5_shape_prior_*); shape_gradient / shape_step(WithShapePrior(ctx, P), ...) add it, and
shape_line_search(ctx, P, xyz, d) halves a step until no cell is inverted.  ExplicitShapeJacobian(ctx) is ExplicitJacobian's
twin for the shape (autograd.ray_shape_jacobian's arrays), the one set of shape operators with diag(J^T W J), and
shape_step_preconditioned the step whose CG is Jacobi-preconditioned with it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import capi, sharding


class _LibraryOperators:
    """The three operators of a capi.Context."""

    def __init__(self, ctx, alpha, q, weight):
        self.ctx, self.alpha, self.q, self.weight = ctx, alpha, q, weight

    def rhs(self, residual):
        from . import autograd
        ctx = self.ctx
        device = autograd._gn_enter(ctx, self.alpha, self.q, "gn_step")
        with torch.cuda.device(device):
            g = residual.detach().to(device=device, dtype=torch.float32)
            if self.weight is not None:
                g = g * autograd._gn_weight(ctx, self.weight, device)
            return autograd._adjoint(ctx, g.contiguous(), device)

    def diagonal(self):
        from . import autograd
        return autograd.gn_diagonal(self.ctx, self.alpha, self.q, self.weight)

    def product(self, v_alpha, v_q):
        from . import autograd
        return autograd.gn_product(self.ctx, self.alpha, self.q, v_alpha, v_q, self.weight)

    def hvp(self, v_alpha, v_q, grad_img):
        from . import autograd
        return autograd.hvp(self.ctx, self.alpha, self.q, v_alpha, v_q, grad_img)


class _LibraryShapeOperators:
    """The two shape operators of a capi.Context, _LibraryOperators' twin: rhs is one vertex adjoint render, product one
    vertex Gauss-Newton product (autograd.vertex_gn_product's one library call).  product comes after rhs, as in CG: it
    uses the scalars rhs sent to the context and the weights rhs put on its GPU.  what: the caller's name in messages."""

    def __init__(self, ctx, alpha, q, weight, what: str = "shape_step"):
        self.ctx, self.alpha, self.q, self.weight, self.what = ctx, alpha, q, weight, what

    def rhs(self, residual):
        """J^T W r, float64 [n_pts, 3]; W r is formed in float32."""
        from . import autograd
        ctx = self.ctx
        device = self.device = autograd._gn_enter(ctx, self.alpha, self.q, self.what)
        with torch.cuda.device(device):
            r = residual.detach().to(device=device, dtype=torch.float32)
            if tuple(r.shape) != (ctx.local_rows, ctx.res_x, 2):
                raise ValueError(f"residual must be [{ctx.local_rows}, {ctx.res_x}, 2], not {list(r.shape)}")
            w = self.w = autograd._gn_weight(ctx, self.weight, device)
            return autograd._vertex_adjoint(ctx, (r if w is None else r * w).contiguous(), device)

    def product(self, p):
        """J^T W J p, float64 [n_pts, 3]."""
        from . import autograd
        with torch.cuda.device(self.device):
            return autograd._vertex_gn_product(self.ctx, p.reshape(1, self.ctx.n_pts, 3).contiguous(), self.w, self.device)[0]


class _SegmentedCSR:
    """A sparse matrix by row and by column, for products that are one gather, one multiply and one segmented sum
    (torch.segment_reduce) each: crow [n_rows + 1] and cols [nnz] as given, and where every column's nonzeros are in a copy
    sorted by column (order: a stable argsort of cols; col_ptr; row_by_col: the row of every nonzero of that copy, from
    repeat_interleave of the rows' lengths).  No atomics: the same bits every call, on the CPU and on a GPU.
    values: the float arrays that come with cols, checked to hold crow's total each; names: what the messages call
    (cols and the values, crow, cols, a column)."""

    def __init__(self, crow, cols, values, n_cols: int, names):
        crow = torch.as_tensor(crow).to(torch.int64).contiguous()
        self.crow, self.n_rows, self.n_cols = crow, crow.shape[0] - 1, int(n_cols)
        self.cols = torch.as_tensor(cols).to(device=crow.device, dtype=torch.int64)
        self.values = tuple(torch.as_tensor(t).to(device=crow.device, dtype=torch.float64) for t in values)
        row = torch.repeat_interleave(torch.arange(self.n_rows, device=crow.device), crow[1:] - crow[:-1])
        if any(t.shape != row.shape for t in (self.cols,) + self.values):
            raise ValueError(f"{names[0]} must hold {names[1]}'s {row.shape[0]} elements each")
        if self.cols.numel() and not (0 <= int(self.cols.min()) and int(self.cols.max()) < self.n_cols):
            raise ValueError(f"{names[2]} must name {names[3]} 0 .. {self.n_cols - 1}")
        self.order = torch.argsort(self.cols, stable=True)
        self.col_ptr = torch.zeros(self.n_cols + 1, dtype=torch.int64, device=crow.device)
        self.col_ptr[1:] = torch.cumsum(torch.bincount(self.cols, minlength=self.n_cols), 0)
        self.row_by_col = row[self.order]

    def by_column(self, values):
        """values (row order) in the order of the copy sorted by column."""
        return values[self.order]

    def to_rows(self, values, v):
        """sum over a row's nonzeros of values * v[col] (values in row order)."""
        return torch.segment_reduce(values * v[self.cols], "sum", offsets=self.crow)

    def to_columns(self, values_c, g):
        """sum over a column's nonzeros of values * g[row] (values in column order)."""
        return torch.segment_reduce(values_c * g[self.row_by_col], "sum", offsets=self.col_ptr)


class _PixelOperators:
    """What the operators over an exported Jacobian share: the matrix's structure (self.csr, whose rows are the pixels), the
    per-pixel weights, and rhs and the weighted half of product over the subclass's jt."""

    def _pixels(self, image, name: str):
        """[n_px, 2] float32 where the matrix lives: a weight or residual image, [n_px, 2] or [rows, res_x, 2]."""
        t = torch.as_tensor(image).detach().to(device=self.csr.crow.device, dtype=torch.float32).reshape(-1, 2)
        if t.shape[0] != self.n_px:
            raise ValueError(f"{name} must hold two values for each of the {self.n_px} pixels")
        return t

    def _w(self):
        w = self.weight
        return (None, None) if w is None else (w[:, 0].to(torch.float64), w[:, 1].to(torch.float64))

    def _w_or_ones(self):
        one = torch.ones(self.n_px, dtype=torch.float64, device=self.csr.crow.device)
        return tuple(one if w is None else w for w in self._w())

    def rhs(self, residual):
        """J^T W r; W r is formed in float32, as the library's right-hand side forms it."""
        g = self._pixels(residual, "residual")
        if self.weight is not None:
            g = g * self.weight
        g = g.to(torch.float64)
        return self.jt(g[:, 0], g[:, 1])

    def _jt_weighted(self, tau, I):
        """J^T W (tau, I): the second half of a product."""
        w_tau, w_I = self._w()
        return self.jt(tau if w_tau is None else w_tau * tau, I if w_I is None else w_I * I)


class JacobianOperators(_PixelOperators):
    """rhs, diagonal and product of gn_step from the Jacobian's CSR arrays (capi.Context.ray_jacobian,
    autograd.ray_jacobian): row_ptr [n_px + 1], col, dz = d tau / d alpha, dI_dalpha, dI_dq [nnz] - torch tensors on any
    one device, the CPU included - n_cells, and weight [n_px, 2] or [rows, res_x, 2] (None: ones).  Everything in float64:

        H v = A^T (w_tau * (A v_a)) + J_I^T (w_I * (J_alpha v_a + J_q v_q)),   J_I^T = (J_alpha^T, J_q^T).

    Neither a CSR product nor its transpose is asked of torch.  A product is one gather, one multiply and one segmented sum
    (torch.segment_reduce): over the CSR rows for J v, and for J^T g over a copy of the values sorted by column, made once
    here (_SegmentedCSR).  No atomics: the same bits every call, on the CPU and on a GPU.  (index_add_ by col is correct
    too and needs no copy, but on the benchmark frame its fp64 atomics take a second per product where the segmented sums
    take milliseconds: DESIGN 4.19.)  Unlike the library's product, J v is not rounded to float32 on the way.
    hvp: what newton_step also needs, (v_alpha, v_q, grad_img) -> (h_alpha, h_q), or None."""

    def __init__(self, row_ptr, col, dz, dI_dalpha, dI_dq, n_cells: int, weight=None, hvp=None):
        self.csr = csr = _SegmentedCSR(row_ptr, col, (dz, dI_dalpha, dI_dq), n_cells,
                                       ("col, dz, dI_dalpha and dI_dq", "row_ptr", "col", "cells"))
        self.row_ptr, self.col, self.n_px, self.n_cells = csr.crow, csr.cols, csr.n_rows, csr.n_cols
        self.dz, self.da, self.dq = csr.values
        self.dz_c, self.da_c, self.dq_c = (csr.by_column(t) for t in csr.values)
        self.weight = None if weight is None else self._pixels(weight, "weight")
        self._hvp = hvp

    def _direction(self, v):
        return None if v is None else torch.as_tensor(v).detach().to(device=self.dz.device, dtype=torch.float64).reshape(self.n_cells)

    def jv(self, v_alpha, v_q):
        """J v per pixel: (tau_dot, I_dot), float64 [n_px] each (a None direction: zero)."""
        va, vq = self._direction(v_alpha), self._direction(v_q)
        zero = torch.zeros(self.n_px, dtype=torch.float64, device=self.dz.device)
        tau = zero if va is None else self.csr.to_rows(self.dz, va)
        I = zero.clone()
        if va is not None:
            I = I + self.csr.to_rows(self.da, va)
        if vq is not None:
            I = I + self.csr.to_rows(self.dq, vq)
        return tau, I

    def jt(self, g_tau, g_I):
        """J^T g per cell: (grad_alpha, grad_q) for the upstream image (g_tau, g_I), float64 [n_px] each."""
        to_cells = self.csr.to_columns
        return to_cells(self.dz_c, g_tau) + to_cells(self.da_c, g_I), to_cells(self.dq_c, g_I)

    def product(self, v_alpha, v_q):
        return self._jt_weighted(*self.jv(v_alpha, v_q))

    def diagonal(self):
        w_tau, w_I = self._w_or_ones()
        to_cells = self.csr.to_columns
        return (to_cells(self.dz_c * self.dz_c, w_tau) + to_cells(self.da_c * self.da_c, w_I), to_cells(self.dq_c * self.dq_c, w_I))

    def hvp(self, v_alpha, v_q, grad_img):
        if self._hvp is None:
            raise RuntimeError("these operators were built from arrays alone: the Jacobian does not hold second derivatives")
        return self._hvp(v_alpha, v_q, grad_img)


class ExplicitJacobian:
    """A context whose Gauss-Newton operators work on the exported Jacobian:

        delta, models = course5_amd.fit.gn_step(course5_amd.fit.ExplicitJacobian(ctx), alpha, q, residual, fit=("q",))

    gn_operators(alpha, q, weight) exports the Jacobian of the frame of `ctx` at (alpha, q) once (autograd.ray_jacobian's
    arrays: one c5_ray_matrix_rows and one c5_ray_jacobian_fill, nnz x 28 bytes on the context's GPU) and returns
    JacobianOperators over it: the right-hand side, the diagonal and every CG iteration's product are then sparse sums
    in float64 with no walk.  It pays where one linearisation serves many products: small and medium frames, many CG
    iterations, LSQR or column norms of the caller's own.  hvp goes to the library (c5_render_hvp), so newton_step works."""

    def __init__(self, ctx):
        self.ctx = ctx

    def gn_operators(self, alpha, q, weight):
        from . import autograd
        ctx = self.ctx
        device = autograd._gn_enter(ctx, alpha, q, "ExplicitJacobian")
        with torch.cuda.device(device):
            crow, col, dz, da, dq = autograd._ray_jacobian_arrays(ctx, device)
            w = autograd._gn_weight(ctx, weight, device)
        library = _LibraryOperators(ctx, alpha, q, weight)
        return JacobianOperators(crow, col, dz, da, dq, ctx.n_cells, w, hvp=library.hvp)


class ShapeJacobianOperators(_PixelOperators):
    """rhs, product and diagonal of shape_step from the coalesced shape Jacobian (autograd.assemble_shape_jacobian: crow
    [n_px + 1], cols [nnz] = 3 * point + coordinate, v_tau = d tau / d xyz, v_I = d I / d xyz) - torch tensors on any one
    device, the CPU included - n_pts, and weight [n_px, 2] or [rows, res_x, 2] (None: ones).  Everything in float64:

        H p = J_tau^T (w_tau * (J_tau p)) + J_I^T (w_I * (J_I p)),     diag(H) = sum_p w_tau J_tau^2 + w_I J_I^2.

    The products are _SegmentedCSR's, as JacobianOperators': one gather, one multiply and one segmented sum
    (torch.segment_reduce) over the CSR rows for J p, and for J^T g over a copy of the values sorted by column, made once
    here.  No atomics: the same bits every call.  Unlike the library's product, J p is not rounded to float32 on the way.
    The vectors are [n_pts, 3]."""

    def __init__(self, crow, cols, v_tau, v_I, n_pts: int, weight=None):
        self.n_pts = int(n_pts)
        self.csr = csr = _SegmentedCSR(crow, cols, (v_tau, v_I), 3 * self.n_pts, ("cols, v_tau and v_I", "crow", "cols", "coordinates"))
        self.crow, self.cols, self.n_px = csr.crow, csr.cols, csr.n_rows
        self.v_tau, self.v_I = csr.values
        self.v_tau_c, self.v_I_c = (csr.by_column(t) for t in csr.values)
        self.weight = None if weight is None else self._pixels(weight, "weight")

    def jv(self, p):
        """J p per pixel: (tau_dot, I_dot), float64 [n_px] each."""
        v = torch.as_tensor(p).detach().to(device=self.crow.device, dtype=torch.float64).reshape(3 * self.n_pts)
        return self.csr.to_rows(self.v_tau, v), self.csr.to_rows(self.v_I, v)

    def jt(self, g_tau, g_I):
        """J^T g, float64 [n_pts, 3], for the upstream image (g_tau, g_I), float64 [n_px] each."""
        return (self.csr.to_columns(self.v_tau_c, g_tau) + self.csr.to_columns(self.v_I_c, g_I)).reshape(self.n_pts, 3)

    def product(self, p):
        return self._jt_weighted(*self.jv(p))

    def diagonal(self):
        """diag(J^T W J) = sum over the pixels of w J^2 on the coalesced matrix, float64 [n_pts, 3]."""
        w_tau, w_I = self._w_or_ones()
        to_points = self.csr.to_columns
        return (to_points(self.v_tau_c * self.v_tau_c, w_tau) + to_points(self.v_I_c * self.v_I_c, w_I)).reshape(self.n_pts, 3)


class ExplicitShapeJacobian:
    """A context whose shape operators work on the exported shape Jacobian:

        d, models = course5_amd.fit.shape_step_preconditioned(course5_amd.fit.ExplicitShapeJacobian(ctx), alpha, q, residual)

    shape_operators(alpha, q, weight) exports the Jacobian of the frame of `ctx` at (alpha, q) and the points the context
    holds once (autograd.ray_shape_jacobian's arrays: c5_ray_matrix_rows / _fill, c5_ray_shape_jacobian_fill and
    c5_face_gradients, coalesced by autograd.assemble_shape_jacobian) and returns ShapeJacobianOperators over it: the
    right-hand side and every CG iteration's product are then sparse sums in float64 with no walk, and diagonal() is the
    exact diag(J^T W J) shape_step_preconditioned wants.  The Jacobian belongs to the points it was exported at:
    after update_points take a fresh object (or call shape_operators again)."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.n_pts = ctx.n_pts
        self.points = ctx.points

    def shape_operators(self, alpha, q, weight):
        from . import autograd
        ctx = self.ctx
        device = autograd._gn_enter(ctx, alpha, q, "ExplicitShapeJacobian")
        with torch.cuda.device(device):
            arrays = autograd._ray_shape_jacobian_arrays(ctx, device)
            a = autograd._plain(alpha).detach().to(device=device, dtype=torch.float64)  # (as autograd.ray_shape_jacobian)
            csr = autograd.assemble_shape_jacobian(arrays[0], arrays[1], a, *arrays[2:], ctx.n_pts)
            w = autograd._gn_weight(ctx, weight, device)
        return ShapeJacobianOperators(*csr, ctx.n_pts, w)


def _host(t, dtype):
    """A tensor or array as a contiguous numpy array of `dtype` on the host (None stays None)."""
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        t = t.detach().to("cpu").numpy()
    return np.ascontiguousarray(t, dtype=dtype)


class _ShardImages:
    """What the operators of a RowShards share: the scalars sent to every part, the whole-image weight, and the cuts."""

    def __init__(self, shards, alpha, q, weight):
        self.shards = shards
        a, qq = _host(alpha, np.float64), _host(q, np.float64)
        for ctx, _rows in shards.parts:
            ctx.update_scalars(a, qq)
        self.weight = shards.whole_image(weight, "weight")

    def _cut(self, image):
        """The whole image's rows of every part (None: None for every part)."""
        return [None if image is None else np.ascontiguousarray(image[rows]) for _ctx, rows in self.shards.parts]

    def _times_weight(self, images):
        """Per part: image * weight in float32, one multiply per channel (a None weight: ones)."""
        return [img if w is None else img * w for img, w in zip(images, self._cut(self.weight))]


class _ShardOperators(_ShardImages):
    """The four operators of a RowShards: every per-cell sum is the exact sum over the whole image, put together from the
    parts' integers."""

    def _exact(self, what, images, d_alpha=None, d_q=None):
        """One kind of exact sum over all parts: bounds on every part, the exponents combined, sums on every part against
        the combined exponents, the words combined, the finish."""
        sh = self.shards
        bounds = [ctx.render_exact_bounds(what, image=img, d_alpha=d_alpha, d_q=d_q) for (ctx, _rows), img in zip(sh.parts, images)]
        ea, eq, _, _ = sharding.combine_exact([tuple(b) + (None, None) for b in bounds])
        words = [ctx.render_exact_sums(what, ea, eq, image=img, d_alpha=d_alpha, d_q=d_q) for (ctx, _rows), img in zip(sh.parts, images)]
        _, _, sa, sq = sharding.combine_exact([(ea, eq) + tuple(w) for w in words])
        return tuple(torch.as_tensor(capi.exact_sums_finish(e, s, sh.res_x, sh.res_y), device=sh.device) for e, s in ((ea, sa), (eq, sq)))

    def rhs(self, residual):
        r = self.shards.whole_image(residual, "residual")
        return self._exact(capi.C5_EXACT_ADJOINT, self._times_weight(self._cut(r)))

    def diagonal(self):
        return self._exact(capi.C5_EXACT_GN_DIAGONAL, self._cut(self.weight))

    def product(self, v_alpha, v_q):
        va, vq = _host(v_alpha, np.float64), _host(v_q, np.float64)
        # the split product: a tangent render on the part's rows, the fp32 multiply, then the exact adjoint of that image
        jv = [ctx.render_tangent(va, vq) for ctx, _rows in self.shards.parts]
        return self._exact(capi.C5_EXACT_ADJOINT, self._times_weight(jv))

    def hvp(self, v_alpha, v_q, grad_img):
        g = self.shards.whole_image(grad_img, "grad_img")
        return self._exact(capi.C5_EXACT_HVP, self._cut(g), _host(v_alpha, np.float64), _host(v_q, np.float64))


class _ShardShapeOperators(_ShardImages):
    """The two operators of a shape fit over a RowShards: the vertex adjoint's sums are the exact sums over the whole image,
    put together from the parts' integers and finished on the first part's context."""

    def _exact(self, images):
        """bounds on every part, the exponents combined (max), sums on every part against the combined exponents, the
        words combined (add), the finish on the first part."""
        sh = self.shards
        bounds = [ctx.render_vertex_exact_bounds(img) for (ctx, _rows), img in zip(sh.parts, images)]
        exps, _ = sharding.combine_vertex_exact([(b, None) for b in bounds])
        words = [ctx.render_vertex_exact_sums(img, exps) for (ctx, _rows), img in zip(sh.parts, images)]
        _, sums = sharding.combine_vertex_exact([(exps, w) for w in words])
        return torch.as_tensor(sh.parts[0][0].vertex_exact_finish(exps, sums), device=sh.device)

    def rhs(self, residual):
        """J^T W r, float64 [n_pts, 3]."""
        r = self.shards.whole_image(residual, "residual")
        return self._exact(self._times_weight(self._cut(r)))

    def product(self, p):
        """J^T W J p, float64 [n_pts, 3]: a vertex tangent render on every part's rows, the fp32 multiply by the part's
        weights, then the exact vertex adjoint of those images."""
        d = _host(p, np.float64)
        return self._exact(self._times_weight([ctx.render_vertex_tangent(d) for ctx, _rows in self.shards.parts]))


class RowShards:
    """An image whose rows are spread over several contexts, as one context to gn_step and newton_step:

        shards = course5_amd.fit.RowShards([(ctx0, rows0), (ctx1, rows1)])
        delta, models = course5_amd.fit.gn_step(shards, alpha, q, residual, weight, fit=("alpha", "q"))

    parts: a list of (ctx, rows).  Every context carries the same grid, image (set_image), view and alpha limit; rows is
    the index array of the image rows that context owns - what its set_row_range or set_row_tiles was given
    (sharding.local_rows).  The rows must partition range(res_y): a row owned twice or by nobody is refused.

    gn_operators(alpha, q, weight) is the hook course5_amd.fit looks for.  The operators take whole-image residual, weight
    and upstream arrays [res_y, res_x, 2], cut them by `rows`, send the scalars to every context, and put every per-cell
    sum together from the parts' integers: render_exact_bounds on every part, sharding.combine_exact, render_exact_sums on
    every part against the combined exponents, combine_exact, capi.exact_sums_finish.  So rhs, diagonal, product and hvp
    - and with them the steps of gn_step and newton_step - are bit for bit those of ONE context over the whole image
    with set_option("exact_sums", 1), however the rows are split.  They return float64 torch tensors on the first
    context's device (a stand-in whose `device` is not an index names a torch device itself).

    shape_operators(alpha, q, weight) is the hook shape_gradient and shape_step look for: rhs(residual) -> J^T W r and
    product(p) -> J^T W J p over the grid's points, float64 [n_pts, 3], the vertex adjoint's sums put together in the same
    way (render_vertex_exact_bounds, sharding.combine_vertex_exact, render_vertex_exact_sums, combine, vertex_exact_finish
    on the first context) - bit for bit those of ONE context over the whole image with set_option("vertex_exact", 1).
    update_points(xyz) sends new points to every context (the outer loop of a shape fit).

    A grid of several components that may interpenetrate (parts that share no face: nothing in the connectivity shows an
    overlap) must have set_option("algorithm", 1) on EVERY context, before the upload.  Left to itself a context finds
    the overlap only from its own rays: one whose rows miss it stays on the walk, the whole-image context falls back to
    sorted lists, and the two take their chords differently - the bars hold either way, the bits do not
    (tests/test_gpu_component_fuzz.py counts it: the exact scalar sums of 3 row splits in 8 differed, profiles/
    component_fuzz.md).  With "algorithm" 1 on every part the identity above holds on such grids too (asserted there).

    This class is about bits, not speed: it uses the host-pointer forms and numpy between them.  Contexts on one device
    are the tested case; contexts on several devices work by construction and are unmeasured."""

    def __init__(self, parts):
        parts = [(ctx, np.asarray(rows, dtype=np.int64).reshape(-1)) for ctx, rows in parts]
        if not parts:
            raise ValueError("RowShards needs at least one (ctx, rows)")
        first = parts[0][0]
        self.res_x, self.res_y, self.n_cells = first.res_x, first.res_y, first.n_cells
        self.n_pts = getattr(first, "n_pts", None)  # (a stand-in for the cell field's fit need not have points)
        for ctx, rows in parts:
            if (ctx.res_x, ctx.res_y, ctx.n_cells) != (self.res_x, self.res_y, self.n_cells):
                raise ValueError("every context of a RowShards carries the same grid and image")
            if len(rows) != ctx.local_rows:
                raise ValueError(f"a context renders {ctx.local_rows} rows and was given {len(rows)}")
        owned = np.sort(np.concatenate([rows for _ctx, rows in parts]))
        if len(owned) != self.res_y or not np.array_equal(owned, np.arange(self.res_y)):
            raise ValueError(f"the rows of the parts must partition range({self.res_y}): every row once, none left out")
        self.parts = parts
        self.device = torch.device("cuda", first.device) if isinstance(first.device, int) else torch.device(first.device)

    def whole_image(self, image, name: str):
        """A whole-image array as float32 [res_y, res_x, 2] on the host (None stays None)."""
        a = _host(image, np.float32)
        if a is not None and a.shape != (self.res_y, self.res_x, 2):
            raise ValueError(f"{name} must be the whole image [{self.res_y}, {self.res_x}, 2], not {list(a.shape)}")
        return a

    def gn_operators(self, alpha, q, weight):
        return _ShardOperators(self, alpha, q, weight)

    def shape_operators(self, alpha, q, weight):
        return _ShardShapeOperators(self, alpha, q, weight)

    def update_points(self, xyz):
        """New coordinates of the grid's points (float64 [n_pts, 3]) to every part."""
        xyz = _host(xyz, np.float64)
        for ctx, _rows in self.parts:
            ctx.update_points(xyz)


def _weighted(residual, weight):
    """W r as the upstream image of the curvature term (float32, as the right-hand side forms it)."""
    g = residual.detach().to(torch.float32)
    if weight is not None:
        g = g * weight.detach().to(device=g.device, dtype=torch.float32)
    return g.contiguous()


def _operators(ctx, alpha, q, weight):
    return ctx.gn_operators(alpha, q, weight) if hasattr(ctx, "gn_operators") else _LibraryOperators(ctx, alpha, q, weight)


class SmoothnessPrior:
    """The smoothness prior of the grid of `ctx` (a capi.Context; of a RowShards any one part's: they carry the same grid) as
    gn_step and newton_step take it (prior=):

        P = course5_amd.fit.SmoothnessPrior(ctx, lambda_q=1e-3)
        delta, models = course5_amd.fit.gn_step(ctx, alpha, q, residual, fit=("q",), prior=P)

    lambda_alpha / lambda_q >= 0 weigh the two fields (0: the field has no prior); penalty "quadratic" or "pseudo_huber"
    (then with delta_alpha / delta_q > 0 for the fields that have a lambda); weighting "tpfa" (face area over the
    centroids' distance) or "unit".  The definitions are include/course5_hip.h's (c5_prior).  The three operators take
    torch tensors [n_cells] in the order of upload_grid, any dtype and device, and return float64 tensors on the context's
    GPU (zeros for a field whose lambda is 0), one library call each on torch's current stream: enqueued in that stream's
    order with no wait under a torch.cuda.Stream of torch's own, waited for on torch's default (null) stream, which the
    library's stream is not ordered against (autograd._enqueue)."""

    PENALTIES = {"quadratic": capi.C5_PRIOR_QUADRATIC, "pseudo_huber": capi.C5_PRIOR_PSEUDO_HUBER}
    WEIGHTINGS = {"unit": capi.C5_PRIOR_UNIT, "tpfa": capi.C5_PRIOR_TPFA}

    def __init__(self, ctx, lambda_alpha: float = 0.0, lambda_q: float = 0.0, penalty: str = "quadratic", weighting: str = "tpfa",
                 delta_alpha=None, delta_q=None):
        if penalty not in self.PENALTIES:
            raise ValueError(f"penalty must be one of {sorted(self.PENALTIES)}, not {penalty!r}")
        if weighting not in self.WEIGHTINGS:
            raise ValueError(f"weighting must be one of {sorted(self.WEIGHTINGS)}, not {weighting!r}")
        for name, lam, delta in (("alpha", lambda_alpha, delta_alpha), ("q", lambda_q, delta_q)):
            if not (lam >= 0.0 and np.isfinite(lam)):
                raise ValueError(f"lambda_{name} must be finite and >= 0, not {lam!r}")
            if penalty == "pseudo_huber" and lam > 0.0 and (delta is None or not (delta > 0.0 and np.isfinite(delta))):
                raise ValueError(f"the pseudo-Huber penalty needs delta_{name} > 0, not {delta!r}")
        self.ctx = ctx
        # (a delta nobody reads is 1: the struct holds a number either way)
        self.prior = capi.Prior(self.PENALTIES[penalty], self.WEIGHTINGS[weighting], lambda_alpha, lambda_q,
                                1.0 if delta_alpha is None else delta_alpha, 1.0 if delta_q is None else delta_q)

    def _call(self, fields, enqueue, with_value: bool = False):
        from . import autograd
        ctx = self.ctx
        with autograd._on_gpu(ctx) as device:
            args = [torch.zeros(ctx.n_cells, dtype=torch.float64, device=device) if t is None else
                    torch.as_tensor(t).detach().to(device=device, dtype=torch.float64).contiguous() for t in fields]
            if any(tuple(t.shape) != (ctx.n_cells,) for t in args):
                raise ValueError(f"every field must hold one value per cell ({ctx.n_cells})")
            out = autograd._cell_pair(ctx, device)
            value = torch.empty(2, dtype=torch.float64, device=device) if with_value else None
            autograd._enqueue(ctx, device, lambda: enqueue(args, value, out))
        return (value, *out) if with_value else out

    def only(self, fields):
        """This prior with the lambda of every field not named in `fields` set to 0: the kernels skip a field left out."""
        p = self.prior
        kept = SmoothnessPrior.__new__(SmoothnessPrior)
        kept.ctx = self.ctx
        kept.prior = capi.Prior(p.penalty, p.weighting, p.lambda_alpha if "alpha" in fields else 0.0,
                                p.lambda_q if "q" in fields else 0.0, p.delta_alpha, p.delta_q)
        return kept

    def value_gradient(self, alpha, q) -> tuple:
        """(value, grad_alpha, grad_q): value float64 [2] = (R(alpha), R(q))."""
        return self._call((alpha, q), lambda a, value, out: self.ctx.prior_gradient_device(self.prior, a[0], a[1], value, *out), True)

    def product(self, alpha, q, v_alpha, v_q) -> tuple:
        """(h_alpha, h_q) = Hess R(alpha, q) (v_alpha, v_q); a None direction is zero."""
        return self._call((alpha, q, v_alpha, v_q), lambda a, _value, out: self.ctx.prior_product_device(self.prior, *a, *out))

    def diagonal(self, alpha, q) -> tuple:
        """(diag_alpha, diag_q) of Hess R(alpha, q)."""
        return self._call((alpha, q), lambda a, _value, out: self.ctx.prior_diagonal_device(self.prior, a[0], a[1], *out))


class WithPrior:
    """A context together with a SmoothnessPrior, as one context to gn_step and newton_step:

        delta, models = course5_amd.fit.newton_step(course5_amd.fit.WithPrior(ctx, P), alpha, q, residual)

    the same as prior=P where the step has that argument (gn_step).  ctx: a capi.Context, or anything gn_step takes in its
    place (RowShards, ExplicitJacobian)."""

    def __init__(self, ctx, prior):
        self.ctx, self.prior = ctx, prior


def _cg_step(ctx, alpha, q, residual, weight, fit, damping, iters, precondition, exact, prior=None):
    """gn_step (exact False: H = J^T W J) and newton_step (exact True: H the exact Hessian of 1/2 sum w r^2); with a
    prior P its gradient joins the right-hand side, its Hessian the operator and its diagonal the preconditioner - once,
    behind whatever sum the context's own operators form."""
    fit = capi.Context._fit(fit, once=True)
    if damping < 0.0 or iters < 1:
        raise ValueError("damping must be >= 0 and iters >= 1")
    if isinstance(ctx, WithPrior):
        if prior is not None:
            raise ValueError("give the prior once: with the context (WithPrior) or as prior=")
        ctx, prior = ctx.ctx, ctx.prior
    if hasattr(prior, "only"):
        prior = prior.only(fit)  # (a field that is not fitted is not computed either)
    ops = _operators(ctx, alpha, q, weight)
    n = alpha.shape[0]
    wr = _weighted(residual, weight) if exact else None

    def pick(a, b):
        return torch.cat([t for name, t in (("alpha", a), ("q", b)) if name in fit])

    def split(x):
        if len(fit) == 2:
            return x[:n], x[n:]
        return (x, None) if fit[0] == "alpha" else (None, x)

    def H(x):
        va, vq = split(x)
        h = pick(*ops.product(va, vq))
        if exact:
            h = h + pick(*ops.hvp(va, vq, wr))
        return h if prior is None else h + pick(*prior.product(alpha, q, va, vq)).to(h.device)

    g = pick(*ops.rhs(residual)).to(torch.float64)  # J^T W r
    d = pick(*ops.diagonal()).to(torch.float64)
    # (a cell no ray crosses: a zero row and column of H and a zero of the right-hand side; its unknown stays 0 - unless
    # a prior couples it to its neighbours)
    dm = d  # the preconditioner's diagonal; damping scales diag(H) = d alone
    if prior is not None:
        g = g + pick(*prior.value_gradient(alpha, q)[1:]).to(g.device)  # J^T W r + grad P
        dm = d + pick(*prior.diagonal(alpha, q)).to(d.device)
    m_inv = torch.where(dm > 0, 1.0 / torch.where(dm > 0, dm, torch.ones_like(dm)), torch.zeros_like(dm)) if precondition else None

    x = torch.zeros_like(g)
    hx = torch.zeros_like(g)
    r = -g
    z = r * m_inv if precondition else r
    p = z.clone()
    rz = float(r @ z)
    models = []
    for _ in range(iters):
        if not rz > 0.0:
            break
        hp = H(p)
        ap = hp + damping * d * p
        curvature = float(p @ ap)
        if not curvature > 0.0:
            if exact and not models:
                x = p.clone()  # (nothing else to return: steepest descent in the preconditioner's metric)
            break
        step = rz / curvature
        x += step * p
        hx += step * hp
        r -= step * ap
        models.append(float(0.5 * (x @ hx) + x @ g))
        z = r * m_inv if precondition else r
        rz_next = float(r @ z)
        p = z + (rz_next / rz) * p
        rz = rz_next
    return split(x), models


def gn_step(ctx, alpha, q, residual, weight=None, fit=("q",), damping: float = 0.0, iters: int = 10, precondition: bool = True,
            prior=None):
    """Up to `iters` iterations of (Jacobi-preconditioned) CG from d = 0 on (H + damping diag(H)) d = -J^T W r over the
    fields named in `fit` ("alpha", "q" or both; the other is held fixed).  Returns ((d_alpha, d_q), models): the step
    (None for a field not fitted) and the model value m(d_i) after every iteration done, as floats.  It stops early when
    the residual of the linear system vanishes or a direction has no curvature.
    prior: a SmoothnessPrior P (None: none, today's path and bits).  CG then runs on
        (H + damping diag(H) + Hess P) d = -(J^T W r + grad P)
    with P taken at (alpha, q): the Jacobi preconditioner is the inverse of diag(H) + diag(Hess P), damping keeps scaling
    diag(H) alone, and models[i] = 1/2 d^T (H + Hess P) d + d^T (J^T W r + grad P).  Only the fields named in `fit` enter,
    and a fitted field whose lambda is 0 gets no term.  A context with operators of its own (RowShards, ExplicitJacobian)
    gets the prior added once, after its own sum."""
    return _cg_step(ctx, alpha, q, residual, weight, fit, damping, iters, precondition, exact=False, prior=prior)


def newton_product(ctx, alpha, q, residual, v_alpha, v_q, weight=None) -> tuple:
    """(h_alpha, h_q) = Hess(1/2 sum w r^2) (v_alpha, v_q) at (alpha, q), r = render(alpha, q) - target the residual image
    ([local_rows, res_x, 2]) and w the per-pixel weights (None: ones): gn_product(v) + hvp(v, grad_img = W r), the
    Gauss-Newton product plus the residual-weighted curvature it leaves out.  v_alpha / v_q [n_cells], either may be None
    (zero).  Two library calls; float64 on the context's GPU."""
    ops = _operators(ctx, alpha, q, weight)
    ga, gq = ops.product(v_alpha, v_q)
    ha, hq = ops.hvp(v_alpha, v_q, _weighted(residual, weight))
    return ga + ha, gq + hq


def newton_step(ctx, alpha, q, residual, weight=None, fit=("q",), damping: float = 0.0, iters: int = 10):
    """gn_step with the exact Hessian: up to `iters` iterations of Jacobi-preconditioned CG from d = 0 on
        (Hess(1/2 sum w r^2) + damping diag(J^T W J)) d = -J^T W r
    over the fields named in `fit`, one gn_product and one hvp per iteration (newton_product); the preconditioner is the
    Gauss-Newton diagonal.  The exact Hessian can be indefinite: the iteration stops at the first direction without
    positive curvature and returns what it has - if that is the very first direction, the preconditioned steepest-descent
    direction itself (its model value is then not appended: the model has no minimum along it).  Returns ((d_alpha, d_q),
    models) as gn_step does.  No line search and no outer loop: the caller owns both.  A smoothness prior comes with the
    context: newton_step(WithPrior(ctx, P), ...) adds it as gn_step(..., prior=P) does."""
    return _cg_step(ctx, alpha, q, residual, weight, fit, damping, iters, True, exact=True)


def view_step(ctx, alpha, q, angles, residual, weight=None, damping: float = 0.0):
    """One Gauss-Newton step for the angles of the view (the pose: what a fit to observations has to find first).  The
    angles ([n_rots] radians) are written into the context's rotation list as autograd.render_view writes them; with
    J = d img / d angles from ONE motion tangent render (n_rots images), r = render_view(alpha, q, angles) - target and W
    the per-pixel weights ([local_rows, res_x, 2]; None: ones) it solves the dense n_rots x n_rots system
        (J^T W J + damping diag(J^T W J)) d = -J^T W r
    in float64.  Returns (d, model): the step, float64 [n_rots] on the context's GPU, and the quadratic model's value
    1/2 d^T J^T W J d + d^T J^T W r there.  No line search and no outer loop: the caller owns both.  An angle the image
    does not depend on (a singular system) needs damping > 0."""
    from . import autograd
    autograd._set_angles(ctx, angles)
    device = autograd._gn_enter(ctx, alpha, q, "view_step")
    J = autograd._motion(ctx, ctx.view_fields(), device).to(torch.float64).reshape(len(ctx.rots), -1)
    r = residual.detach().to(device=device, dtype=torch.float64).reshape(-1)
    if r.shape[0] != J.shape[1]:
        raise ValueError(f"residual must be [{ctx.local_rows}, {ctx.res_x}, 2]")
    w = autograd._gn_weight(ctx, weight, device)
    JW = J if w is None else J * w.to(torch.float64).reshape(1, -1)
    H = JW @ J.T
    g = JW @ r
    d = torch.linalg.solve(H + damping * torch.diag(torch.diagonal(H)), -g)
    return d, float(0.5 * d @ H @ d + d @ g)


class ShapePrior:
    """The shape prior of the grid of `ctx` (a capi.Context; of a RowShards any one part's: they carry the same grid): the
    elastic energy lam * sum V0 psi(F) of the points against a rest shape (include/course5_hip.h: c5_shape_prior).

        P = course5_amd.fit.ShapePrior(ctx, 1e-2)                      # rest: the points the context holds now
        d, models = course5_amd.fit.shape_step(course5_amd.fit.WithShapePrior(ctx, P), alpha, q, residual)
        t = course5_amd.fit.shape_line_search(ctx, P, ctx.points, d)   # no cell of xyz + t d is inverted

    energy "neo_hookean" (rotation-invariant, a barrier against inversion, kappa >= 0 its volume term) or "dirichlet"
    (quadratic).  rest: float64 [n_pts, 3] in the order of upload_grid, None for the points the context holds, or False
    to keep the rest shape the context already has.  The rest shape lives on the context until the next upload_grid;
    update_points does not touch it.  The operators take coordinates [n_pts, 3] (torch tensors or arrays, any dtype and
    device) and return float64 tensors on the context's GPU, one library call each on torch's current stream, under
    SmoothnessPrior's stream rules (autograd._enqueue)."""

    ENERGIES = {"dirichlet": capi.C5_SHAPE_DIRICHLET, "neo_hookean": capi.C5_SHAPE_NEO_HOOKEAN}

    def __init__(self, ctx, lam: float, energy: str = "neo_hookean", kappa: float = 1.0, rest=None):
        if energy not in self.ENERGIES:
            raise ValueError(f"energy must be one of {sorted(self.ENERGIES)}, not {energy!r}")
        for name, v in (("lam", lam), ("kappa", kappa)):
            if not (v >= 0.0 and np.isfinite(v)):
                raise ValueError(f"{name} must be finite and >= 0, not {v!r}")
        self.ctx = ctx
        self.prior = capi.ShapePrior(self.ENERGIES[energy], lam, kappa)
        self.n_degenerate = None
        if ctx is not None and rest is not False:
            self.n_degenerate = ctx.shape_prior_rest(None if rest is None else _host(rest, np.float64))

    def _points(self, t, device):
        t = torch.as_tensor(t).detach().to(device=device, dtype=torch.float64).contiguous()
        if tuple(t.shape) != (self.ctx.n_pts, 3):
            raise ValueError(f"coordinates must be [n_pts, 3] = [{self.ctx.n_pts}, 3], not {list(t.shape)}")
        return t

    def _call(self, arrays, enqueue, outputs):
        """enqueue(args, outs) with `arrays` as float64 [n_pts, 3] tensors on the context's GPU and outs made by outputs(device)."""
        from . import autograd
        ctx = self.ctx
        with autograd._on_gpu(ctx) as device:
            args = [None if t is None else self._points(t, device) for t in arrays]
            outs = outputs(device)
            autograd._enqueue(ctx, device, lambda: enqueue(args, outs))
        return outs

    def _vector(self, device):
        return torch.empty((self.ctx.n_pts, 3), dtype=torch.float64, device=device)

    def value_gradient(self, xyz) -> tuple:
        """(value, grad): a float64 [1] tensor (+inf where the Neo-Hookean energy meets an inverted cell) and float64 [n_pts, 3]."""
        value, grad = self._call((xyz,), lambda a, o: self.ctx.shape_prior_gradient_device(self.prior, a[0], o[0], None, o[1]),
                                 lambda device: (torch.empty(1, dtype=torch.float64, device=device), self._vector(device)))
        return value, grad

    def product(self, xyz, v) -> torch.Tensor:
        """Hess R(xyz) v, float64 [n_pts, 3]."""
        return self._call((xyz, v), lambda a, o: self.ctx.shape_prior_product_device(self.prior, a[0], a[1], o[0]),
                          lambda device: (self._vector(device),))[0]

    def diagonal(self, xyz) -> torch.Tensor:
        """The diagonal of Hess R(xyz), float64 [n_pts, 3]."""
        return self._call((xyz,), lambda a, o: self.ctx.shape_prior_diagonal_device(self.prior, a[0], o[0]),
                          lambda device: (self._vector(device),))[0]

    def quality(self, xyz) -> tuple:
        """(ratio, n_inverted): J = det F per cell at xyz, float64 [n_cells] on the context's GPU in the order of
        upload_grid, and the number of inverted cells as an int (read back: this call waits)."""
        ratio, n_inv = self._call((xyz,), lambda a, o: self.ctx.shape_prior_quality_device(a[0], o[0], o[1]),
                                  lambda device: (torch.empty(self.ctx.n_cells, dtype=torch.float64, device=device),
                                                  torch.zeros(1, dtype=torch.int64, device=device)))
        return ratio, int(n_inv.item())

    def feasible(self, xyz) -> bool:
        """No cell is inverted at xyz."""
        return self.quality(xyz)[1] == 0


class WithShapePrior:
    """A context together with a ShapePrior, as one context to shape_gradient and shape_step:

        d, models = course5_amd.fit.shape_step(course5_amd.fit.WithShapePrior(ctx, P), alpha, q, residual)

    ctx: a capi.Context, or anything shape_step takes in its place (RowShards).  The prior is taken at the points the
    context holds (ctx.points; of a RowShards its first part's) and enters once, after whatever sum the context's own
    operators form."""

    def __init__(self, ctx, prior):
        self.ctx, self.prior = ctx, prior

    def points(self):
        ctx = self.ctx
        return (ctx.parts[0][0] if hasattr(ctx, "parts") else ctx).points


def shape_line_search(ctx, P, xyz, d, shrink: float = 0.5, max_halvings: int = 30) -> float:
    """The largest t in 1, shrink, shrink^2, ... for which no cell is inverted at xyz + t d (P.quality: one cell launch per
    trial, no render): the feasibility half of a line search, the smallest useful piece of the loop around shape_step.
    xyz, d: [n_pts, 3].  Returns t as a float; 0.0 if max_halvings trials did not find one (xyz itself is then the only
    point known feasible - or is not feasible either).  ctx is the context whose grid P belongs to."""
    from . import autograd
    if P.ctx is not ctx:
        raise ValueError("the prior belongs to another context")
    if not 0.0 < shrink < 1.0:
        raise ValueError("shrink must lie in (0, 1)")
    with autograd._on_gpu(ctx) as device:
        x, step = P._points(xyz, device), P._points(d, device)
    t = 1.0
    for _ in range(max_halvings + 1):
        if P.feasible(x + t * step):
            return t
        t *= shrink
    return 0.0


def _split_shape_prior(ctx):
    """(ctx, prior, points): a WithShapePrior taken apart (prior None: a plain context)."""
    if isinstance(ctx, WithShapePrior):
        return ctx.ctx, ctx.prior, ctx.points()
    return ctx, None, None


def _shape_operators(ctx, alpha, q, weight, what):
    """The context's own shape operators where it has them, else the library's."""
    if hasattr(ctx, "shape_operators"):
        return ctx.shape_operators(alpha, q, weight)
    return _LibraryShapeOperators(ctx, alpha, q, weight, what)


def _shape_loss(r, w):
    """(g, loss): g = w r in float32 and 1/2 sum w r^2 summed in float64, where r lives (w None: ones)."""
    g = (r if w is None else r * w).contiguous()
    return g, 0.5 * float((g.to(torch.float64) * r.to(torch.float64)).sum())


def shape_gradient(ctx, alpha, q, residual, weight=None):
    """The loss 1/2 sum w r^2 of a fit of the grid's SHAPE and its gradient with respect to the points the context holds
    (capi.Context.update_points, autograd.render_mesh): r = frame - target the residual image, w the per-pixel weights
    ([local_rows, res_x, 2]; None: ones).  Returns (loss, grad_xyz): a float and float64 [n_pts, 3] on the context's GPU,
    from ONE vertex adjoint render on g = w r.  The building block of a descent loop, no more: step size, line search and
    the loop are the caller's.
    A context may bring its own operators, as for gn_step: if it has a method shape_operators(alpha, q, weight) returning
    an object with rhs(residual) -> J^T W r and product(p) -> J^T W J p (float64 [n_pts, 3] tensors), the gradient is its
    rhs - RowShards, whose residual and weight are whole images [res_y, res_x, 2].
    WithShapePrior(ctx, P) in place of ctx: the loss gains R and the gradient grad R, at the points the context holds."""
    ctx, prior, points = _split_shape_prior(ctx)
    if prior is not None:  # the loss and the gradient gain R and grad R at the points the context holds
        loss, grad = shape_gradient(ctx, alpha, q, residual, weight)
        value, g = prior.value_gradient(points)
        return loss + float(value[0]), grad + g.to(grad.device)
    grad = _shape_operators(ctx, alpha, q, weight, "shape_gradient").rhs(residual)
    r = torch.as_tensor(residual).detach().to(device=grad.device, dtype=torch.float32)
    w = None if weight is None else torch.as_tensor(weight).detach().to(device=grad.device, dtype=torch.float32)
    return _shape_loss(r, w)[1], grad


def _shape_cg(JtWr, H, damping, iters, free, n_pts, diagonal=None):
    """shape_step's iteration on the two operators: JtWr() -> J^T W r, H(p) -> J^T W J p, float64 [n_pts, 3].  diagonal:
    None (plain CG), or a function returning the diagonal of H's operator, float64 [n_pts, 3]: CG is then preconditioned by
    the inverse of diagonal() + damping (0 where that is not positive, and in the rows `free` fixes)."""
    g = JtWr()
    keep = None
    if free is not None:
        keep = torch.as_tensor(free, device=g.device)
        if keep.dtype != torch.bool or tuple(keep.shape) != (n_pts,):
            raise ValueError(f"free must be bool [{n_pts}]")
        keep = keep.to(torch.float64).reshape(-1, 1)

    def fixed(v):
        return v if keep is None else v * keep

    def dot(a, b):
        return float((a * b).sum())

    g = fixed(g)
    x = torch.zeros_like(g)
    hx = torch.zeros_like(g)  # (H + damping I) x
    res = -g
    models = []
    m_inv = None
    if diagonal is not None:
        m = diagonal().to(device=g.device, dtype=torch.float64).reshape(n_pts, 3) + damping
        m_inv = fixed(torch.where(m > 0, 1.0 / torch.where(m > 0, m, torch.ones_like(m)), torch.zeros_like(m)))
    z = res if m_inv is None else res * m_inv
    p = z.clone()
    rz = dot(res, z)
    for _ in range(iters):
        if not rz > 0.0:
            break
        ap = fixed(H(p)) + damping * p
        curvature = dot(p, ap)
        if not curvature > 0.0:
            break
        step = rz / curvature
        x += step * p
        hx += step * ap
        res -= step * ap
        models.append(0.5 * dot(x, hx) + dot(x, g))
        z = res if m_inv is None else res * m_inv
        rz_next = dot(res, z)
        p = z + (rz_next / rz) * p
        rz = rz_next
    return x, models


def shape_step(ctx, alpha, q, residual, weight=None, damping: float = 1e-3, iters: int = 10, free=None):
    """One Gauss-Newton step of a fit of the grid's SHAPE: up to `iters` iterations of CG from d = 0 on
        (J^T W J + damping I) d = -J^T W r
    over the points the context holds, J = d frame / d xyz at them (alpha, q the scalars), r = frame - target the residual
    image, W the per-pixel weights ([local_rows, res_x, 2]; None: ones).  Every iteration is one vertex Gauss-Newton
    product (autograd.vertex_gn_product: J^T W J p in one library call, the vertex adjoint of W * fp32(J p)) on the device,
    float64, on torch's current stream.  free: bool [n_pts]
    or None (all); the points outside it stay fixed - their rows of every vector are zeroed.  Returns (d_xyz, models):
    float64 [n_pts, 3] on the context's GPU and, after every iteration done, the model 1/2 d^T (H + damping I) d +
    d^T J^T W r as a float.  It stops early when the residual of the linear system vanishes or a direction has no
    curvature.  No line search and no outer loop: the caller owns both (update_points(xyz + d), render, again).
    CG amplifies last-bit differences of J^T W (J p) from iteration to iteration: with set_option("vertex_exact", 1) on the
    context the steps are the same bits every run.  A context's own operators (shape_operators: shape_gradient) are used
    where it has them - over RowShards the step is bit for bit the one context's, however the rows are split.
    A shape prior comes with the context: shape_step(WithShapePrior(ctx, P), ...) runs CG on
        (J^T W J + damping I + Hess R) d = -(J^T W r + grad R)
    with R taken at the points the context holds, one c5_shape_prior_product more per iteration; models[i] then holds the
    prior's terms too.  The Neo-Hookean Hessian can be indefinite: the iteration stops at a direction without curvature.
    shape_step_preconditioned is the same step with a Jacobi preconditioner from the exported Jacobian."""
    return _shape_step(ctx, alpha, q, residual, weight, damping, iters, free, False)


def shape_step_preconditioned(ctx, alpha, q, residual, weight=None, damping: float = 1e-3, iters: int = 10, free=None):
    """shape_step with Jacobi-preconditioned CG: the same system, the same arguments and the same returns (models[i] is the same
    model), preconditioned by the inverse of diag(J^T W J) + damping (+ the prior's diagonal at the points the context holds,
    under WithShapePrior); the rows `free` fixes get 0.  On graded grids diag(J^T W J) spans orders of magnitude from point to
    point, which damping I does not scale with, and plain CG converges slowly.  The diagonal of the data term cannot be summed
    per segment (a ray meets a point through several faces, and their terms add before they are squared): it comes from the
    exported Jacobian, so the context's operators must offer diagonal() - ExplicitShapeJacobian(ctx) does; a plain context or a
    RowShards raises ValueError.  A function of its own, not an argument of shape_step: shape_step keeps its parameters and runs
    the code and returns the bits it did."""
    return _shape_step(ctx, alpha, q, residual, weight, damping, iters, free, True)


def _shape_step(ctx, alpha, q, residual, weight, damping, iters, free, precondition):
    """shape_step (precondition False) and shape_step_preconditioned (True): the operators, the prior's terms added to each
    once, _shape_cg."""
    if damping < 0.0 or iters < 1:
        raise ValueError("damping must be >= 0 and iters >= 1")
    ctx, prior, points = _split_shape_prior(ctx)
    ops = _shape_operators(ctx, alpha, q, weight, "shape_step")
    if precondition and not hasattr(ops, "diagonal"):
        raise ValueError("shape_step_preconditioned needs diag(J^T W J), which only the exported Jacobian has: give "
                         "course5_amd.fit.ExplicitShapeJacobian(ctx) in place of the context")

    def JtWr():
        g = ops.rhs(residual)
        return g if prior is None else g + prior.value_gradient(points)[1].to(g.device)

    def H(p):
        h = ops.product(p)
        return h if prior is None else h + prior.product(points, p).to(h.device)

    def diagonal():
        d = ops.diagonal()
        return d if prior is None else d + prior.diagonal(points).to(d.device)

    return _shape_cg(JtWr, H, damping, iters, free, ctx.n_pts, diagonal if precondition else None)
