"""The render as a differentiable torch function of the cells' scalars.

    img = course5_amd.autograd.render(ctx, alpha, q)     # [local_rows, res_x, 2] float32 on ctx's GPU (tau, I)
    loss = (img * W).sum(); loss.backward()              # alpha.grad, q.grad: d loss / d AbsorpCoef, d loss / d radEnLooseRate

    with torch.autograd.forward_ad.dual_level():         # forward mode: the image's change for a change of the scalars
        img = render(ctx, fwAD.make_dual(alpha, d_alpha), q)
        img_dot = fwAD.unpack_dual(img).tangent          # [local_rows, res_x, 2] float32 (tau_dot, I_dot)
    img, img_dot = torch.func.jvp(lambda a, b: render(ctx, a, b), (alpha, q), (d_alpha, d_q))   # the same

    J = torch.func.jacfwd(lambda th: render(ctx, f(th), q))(theta)      # [local_rows, res_x, 2, P]: one batched tangent
    J = torch.func.jacrev(lambda a: losses(render(ctx, a, q)))(alpha)   # [L, n_cells]: one batched adjoint

`ctx` is a capi.Context with grid, image, rows, view (and solids) set; alpha and q hold one value per cell in the order of
its upload_grid.  The backward pass is the library's adjoint render (c5_render_adjoint_device), the forward-mode
derivative (jvp) its tangent render (c5_render_tangent_device): the derivative of the reference's integral as written,
alpha limit and all (include/course5_hip.h).  Under torch.func.vmap - jacfwd, jacrev, vmap over jvp or over vjp's function -
a batch of tangents or cotangents goes to the batched renders (c5_render_tangent_batch_device,
c5_render_adjoint_batch_device) in one call: every ray is walked once for several directions.  A batch of scalar fields
(vmap over alpha or q themselves) and second derivatives (hessian, jacrev of jacrev, double backward, ...) raise.

Forward: alpha and q on the context's GPU go to it through c5_update_scalars_device (gathered on the device; the call waits
for the stream), others through c5_update_scalars, i.e. through host memory; then the frame is rendered on torch's current
stream and waited for (a C5_RETRY renders it again).  The image is the same bits either way.  Backward: the adjoint on
torch's current stream, waited for likewise; gradients come back in the dtype and on the device of alpha and q.  jvp: the
tangents of alpha and q (None: zero) go to the context's GPU as float64, the tangent render runs on torch's current stream
and is waited for; the image's tangent is float32 on the context's GPU, like the image.

The context holds ONE set of scalars: a backward or jvp whose forward's scalars have since been replaced (another forward,
an update_scalars) uploads its own again, from the copy the forward kept (on the GPU when they came from there).  A
backward or jvp after the view, image, rows, solids, alpha limit or grid changed raises instead of differentiating a frame
other than the one rendered.  The gradients are fp64 sums added by atomics in arrival order: not bit-reproducible from run
to run, unless the context's option "adjoint_exact" is 1 (ctx.set_option("adjoint_exact", 1): the backward calls
render_adjoint_device, which then returns the exact integer sums - the same bits every run); the tangent is, batched or not.

render_view(ctx, alpha, q, angles) is render with the view's angles as a third differentiable input: angles [n_rots]
(radians) are written into the context's current rotation list (axes and x0 kept) before the frame is rendered.  Its
derivative in the angles is the library's motion tangent render (c5_render_motion_tangent_device): backward is ONE such
call for all the angles and grad_angles[i] = sum g * d img / d angle_i in fp64; jvp is one call for the one affine field
sum_i t_i field_i; under vmap, batches of angle tangents go to one batched call and batches of cotangents share one.
Pixels that gain or lose coverage when the view turns are not differentiated (include/course5_hip.h): the derivative is
that of the smooth piece every pixel is on.  alpha and q are differentiated as by render.

render_mesh(ctx, xyz, alpha, q) is render with the grid's points as a differentiable input: xyz [n_pts, 3] in the order
and the coordinates of upload_grid go to the context through c5_update_points when they differ from the ones it holds
(connectivity, weld groups and cell order stay; through host memory, the call waits for the stream).  Backward is ONE
vertex adjoint render (c5_render_vertex_adjoint_device) for xyz and the adjoint render for alpha and q, whichever
needs_input_grad asks for; a point welded to another at upload gets a zero gradient, its representative the group's sum.
By default a tangent on xyz (jvp, jacfwd) raises, as second derivatives do; tangents on alpha and q go through the
tangent render as in render.  Under vmap a batch of cotangents (jacrev, vmap over a vjp) goes to ONE batched vertex
adjoint call (c5_render_vertex_adjoint_batch_device): one walk per ray for up to "batch_width" cotangents.

render_mesh(ctx, xyz, alpha, q, forward_xyz=True) has forward mode in the points too: a tangent on xyz (torch.func.jvp,
forward_ad dual tensors, jacfwd) goes to ONE vertex tangent render (c5_render_vertex_tangent_device), added in float32 to
the scalar tangent's image when alpha or q carry tangents as well; under vmap a batch of xyz tangents goes to one batched
call.  The rows of points welded to another at upload are not read.  Cotangents and second derivatives are as without
the switch.  It is a switch, not the default, because the refusal of forward mode in xyz is behaviour callers (and a test)
rely on: nothing changes for a caller that does not ask.

Beside render, two operators for Gauss-Newton fits (course5_amd.fit): gn_product(ctx, alpha, q, v_alpha, v_q, weight) =
J^T W J v and gn_diagonal(ctx, alpha, q, weight) = diag(J^T W J), one library call each (c5_render_gn_product_device,
c5_render_gn_diagonal_device).  They upload the scalars as the forward does, return float64 tensors on the context's GPU
without a graph, and raise under a differentiating torch.func transform.

The shape has the same operator: vertex_gn_product(ctx, alpha, q, v_xyz, weight) = J^T W J v with J the frame's Jacobian
in the points the context holds (render_mesh's derivative in xyz), one library call (c5_render_vertex_gn_product_device)
with gn_product's conventions; course5_amd.fit.shape_step's CG calls it once per iteration.

Second derivatives through render itself raise, but the exact second-order operator in the scalars is there as a call of
its own: hvp(ctx, alpha, q, v_alpha, v_q, grad_img) = Hess(sum_p grad_img_p . img_p) v, one library call
(c5_render_hvp_device), with gn_product's conventions.  course5_amd.fit.newton_product / newton_step build the exact
Hessian of a least-squares fit from it.

ray_matrix(ctx) hands out the operator itself: the frame's per-pixel (cell, chord) lists as a torch.sparse_csr_tensor on the
context's GPU (c5_ray_matrix_rows_device, c5_ray_matrix_fill_device), for solvers that want A and not only A v and A^T g.

prior(ctx, alpha, q, prior) is the regulariser such a fit needs: the smoothness prior R(alpha) + R(q) over the grid's
interior faces (capi.Prior; include/course5_hip.h: c5_prior_*), a float64 scalar differentiable TWICE in alpha and q - the
forward is one c5_prior_gradient_device, which leaves the gradient too, and the second derivative is one
c5_prior_product_device.  It needs the grid alone: no image, no view, and not the context's own scalars.

shape_prior(ctx, xyz, prior) is the regulariser of a SHAPE fit: the elastic energy of the coordinates xyz [n_pts, 3] against
the rest shape the context holds (ctx.shape_prior_rest; capi.ShapePrior; include/course5_hip.h: c5_shape_prior_*), a
float64 scalar differentiable twice in xyz exactly as prior is in its fields - one c5_shape_prior_gradient_device for value
and gradient, one c5_shape_prior_product_device for the second derivative.  The context's own points play no part.
"""
from __future__ import annotations

from contextlib import contextmanager, nullcontext

import numpy as np
import torch

from . import capi


def _use_torch_stream(ctx: capi.Context, device: torch.device) -> None:
    stream = torch.cuda.current_stream(device)
    if ctx.stream_ptr != stream.cuda_stream:
        ctx.set_stream(stream.cuda_stream)
    if stream.cuda_stream == 0:
        # torch's default stream is the null stream, which the library takes for "its own stream": not ordered against
        # each other, so what torch has queued (the inputs) is waited for here
        stream.synchronize()


def _run(ctx: capi.Context, enqueue) -> None:
    for _ in range(3):
        enqueue()
        if ctx.synchronize() == capi.C5_OK:
            return
    raise capi.C5Error(capi.C5_RETRY, "the frame kept needing to be rendered again")


@contextmanager
def _on_gpu(ctx: capi.Context, unwrapped: bool = False):
    """The context's GPU as torch's current device, and as what the block gets.  unwrapped: torch.func's dispatch is off
    inside (under torch.func.jvp / vmap the arguments arrive wrapped, with no storage of their own: the library reads
    plain tensors, _plain's)."""
    device = torch.device("cuda", ctx.device)
    with torch._C._DisableFuncTorch() if unwrapped else nullcontext(), torch.cuda.device(device):
        yield device


def _launch(ctx: capi.Context, device: torch.device, enqueue) -> None:
    """enqueue() on torch's current stream, after what torch has queued there (the call's inputs), and waited for."""
    _use_torch_stream(ctx, device)
    _run(ctx, enqueue)


def _plain(t: torch.Tensor) -> torch.Tensor:
    """t without torch.func's wrappers."""
    while torch._C._functorch.is_functorch_wrapped_tensor(t):
        t = torch._C._functorch.get_unwrapped(t)
    return t


def _lift(t: torch.Tensor, dim, k: int) -> torch.Tensor:
    """_plain(t) with its batch dimension first; an unbatched one (dim None) is the same for every one of the k."""
    t = _plain(t).detach()
    return t.movedim(dim, 0) if dim is not None else t.expand(k, *t.shape)


def _cell_pair(ctx: capi.Context, device: torch.device, *k) -> tuple:
    """Two float64 [*k, n_cells] results on the context's GPU."""
    return tuple(torch.empty((*k, ctx.n_cells), dtype=torch.float64, device=device) for _ in range(2))


def _frames(ctx: capi.Context, device: torch.device, *k) -> torch.Tensor:
    """A float32 [*k, local_rows, res_x, 2] result on the context's GPU."""
    return torch.empty((*k, ctx.local_rows, ctx.res_x, 2), dtype=torch.float32, device=device)


class _Scalars:
    """The scalars one forward uploaded (float64: numpy arrays on the host, or torch tensors on the context's GPU); the
    context's scalars_owner while they are the ones it holds."""
    __slots__ = ("alpha", "q")

    def __init__(self, alpha, q):
        self.alpha, self.q = alpha, q


def _scalars_of(ctx: capi.Context, alpha: torch.Tensor, q: torch.Tensor) -> _Scalars:
    """alpha and q as the context takes them: float64 on its GPU when they are there, else numpy arrays on the host.  A copy
    of their own either way: the caller may change alpha and q in place before a backward."""
    if alpha.shape != (ctx.n_cells,) or q.shape != (ctx.n_cells,):
        raise ValueError(f"alpha and q must hold one value per cell ({ctx.n_cells})")
    if all(t.is_cuda and t.device.index == ctx.device for t in (alpha, q)):
        return _Scalars(*(t.detach().to(dtype=torch.float64, copy=True).contiguous() for t in (alpha, q)))
    return _Scalars(*(t.detach().to("cpu", torch.float64).contiguous().numpy().copy() for t in (alpha, q)))


def _upload(ctx: capi.Context, owner: _Scalars) -> None:
    if isinstance(owner.alpha, torch.Tensor):
        with _on_gpu(ctx) as device:
            _use_torch_stream(ctx, device)
            ctx.update_scalars_device(owner.alpha, owner.q)
    else:
        ctx.update_scalars(owner.alpha, owner.q)
    ctx.scalars_owner = owner


def _current(fctx, what: str) -> capi.Context:
    """The context of fctx, holding the scalars of fctx's forward again; raises if it no longer renders that frame."""
    ctx: capi.Context = fctx.c5
    if ctx.frame_state != fctx.state:
        raise RuntimeError("course5_amd.autograd.render: the context's view, image, rows, solids, alpha limit or grid "
                           f"changed since the forward pass; render again before calling {what}")
    if ctx.scalars_owner is not fctx.owner:
        _upload(ctx, fctx.owner)
    return ctx


def _differentiating_levels() -> int:
    """torch.func transforms that differentiate (grad / vjp, jvp) around the current call."""
    from torch._C._functorch import TransformType
    from torch._functorch.pyfunctorch import retrieve_all_functorch_interpreters
    return sum(i.key() in (TransformType.Grad, TransformType.Jvp) for i in retrieve_all_functorch_interpreters())


def _first_order(fctx, what: str) -> None:
    # a forward recorded under two differentiating transforms (hessian, jacrev of jacrev, jvp of grad, ...) is being
    # differentiated twice: the derivative renders have no derivatives of their own
    if getattr(fctx, "levels", 0) > 1:
        raise RuntimeError(f"course5_amd.autograd.render: second derivatives are not supported ({what} of a render that is "
                           "itself being differentiated)")


def _no_second(what: str):
    raise RuntimeError(f"course5_amd.autograd.render: second derivatives are not supported (the {what} render has no "
                       "derivative of its own)")


def _unbatched_primals(in_dims) -> None:
    if any(d is not None for d in in_dims):
        raise RuntimeError("course5_amd.autograd.render: vmap over alpha or q themselves (a batch of scalar fields) is not "
                           "supported; batches of tangents or cotangents (jacfwd, jacrev, vmap over jvp / vjp) are")


def _tangent_arg(t, device: torch.device):
    return None if t is None else _plain(t).detach().to(device=device, dtype=torch.float64).contiguous()


class _Operator(torch.autograd.Function):
    """A derivative render of the frame of `fr` (the forward's autograd context, the first argument) as a Function of its
    own, so that torch.func can batch it (vmap); the primals after `fr` only mark what the result depends on.  It has no
    derivative: backward and jvp refuse, naming the render (`what`).  A subclass gives what, forward and vmap."""
    what = ""

    @staticmethod
    def setup_context(fctx, inputs, output):
        pass

    @classmethod
    def backward(cls, fctx, *grads):
        _no_second(cls.what)

    @classmethod
    def jvp(cls, fctx, *tangents):
        _no_second(cls.what)


class _Tangent(_Operator):
    """J v: the tangent render of the frame of `fr` (the forward's autograd context); alpha and q only mark what the
    result depends on.  Batched under vmap."""
    what = "tangent"

    @staticmethod
    def forward(fr, alpha, q, alpha_t, q_t):
        ctx = _current(fr, "jvp")
        with _on_gpu(ctx, unwrapped=True) as device:
            da, dq = _tangent_arg(alpha_t, device), _tangent_arg(q_t, device)
            out = _frames(ctx, device)
            _launch(ctx, device, lambda: ctx.render_tangent_device(da, dq, out))
        return out

    @staticmethod
    def vmap(info, in_dims, fr, alpha, q, alpha_t, q_t):
        _unbatched_primals(in_dims[1:3])
        ctx = _current(fr, "jvp")
        k = info.batch_size
        with _on_gpu(ctx, unwrapped=True) as device:
            da, dq = (None if t is None else _lift(t, d, k).to(device=device, dtype=torch.float64).contiguous()
                      for t, d in ((alpha_t, in_dims[3]), (q_t, in_dims[4])))
            out = _frames(ctx, device, k)
            _launch(ctx, device, lambda: ctx.render_tangent_batch_device(da, dq, out, n=k))
        return out, 0


def _adjoint(ctx: capi.Context, g: torch.Tensor, device: torch.device) -> tuple:
    """(grad_alpha, grad_q), float64 [n_cells] each on the context's GPU: the adjoint render for the upstream image g
    (float32, contiguous, there), on torch's current stream."""
    ga, gq = _cell_pair(ctx, device)
    _launch(ctx, device, lambda: ctx.render_adjoint_device(g, ga, gq))
    return ga, gq


class _Adjoint(_Operator):
    """J^T g: the adjoint render of the frame of `fr`; (grad_alpha, grad_q) float64 on the context's GPU.  Batched under
    vmap."""
    what = "adjoint"

    @staticmethod
    def forward(fr, alpha, q, grad_img):
        ctx = _current(fr, "backward")
        with _on_gpu(ctx, unwrapped=True) as device:
            return _adjoint(ctx, _plain(grad_img).detach().to(device=device, dtype=torch.float32).contiguous(), device)

    @staticmethod
    def vmap(info, in_dims, fr, alpha, q, grad_img):
        _unbatched_primals(in_dims[1:3])
        ctx = _current(fr, "backward")
        with _on_gpu(ctx, unwrapped=True) as device:
            g = _lift(grad_img, in_dims[3], info.batch_size).to(device=device, dtype=torch.float32).contiguous()
            k = g.shape[0]
            ga, gq = _cell_pair(ctx, device, k)
            _launch(ctx, device, lambda: ctx.render_adjoint_batch_device(g, ga, gq, n=k))
        return (ga, gq), (0, 0)


def _scalar_grads(fctx, ga: torch.Tensor, gq: torch.Tensor, i_alpha: int, i_q: int) -> tuple:
    """The adjoint's (ga, gq) in the dtype and on the device of alpha and q; None for the one needs_input_grad (at i_alpha,
    i_q) does not ask for."""
    return tuple(g.to(device=dev, dtype=dtype) if fctx.needs_input_grad[i] else None
                 for g, (dtype, dev), i in zip((ga, gq), fctx.meta, (i_alpha, i_q)))


def _tangent_sum(fctx, alpha, q, alpha_t, q_t, other):
    """The scalar tangent's image when alpha or q carry a tangent, plus other() (the image of another input's tangent) when
    there is one, added in float32; None when there is neither."""
    out = _Tangent.apply(fctx, alpha, q, alpha_t, q_t) if alpha_t is not None or q_t is not None else None
    if other is not None:
        t = other()
        out = t if out is None else out + t
    return out


class _Render(torch.autograd.Function):
    @staticmethod
    def forward(ctx: capi.Context, alpha: torch.Tensor, q: torch.Tensor):
        owner = _scalars_of(ctx, alpha, q)
        with _on_gpu(ctx) as device:
            _upload(ctx, owner)  # (setup_context takes it from the context's scalars_owner)
            out = _frames(ctx, device)
            _launch(ctx, device, lambda: ctx.render_device(out.data_ptr()))
        return out

    @staticmethod
    def setup_context(fctx, inputs, output):
        ctx, alpha, q = inputs
        fctx.c5 = ctx
        fctx.state = ctx.frame_state
        fctx.owner = ctx.scalars_owner  # (forward has just set it)
        fctx.meta = ((alpha.dtype, alpha.device), (q.dtype, q.device))
        fctx.primals = (alpha, q)
        fctx.levels = _differentiating_levels()

    @staticmethod
    def backward(fctx, grad_img: torch.Tensor):
        _first_order(fctx, "backward")
        alpha, q = fctx.primals
        return (None, *_scalar_grads(fctx, *_Adjoint.apply(fctx, alpha, q, grad_img), 1, 2))

    @staticmethod
    def jvp(fctx, _ctx_tangent, alpha_t, q_t):
        _current(fctx, "jvp")
        _first_order(fctx, "jvp")
        alpha, q = getattr(fctx, "primals", (None, None))
        return _Tangent.apply(fctx, alpha, q, alpha_t, q_t)

    @staticmethod
    def vmap(info, in_dims, ctx, alpha, q):
        # jacfwd and vmap over jvp batch the tangents only: the frame itself is rendered once
        _unbatched_primals(in_dims[1:])
        return _Render.apply(ctx, alpha, q), None


def render(ctx: capi.Context, alpha: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """The frame of `ctx` with the cells' scalars alpha (AbsorpCoef) and q (radEnLooseRate), differentiable in both.
    Second derivatives of it raise; the Hessian-vector product in (alpha, q) is hvp(), an operator of its own."""
    return _Render.apply(ctx, alpha, q)


# ---- the view's angles as an input ------------------------------------------------------------------------------------

def _set_angles(ctx: capi.Context, angles: torch.Tensor) -> None:
    a = _plain(angles).detach().to("cpu", torch.float64).reshape(-1).numpy()
    if a.shape != (len(ctx.rots),):
        raise ValueError(f"angles must hold one value per rotation of the context's view ({len(ctx.rots)})")
    rots = ctx.rots.copy()
    rots[:, 1] = a
    ctx.set_view(rots)


def _motion(ctx: capi.Context, fields, device: torch.device) -> torch.Tensor:
    """[K, local_rows, res_x, 2] float32 on the context's GPU: the motion tangent render for fields [K, 12] (numpy)."""
    with _on_gpu(ctx, unwrapped=True):
        out = _frames(ctx, device, len(fields))
        _launch(ctx, device, lambda: ctx.render_motion_tangent_device(fields, out))
    return out


class _ViewTangent(_Operator):
    """d img / d angles . t: one motion tangent render for the field sum_i t_i field_i.  Batched under vmap."""
    what = "motion tangent"

    @staticmethod
    def forward(fr, alpha, q, angles, angles_t):
        ctx = _current(fr, "jvp")
        t = _plain(angles_t).detach().to("cpu", torch.float64).reshape(1, -1).numpy()
        return _motion(ctx, t @ ctx.view_fields(), torch.device("cuda", ctx.device))[0]

    @staticmethod
    def vmap(info, in_dims, fr, alpha, q, angles, angles_t):
        _unbatched_primals(in_dims[1:4])
        ctx = _current(fr, "jvp")
        t = _lift(angles_t, in_dims[4], info.batch_size).to("cpu", torch.float64).reshape(info.batch_size, -1).numpy()
        return _motion(ctx, t @ ctx.view_fields(), torch.device("cuda", ctx.device)), 0


class _ViewAdjoint(_Operator):
    """grad_angles[i] = sum g * d img / d angle_i, summed in fp64: one motion tangent render for all the angles.  A batch
    of upstream images (vmap) shares it."""
    what = "motion tangent"

    @staticmethod
    def forward(fr, alpha, q, angles, grad_img):
        ctx = _current(fr, "backward")
        device = torch.device("cuda", ctx.device)
        imgs = _motion(ctx, ctx.view_fields(), device)
        with torch._C._DisableFuncTorch():
            g = _plain(grad_img).detach().to(device=device, dtype=torch.float64)
            return (imgs.to(torch.float64) * g).sum(dim=(1, 2, 3))

    @staticmethod
    def vmap(info, in_dims, fr, alpha, q, angles, grad_img):
        _unbatched_primals(in_dims[1:4])
        ctx = _current(fr, "backward")
        device = torch.device("cuda", ctx.device)
        imgs = _motion(ctx, ctx.view_fields(), device)
        with torch._C._DisableFuncTorch():
            g = _lift(grad_img, in_dims[4], info.batch_size).to(device=device, dtype=torch.float64)
            return torch.einsum("kyxc,nyxc->kn", g, imgs.to(torch.float64)), 0


class _RenderView(torch.autograd.Function):
    @staticmethod
    def forward(ctx: capi.Context, alpha: torch.Tensor, q: torch.Tensor, angles: torch.Tensor):
        _set_angles(ctx, angles)
        return _Render.forward(ctx, alpha, q)

    @staticmethod
    def setup_context(fctx, inputs, output):
        ctx, alpha, q, angles = inputs
        _Render.setup_context(fctx, (ctx, alpha, q), output)
        fctx.primals = (alpha, q, angles)
        fctx.angles_meta = (angles.dtype, angles.device)

    @staticmethod
    def backward(fctx, grad_img: torch.Tensor):
        _first_order(fctx, "backward")
        alpha, q, angles = fctx.primals
        ga_out = gq_out = gv_out = None
        if fctx.needs_input_grad[1] or fctx.needs_input_grad[2]:
            ga_out, gq_out = _scalar_grads(fctx, *_Adjoint.apply(fctx, alpha, q, grad_img), 1, 2)
        if fctx.needs_input_grad[3]:
            dtype, dev = fctx.angles_meta
            gv_out = _ViewAdjoint.apply(fctx, alpha, q, angles, grad_img).to(device=dev, dtype=dtype)
        return None, ga_out, gq_out, gv_out

    @staticmethod
    def jvp(fctx, _ctx_tangent, alpha_t, q_t, angles_t):
        _current(fctx, "jvp")
        _first_order(fctx, "jvp")
        alpha, q, angles = getattr(fctx, "primals", (None, None, None))
        return _tangent_sum(fctx, alpha, q, alpha_t, q_t,
                            None if angles_t is None else lambda: _ViewTangent.apply(fctx, alpha, q, angles, angles_t))

    @staticmethod
    def vmap(info, in_dims, ctx, alpha, q, angles):
        _unbatched_primals(in_dims[1:])
        return _RenderView.apply(ctx, alpha, q, angles), None


def render_view(ctx: capi.Context, alpha: torch.Tensor, q: torch.Tensor, angles: torch.Tensor) -> torch.Tensor:
    """The frame of `ctx` with the scalars alpha and q and the view's angles `angles` ([n_rots] radians, written into the
    context's current rotation list; axes and x0 are kept), differentiable in all three."""
    return _RenderView.apply(ctx, alpha, q, angles)


# ---- the grid's points as an input -------------------------------------------------------------------------------------

def _set_points(ctx: capi.Context, xyz: torch.Tensor) -> None:
    p = _plain(xyz).detach().to("cpu", torch.float64).contiguous().numpy()
    if p.shape != (ctx.n_pts, 3):
        raise ValueError(f"xyz must hold the grid's points, [{ctx.n_pts}, 3]")
    if not np.array_equal(p, ctx.points):
        ctx.update_points(p)


def _vertex_adjoint(ctx: capi.Context, g: torch.Tensor, device: torch.device) -> torch.Tensor:
    """[n_pts, 3] float64 on the context's GPU: the vertex adjoint render for the upstream image g (float32, there)."""
    out = torch.empty((ctx.n_pts, 3), dtype=torch.float64, device=device)
    _launch(ctx, device, lambda: ctx.render_vertex_adjoint_device(g, out))
    return out


def _vertex_adjoint_batch(ctx: capi.Context, g: torch.Tensor, device: torch.device) -> torch.Tensor:
    """[K, n_pts, 3] float64 on the context's GPU: the batched vertex adjoint render for the upstream images g
    ([K, local_rows, res_x, 2] float32, contiguous, there)."""
    k = g.shape[0]
    out = torch.empty((k, ctx.n_pts, 3), dtype=torch.float64, device=device)
    _launch(ctx, device, lambda: ctx.render_vertex_adjoint_batch_device(g, out, n=k))
    return out


class _VertexAdjoint(_Operator):
    """d loss / d xyz: the vertex adjoint render of the frame of `fr`, float64 [n_pts, 3] on the context's GPU.  A batch of
    upstream images (vmap) is one batched call: [K, n_pts, 3]."""
    what = "vertex adjoint"

    @staticmethod
    def forward(fr, xyz, grad_img):
        ctx = _current(fr, "backward")
        with _on_gpu(ctx, unwrapped=True) as device:
            g = _plain(grad_img).detach().to(device=device, dtype=torch.float32).contiguous()
            return _vertex_adjoint(ctx, g, device)

    @staticmethod
    def vmap(info, in_dims, fr, xyz, grad_img):
        _unbatched_primals(in_dims[1:2])
        ctx = _current(fr, "backward")
        with _on_gpu(ctx, unwrapped=True) as device:
            g = _lift(grad_img, in_dims[2], info.batch_size).to(device=device, dtype=torch.float32).contiguous()
            return _vertex_adjoint_batch(ctx, g, device), 0


def _vertex_tangent(ctx: capi.Context, d: torch.Tensor, device: torch.device) -> torch.Tensor:
    """[K, local_rows, res_x, 2] float32 on the context's GPU: the vertex tangent render for the displacement fields d
    ([K, n_pts, 3] float64, contiguous, there)."""
    k = d.shape[0]
    out = _frames(ctx, device, k)
    _launch(ctx, device, lambda: ctx.render_vertex_tangent_device(d, out, n=k))
    return out


class _VertexTangent(_Operator):
    """d img / d xyz . t: one vertex tangent render of the frame of `fr`.  Batched under vmap."""
    what = "vertex tangent"

    @staticmethod
    def forward(fr, xyz, xyz_t):
        ctx = _current(fr, "jvp")
        with _on_gpu(ctx, unwrapped=True) as device:
            d = _tangent_arg(xyz_t, device).reshape(1, ctx.n_pts, 3)
            return _vertex_tangent(ctx, d, device)[0]

    @staticmethod
    def vmap(info, in_dims, fr, xyz, xyz_t):
        _unbatched_primals(in_dims[1:2])
        ctx = _current(fr, "jvp")
        k = info.batch_size
        with _on_gpu(ctx, unwrapped=True) as device:
            d = _lift(xyz_t, in_dims[2], k).to(device=device, dtype=torch.float64).reshape(k, ctx.n_pts, 3).contiguous()
            return _vertex_tangent(ctx, d, device), 0


class _RenderMesh(torch.autograd.Function):
    @staticmethod
    def forward(ctx: capi.Context, xyz: torch.Tensor, alpha: torch.Tensor, q: torch.Tensor):
        _set_points(ctx, xyz)
        return _Render.forward(ctx, alpha, q)

    @staticmethod
    def setup_context(fctx, inputs, output):
        ctx, xyz, alpha, q = inputs
        _Render.setup_context(fctx, (ctx, alpha, q), output)
        fctx.primals = (xyz, alpha, q)
        fctx.xyz_meta = (xyz.dtype, xyz.device)

    @staticmethod
    def backward(fctx, grad_img: torch.Tensor):
        _first_order(fctx, "backward")
        xyz, alpha, q = fctx.primals
        gx_out = ga_out = gq_out = None
        if fctx.needs_input_grad[1]:
            dtype, dev = fctx.xyz_meta
            gx_out = _VertexAdjoint.apply(fctx, xyz, grad_img).to(device=dev, dtype=dtype)
        if fctx.needs_input_grad[2] or fctx.needs_input_grad[3]:
            ga_out, gq_out = _scalar_grads(fctx, *_Adjoint.apply(fctx, alpha, q, grad_img), 2, 3)
        return None, gx_out, ga_out, gq_out

    @staticmethod
    def jvp(fctx, _ctx_tangent, xyz_t, alpha_t, q_t):
        _current(fctx, "jvp")
        _first_order(fctx, "jvp")
        # (torch.func hands every input a tangent, zeros for the ones it does not differentiate: J 0 = 0 needs no render)
        if xyz_t is not None and bool((_plain(xyz_t) != 0).any()):
            raise RuntimeError("course5_amd.autograd.render_mesh: forward mode in the points is not supported (there is no "
                               "per-vertex tangent render); use backward / vjp for xyz, or render_view for a rigid motion")
        xyz, alpha, q = getattr(fctx, "primals", (None, None, None))
        return _tangent_sum(fctx, alpha, q, alpha_t, q_t, None)

    @staticmethod
    def vmap(info, in_dims, ctx, xyz, alpha, q):
        _unbatched_primals(in_dims[1:])
        return _RenderMesh.apply(ctx, xyz, alpha, q), None


class _RenderMeshForward(_RenderMesh):
    """_RenderMesh with forward mode in the points: a tangent on xyz goes to one vertex tangent render."""

    @staticmethod
    def jvp(fctx, _ctx_tangent, xyz_t, alpha_t, q_t):
        _current(fctx, "jvp")
        _first_order(fctx, "jvp")
        xyz, alpha, q = getattr(fctx, "primals", (None, None, None))
        # (torch.func hands every input a tangent, zeros for the ones it does not differentiate: J 0 = 0 needs no render)
        moved = xyz_t is not None and bool((_plain(xyz_t) != 0).any())
        return _tangent_sum(fctx, alpha, q, alpha_t, q_t, (lambda: _VertexTangent.apply(fctx, xyz, xyz_t)) if moved else None)

    @staticmethod
    def vmap(info, in_dims, ctx, xyz, alpha, q):
        _unbatched_primals(in_dims[1:])
        return _RenderMeshForward.apply(ctx, xyz, alpha, q), None


def render_mesh(ctx: capi.Context, xyz: torch.Tensor, alpha: torch.Tensor, q: torch.Tensor, forward_xyz: bool = False) -> torch.Tensor:
    """The frame of `ctx` with the grid's points xyz ([n_pts, 3], the order and coordinates of upload_grid; sent to the
    context when they differ from the ones it holds) and the scalars alpha and q, differentiable in all three.  Reverse
    mode in xyz is one vertex adjoint render per backward (under vmap, one batched render for all the cotangents); second
    derivatives raise.  With ctx.set_option("vertex_exact", 1) the calls the backward and its vmap rule make return the exact
    vertex adjoint sums: the gradient in xyz is the same bits every run, under either cell order, and a batch's slices are
    the single calls' (no function of its own: the option is the library's).
    forward_xyz False (the default): forward mode in xyz raises, as it always has - callers and a test rely on that
    refusal, which is why forward mode is a switch and not the new default.  forward_xyz True: a tangent on xyz
    (torch.func.jvp, forward_ad, jacfwd) goes to ONE vertex tangent render, batched under vmap, and is added to the scalar
    tangent's image when alpha or q carry tangents too."""
    return (_RenderMeshForward if forward_xyz else _RenderMesh).apply(ctx, xyz, alpha, q)


# ---- Gauss-Newton operators ------------------------------------------------------------------------------------------
# H v = J^T W J v and diag(J^T W J) of the frame with the scalars (alpha, q): what a Gauss-Newton / CG fit calls in its
# inner loop (course5_amd.fit).  Operators, not differentiable functions: the results carry no graph.

def _gn_enter(ctx: capi.Context, alpha: torch.Tensor, q: torch.Tensor, what: str) -> torch.device:
    if _differentiating_levels():
        raise RuntimeError(f"course5_amd.autograd.{what}: it is an operator with no derivative of its own (second derivatives "
                           "are not supported); call it outside torch.func.grad / vjp / jvp")
    _upload(ctx, _scalars_of(ctx, _plain(alpha), _plain(q)))
    return torch.device("cuda", ctx.device)


def _gn_weight(ctx: capi.Context, weight, device: torch.device):
    if weight is None:
        return None
    w = _plain(weight).detach().to(device=device, dtype=torch.float32).contiguous()
    if tuple(w.shape) != (ctx.local_rows, ctx.res_x, 2):
        raise ValueError(f"weight must be [{ctx.local_rows}, {ctx.res_x}, 2], not {list(w.shape)}")
    return w


def gn_product(ctx: capi.Context, alpha: torch.Tensor, q: torch.Tensor, v_alpha, v_q, weight=None) -> tuple:
    """(h_alpha, h_q) = J^T W J (v_alpha, v_q) for the frame of `ctx` with the scalars alpha and q: v_alpha / v_q [n_cells]
    or [K, n_cells] (either may be None: zero), weight [local_rows, res_x, 2] (None: ones).  float64 on the context's GPU,
    shaped like the directions.  One library call (c5_render_gn_product_device) on torch's current stream.  With
    ctx.set_option("exact_sums", 1) the sums are exact: the same bits every call, those of the exact adjoint of
    weight * fp32(J v)."""
    device = _gn_enter(ctx, alpha, q, "gn_product")
    given = [v for v in (v_alpha, v_q) if v is not None]
    if not given or any(v.shape != given[0].shape for v in given) or given[0].ndim not in (1, 2) or given[0].shape[-1] != ctx.n_cells:
        raise ValueError(f"v_alpha and / or v_q must be [{ctx.n_cells}] or [K, {ctx.n_cells}], of one shape")
    single = given[0].ndim == 1
    with _on_gpu(ctx):
        va, vq = (None if v is None else _plain(v).detach().to(device=device, dtype=torch.float64).reshape(-1, ctx.n_cells).contiguous()
                  for v in (v_alpha, v_q))
        w = _gn_weight(ctx, weight, device)
        k = (va if va is not None else vq).shape[0]
        ha, hq = _cell_pair(ctx, device, k)
        _launch(ctx, device, lambda: ctx.render_gn_product_device(va, vq, w, ha, hq, None, n=k))
    return (ha[0], hq[0]) if single else (ha, hq)


def _vertex_gn_product(ctx: capi.Context, v: torch.Tensor, w, device: torch.device) -> torch.Tensor:
    """vertex_gn_product's library call for the scalars the context holds: v float64 [K, n_pts, 3] contiguous, w float32
    [local_rows, res_x, 2] or None, both on `device` -> float64 [K, n_pts, 3]."""
    k = v.shape[0]
    h = torch.empty((k, ctx.n_pts, 3), dtype=torch.float64, device=device)
    _launch(ctx, device, lambda: ctx.render_vertex_gn_product_device(v, w, h, None, n=k))
    return h


def vertex_gn_product(ctx: capi.Context, alpha: torch.Tensor, q: torch.Tensor, v_xyz: torch.Tensor, weight=None) -> torch.Tensor:
    """h_xyz = J^T W J v_xyz for the frame of `ctx` with the scalars alpha and q and the points the context holds, J the
    Jacobian of the frame with respect to those points (render_mesh's derivative in xyz): v_xyz [n_pts, 3] or [K, n_pts, 3]
    (the rows of points welded to another are not read), weight [local_rows, res_x, 2] (None: ones).  float64 on the
    context's GPU, shaped like v_xyz, zero on points welded to another.  One library call
    (c5_render_vertex_gn_product_device) on torch's current stream for what render_mesh's jvp, a multiply and its vjp take
    two renders for.  With ctx.set_option("vertex_exact", 1) the sums are exact: the same bits every call, those of the
    exact vertex adjoint of weight * fp32(J v)."""
    device = _gn_enter(ctx, alpha, q, "vertex_gn_product")
    if v_xyz is None or v_xyz.ndim not in (2, 3) or tuple(v_xyz.shape[-2:]) != (ctx.n_pts, 3) or v_xyz.shape[0] == 0:
        raise ValueError(f"v_xyz must be [{ctx.n_pts}, 3] or [K, {ctx.n_pts}, 3]")
    single = v_xyz.ndim == 2
    with _on_gpu(ctx):
        v = _plain(v_xyz).detach().to(device=device, dtype=torch.float64).reshape(-1, ctx.n_pts, 3).contiguous()
        h = _vertex_gn_product(ctx, v, _gn_weight(ctx, weight, device), device)
    return h[0] if single else h


def gn_diagonal(ctx: capi.Context, alpha: torch.Tensor, q: torch.Tensor, weight=None) -> tuple:
    """(d_alpha, d_q) = diag(J^T W J), float64 [n_cells] each on the context's GPU (c5_render_gn_diagonal_device on
    torch's current stream).  With ctx.set_option("exact_sums", 1) the sums are exact: the same bits every call."""
    device = _gn_enter(ctx, alpha, q, "gn_diagonal")
    with _on_gpu(ctx):
        w = _gn_weight(ctx, weight, device)
        da, dq = _cell_pair(ctx, device)
        _launch(ctx, device, lambda: ctx.render_gn_diagonal_device(w, da, dq))
    return da, dq


def hvp(ctx: capi.Context, alpha: torch.Tensor, q: torch.Tensor, v_alpha, v_q, grad_img) -> tuple:
    """(h_alpha, h_q) = Hess(phi) (v_alpha, v_q), phi = sum_p grad_img_p . img_p, for the frame of `ctx` with the scalars
    alpha and q: the exact second derivative of the frame in the cells' scalars, weighted by the upstream image grad_img
    [local_rows, res_x, 2] and applied to the direction v_alpha / v_q [n_cells] (either may be None: zero).  Channel 0 of
    grad_img has no effect (tau is linear in alpha).  float64 [n_cells] each on the context's GPU, no graph.  One library
    call (c5_render_hvp_device) on torch's current stream.  With ctx.set_option("exact_sums", 1) the sums are exact: the
    same bits every call."""
    device = _gn_enter(ctx, alpha, q, "hvp")
    given = [v for v in (v_alpha, v_q) if v is not None]
    if not given or any(tuple(v.shape) != (ctx.n_cells,) for v in given):
        raise ValueError(f"v_alpha and / or v_q must be [{ctx.n_cells}]")
    with _on_gpu(ctx):
        va, vq = (None if v is None else _plain(v).detach().to(device=device, dtype=torch.float64).contiguous() for v in (v_alpha, v_q))
        g = _plain(grad_img).detach().to(device=device, dtype=torch.float32).contiguous()
        if tuple(g.shape) != (ctx.local_rows, ctx.res_x, 2):
            raise ValueError(f"grad_img must be [{ctx.local_rows}, {ctx.res_x}, 2], not {list(g.shape)}")
        ha, hq = _cell_pair(ctx, device)
        _launch(ctx, device, lambda: ctx.render_hvp_device(va, vq, g, ha, hq))
    return ha, hq


def _ray_rows(ctx: capi.Context, device: torch.device) -> tuple:
    """What every export starts with: (crow int64 [local_px + 1] on `device`, nnz, the length to allocate for the arrays of
    its fill: an empty torch tensor has no data pointer to hand over) - c5_ray_matrix_rows_device on torch's current stream."""
    crow = torch.empty(ctx.local_rows * ctx.res_x + 1, dtype=torch.int64, device=device)
    _use_torch_stream(ctx, device)
    nnz = ctx.ray_matrix_rows_device(crow)  # (waits and retries by itself)
    return crow, nnz, max(nnz, 1)


def ray_matrix(ctx: capi.Context, with_depth: bool = False):
    """The ray matrix A of the frame `ctx` would render now: a torch.sparse_csr_tensor [local_rows * res_x, n_cells],
    float64, on the context's GPU, A[pixel, cell] = the chord of the pixel's ray through the cell (rows: local pixels lrow *
    res_x + col; columns: cells in the order of upload_grid; within a row the deepest segment first).  A @ alpha is channel
    0 of render() (tau) in fp64, and A.T @ g is render_adjoint's grad_alpha for the upstream image (g, 0).  Channel 1 is
    not linear in alpha: ray_jacobian gives its derivatives.  Indices are int32 while nnz < 2^31, else int64.  with_depth: (A, z_exit),
    z_exit float64 [nnz]: every segment's far end in view space, in the order of A.values().  Built on torch's current
    stream (c5_ray_matrix_rows_device, c5_ray_matrix_fill_device) and waited for; no graph: A does not depend on the
    scalars.  Bit-reproducible."""
    n_px = ctx.local_rows * ctx.res_x
    with _on_gpu(ctx) as device:
        crow, nnz, n = _ray_rows(ctx, device)
        col = torch.empty(n, dtype=torch.int32, device=device)
        dz = torch.empty(n, dtype=torch.float64, device=device)
        z_exit = torch.empty(n, dtype=torch.float64, device=device) if with_depth else None
        _run(ctx, lambda: ctx.ray_matrix_fill_device(crow, col, dz, z_exit))
        if nnz < 2 ** 31:
            crow = crow.to(torch.int32)
        else:
            col = col.to(torch.int64)
        A = torch.sparse_csr_tensor(crow, col[:nnz], dz[:nnz], size=(n_px, ctx.n_cells))
    return (A, z_exit[:nnz]) if with_depth else A


def _ray_jacobian_arrays(ctx: capi.Context, device: torch.device) -> tuple:
    """(crow int64 [local_px + 1], col int32 [nnz], dz, dI_dalpha, dI_dq float64 [nnz]) on `device`, for the scalars the
    context holds: c5_ray_matrix_rows_device and c5_ray_jacobian_fill_device on torch's current stream, waited for."""
    crow, nnz, n = _ray_rows(ctx, device)
    col = torch.empty(n, dtype=torch.int32, device=device)
    dz, da, dq = (torch.empty(n, dtype=torch.float64, device=device) for _ in range(3))
    _run(ctx, lambda: ctx.ray_jacobian_fill_device(crow, col, dz, da, dq))
    return crow, col[:nnz], dz[:nnz], da[:nnz], dq[:nnz]


def ray_jacobian(ctx: capi.Context, alpha=None, q=None) -> tuple:
    """(A, J_alpha, J_q): the Jacobian of the frame `ctx` would render now with respect to the cells' scalars, as three
    torch.sparse_csr_tensor [local_rows * res_x, n_cells], float64, on the context's GPU: A[pixel, cell] = d tau / d alpha
    (ray_matrix's A, bit for bit), J_alpha[pixel, cell] = d I / d alpha, J_q[pixel, cell] = d I / d Q (rows: local pixels
    lrow * res_x + col; columns: cells in the order of upload_grid; within a row the deepest segment first; explicit zeros
    where a cell is inactive, and in J_alpha where its alpha is clamped).  The three share one crow_indices / col_indices
    storage; indices are int32 while nnz < 2^31, else int64.  alpha and q: the scalars to differentiate at (both or
    neither; None: those the context holds).  Built on torch's current stream (c5_ray_matrix_rows_device,
    c5_ray_jacobian_fill_device) and waited for; the results carry no graph.  Bit-reproducible."""
    if (alpha is None) != (q is None):
        raise ValueError("give both alpha and q, or neither")
    if alpha is not None:
        _gn_enter(ctx, alpha, q, "ray_jacobian")
    with _on_gpu(ctx) as device:
        crow, col, dz, da, dq = _ray_jacobian_arrays(ctx, device)
        if dz.shape[0] < 2 ** 31:
            crow = crow.to(torch.int32)
        else:
            col = col.to(torch.int64)
        size = (ctx.local_rows * ctx.res_x, ctx.n_cells)
        # (check_invariants off: one storage, not three validated copies)
        return tuple(torch.sparse_csr_tensor(crow, col, v, size=size, check_invariants=False) for v in (dz, da, dq))


def _ray_shape_jacobian_arrays(ctx: capi.Context, device: torch.device) -> tuple:
    """(crow int64 [local_px + 1], col int32 [nnz], dI_ddz float64 [nnz], faces uint8 [nnz], bary float64 [nnz, 2, 3],
    face_points int32 [n_cells, 4, 3], dw_dxyz float64 [n_cells, 4, 3]) on `device`, for the scalars, points and view the
    context holds: c5_ray_matrix_rows_device, c5_ray_matrix_fill_device, c5_ray_shape_jacobian_fill_device and
    c5_face_gradients_device on torch's current stream, waited for."""
    crow, nnz, n = _ray_rows(ctx, device)
    col = torch.zeros(n, dtype=torch.int32, device=device)
    dz, dI = (torch.empty(n, dtype=torch.float64, device=device) for _ in range(2))
    faces = torch.zeros(n, dtype=torch.uint8, device=device)
    bary = torch.zeros((n, 2, 3), dtype=torch.float64, device=device)
    fp = torch.zeros((max(ctx.n_cells, 1), 4, 3), dtype=torch.int32, device=device)
    dw = torch.zeros((max(ctx.n_cells, 1), 4, 3), dtype=torch.float64, device=device)
    _run(ctx, lambda: ctx.ray_matrix_fill_device(crow, col, dz))
    _run(ctx, lambda: ctx.ray_shape_jacobian_device(crow, dI, faces, bary))
    if ctx.n_cells > 0:
        _run(ctx, lambda: ctx.face_gradients_device(fp, dw))
    return crow, col[:nnz], dI[:nnz], faces[:nnz], bary[:nnz], fp[:ctx.n_cells], dw[:ctx.n_cells]


def assemble_shape_jacobian(row_ptr, col, alpha, dI_ddz, faces, bary, face_points, dw_dxyz, n_pts: int) -> tuple:
    """The shape Jacobian's per-segment arrays (capi.Context.ray_shape_jacobian) as ONE coalesced CSR structure with two
    value arrays: (crow int64 [n_px + 1], cols int64 [nnz_J], v_tau, v_I float64 [nnz_J]) with
        d tau[p] / d xyz[v][j] = v_tau at (row p, column 3 v + j),     d I[p] / d xyz[v][j] = v_I there.
    Torch ops on the arrays' device (the CPU included).  A segment expands to up to 18 entries - two faces, three vertices,
    three coordinates, + at the exit face and - at the entry face, a face whose bit is clear none; entries of the same
    (pixel, column) are added in the order of the segments (a stable sort by the key): the same bits every call.  alpha:
    the cells' raw alpha [n_cells] (d tau / d dz), in the order of upload_grid."""
    row_ptr = torch.as_tensor(row_ptr).to(torch.int64)
    dev = row_ptr.device
    n_px, n_col = row_ptr.shape[0] - 1, 3 * int(n_pts)
    col = torch.as_tensor(col).to(device=dev, dtype=torch.int64)
    faces = torch.as_tensor(faces).to(device=dev, dtype=torch.int64)
    f64 = lambda t: torch.as_tensor(t).detach().to(device=dev, dtype=torch.float64)  # noqa: E731
    alpha, dI, bary, dw = f64(alpha), f64(dI_ddz), f64(bary).reshape(-1, 2, 3), f64(dw_dxyz).reshape(-1, 4, 3)
    fpts = torch.as_tensor(face_points).to(device=dev, dtype=torch.int64).reshape(-1, 4, 3)
    nnz = col.shape[0]
    if not (dI.shape[0] == faces.shape[0] == bary.shape[0] == nnz == int(row_ptr[-1])):
        raise ValueError(f"col, dI_ddz, faces and bary must hold row_ptr's {int(row_ptr[-1])} elements each")
    row = torch.repeat_interleave(torch.arange(n_px, device=dev), row_ptr[1:] - row_ptr[:-1])
    f = torch.stack([faces & 3, (faces >> 2) & 3], 1)                      # [nnz, 2]: exit, entry
    on = torch.stack([(faces >> 4) & 1, (faces >> 5) & 1], 1).to(torch.bool)
    c2 = col[:, None].expand(-1, 2)
    pts = fpts[c2, f]                                                       # [nnz, 2, 3 (vertex)]
    g = dw[c2, f]                                                           # [nnz, 2, 3 (coordinate)]
    sign = torch.tensor([1.0, -1.0], dtype=torch.float64, device=dev)
    coef = bary * sign[None, :, None]
    vals = coef[:, :, :, None] * g[:, :, None, :]                           # [nnz, 2, 3, 3]
    cols = 3 * pts[:, :, :, None] + torch.arange(3, device=dev)
    keep = on[:, :, None, None].expand(-1, -1, 3, 3).reshape(-1)
    key = (row[:, None, None, None] * n_col + cols).reshape(-1)[keep]
    seg = torch.arange(nnz, device=dev)[:, None, None, None].expand(-1, 2, 3, 3).reshape(-1)[keep]
    vals = vals.reshape(-1)[keep]
    order = torch.argsort(key, stable=True)
    key, seg, vals = key[order], seg[order], vals[order]
    ukey, counts = torch.unique_consecutive(key, return_counts=True)
    offsets = torch.zeros(ukey.shape[0] + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0)
    if ukey.shape[0]:
        v_tau = torch.segment_reduce(vals * alpha[col[seg]], "sum", offsets=offsets)
        v_I = torch.segment_reduce(vals * dI[seg], "sum", offsets=offsets)
    else:
        v_tau = v_I = torch.zeros(0, dtype=torch.float64, device=dev)
    crow = torch.zeros(n_px + 1, dtype=torch.int64, device=dev)
    crow[1:] = torch.cumsum(torch.bincount(torch.div(ukey, n_col, rounding_mode="floor"), minlength=n_px), 0)
    return crow, ukey % n_col, v_tau, v_I


def ray_shape_jacobian(ctx: capi.Context, alpha: torch.Tensor, q: torch.Tensor) -> tuple:
    """(J_tau, J_I): the Jacobian of the frame `ctx` would render now, with the scalars alpha and q, with respect to the
    points the context holds, as two torch.sparse_csr_tensor [local_rows * res_x, 3 * n_pts], float64, on the context's GPU:
    J_tau[pixel, 3 v + j] = d tau / d xyz[v][j], J_I[pixel, 3 v + j] = d I / d xyz[v][j] (rows: local pixels lrow * res_x +
    col; points in the order of upload_grid; the columns of points welded to another are empty).  Row p is
    render_vertex_adjoint's gradient for the upstream image (1, 0) / (0, 1) at p, and J @ d_xyz.reshape(-1) is
    render_vertex_tangent's image in fp64.  The two share one crow_indices / col_indices storage.  Built from the
    library's per-segment arrays (c5_ray_matrix_*, c5_ray_shape_jacobian_fill_device, c5_face_gradients_device) on
    torch's current stream, waited for, and assembled with torch ops (assemble_shape_jacobian: 18 entries per segment
    before they are coalesced - small and medium frames); no graph.  Bit-reproducible."""
    device = _gn_enter(ctx, alpha, q, "ray_shape_jacobian")
    with _on_gpu(ctx):
        arrays = _ray_shape_jacobian_arrays(ctx, device)
        a = _plain(alpha).detach().to(device=device, dtype=torch.float64)
        crow, cols, v_tau, v_I = assemble_shape_jacobian(arrays[0], arrays[1], a, *arrays[2:], ctx.n_pts)
        size = (ctx.local_rows * ctx.res_x, 3 * ctx.n_pts)
        # (check_invariants off: one storage, not two validated copies)
        return tuple(torch.sparse_csr_tensor(crow, cols, v, size=size, check_invariants=False) for v in (v_tau, v_I))


# ---- the smoothness prior ----------------------------------------------------------------------------------------------
# R(alpha) + R(q) of capi.Prior as a differentiable function of the two fields: the value and the gradient come from ONE
# c5_prior_gradient_device, the second derivative (reverse over reverse, jvp of grad) from ONE c5_prior_product_device.
# The calls are enqueued on torch's current stream.  On a stream of torch's own that orders them with what torch does
# there, before and after, and nothing is waited for.  Torch's DEFAULT stream is the null stream, which the library takes
# for "its own stream" - one the null stream does not synchronise with: there the call is waited for before torch reads
# its outputs (or hands its inputs back to the allocator), as every other operator of this module does (_launch).

def _enqueue(ctx: capi.Context, device: torch.device, enqueue) -> None:
    """enqueue() - library calls that take no per-view setup - on torch's current stream, after what torch has queued
    there; waited for where that is the null stream, left to the stream's order elsewhere."""
    _use_torch_stream(ctx, device)
    if ctx.stream_ptr == 0:
        _run(ctx, enqueue)
    else:
        enqueue()


def _no_prior_vmap():
    raise RuntimeError("course5_amd.autograd.prior: vmap (a batch of fields, tangents or cotangents) is not supported; "
                       "call it once per field")


def _prior_fields(ctx: capi.Context, device: torch.device, *ts) -> tuple:
    out = tuple(None if t is None else _plain(t).detach().to(device=device, dtype=torch.float64).contiguous() for t in ts)
    if any(t is not None and tuple(t.shape) != (ctx.n_cells,) for t in out):
        raise ValueError(f"alpha and q must hold one value per cell ({ctx.n_cells})")
    return out


def _no_prior_third(*_args):
    raise RuntimeError("course5_amd.autograd.prior: derivatives beyond the second are not supported (the prior's Hessian "
                       "product has no derivative of its own)")


class _PriorProduct(_Operator):
    """Hess R(x) v: one c5_prior_product_device at the point `fr` kept.  It has no derivative of its own."""
    what = "smoothness prior's Hessian product"
    backward = staticmethod(_no_prior_third)
    jvp = staticmethod(_no_prior_third)

    @staticmethod
    def forward(fr, alpha, q, v_alpha, v_q):
        ctx: capi.Context = fr.c5
        with _on_gpu(ctx, unwrapped=True) as device:
            va, vq = (torch.zeros(ctx.n_cells, dtype=torch.float64, device=device) if v is None else v
                      for v in _prior_fields(ctx, device, v_alpha, v_q))
            ha, hq = _cell_pair(ctx, device)
            _enqueue(ctx, device, lambda: ctx.prior_product_device(fr.prior, fr.point[0], fr.point[1], va, vq, ha, hq))
        return ha, hq

    @staticmethod
    def vmap(info, in_dims, *args):
        _no_prior_vmap()


class _PriorGradient(torch.autograd.Function):
    """grad R at the point of `fr`, as the forward's call left it (no call of its own); its derivative is _PriorProduct."""

    @staticmethod
    def forward(fr, alpha, q):
        return tuple(g.clone() for g in fr.grads)

    @staticmethod
    def setup_context(fctx, inputs, output):
        fctx.fr, fctx.primals = inputs[0], inputs[1:]
        fctx.meta = inputs[0].meta

    @staticmethod
    def backward(fctx, g_alpha, g_q):
        alpha, q = fctx.primals
        ha, hq = _PriorProduct.apply(fctx.fr, alpha, q, g_alpha, g_q)
        return (None, *_scalar_grads(fctx, ha, hq, 1, 2))

    @staticmethod
    def jvp(fctx, _fr_tangent, alpha_t, q_t):
        alpha, q = fctx.primals
        return _PriorProduct.apply(fctx.fr, alpha, q, alpha_t, q_t)

    @staticmethod
    def vmap(info, in_dims, *args):
        _no_prior_vmap()


class _PriorValue(torch.autograd.Function):
    @staticmethod
    def forward(ctx: capi.Context, alpha: torch.Tensor, q: torch.Tensor, prior: capi.Prior):
        with _on_gpu(ctx, unwrapped=True) as device:
            a, b = _prior_fields(ctx, device, alpha, q)
            value = torch.empty(2, dtype=torch.float64, device=device)
            ga, gq = _cell_pair(ctx, device)
            _enqueue(ctx, device, lambda: ctx.prior_gradient_device(prior, a, b, value, ga, gq))
            ctx.prior_last = ((a, b), (ga, gq))  # (setup_context takes them from here)
            return value[0] + value[1]

    @staticmethod
    def setup_context(fctx, inputs, output):
        ctx, alpha, q, prior = inputs
        fctx.c5, fctx.prior = ctx, prior
        fctx.point, fctx.grads = ctx.prior_last  # (forward has just set it)
        fctx.meta = ((alpha.dtype, alpha.device), (q.dtype, q.device))
        fctx.primals = (alpha, q)

    @staticmethod
    def backward(fctx, g_value: torch.Tensor):
        alpha, q = fctx.primals
        ga, gq = _PriorGradient.apply(fctx, alpha, q)
        ga, gq = _scalar_grads(fctx, ga, gq, 1, 2)
        return (None, None if ga is None else g_value.to(ga.device) * ga, None if gq is None else g_value.to(gq.device) * gq, None)

    @staticmethod
    def jvp(fctx, _ctx_tangent, alpha_t, q_t, _prior_tangent):
        # The value's tangent is grad R . t, with grad R through _PriorGradient: no call of its own, and a derivative of
        # the tangent (torch.func.grad of a jvp, forward_ad under create_graph) finds the Hessian product there.  Forward
        # over forward does not: torch.func drops the outer tangent of what a jvp rule computes from its saved inputs.
        from torch._C._functorch import TransformType
        from torch._functorch.pyfunctorch import retrieve_all_functorch_interpreters
        levels = [i.key() for i in retrieve_all_functorch_interpreters()]
        if sum(k == TransformType.Jvp for k in levels) > 1:
            raise RuntimeError("course5_amd.autograd.prior: torch.func.jvp of a jvp (forward over forward) is not supported; "
                               "take the second derivative as jvp of grad, grad of jvp, or by double backward")
        alpha, q = fctx.primals
        if _differentiating_levels() > 1 or alpha.requires_grad or q.requires_grad:
            ga, gq = _PriorGradient.apply(fctx, alpha, q)
        else:  # (nothing can differentiate the tangent: the gradient as the forward left it)
            ga, gq = fctx.grads
        out = None
        for g, t in ((ga, alpha_t), (gq, q_t)):
            if t is not None:
                term = (g * t.to(device=g.device, dtype=g.dtype)).sum()
                out = term if out is None else out + term
        return out

    @staticmethod
    def vmap(info, in_dims, *args):
        _no_prior_vmap()


def prior(ctx: capi.Context, alpha: torch.Tensor, q: torch.Tensor, prior: capi.Prior) -> torch.Tensor:
    """R(alpha) + R(q): the smoothness prior `prior` (capi.Prior) of the grid of `ctx` at the fields alpha and q ([n_cells],
    the order of upload_grid), a float64 scalar on the context's GPU.  Needs a grid and nothing else; the context's own
    scalars play no part.  Differentiable in alpha and q: the forward is one c5_prior_gradient_device on torch's current
    stream, which leaves the gradient too (torch.autograd.grad and torch.func.grad make no further call); the second
    derivative - reverse over reverse (create_graph=True), torch.func.jvp(torch.func.grad(f), ...), torch.func.grad of a
    jvp - is one c5_prior_product_device.  Derivatives beyond the second, jvp of a jvp and vmap raise.  Bit-reproducible.
    Under a torch.cuda.Stream of torch's own the calls are only enqueued, in that stream's order; on torch's default (null)
    stream, which the library's stream is not ordered against, each call is waited for."""
    return _PriorValue.apply(ctx, alpha, q, prior)


# ---- the shape prior ---------------------------------------------------------------------------------------------------
# R(xyz) of capi.ShapePrior as a differentiable function of the points, built as prior is: the value and the gradient come
# from ONE c5_shape_prior_gradient_device, the second derivative from ONE c5_shape_prior_product_device, on the same stream
# rules (_enqueue).

def _no_shape_vmap():
    raise RuntimeError("course5_amd.autograd.shape_prior: vmap (a batch of point sets, tangents or cotangents) is not supported; "
                       "call it once per point set")


def _shape_points(ctx: capi.Context, device: torch.device, t):
    if t is None:
        return None
    t = _plain(t).detach().to(device=device, dtype=torch.float64).contiguous()
    if tuple(t.shape) != (ctx.n_pts, 3):
        raise ValueError(f"xyz must be [n_pts, 3] = [{ctx.n_pts}, 3], not {list(t.shape)}")
    return t


def _no_shape_third(*_args):
    raise RuntimeError("course5_amd.autograd.shape_prior: derivatives beyond the second are not supported (the shape prior's "
                       "Hessian product has no derivative of its own)")


class _ShapeProduct(_Operator):
    """Hess R(xyz) v: one c5_shape_prior_product_device at the point `fr` kept.  It has no derivative of its own."""
    what = "shape prior's Hessian product"
    backward = staticmethod(_no_shape_third)
    jvp = staticmethod(_no_shape_third)

    @staticmethod
    def forward(fr, xyz, v):
        ctx: capi.Context = fr.c5
        with _on_gpu(ctx, unwrapped=True) as device:
            vv = _shape_points(ctx, device, v)
            h = torch.empty((ctx.n_pts, 3), dtype=torch.float64, device=device)
            _enqueue(ctx, device, lambda: ctx.shape_prior_product_device(fr.prior, fr.point, vv, h))
        return h

    @staticmethod
    def vmap(info, in_dims, *args):
        _no_shape_vmap()


class _ShapeGradient(torch.autograd.Function):
    """grad R at the point of `fr`, as the forward's call left it (no call of its own); its derivative is _ShapeProduct."""

    @staticmethod
    def forward(fr, xyz):
        return fr.grad.clone()

    @staticmethod
    def setup_context(fctx, inputs, output):
        fctx.fr, fctx.xyz = inputs

    @staticmethod
    def backward(fctx, g):
        dtype, dev = fctx.fr.meta
        return None, _ShapeProduct.apply(fctx.fr, fctx.xyz, g).to(device=dev, dtype=dtype)

    @staticmethod
    def jvp(fctx, _fr_tangent, xyz_t):
        return _ShapeProduct.apply(fctx.fr, fctx.xyz, xyz_t)

    @staticmethod
    def vmap(info, in_dims, *args):
        _no_shape_vmap()


class _ShapeValue(torch.autograd.Function):
    @staticmethod
    def forward(ctx: capi.Context, xyz: torch.Tensor, prior: capi.ShapePrior):
        with _on_gpu(ctx, unwrapped=True) as device:
            x = _shape_points(ctx, device, xyz)
            value = torch.empty(1, dtype=torch.float64, device=device)
            grad = torch.empty((ctx.n_pts, 3), dtype=torch.float64, device=device)
            _enqueue(ctx, device, lambda: ctx.shape_prior_gradient_device(prior, x, value, None, grad))
            ctx.shape_prior_last = (x, grad)  # (setup_context takes them from here)
            return value[0].clone()

    @staticmethod
    def setup_context(fctx, inputs, output):
        ctx, xyz, prior = inputs
        fctx.c5, fctx.prior = ctx, prior
        fctx.point, fctx.grad = ctx.shape_prior_last  # (forward has just set it)
        fctx.meta = (xyz.dtype, xyz.device)
        fctx.xyz = xyz

    @staticmethod
    def backward(fctx, g_value: torch.Tensor):
        dtype, dev = fctx.meta
        g = _ShapeGradient.apply(fctx, fctx.xyz).to(device=dev, dtype=dtype)
        return None, g_value.to(g.device) * g, None

    @staticmethod
    def jvp(fctx, _ctx_tangent, xyz_t, _prior_tangent):
        # as _PriorValue.jvp: the value's tangent is grad R . t with grad R through _ShapeGradient where something can
        # differentiate the tangent, and forward over forward is refused
        from torch._C._functorch import TransformType
        from torch._functorch.pyfunctorch import retrieve_all_functorch_interpreters
        levels = [i.key() for i in retrieve_all_functorch_interpreters()]
        if sum(k == TransformType.Jvp for k in levels) > 1:
            raise RuntimeError("course5_amd.autograd.shape_prior: torch.func.jvp of a jvp (forward over forward) is not supported; "
                               "take the second derivative as jvp of grad, grad of jvp, or by double backward")
        if xyz_t is None:
            return None
        xyz = fctx.xyz
        g = _ShapeGradient.apply(fctx, xyz) if _differentiating_levels() > 1 or xyz.requires_grad else fctx.grad
        return (g * xyz_t.to(device=g.device, dtype=g.dtype)).sum()

    @staticmethod
    def vmap(info, in_dims, *args):
        _no_shape_vmap()


def shape_prior(ctx: capi.Context, xyz: torch.Tensor, prior: capi.ShapePrior) -> torch.Tensor:
    """R(xyz): the shape prior `prior` (capi.ShapePrior) of the grid of `ctx` against the rest shape it holds
    (ctx.shape_prior_rest) at the coordinates xyz ([n_pts, 3], the order of upload_grid), a float64 scalar on the context's
    GPU; +inf under the Neo-Hookean energy where a cell is inverted (the gradient stays finite).  The context's own points
    play no part.  Differentiable in xyz exactly as prior is in its fields: the forward is one
    c5_shape_prior_gradient_device on torch's current stream, which leaves the gradient too (torch.autograd.grad and
    torch.func.grad make no further call); the second derivative - reverse over reverse (create_graph=True),
    torch.func.jvp(torch.func.grad(f), ...), torch.func.grad of a jvp - is one c5_shape_prior_product_device.  Derivatives
    beyond the second, jvp of a jvp and vmap raise.  Bit-reproducible.  The stream rules are prior's."""
    return _ShapeValue.apply(ctx, xyz, prior)


__all__ = ["render", "render_view", "render_mesh", "gn_product", "gn_diagonal", "vertex_gn_product", "hvp", "ray_matrix", "ray_jacobian",
           "ray_shape_jacobian", "assemble_shape_jacobian", "prior", "shape_prior"]
