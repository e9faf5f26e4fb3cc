"""The render as a differentiable torch function of the cells' scalars.

    img = course5_amd.autograd.render(ctx, alpha, q)     # [local_rows, res_x, 2] float32 on ctx's GPU (tau, I)
    loss = (img * W).sum(); loss.backward()              # alpha.grad, q.grad: d loss / d AbsorpCoef, d loss / d radEnLooseRate

    with torch.autograd.forward_ad.dual_level():         # forward mode: the image's change for a change of the scalars
        img = render(ctx, fwAD.make_dual(alpha, d_alpha), q)
        img_dot = fwAD.unpack_dual(img).tangent          # [local_rows, res_x, 2] float32 (tau_dot, I_dot)
    img, img_dot = torch.func.jvp(lambda a, b: render(ctx, a, b), (alpha, q), (d_alpha, d_q))   # the same

`ctx` is a capi.Context with grid, image, rows, view (and solids) set; alpha and q hold one value per cell in the order of
its upload_grid.  The backward pass is the library's adjoint render (c5_render_adjoint_device), the forward-mode
derivative (jvp) its tangent render (c5_render_tangent_device): the derivative of the reference's integral as written,
alpha limit and all (include/course5_hip.h).

Forward: the scalars go to the context through c5_update_scalars, i.e. through host memory (16 bytes per cell each way:
~16 MB and a few ms for the 1M-cell C3 grid; the library has no device-pointer upload), then the frame is rendered on
torch's current stream and waited for (a C5_RETRY renders it again).  Backward: the adjoint on torch's current stream,
waited for likewise; gradients come back in the dtype and on the device of alpha and q.  jvp: the tangents of alpha and
q (None: zero) go to the context's GPU as float64, the tangent render runs on torch's current stream and is waited for;
the image's tangent is float32 on the context's GPU, like the image.

The context holds ONE set of scalars: a backward or jvp whose forward's scalars have since been replaced (another forward,
an update_scalars) uploads its own again.  A backward or jvp after the view, image, rows, solids, alpha limit or grid
changed raises instead of differentiating a frame other than the one rendered.  The gradients are fp64 sums added by
atomics in arrival order: not bit-reproducible from run to run; the tangent is.
"""
from __future__ import annotations

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


def _plain(t: torch.Tensor) -> torch.Tensor:
    """t without torch.func's wrappers."""
    while torch._C._functorch.is_functorch_wrapped_tensor(t):
        t = torch._C._functorch.get_unwrapped(t)
    return t


class _Scalars:
    """The scalars one forward uploaded; the context's scalars_owner while they are the ones it holds."""
    __slots__ = ("alpha", "q")

    def __init__(self, alpha, q):
        self.alpha, self.q = alpha, q


def _current(fctx, what: str) -> capi.Context:
    """The context of fctx, holding the scalars of fctx's forward again; raises if it no longer renders that frame."""
    ctx: capi.Context = fctx.c5
    if ctx.frame_state != fctx.state:
        raise RuntimeError("course5_amd.autograd.render: the context's view, image, rows, solids, alpha limit or grid "
                           f"changed since the forward pass; render again before calling {what}")
    if ctx.scalars_owner is not fctx.owner:
        ctx.update_scalars(fctx.owner.alpha, fctx.owner.q)
        ctx.scalars_owner = fctx.owner
    return ctx


class _Render(torch.autograd.Function):
    @staticmethod
    def forward(ctx: capi.Context, alpha: torch.Tensor, q: torch.Tensor):
        if alpha.shape != (ctx.n_cells,) or q.shape != (ctx.n_cells,):
            raise ValueError(f"alpha and q must hold one value per cell ({ctx.n_cells})")
        a_host = alpha.detach().to("cpu", torch.float64).contiguous().numpy().copy()
        q_host = q.detach().to("cpu", torch.float64).contiguous().numpy().copy()
        ctx.update_scalars(a_host, q_host)
        ctx.scalars_owner = _Scalars(a_host, q_host)  # (setup_context takes it from here)
        device = torch.device("cuda", ctx.device)
        out = torch.empty((ctx.local_rows, ctx.res_x, 2), dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            _use_torch_stream(ctx, device)
            _run(ctx, lambda: ctx.render_device(out.data_ptr()))
        return out

    @staticmethod
    def setup_context(fctx, inputs, output):
        ctx, alpha, q = inputs
        fctx.c5 = ctx
        fctx.state = ctx.frame_state
        fctx.owner = ctx.scalars_owner  # (forward has just set it)
        fctx.meta = ((alpha.dtype, alpha.device), (q.dtype, q.device))

    @staticmethod
    def backward(fctx, grad_img: torch.Tensor):
        ctx = _current(fctx, "backward")
        device = torch.device("cuda", ctx.device)
        g = grad_img.to(device=device, dtype=torch.float32).contiguous()
        ga = torch.empty(ctx.n_cells, dtype=torch.float64, device=device)
        gq = torch.empty(ctx.n_cells, dtype=torch.float64, device=device)
        with torch.cuda.device(device):
            _use_torch_stream(ctx, device)
            _run(ctx, lambda: ctx.render_adjoint_device(g, ga, gq))
        (a_dtype, a_dev), (q_dtype, q_dev) = fctx.meta
        ga_out = ga.to(device=a_dev, dtype=a_dtype) if fctx.needs_input_grad[1] else None
        gq_out = gq.to(device=q_dev, dtype=q_dtype) if fctx.needs_input_grad[2] else None
        return None, ga_out, gq_out

    @staticmethod
    def jvp(fctx, _ctx_tangent, alpha_t, q_t):
        ctx = _current(fctx, "jvp")
        device = torch.device("cuda", ctx.device)
        # under torch.func.jvp the tangents arrive wrapped (no storage of their own): the library reads plain tensors
        with torch._C._DisableFuncTorch(), torch.cuda.device(device):
            da = None if alpha_t is None else _plain(alpha_t).detach().to(device=device, dtype=torch.float64).contiguous()
            dq = None if q_t is None else _plain(q_t).detach().to(device=device, dtype=torch.float64).contiguous()
            out = torch.empty((ctx.local_rows, ctx.res_x, 2), dtype=torch.float32, device=device)
            _use_torch_stream(ctx, device)
            _run(ctx, lambda: ctx.render_tangent_device(da, dq, out))
        return out


def render(ctx: capi.Context, alpha: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """The frame of `ctx` with the cells' scalars alpha (AbsorpCoef) and q (radEnLooseRate), differentiable in both."""
    return _Render.apply(ctx, alpha, q)


__all__ = ["render"]
