"""Stand-ins for the reference's *unchanged* PyTorch networks, for stand-alone use.

The hot path calls three small coordinate MLPs that the reference keeps in
``model/networks`` (north_star: "unchanged"): the SDF field inside
``DMTetGeometry`` (``/root/reference/model/geometry/dmtet.py:187-212``), the
texture field and the DINO-feature field sampled per pixel in ``shade``
(``/root/reference/model/render/render.py:54,61``), plus the light MLP
(``/root/reference/model/render/light.py:169-193``).  When this package is
overlaid on the reference tree those classes are imported from there; when it
runs alone (tests, ``bench.py``) it needs networks of the same architecture and
with the same ``state_dict`` layout (``in_layer.*``, ``mlp.network.{0,2,..}.weight``,
``min_max``) so reference checkpoints load.  Plain PyTorch; rocBLAS / hipBLASLt GEMMs.

Same mathematics as the reference classes, evaluated faster for long point lists on the GPU (all equal to fp32 rounding, see
DESIGN.md "What is not a HIP kernel"): split-K weight gradients (``_LinearSplitK``), ReLU in the GEMM epilogue
(``_LinearReLUSplitK``), the per-image feature as a [B,C] GEMM plus a per-point add folded into the ReLU pass
(``CoordMLP._forward_indexed``), the input stage [x, sin, cos, 1] from one HIP kernel with the first bias as a weight column
(``CoordMLP._fused_input``), the output stage Linear(256 -> C <= 16) [+ sigmoid] [+ min_max] and its adjoint as one HIP pass over the
hidden vectors each way (``_FieldStackHead``, csrc/fieldhead.hip), and the frequency table kept on the device.  Short lists take the plain
torch path, except the one that needs double backward: points that require grad through the 256-wide SDF field (the eikonal regulariser)
take hand-written value / gradient / adjoint chains (``_field_value``, ``USE_FIELD_GRAD``).  The weight-modulated
field (``CoordMLP_Mod``) takes the same routes with its effective weights when ``USE_FIELD_MOD`` is on.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F


# When True every class below evaluates exactly the way the reference's model/networks classes do -- per-point feature
# concatenation (MLPs.py:84-90), one plain Linear per layer, the frequency table copied host -> device in every forward
# (HarmonicEmbedding.py:41), no HIP input stage, no split-K, no fused ReLU epilogues, no per-image feature path: what a maintainer
# gets who overlays only model/geometry + model/render and keeps the reference's own networks.  bench.py --networks reference.
REFERENCE_FORMULATION = False


def reference_formulation(enable=True):
    global REFERENCE_FORMULATION
    REFERENCE_FORMULATION = bool(enable)
    return REFERENCE_FORMULATION


def _activation(name):
    table = {"tanh": nn.Tanh, "sigmoid": nn.Sigmoid, "relu": nn.ReLU}
    if name not in table:
        raise NotImplementedError(name)
    return table[name]()


class HarmonicEmbedding(nn.Module):
    """[sin(2^k s x), cos(2^k s x)], k<n  (reference networks/HarmonicEmbedding.py:33-44)."""

    def __init__(self, n_harmonic_functions=10, scalar=1.0):
        super().__init__()
        self.frequencies = scalar * (2.0 ** torch.arange(n_harmonic_functions))  # plain attribute, not in the state_dict
        self._on_device = {}

    def _frequencies(self, device):
        # the reference copies the table host->device in every forward (HarmonicEmbedding.py:41): a pageable copy that blocks the
        # host until the stream drains.  Same values, copied once per device.
        f = self._on_device.get(device)
        if f is None:
            f = self._on_device[device] = self.frequencies.to(device)
        return f

    def forward(self, x):
        freq = self.frequencies.to(x.device) if REFERENCE_FORMULATION else self._frequencies(x.device)
        ang = (x[..., None] * freq).reshape(*x.shape[:-1], -1)
        return torch.cat((ang.sin(), ang.cos()), dim=-1)


USE_FIELD_STACK = True  # the hidden stack of a field as one autograd node with MFMA input-gradient GEMMs (_FieldStack)
USE_FIELD_HEAD = True  # ... and the output stage Linear(256 -> C <= 16) [+ sigmoid] [+ min_max] in the same node (_FieldStackHead)
# A head without activation and map (the deformation field) keeps the library GEMM in the FORWARD: its values are vertex offsets, and the
# rasteriser's edge blending turns a last-bit difference there into 4e-6 of a pixel's colour; with the same product as before, the step's
# images stay within rounding of what they were.  Its backward is the fused pass all the same.
_PLAIN_HEAD_FORWARD_GEMM = True
SPLITK_MIN_ROWS = 65536  # point lists at least this long take the split-K weight gradient below
SPLITK_PARTS = 16


class _LinearSplitK(torch.autograd.Function):
    """y = x @ W^T for a long point list x [M,K] (M ~ 2e5) and a small weight W [N,K].

    Forward and the input gradient are the GEMMs autograd would issue.  The weight gradient g^T x is a [N,M] x [M,K] product with
    a tiny output and a huge reduction: as ONE GEMM rocBLAS/hipBLASLt reach 65 TFLOP/s on gfx950 (409 us tuned, 606 us untuned at
    M=204800, N=K=256); cut into SPLITK_PARTS row blocks and issued as a batched GEMM + a sum of the partial products it takes
    222 us (a throw-away micro-benchmark, not kept).  Same sum, different association: equal to fp32 rounding (7e-6 relative).
    The backward is written with differentiable torch ops, so double backward (create_graph=True) still works.
    """

    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        return x.mm(weight.t())

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        gx = g.mm(weight) if ctx.needs_input_grad[0] else None
        gw = None
        if ctx.needs_input_grad[1]:
            gw = _split_k_weight_grad(g.contiguous(), x)
        return gx, gw


def _split_k_weight_grad(g, x):
    s, m = SPLITK_PARTS, x.shape[0]
    return torch.bmm(g.view(s, m // s, g.shape[1]).transpose(1, 2), x.view(s, m // s, x.shape[1])).sum(0)


_ZERO_BIAS = {}


def _zero_bias(x, weight):
    key = (x.device, weight.shape[0])
    b = _ZERO_BIAS.get(key)
    if b is None:
        b = _ZERO_BIAS[key] = torch.zeros(weight.shape[0], dtype=x.dtype, device=x.device)
    return b


class _LinearReLUSplitK(torch.autograd.Function):
    """relu(x @ W^T + b) for a long point list: the bias add and the ReLU ride in the GEMM epilogue (hipBLASLt through
    torch._addmm_activation: 235 us against 215 + 85 us for GEMM + a separate ReLU pass at M=204800, N=K=256; bit-identical
    values), the weight gradient is the split-K batched GEMM of _LinearSplitK."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        y = torch._addmm_activation(_zero_bias(x, weight) if bias is None else bias, x, weight.t(), use_gelu=False)
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        g = torch.ops.aten.threshold_backward(g.contiguous(), y, 0)
        gx = g.mm(weight) if ctx.needs_input_grad[0] else None
        gw = _split_k_weight_grad(g, x) if ctx.needs_input_grad[1] else None
        gb = g.sum(0) if ctx.needs_input_grad[2] else None
        return gx, gw, gb


class _FieldStack(torch.autograd.Function):
    """The hidden stack of a coordinate field over a long point list as ONE autograd node:

        y0 = relu(x_emb W_in^T)                                   in_layer (bias folded into W_in's last column)
        y1 = relu(y0 W_first^T + per_image[index])                only for fields with a per-image feature
        y_i = relu(y_{i-1} W_i^T)                                 the 256 -> 256 hidden layers

    Forward as before (ReLU in the GEMM epilogue).  Backward: every input-gradient GEMM is csrc/gemm.hip (hand-written fp32 MFMA)
    with the previous layer's ReLU adjoint in its epilogue, g_{i-1} = (g_i W_i) * (y_{i-1} > 0), so of the n+1 threshold_backward
    passes over [M,256] only the first (for the stack's own output) is left, and the per-image layer needs a plain segment sum instead
    of the masked one.  Weight gradients are the split-K batched GEMMs.  First-order only (the regulariser's short lists never get here).
    """

    @staticmethod
    def forward(ctx, x_emb, w_in, per_image, index, w_first, *hidden):
        ys = _stack_forward(x_emb, w_in, per_image, index, w_first, hidden)
        ctx.save_for_backward(x_emb, w_in, index, w_first, *hidden, *ys)
        ctx.n_hidden, ctx.n_images = len(hidden), (per_image.shape[0] if per_image is not None else 0)
        return ys[-1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        saved = ctx.saved_tensors
        x_emb, w_in, index, w_first = saved[:4]
        hidden, ys = saved[4:4 + ctx.n_hidden], saved[4 + ctx.n_hidden:]
        g = torch.ops.aten.threshold_backward(g.contiguous(), ys[-1], 0)
        g_x, g_in, g_rows, g_first, g_hidden = _stack_backward(g, x_emb, w_in, index, w_first, hidden, ys, ctx.n_images, ctx.needs_input_grad[0])
        return (g_x, g_in, g_rows, None, g_first, *g_hidden)


def _stack_forward(x_emb, w_in, per_image, index, w_first, hidden):
    """[y0, (y1,) .. y_n] of _FieldStack."""
    from . import ops

    zero = _zero_bias(x_emb, w_in)
    ys = [torch._addmm_activation(zero, x_emb, w_in.t(), use_gelu=False)]
    if w_first is not None:
        y = ys[0].mm(w_first.t())
        ops.rows_add_relu_raw_(y, per_image, index)
        ys.append(y)
    for w in hidden:
        ys.append(torch._addmm_activation(zero, ys[-1], w.t(), use_gelu=False))
    return ys


def _stack_backward(g, x_emb, w_in, index, w_first, hidden, ys, n_images, need_x):
    """_FieldStack's backward from g = the gradient of ys[-1] with that layer's ReLU adjoint applied -> (g_x, g_in, g_rows, g_first, g_hidden)."""
    from . import ops

    n_hidden = len(hidden)
    g_hidden = []
    for i in range(n_hidden - 1, -1, -1):
        y_prev = ys[len(ys) - n_hidden - 1 + i]
        g_hidden.append(_split_k_weight_grad(g, y_prev))
        g = ops.gemm_nn_relumask(g, hidden[i], y_prev)
    g_hidden.reverse()
    g_rows = g_first = None
    if w_first is not None:
        g_rows = ops.rows_segsum_raw(g, index, n_images)
        g_first = _split_k_weight_grad(g, ys[0])
        g = ops.gemm_nn_relumask(g, w_first, ys[0])
    g_in = _split_k_weight_grad(g, x_emb)
    g_x = g.mm(w_in) if need_x else None
    return g_x, g_in, g_rows, g_first, g_hidden


class _FieldStackHead(torch.autograd.Function):
    """_FieldStack with the field's output stage in the same node (csrc/fieldhead.hip):

        out = act(y_n W_head^T) * scale + lo                      Linear(256 -> C <= 16), none / sigmoid, the min_max map

    The forward reads y_n once; the backward starts with ONE pass over y_n that applies the map's, the activation's and the Linear's
    adjoints, masks the result with (y_n > 0) -- so the stack's last threshold_backward pass is gone too -- and sums the head's weight
    gradient (deterministically: per-work-group partial sums, added in a fixed order).  First-order only, like _FieldStack.
    """

    @staticmethod
    def forward(ctx, x_emb, w_in, per_image, index, w_first, w_head, lo, scale, act, *hidden):
        from . import ops

        ys = _stack_forward(x_emb, w_in, per_image, index, w_first, hidden)
        if _PLAIN_HEAD_FORWARD_GEMM and not act and scale is None:
            s, out = None, ys[-1].mm(w_head.t())
        else:
            s, out = ops.field_head_fwd(ys[-1], w_head, lo, scale, act)
        ctx.save_for_backward(x_emb, w_in, index, w_first, w_head, scale, s if act else None, *hidden, *ys)  # (s: the sigmoid's adjoint)
        ctx.n_hidden, ctx.n_images, ctx.act = len(hidden), (per_image.shape[0] if per_image is not None else 0), act
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from . import ops

        saved = ctx.saved_tensors
        x_emb, w_in, index, w_first, w_head, scale, s = saved[:7]
        hidden, ys = saved[7:7 + ctx.n_hidden], saved[7 + ctx.n_hidden:]
        g, g_head = ops.field_head_bwd(g, s, ys[-1], w_head, scale, ctx.act)
        g_x, g_in, g_rows, g_first, g_hidden = _stack_backward(g, x_emb, w_in, index, w_first, hidden, ys, ctx.n_images, ctx.needs_input_grad[0])
        return (g_x, g_in, g_rows, None, g_first, g_head, None, None, None, *g_hidden)


USE_FIELD_GRAD = True  # a short point list that REQUIRES GRAD through a scalar 256-wide field: value, input gradient and the adjoint of
# that gradient as the hand-written chains below (_FieldValue / _FieldInputGrad) instead of autograd's general double backward


def _tn_products(p, q):
    """[p_i^T q_i] for stacks p [n,M,256] and q [n,M,C]: the weight gradients of a short list.  Every product has a tiny output and an
    M-long reduction; all layers go through one split-K launch of csrc/gemm.hip and one that adds the partial products in a fixed order."""
    from . import ops

    return ops.gemm_tn_splitk(p, q)


def _field_grad_chain(s, y, w_head, hidden):
    """b_0 .. b_L [L + 1, M, 256]: b_L = (s w_h) * (y_L > 0), b_(l-1) = (b_l W_l) * (y_(l-1) > 0)."""
    from . import ops

    n_hidden = len(hidden)
    b = torch.empty_like(y)
    ops.field_grad_head_fwd(s, w_head, y[n_hidden], out=b[n_hidden])
    for l in range(n_hidden, 0, -1):
        ops.gemm_nn_relumask(b[l], hidden[l - 1], y[l - 1], out=b[l - 1])
    return b


class _FieldInputGrad(torch.autograd.Function):
    """The gradient pass of _FieldValue as a node of its own, so that it can be differentiated in turn (the eikonal regulariser:
    autograd.grad(sdf, points, create_graph=True), a loss on the result, backward to the weights).  With D_l = (y_l > 0):

        forward    b_L = (s w_h) * D_L,  b_(l-1) = (b_l W_l) * D_(l-1),  g_x = J_e(x)^T (b_0 W_in)
        backward   given lam = d/d g_x:  dv = J_e(x) lam,  t_0 = (dv W_in^T) * D_0,  t_l = (t_(l-1) W_l^T) * D_l,
                   dW_in = b_0^T dv,  dW_l = b_l^T t_(l-1),  dw_h = sum_m s[m] t_L[m,:],  ds = t_L w_h^T

    A ReLU stack is piecewise linear: the masks are constants of the point, so the backward is a second forward pass with frozen masks
    plus one weight-gradient product per layer -- no second derivative of any layer.  The points enter detached: the second-order
    gradient with respect to x (the embedding's Hessian) is not provided, autograd.grad for it raises "not used in the graph", and a
    plain backward() leaves it out."""

    @staticmethod
    def forward(ctx, s, x, y, w_in, w_head, freq, symmetrize, *hidden):
        from . import ops

        b = _field_grad_chain(s, y, w_head, hidden)
        ctx.save_for_backward(s, x, y, w_in, w_head, freq, b, *hidden)
        ctx.symmetrize = symmetrize
        return ops.harmonic_embed_bwd_raw(b[0].mm(w_in), x, freq, symmetrize, True)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, lam):
        from . import ops

        s, x, y, w_in, w_head, freq, b = ctx.saved_tensors[:7]
        hidden = ctx.saved_tensors[7:]
        n_hidden = len(hidden)
        need = ctx.needs_input_grad  # (s, x, y, w_in, w_head, freq, symmetrize, *hidden)
        dv = ops.harmonic_embed_jvp(x, lam, freq, ctx.symmetrize, True)
        t = torch.empty_like(y)  # t_0 .. t_L
        ops.gemm_nt_relumask(dv, w_in, y[0], out=t[0])
        for l in range(1, n_hidden + 1):
            ops.gemm_nt_relumask(t[l - 1], hidden[l - 1], y[l], out=t[l])
        g_in = _tn_products(b[:1], dv[None])[0] if need[3] else None
        g_head, g_s = ops.field_grad_head_bwd(s, t[n_hidden], w_head, need_s=need[0]) if (need[4] or need[0]) else (None, None)
        g_hidden = [None] * n_hidden
        if any(need[7:]):
            prods = _tn_products(b[1:], t[:-1])
            g_hidden = [prods[l] if need[7 + l] else None for l in range(n_hidden)]
        return (g_s, None, None, g_in, g_head if need[4] else None, None, None, *g_hidden)


class _FieldWeightTap(torch.autograd.Function):
    """Where _FieldValue's FIRST-ORDER weight gradients are computed: dW_in = b_0^T e, dW_l = b_l^T y_(l-1), dw_h = s^T y_L.

    A Function's backward cannot know which of its input gradients the engine wants, and the regulariser asks for d sdf / d points alone:
    six products per call would be computed and thrown away.  So the weights reach _FieldValue through this node: its forward returns an
    [M,1] buffer that nobody reads (no launch), _FieldValue hands the buffer's "gradient" s on unchanged, and the engine runs this backward
    only when a weight gradient is wanted -- never under autograd.grad(sdf, points).  ``box`` is filled by _FieldValue.forward with the
    embedding and the activations.  First-order only."""

    @staticmethod
    def forward(ctx, box, m, w_in, w_head, *hidden):
        ctx.box = box
        ctx.save_for_backward(w_head, *hidden)
        return torch.empty((m, 1), dtype=w_in.dtype, device=w_in.device)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, s):
        e, y = ctx.box["e"], ctx.box["y"]
        w_head, hidden = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        need = ctx.needs_input_grad  # (box, m, w_in, w_head, *hidden)
        b = _field_grad_chain(s, y, w_head, hidden)
        g_in = _tn_products(b[:1], e[None])[0] if need[2] else None
        g_head = s.reshape(1, -1).mm(y[-1]) if need[3] else None
        g_hidden = [None] * len(hidden)
        if any(need[4:]):
            prods = _tn_products(b[1:], y[:-1])
            g_hidden = [prods[l] if need[4 + l] else None for l in range(len(hidden))]
        return (None, None, g_in, g_head, *g_hidden)


class _FieldValue(torch.autograd.Function):
    """A scalar coordinate field over a short point list that requires grad, out = y_L w_h^T with y_0 = relu(embed(x) W_in^T) (the
    in_layer's bias folded in as the ones column) and y_l = relu(y_(l-1) W_l^T): the library GEMMs of _stack_forward, written into one
    [L + 1, M, 256] buffer, and a backward that is itself a differentiable node (_FieldInputGrad; no once_differentiable here).  The
    weights' own first-order gradients go through ``tap`` (_FieldWeightTap); use :func:`_field_value`."""

    @staticmethod
    def forward(ctx, x, tap, box, w_in, w_head, freq, symmetrize, *hidden):
        from . import ops

        e = ops.harmonic_embed_raw(x, freq, symmetrize, True)
        y = torch.empty((len(hidden) + 1, x.shape[0], 256), dtype=torch.float32, device=x.device)
        zero = _zero_bias(e, w_in)
        torch._addmm_activation(zero, e, w_in.t(), use_gelu=False, out=y[0])
        for l, w in enumerate(hidden):
            torch._addmm_activation(zero, y[l], w.t(), use_gelu=False, out=y[l + 1])
        box.update(e=e, y=y)
        ctx.save_for_backward(x, y, w_in, w_head, freq, *hidden)
        ctx.symmetrize = bool(symmetrize)
        return y[-1].mm(w_head.t())

    @staticmethod
    def backward(ctx, s):
        x, y, w_in, w_head, freq = ctx.saved_tensors[:5]
        hidden = ctx.saved_tensors[5:]
        g_x = _FieldInputGrad.apply(s, x.detach(), y, w_in, w_head, freq, ctx.symmetrize, *hidden) if ctx.needs_input_grad[0] else None
        return (g_x, s if ctx.needs_input_grad[1] else None, None, None, None, None, None, *([None] * len(hidden)))


def _field_value(x, w_in, w_head, freq, symmetrize, *hidden):
    box = {}
    tap = _FieldWeightTap.apply(box, x.shape[0], w_in, w_head, *hidden)
    return _FieldValue.apply(x, tap, box, w_in, w_head, freq, symmetrize, *hidden)


def _long_list(x, weight):
    return (x.is_cuda and x.dim() == 2 and x.shape[0] >= SPLITK_MIN_ROWS and x.shape[0] % SPLITK_PARTS == 0 and x.is_contiguous()
            and x.dtype == torch.float32 and torch.is_grad_enabled() and weight.requires_grad)


def linear(x, weight, bias=None):
    """F.linear, with the split-K weight gradient for long point lists on the GPU."""
    if bias is None and _long_list(x, weight):
        return _LinearSplitK.apply(x, weight)
    return F.linear(x, weight, bias)


def linear_relu(x, weight, bias=None):
    """relu(F.linear(x, weight, bias)); epilogue-fused with the split-K weight gradient for long point lists on the GPU."""
    if _long_list(x, weight):
        return _LinearReLUSplitK.apply(x, weight, bias)
    if (x.is_cuda and x.dim() == 2 and x.shape[0] >= SPLITK_MIN_ROWS and x.dtype == torch.float32
            and not (torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)))):
        return torch._addmm_activation(_zero_bias(x, weight) if bias is None else bias, x, weight.t(), use_gelu=False)  # e.g. the SDF grid pass
    return torch.relu_(F.linear(x, weight, bias))


class MLP(nn.Module):
    """Bias-free Linear/ReLU stack (reference networks/MLPs.py:9-32)."""

    def __init__(self, cin, cout, num_layers, nf=256, dropout=0, activation=None):
        super().__init__()
        assert num_layers >= 1
        dims = [cin] + [nf] * (num_layers - 1) + [cout]
        layers = []
        for i in range(num_layers):
            if i > 0:
                layers.append(nn.ReLU(inplace=True))
            layers.append(nn.Linear(dims[i], dims[i + 1], bias=False))
            if dropout and 0 < i < num_layers - 1:
                layers.append(nn.Dropout(dropout))
        if activation is not None:
            layers.append(_activation(activation))
        self.network = nn.Sequential(*layers)

    def forward(self, x, first_weight=None, per_image=None, index=None):
        """Plain stack; or, with ``first_weight`` [nf,K], ``per_image`` [B,nf] and ``index`` [P] (CoordMLP's per-image feature
        path), the first Linear is evaluated as x @ first_weight^T + per_image[index], the addend folded into the ReLU pass."""
        if REFERENCE_FORMULATION and first_weight is None:
            return self.network(x)
        layers = list(self.network)
        i = 0
        if first_weight is not None:
            assert isinstance(layers[0], nn.Linear) and layers[0].bias is None
            x = linear(x, first_weight)
            if len(layers) > 1 and isinstance(layers[1], nn.ReLU) and x.is_cuda:
                from . import ops

                x = ops.rows_add_relu_(x, per_image, index)  # one in-place pass: + per_image[index], ReLU
                i = 2
            else:
                x = x + per_image[index]
                i = 1
        while i < len(layers):
            layer = layers[i]
            if isinstance(layer, nn.Linear) and i + 1 < len(layers) and isinstance(layers[i + 1], nn.ReLU):
                x = linear_relu(x, layer.weight, layer.bias)
                i += 2
                continue
            x = linear(x, layer.weight, layer.bias) if isinstance(layer, nn.Linear) else layer(x)
            i += 1
        return x


class CoordMLP(nn.Module):
    """Harmonic embedding -> in_layer (+feat concat) -> MLP (reference networks/MLPs.py:35-101)."""

    def __init__(self, cin, cout, num_layers, nf=256, dropout=0, activation=None, min_max=None, n_harmonic_functions=10,
                 embedder_scalar=1, embed_concat_pts=True, extra_feat_dim=0, symmetrize=False, in_layer_relu=False):
        super().__init__()
        self.extra_feat_dim = extra_feat_dim
        if n_harmonic_functions > 0:
            self.embedder = HarmonicEmbedding(n_harmonic_functions, embedder_scalar)
            dim_in = cin * 2 * n_harmonic_functions + (cin if embed_concat_pts else 0)
            self.embed_concat_pts = embed_concat_pts
        else:
            self.embedder = None
            dim_in = cin
        self.in_layer = nn.Linear(dim_in, nf)
        self.relu = nn.ReLU(inplace=True)
        self.mlp = MLP(nf + extra_feat_dim, cout, num_layers, nf, dropout, activation)
        self.symmetrize = symmetrize
        if min_max is not None:
            self.register_buffer("min_max", min_max)
        else:
            self.min_max = None
        self.bsdf = None
        self.in_layer_relu = in_layer_relu

    @property
    def indexed_feat(self):  # sample(x, feat=[B,C], feat_index=[P]) is understood (not in the reference formulation)
        return not REFERENCE_FORMULATION

    def forward(self, x, feat=None, feat_index=None):
        """``feat_index`` (int64 [P], optional, not in the reference signature): ``feat`` is then one row per IMAGE and point p uses
        row feat_index[p].  The reference concatenates the per-point copy of the feature to the hidden vector and multiplies by
        the [nf, nf+C] weight (MLPs.py:84-90); with W = [W_h | W_f] that product is relu(h) W_h^T + (relu(feat) W_f^T)[index]:
        the feature half becomes a [B,C] x [C,nf] GEMM and a row gather instead of a [P,C] x [C,nf] GEMM over 2e5 points
        (and its two backward GEMMs), and the [P, nf+C] concatenation disappears.  Same sum, equal to fp32 rounding."""
        assert (feat is None and self.extra_feat_dim == 0) or (feat.shape[-1] == self.extra_feat_dim)
        if REFERENCE_FORMULATION:
            return self._forward_reference(x, feat if feat_index is None or feat is None else feat[feat_index])
        if feat_index is not None and feat is not None and x.dim() == 2 and isinstance(self.mlp.network[0], nn.Linear) \
                and self.mlp.network[0].bias is None:
            return self._forward_indexed(x, feat, feat_index)
        if feat_index is not None and feat is not None:
            feat = feat[feat_index]
        if feat is None and self._stack_ok(x, False):
            return self._stacked(x, None, None)
        if feat is None and self._field_grad_ok(x):
            return self._field_grad(x)
        if feat is None and self._fused_input_ok(x):
            out = self.mlp(self._fused_input(x))
            if self.min_max is not None:
                out = out * (self.min_max[:, 1] - self.min_max[:, 0]) + self.min_max[:, 0]
            return out
        if self.symmetrize:
            x = torch.cat([x[..., :1].abs(), x[..., 1:]], -1)
        h = x
        if self.embedder is not None:
            h = self.embedder(x)
            if self.embed_concat_pts:
                h = torch.cat([x, h], -1)
        if feat is None:  # relu(in_layer(.)) feeds the stack directly: one fused Linear+ReLU
            out = self.mlp(linear_relu(h, self.in_layer.weight, self.in_layer.bias))
        else:
            h = self.in_layer(h)
            if self.in_layer_relu:
                h = self.relu(h)
            while feat.dim() < h.dim():
                feat = feat.unsqueeze(1)
            h = torch.cat([h, feat.expand(*h.shape[:-1], -1)], dim=-1)
            out = self.mlp(self.relu(h))
        if self.min_max is not None:
            out = out * (self.min_max[:, 1] - self.min_max[:, 0]) + self.min_max[:, 0]
        return out

    def _forward_reference(self, x, feat):
        """The reference's own evaluation order (MLPs.py:73-98)."""
        if self.symmetrize:
            xs, ys, zs = x.unbind(-1)
            x = torch.stack([xs.abs(), ys, zs], -1)
        x_in = x
        if self.embedder is not None:
            x_in = self.embedder(x)
            if self.embed_concat_pts:
                x_in = torch.cat([x, x_in], -1)
        x_in = self.in_layer(x_in)
        if self.in_layer_relu:
            x_in = self.relu(x_in)
        if feat is not None:
            for _ in range(x_in.dim() - feat.dim()):
                feat = feat.unsqueeze(1)
            x_in = torch.cat([x_in, feat.expand(*x_in.shape[:-1], -1)], dim=-1)
        out = self.mlp(self.relu(x_in))
        if self.min_max is not None:
            out = out * (self.min_max[:, 1] - self.min_max[:, 0]) + self.min_max[:, 0]
        return out

    def _fused_input_ok(self, x):
        """Long point list on the GPU with the standard input stage (embedding + concatenated points): one HIP kernel builds
        [x, sin, cos, 1] and the in_layer's bias rides as the weight column that multiplies the ones (K = 64 for 10 frequencies)."""
        return (x.is_cuda and x.dim() == 2 and x.shape[1] == 3 and x.shape[0] >= SPLITK_MIN_ROWS and x.dtype == torch.float32
                and self.embedder is not None and self.embed_concat_pts and self.in_layer.bias is not None)

    def _fused_input(self, x):
        """relu(in_layer([x, embed(x)])) for a long point list (first-order differentiable)."""
        from . import ops

        h = ops.harmonic_embed(x, self.embedder._frequencies(x.device), symmetrize=self.symmetrize, ones=True)
        return linear_relu(h, self._w_in(), None)

    def _field_grad_ok(self, x):
        """A short list of points that REQUIRE GRAD through a scalar field of the standard shape (the SDF under the eikonal regulariser):
        embedding + concatenated points (an even number of frequencies: K = 4 + 6n is then a multiple of 4), a biased in_layer of 256
        outputs, bias-free 256 x 256 Linear/ReLU pairs, one bias-free Linear(256 -> 1); nothing else behind it.  Everything else -- the
        grad-free grid pass, points that do not require grad, narrow nets, features -- keeps its path."""
        if not self._field_grad_input_ok(x):
            return False
        layers = list(self.mlp.network)
        if len(layers) < 3 or len(layers) % 2 == 0:
            return False
        for i, layer in enumerate(layers[:-1]):
            if i % 2 == 1 and not isinstance(layer, nn.ReLU):
                return False
            if i % 2 == 0 and not (isinstance(layer, nn.Linear) and layer.bias is None and tuple(layer.weight.shape) == (256, 256)):
                return False
        head = layers[-1]
        return isinstance(head, nn.Linear) and head.bias is None and tuple(head.weight.shape) == (1, 256) and head.weight.dtype == torch.float32

    def _field_grad_input_ok(self, x):
        """_field_grad_ok without the walk over self.mlp's layers: the point list, the embedding and the in_layer (shared with CoordMLP_Mod,
        whose layers are effective weights rather than modules)."""
        return (USE_FIELD_GRAD and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == 3 and 1 <= x.shape[0] < SPLITK_MIN_ROWS
                and x.requires_grad and torch.is_grad_enabled() and self.embedder is not None and self.embed_concat_pts
                and len(self.embedder.frequencies) % 2 == 0 and self.in_layer.bias is not None and self.in_layer.weight.shape[0] == 256
                and self.in_layer.weight.dtype == torch.float32 and self.min_max is None and self.extra_feat_dim == 0)

    def _field_grad(self, x):
        layers = list(self.mlp.network)
        return _field_value(x, self._w_in(), layers[-1].weight, self.embedder._frequencies(x.device), bool(self.symmetrize),
                            *[l.weight for l in layers[:-1:2]])

    def _stack_ok(self, x, with_feat):
        """The whole hidden stack as one autograd node (_FieldStack): long list, training, 256-wide bias-free Linear/ReLU pairs."""
        if not self._stack_input_ok(x):
            return False
        layers = list(self.mlp.network)
        n_pairs = 0
        while 2 * n_pairs + 1 < len(layers) and isinstance(layers[2 * n_pairs], nn.Linear) and isinstance(layers[2 * n_pairs + 1], nn.ReLU):
            lin = layers[2 * n_pairs]
            want_in = 256 + (self.extra_feat_dim if (with_feat and n_pairs == 0) else 0)
            if lin.bias is not None or tuple(lin.weight.shape) != (256, want_in):
                return False
            n_pairs += 1
        return n_pairs >= 1

    def _stack_input_ok(self, x):
        """_stack_ok without the walk over self.mlp's layers (shared with CoordMLP_Mod)."""
        return bool(USE_FIELD_STACK and self._fused_input_ok(x) and torch.is_grad_enabled() and x.shape[0] % SPLITK_PARTS == 0
                    and self.in_layer.weight.requires_grad and self.in_layer.weight.shape[0] == 256)

    def _fused_head(self, tail):
        """(weight, lo, scale, act) when ``tail`` -- the layers behind the stack's Linear/ReLU pairs -- is exactly one bias-free
        Linear(256 -> C <= 16), optionally followed by a Sigmoid, with an optional min_max: the output stage _FieldStackHead fuses.
        None for everything else (tanh, dropout, a biased head ...), which keeps the layer-by-layer tail of _stacked.  Reached only
        from _stacked, that is behind _stack_ok: long lists with grad enabled -- never the SDF's grad-free grid pass or a short list."""
        if not 1 <= len(tail) <= 2 or not isinstance(tail[0], nn.Linear) or tail[0].bias is not None:
            return None
        if len(tail) == 2 and not isinstance(tail[1], nn.Sigmoid):
            return None
        return self._fused_head_of(tail[0].weight, len(tail) - 1)

    def _fused_head_of(self, weight, act):
        """_fused_head for a bias-free head given by its weight [C,256] (shared with CoordMLP_Mod)."""
        if not USE_FIELD_HEAD or weight.shape[1] != 256 or not 1 <= weight.shape[0] <= 16 or weight.dtype != torch.float32:
            return None
        lo = scale = None
        if self.min_max is not None:
            if tuple(self.min_max.shape) != (weight.shape[0], 2) or self.min_max.requires_grad or self.min_max.dtype != torch.float32:
                return None
            lo = self.min_max[:, 0].contiguous()
            scale = self.min_max[:, 1] - self.min_max[:, 0]
        return weight, lo, scale, act

    def _w_in(self):
        """The in_layer's weight with its bias as the column that multiplies the embedding's ones."""
        return torch.cat([self.in_layer.weight, self.in_layer.bias[:, None]], dim=1)

    def _stack_node(self, x, per_image, index, w_first, hidden, head):
        """The stack node over the fused input stage for the 256 x 256 weights ``hidden``: with the output stage ``head`` (what _fused_head /
        _fused_head_of returned) in it, or without (None: the caller runs the tail).  Shared with CoordMLP_Mod, whose weights are tensors."""
        from . import ops

        x_emb = ops.harmonic_embed(x, self.embedder._frequencies(x.device), symmetrize=self.symmetrize, ones=True)
        if head is not None:
            return _FieldStackHead.apply(x_emb, self._w_in(), per_image, index, w_first, *head, *hidden)
        return _FieldStack.apply(x_emb, self._w_in(), per_image, index, w_first, *hidden)

    def _stacked(self, x, feat, feat_index):
        layers = list(self.mlp.network)
        pairs, i = [], 0
        while i + 1 < len(layers) and isinstance(layers[i], nn.Linear) and isinstance(layers[i + 1], nn.ReLU):
            pairs.append(layers[i])
            i += 2
        per_image = w_first = None
        if feat is not None:
            first, pairs = pairs[0].weight, pairs[1:]
            per_image = F.linear(torch.relu(feat), first[:, 256:])  # [B, 256]
            w_first = first[:, :256].contiguous()
        head = self._fused_head(layers[i:])
        h = self._stack_node(x, per_image, feat_index if feat is not None else None, w_first, [l.weight for l in pairs], head)
        if head is not None:
            return h
        for layer in layers[i:]:
            h = linear(h, layer.weight, layer.bias) if isinstance(layer, nn.Linear) else layer(h)
        if self.min_max is not None:
            h = h * (self.min_max[:, 1] - self.min_max[:, 0]) + self.min_max[:, 0]
        return h

    def _forward_indexed(self, x, feat, feat_index):
        if self._stack_ok(x, True):
            return self._stacked(x, feat, feat_index)
        if self._fused_input_ok(x):
            h = self._fused_input(x)
        else:
            if self.symmetrize:
                x = torch.cat([x[..., :1].abs(), x[..., 1:]], -1)
            h = x
            if self.embedder is not None:
                h = self.embedder(x)
                if self.embed_concat_pts:
                    h = torch.cat([x, h], -1)
            h = linear_relu(h, self.in_layer.weight, self.in_layer.bias)
        nf = h.shape[-1]
        weight = self.mlp.network[0].weight
        per_image = F.linear(torch.relu(feat), weight[:, nf:])  # [B, nf]
        out = self.mlp(h, first_weight=weight[:, :nf].contiguous(), per_image=per_image, index=feat_index)
        if self.min_max is not None:
            out = out * (self.min_max[:, 1] - self.min_max[:, 0]) + self.min_max[:, 0]
        return out

    def sample(self, x, feat=None, feat_index=None):
        return self.forward(x, feat, feat_index)


# ---------------------------------------------------------------------------------------------------------------------------------
# Weight-modulated field of the pan-category model (Fauna): same classes and state_dict layout as the reference's
# CoordMLP_Mod / MLP_Mod / Linear_Mod (networks/MLPs.py:104-247).  One 128-d embedding per batch modulates and demodulates every
# layer's weight (StyleGAN2 style); plain torch, unless USE_FIELD_MOD is on.
#
# A Linear_Mod is a bias-free Linear whose weight is a function of the style, so with the effective weights W'_l in hand the field is the
# Linear/ReLU stack CoordMLP's routes are made for (linear_relu, _FieldStack / _FieldStackHead, _field_value).  OFF
# unless A3D_FIELD_MOD=1: switching a route on by default changes recorded behaviour.
USE_FIELD_MOD = os.environ.get("A3D_FIELD_MOD", "0") not in ("0", "")


class Linear_Mod(nn.Module):
    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty((out_features, in_features)))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_features))
        else:
            self.register_parameter("bias", None)
        nn.init.kaiming_uniform_(self.weight, a=5 ** 0.5)
        if self.bias is not None:
            fan_in, _ = nn.init._calculate_fan_in_and_fan_out(self.weight)
            bound = 1 / fan_in ** 0.5 if fan_in > 0 else 0
            nn.init.uniform_(self.bias, -bound, bound)

    def effective_weight(self, style):
        """W'[o,i] = W[o,i] s[i] / sqrt(sum_j (W[o,j] s[j])^2 + 1e-5): the weight forward multiplies with, the reference's three statements
        (MLPs.py:234-240) in their order.  Differentiable with respect to the weight and the style."""
        if style.dim() > 1:  # one style per batch: the first row (MLPs.py:233-235)
            style = style.reshape(-1, style.shape[-1])[0]
        weight = self.weight * style.unsqueeze(0)
        return weight / ((weight * weight).sum(dim=-1, keepdim=True) + 1e-5).sqrt()

    def forward(self, x, style):
        return F.linear(x, self.effective_weight(style), self.bias)


class MLP_Mod(nn.Module):
    def __init__(self, cin, cout, num_layers, nf=256, dropout=0, activation=None):
        super().__init__()
        assert num_layers >= 1
        self.num_layers = num_layers
        if num_layers == 1:
            self.network = Linear_Mod(cin, cout, bias=False)
        else:
            self.relu = nn.ReLU(inplace=True)
            for i in range(num_layers):
                setattr(self, f"linear_{i}", Linear_Mod(cin if i == 0 else nf, cout if i == num_layers - 1 else nf, bias=False))

    def layers(self):
        return [self.network] if self.num_layers == 1 else [getattr(self, f"linear_{i}") for i in range(self.num_layers)]

    def effective_weights(self, style):
        """[W'_0 .. W'_(L-1)]: every layer's modulated and demodulated weight for one style, bit for bit what Linear_Mod.forward builds."""
        return [layer.effective_weight(style) for layer in self.layers()]

    def forward(self, x, style):
        if self.num_layers == 1:
            return self.network(x, style)
        for i in range(self.num_layers):
            x = getattr(self, f"linear_{i}")(x, style)
            if i < self.num_layers - 1:
                x = self.relu(x)
        return x


class CoordMLP_Mod(nn.Module):
    def __init__(self, cin, cout, num_layers, nf=256, dropout=0, activation=None, min_max=None, n_harmonic_functions=10, embedder_scalar=1,
                 embed_concat_pts=True, extra_feat_dim=0, symmetrize=False, condition_dim=128):
        super().__init__()
        self.extra_feat_dim, self.condition_dim = extra_feat_dim, condition_dim
        if n_harmonic_functions > 0:
            self.embedder = HarmonicEmbedding(n_harmonic_functions, embedder_scalar)
            dim_in = cin * 2 * n_harmonic_functions + (cin if embed_concat_pts else 0)
            self.embed_concat_pts = embed_concat_pts
        else:
            self.embedder = None
            dim_in = cin
        self.in_layer = nn.Linear(dim_in, nf)
        self.relu = nn.ReLU(inplace=True)
        self.mlp = MLP_Mod(nf, cout, num_layers, nf, dropout, activation)
        self.style_mlp = MLP(condition_dim, nf, 2, nf, dropout, None)
        self.dropout = dropout
        self.symmetrize = symmetrize
        if min_max is not None:
            self.register_buffer("min_max", min_max)
        else:
            self.min_max = None
        self.bsdf = None

    # the halves of CoordMLP's gates that look at the point list, the embedding and the in_layer -- the same functions, not copies
    _fused_input_ok = CoordMLP._fused_input_ok
    _fused_input = CoordMLP._fused_input
    _stack_input_ok = CoordMLP._stack_input_ok
    _field_grad_input_ok = CoordMLP._field_grad_input_ok
    _fused_head_of = CoordMLP._fused_head_of
    _w_in = CoordMLP._w_in
    _stack_node = CoordMLP._stack_node

    def _field_mod_ok(self, x, feat):
        """USE_FIELD_MOD's gate: a float32 point list [M,3] on the GPU, the standard input stage (embedding with concatenated points, an
        even number of frequencies), width 256, at least one hidden layer, no dropout, one float32 style of condition_dim columns.
        Everything else -- narrow nets, no embedder, CPU, float64, inputs an autocast region cast -- takes the plain torch code."""
        if not (USE_FIELD_MOD and not REFERENCE_FORMULATION and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
                and x.shape[1] == 3 and x.shape[0] >= 1 and not torch.is_autocast_enabled()
                and self.embedder is not None and self.embed_concat_pts and len(self.embedder.frequencies) % 2 == 0
                and self.in_layer.bias is not None and self.in_layer.weight.dtype == torch.float32 and self.in_layer.weight.shape[0] == 256
                and self.mlp.num_layers >= 2 and not getattr(self, "dropout", 0)
                and feat.is_cuda and feat.dtype == torch.float32 and feat.shape[-1] == self.condition_dim):
            return False
        layers = self.mlp.layers()
        return (all(tuple(l.weight.shape) == (256, 256) for l in layers[:-1]) and layers[-1].weight.shape[1] == 256
                and all(l.weight.dtype == torch.float32 and l.bias is None for l in layers))

    def _forward_field(self, x, feat):
        """The field with its effective weights W'_l (MLP_Mod.effective_weights, once per call) on CoordMLP's routes: a bias-free Linear/ReLU
        stack of width 256 behind the fused input stage.  The kernels return gradients with respect to W'_l; autograd carries them through
        the modulation statements to the weights, the style network and the embedding.  Inherited limits: the stack nodes are once
        differentiable, and _field_value gives no second-order gradient with respect to the points."""
        *hidden, w_head = self.mlp.effective_weights(self.style_mlp(feat))
        if self._stack_input_ok(x):  # a long list with grad enabled
            head = self._fused_head_of(w_head, 0)
            out = self._stack_node(x, None, None, None, hidden, head)
            if head is not None:
                return out
            out = linear(out, w_head)
        elif self._field_grad_input_ok(x) and tuple(w_head.shape) == (1, 256):  # the eikonal call: a short list that requires grad
            return _field_value(x, self._w_in(), w_head, self.embedder._frequencies(x.device), bool(self.symmetrize), *hidden)
        else:  # grad disabled (the grid pass), or nothing that needs the hand-written backward: ReLU in the epilogue where the list is long
            if self._fused_input_ok(x):
                h = self._fused_input(x)
            else:
                if self.symmetrize:
                    x = torch.cat([x[..., :1].abs(), x[..., 1:]], -1)
                h = linear_relu(torch.cat([x, self.embedder(x)], -1), self.in_layer.weight, self.in_layer.bias)
            for w in hidden:
                h = linear_relu(h, w)
            out = linear(h, w_head)
        if self.min_max is not None:
            out = out * (self.min_max[:, 1] - self.min_max[:, 0]) + self.min_max[:, 0]
        return out

    def forward(self, x, feat=None):
        assert feat is not None and feat.shape[-1] == self.condition_dim
        if self._field_mod_ok(x, feat):
            return self._forward_field(x, feat)
        if self.symmetrize:
            x = torch.cat([x[..., :1].abs(), x[..., 1:]], -1)
        x_in = x
        if self.embedder is not None:
            x_in = self.embedder(x)
            if self.embed_concat_pts:
                x_in = torch.cat([x, x_in], -1)
        x_in = self.relu(self.in_layer(x_in))
        out = self.mlp(x_in, self.style_mlp(feat))
        if self.min_max is not None:
            out = out * (self.min_max[:, 1] - self.min_max[:, 0]) + self.min_max[:, 0]
        return out

    def sample(self, x, feat=None):
        return self.forward(x, feat)
