"""PyTorch autograd modules over the gfx950 operator modules (neus2_amd.module): `Encoding`, `Network` and
`NetworkWithInputEncoding` with the constructor arguments, shapes and attributes PyTorch code written for tiny-cuda-nn's
torch extension expects, so that such code runs on these kernels by changing its import (`import tinycudann as tcnn`
resolves to this file through the top-level re-export).

Each class is a torch.nn.Module with one fp32 `params` Parameter. forward(x) takes [B, n_input_dims] for any B >= 1,
pads B with zero rows to a multiple of 128 (the kernels' batch granularity) and returns [B, n_output_dims]. Autograd is
complete to second order in the input: `grad(y, x, create_graph=True)` followed by `.backward()` (an eikonal loss) gives
gradients for `params`, `x` and the first gradient's `grad_outputs`, through neus_module_backward_backward_input. The
double backward is exact for every hidden and output activation of the FullyFusedMLP (the networks are created with
"second_order": "exact", which adds the act'' terms of Softplus, Squareplus, Sigmoid and Exponential to tiny-cuda-nn's
chain; for ReLU / None with a linear output the two coincide) and is provided for encodings without a SphericalHarmonics
segment (no second derivative of it is implemented); a cotangent for the parameter gradient (a gradient of a gradient in
the parameters) is not supported.

Encodings: grids (HashGrid / Grid / DenseGrid / TiledGrid: 2, 3 or 4 input dims, 1, 2, 4 or 8 features per level, "type" Hash /
Dense / Tiled, "interpolation" Linear / Smoothstep; with Smoothstep the double backward carries the grid's diagonal second
derivatives; "gradient_scatter": "binned" in a grid's config makes its `params.grad` bitwise repeatable: int64 fixed-point sums
in place of float atomics), and the parameter-free Identity, Frequency, SphericalHarmonics, TriangleWave (1-16 frequencies), OneBlob
(n_bins a power of two up to 128), OneBlobFrequency / NRC (TriangleWave over 3 dims, OneBlob over 5, Identity over the rest;
at least 8 dims) and Composite (of the five segment types), whose `params` is an empty Parameter. OneBlob's second
derivative is continuous and TriangleWave's is zero: both support the double backward.

Networks: "otype" FullyFusedMLP (n_neurons 16, 32, 64 or 128) or CutlassMLP (n_neurons any multiple of 16 from 16 to 512:
the way to a 256- or 512-wide network, as in tiny-cuda-nn), 1 to 32 hidden layers, up to 128 input and output dims; the
config is passed through to the native module, which validates it. A CutlassMLP also takes "activation": "Sine" (a SIREN,
initialised as tiny-cuda-nn's: first matrix U(+-30 / fan_in), the others U(+-sqrt(6 / fan_in))), with the exact double
backward; a FullyFusedMLP refuses it, and no otype takes it as "output_activation".

Two autograd Functions talk to a small backend object (`NativeBackend` over module.Module by default):
    n_params, n_input_dims, n_output_dims (the backend's, possibly padded, output width), param_dtype, output_dtype,
    supports_double_backward, batch_capacity (None: unlimited), with_capacity(n), initialize_params(seed),
    inference(x, p) -> y
    fwd(x, p, prepare_input_gradients) -> (ctx, y)
    bwd(ctx, x, p, dL_dy, want_dx, want_dparams) -> (dL_dx | None, dL_dparams | None)
    bwd_bwd_input(ctx, x, p, u, dL_dy, want_dparams, want_ddLdy, want_dx) -> (dS_dparams, dS_ddLdy, dS_dx), S = u . dL_dx
with x [n, n_input_dims] f32, p the parameters in param_dtype, y / dL_dy [n, n_output_dims] in output_dtype, parameter
gradients fp32.
"""
from __future__ import annotations

import json

import torch

from . import module as _module

BATCH_GRANULARITY = 128
INITIAL_BATCH_CAPACITY = 1 << 14  # rows the native module is created for; a larger batch re-creates it larger


def _round_up(n, k):
    return (n + k - 1) // k * k


class NativeBackend:
    """module.Module behind the backend interface. The parameters live outside the native module, so a larger batch
    capacity is a new module (with_capacity) and nothing else changes."""

    def __init__(self, factory, batch_capacity):
        self._factory = factory
        self.batch_capacity = _round_up(max(int(batch_capacity), 1), BATCH_GRANULARITY)
        self.m = factory(self.batch_capacity)
        self.n_params = self.m.n_params
        self.n_input_dims = self.m.n_input_dims
        self.n_output_dims = self.m.n_output_dims
        fp32 = self.m.precision == "fp32"
        self.param_dtype = self.output_dtype = torch.float32 if fp32 else torch.float16
        hp = self.m.hyperparams()
        enc = hp.get("encoding", hp)
        has_sh = any(e.get("otype") == "SphericalHarmonics" for e in [enc] + list(enc.get("nested", [])))
        self.supports_double_backward = not has_sh

    def with_capacity(self, n):
        if n <= self.batch_capacity:
            return self
        return NativeBackend(self._factory, max(n, 2 * self.batch_capacity))

    def initialize_params(self, seed):
        return self.m.initialize_params(seed)

    def inference(self, x, p):
        return self.m.inference(x, p)

    def fwd(self, x, p, prepare_input_gradients):
        ctx, y = self.m.forward(x, p, prepare_input_gradients=prepare_input_gradients)
        ctx.output = y  # the backward of an output activation other than None needs the forward's output
        return ctx, y

    def bwd(self, ctx, x, p, dL_dy, want_dx, want_dparams):
        dx = torch.empty((x.shape[0], self.n_input_dims), dtype=torch.float32, device=x.device) if want_dx else None
        dp = torch.empty(self.n_params, dtype=torch.float32, device=x.device) if want_dparams else None
        mode = _module.GradientMode.Overwrite if want_dparams else _module.GradientMode.Ignore
        self.m.backward(ctx, x, dL_dy, p, dL_dparams=dp, dL_dinput=dx, mode=mode, output=getattr(ctx, "output", None))
        return dx, dp

    def bwd_bwd_input(self, ctx, x, p, u, dL_dy, want_dparams, want_ddLdy, want_dx):
        dp = torch.empty(self.n_params, dtype=torch.float32, device=x.device) if want_dparams else None
        ddy = torch.empty_like(dL_dy) if want_ddLdy else None
        dx = torch.empty((x.shape[0], self.n_input_dims), dtype=torch.float32, device=x.device) if want_dx else None
        mode = _module.GradientMode.Overwrite if want_dparams else _module.GradientMode.Ignore
        self.m.backward_backward_input(ctx, x, u, dL_dy, p, dL_dparams=dp, dL_ddLdoutput=ddy, mode=mode, dL_dinput=dx)
        return dp, ddy, dx


class _Forward(torch.autograd.Function):
    """y = f(x, params). The parameter arrives in fp32 and is cast to the backend's precision here, so autograd sees the
    fp32 Parameter and its gradient comes back fp32 without a round trip through fp16."""

    @staticmethod
    def forward(ctx, be, x, params, loss_scale):
        p = params.detach().to(be.param_dtype).contiguous()
        nctx, y = be.fwd(x, p, bool(ctx.needs_input_grad[1]))
        ctx.be, ctx.nctx, ctx.loss_scale = be, nctx, loss_scale
        ctx.save_for_backward(x, params, p)
        return y

    @staticmethod
    def backward(ctx, dL_dy):
        x, params, p = ctx.saved_tensors
        want_dx, want_dp = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if dL_dy is None or not (want_dx or want_dp):
            return None, None, None, None
        dx, dp = _Backward.apply(ctx.be, ctx.nctx, x, params, p, dL_dy, ctx.loss_scale, want_dx, want_dp)
        return None, dx, dp, None


class _Backward(torch.autograd.Function):
    """(dL_dx, dL_dparams) = backward of _Forward; its own backward is the double backward in the input."""

    @staticmethod
    def forward(ctx, be, nctx, x, params, p, dL_dy, loss_scale, want_dx, want_dp):
        ctx.set_materialize_grads(False)
        # the loss scale keeps small gradients out of the fp16 subnormals inside the backend; every result that is linear
        # in dL_dy is divided by it again
        g = (dL_dy.detach().float() * loss_scale).to(be.output_dtype).contiguous()
        dx, dp = be.bwd(nctx, x, p, g, want_dx, want_dp)
        ctx.be, ctx.nctx, ctx.loss_scale = be, nctx, loss_scale
        ctx.save_for_backward(x, p, g)
        inv = 1.0 / loss_scale
        return (dx * inv if dx is not None else None), (dp * inv if dp is not None else None)

    @staticmethod
    def backward(ctx, u, g_dp):
        if g_dp is not None:
            raise RuntimeError("double backward: a cotangent for the parameter gradient (a gradient of dL/dparams) is not supported; "
                               "only gradients of dL/dinput are (backward_backward_input)")
        _, _, want_x, want_p, _, want_g, _, _, _ = ctx.needs_input_grad
        if u is None or not (want_x or want_p or want_g):
            return (None,) * 9
        be = ctx.be
        if not be.supports_double_backward:
            raise RuntimeError("double backward is not supported for this module: it is provided for encodings without a "
                               "SphericalHarmonics segment (no second derivative of the spherical harmonics is implemented)")
        x, p, g = ctx.saved_tensors
        dp, ddy, dx = be.bwd_bwd_input(ctx.nctx, x, p, u.detach().float().contiguous(), g, want_p, want_g, want_x)
        inv = 1.0 / ctx.loss_scale
        # dS/d(dL_dy) = J u does not depend on dL_dy: the scale does not enter it
        return (None, None, dx * inv if dx is not None else None, dp * inv if dp is not None else None, None, ddy, None, None, None)


class Module(torch.nn.Module):
    """Base of the three modules: the fp32 `params` Parameter, padding / slicing and the autograd Functions over a
    backend. Subclasses give `_make_backend(batch_capacity)`; a `backend` argument replaces it (tests)."""

    def __init__(self, seed=1337, backend=None, n_output_dims=None, loss_scale=None):
        super().__init__()
        self.seed = seed
        self._backend = backend if backend is not None else self._make_backend(INITIAL_BATCH_CAPACITY)
        be = self._backend
        self.n_input_dims = be.n_input_dims
        self.n_output_dims = be.n_output_dims if n_output_dims is None else n_output_dims
        self.dtype = be.output_dtype
        self.loss_scale = float(loss_scale) if loss_scale is not None else (128.0 if be.output_dtype == torch.float16 else 1.0)
        self.params = torch.nn.Parameter(self.initialize_params(seed), requires_grad=True)

    def _make_backend(self, batch_capacity):
        raise NotImplementedError

    def _be(self, n=0):
        if self._backend is None:
            self._backend = self._make_backend(max(n, INITIAL_BATCH_CAPACITY))
        if self._backend.batch_capacity is not None and n > self._backend.batch_capacity:
            self._backend = self._backend.with_capacity(n)
        return self._backend

    def initialize_params(self, seed=1337):
        return self._be().initialize_params(seed).float()

    def forward(self, x):
        if x.dim() != 2 or x.shape[1] != self.n_input_dims:
            raise ValueError(f"expected an input of shape [B, {self.n_input_dims}], got {tuple(x.shape)}")
        B = x.shape[0]
        if B < 1:
            raise ValueError("expected at least one input row")
        n = _round_up(B, BATCH_GRANULARITY)
        be = self._be(n)
        x = x.to(device=self.params.device, dtype=torch.float32)
        if n != B:
            x = torch.nn.functional.pad(x, (0, 0, 0, n - B))
        x = x.contiguous()
        if not torch.is_grad_enabled() or not (x.requires_grad or self.params.requires_grad):
            y = be.inference(x.detach(), self.params.detach().to(be.param_dtype).contiguous())
        else:
            y = _Forward.apply(be, x, self.params, self.loss_scale)
        return y[:B, :self.n_output_dims]

    def free_temporary_memory(self):
        """Nothing to free: the backend's scratch belongs to the native module and is released with it."""

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_backend"] = None  # the native handle is not picklable; the backend is rebuilt on first use
        return state

    def extra_repr(self):
        return f"n_input_dims={self.n_input_dims}, n_output_dims={self.n_output_dims}, seed={self.seed}, dtype={self.dtype}"


def _text(cfg):
    return json.loads(cfg) if isinstance(cfg, str) else dict(cfg)


class Encoding(Module):
    """Encoding(n_input_dims, encoding_config, seed=1337, dtype=None): a grid (2 - 4 input dims), or a parameter-free Identity /
    Frequency / SphericalHarmonics / TriangleWave / OneBlob / NRC / Composite encoding (`params` is then empty). dtype None / torch.float16: fp16 table
    and output (loss_scale 128); torch.float32: the fp32 encoding (loss_scale 1)."""

    def __init__(self, n_input_dims, encoding_config, seed=1337, dtype=None):
        if dtype not in (None, torch.float16, torch.float32):
            raise ValueError("Encoding: dtype must be None, torch.float16 or torch.float32")
        self.encoding_config = dict(_text(encoding_config), output_layout="AoS", gradient_precision="fp32")
        self._n_in = int(n_input_dims)
        self._precision = _module.Precision.Fp32 if dtype == torch.float32 else _module.Precision.Fp16
        super().__init__(seed=seed)

    def _make_backend(self, batch_capacity):
        return NativeBackend(lambda cap: _module.Module.create_encoding(self.encoding_config, cap, self._n_in, self._precision), batch_capacity)

    def extra_repr(self):
        return super().extra_repr() + f", encoding={self.encoding_config}"


class Network(Module):
    """Network(n_input_dims, n_output_dims, network_config, seed=1337): a FullyFusedMLP (width 16 / 32 / 64 / 128) or a
    CutlassMLP (any multiple of 16 up to 512; also with "activation": "Sine") on the raw input."""

    def __init__(self, n_input_dims, n_output_dims, network_config, seed=1337):
        self.network_config = dict(_text(network_config), gradient_precision="fp32", second_order="exact")
        self._n_in, self._n_out = int(n_input_dims), int(n_output_dims)
        super().__init__(seed=seed, n_output_dims=self._n_out)

    def _make_backend(self, batch_capacity):
        return NativeBackend(lambda cap: _module.Module.create_network(self._n_in, self._n_out, self.network_config, cap), batch_capacity)

    def extra_repr(self):
        return super().extra_repr() + f", network={self.network_config}"


class NetworkWithInputEncoding(Module):
    """NetworkWithInputEncoding(n_input_dims, n_output_dims, encoding_config, network_config, seed=1337): a grid (2 - 4 dims),
    Identity, Frequency, SphericalHarmonics, TriangleWave, OneBlob, NRC or Composite encoding in front of a FullyFusedMLP, as one module with
    parameters [network | grid] (the network alone for the parameter-free encodings)."""

    def __init__(self, n_input_dims, n_output_dims, encoding_config, network_config, seed=1337):
        self.encoding_config = _text(encoding_config)
        self.network_config = dict(_text(network_config), gradient_precision="fp32", second_order="exact")
        self._n_in, self._n_out = int(n_input_dims), int(n_output_dims)
        super().__init__(seed=seed, n_output_dims=self._n_out)

    def _make_backend(self, batch_capacity):
        return NativeBackend(lambda cap: _module.Module.create_network_with_input_encoding(
            self._n_in, self._n_out, self.encoding_config, self.network_config, cap), batch_capacity)

    def extra_repr(self):
        return super().extra_repr() + f", encoding={self.encoding_config}, network={self.network_config}"
