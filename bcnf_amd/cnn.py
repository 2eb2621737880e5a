"""The CNN feature network (the reference's src/bcnf/models/cnn.py): per-image convolution stacks over the frames of
the camera videos, then one Linear over the cameras' concatenated features.

Same kwargs, submodule names and state_dict keys (`cnn_layers.<i>.<0, 4, 8, ...>.{weight, bias}`, `final_layer.*`), the
same padding rule -- layer i + 1 is padded from kernel_sizes[i] and strides[i], the reference's index quirk -- and the
same CPU-RNG consumption while it is built (the example_camera_input draw, each Conv2d's init, and the shape probe,
which runs the layers built so far with their Dropout modules in training mode), so the same torch.manual_seed gives
the reference's initial state_dict bit for bit.

On fp32 GPU tensors each Conv2d -> ReLU -> Dropout -> MaxPool2d(2, 2) group inside the kernels' limits (stride 1,
ksize <= 8, channels <= 32, padding <= ksize - 1; include/bcnf_amd.h "CNN layer") is ONE launch each way
(_ConvBlockFn: bcnf_conv_block_forward / bcnf_conv_block_backward) that keeps only the pooled output and one byte per
pooled element, and `final_layer` runs on the MFMA GEMMs; CPU tensors, other strides and shapes, and `fused = False`
run the torch modules themselves.
"""
from __future__ import annotations

import torch
from torch import nn

from bcnf_amd.feature_network import (FEATURE_NETWORKS, FeatureNetwork, FeatureRngMixin, HIPLinear, _on_kernels,
                                      _rows_linear)

CONV_MAX_K = 8             # bcnf_conv_block_*: ksize <= 8, channels <= 32 (include/bcnf_amd.h)
CONV_MAX_C = 32
_WORK_FLOATS: dict = {}    # shape arguments -> floats of the backward's partials (bcnf_conv_block_work_bytes)


class _ConvBlockFn(torch.autograd.Function):
    """maxpool2x2(dropout(relu(conv2d(x, weight, bias)))) in ONE launch each way. The forward saves x and one code
    byte per pooled element (the window's winner and whether it is positive); the backward needs no RNG."""

    @staticmethod
    def forward(ctx, x, weight, bias, pad_h, pad_w, p, rng, salt):
        from bcnf_amd import _native as N
        n, c_in, h, w = x.shape
        c_out, _, k, _ = weight.shape
        hc, wc = h + 2 * pad_h - k + 1, w + 2 * pad_w - k + 1
        y = torch.empty((n, c_out, hc // 2, wc // 2), dtype=torch.float32, device=x.device)
        save = any(ctx.needs_input_grad)     # all False under no_grad: nothing is saved at inference
        code = torch.empty(y.shape, dtype=torch.uint8, device=x.device) if save else None
        N.call("bcnf_conv_block_forward", x, weight, bias, n, c_in, h, w, c_out, k, pad_h, pad_w, float(p),
               rng if p > 0.0 else None, int(salt), y, code, N.stream_handle(x.device))
        if save:
            ctx.save_for_backward(x, weight, code)
        ctx.args = (n, c_in, h, w, c_out, k, pad_h, pad_w, float(p))
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        from bcnf_amd import _native as N
        x, weight, code = ctx.saved_tensors
        dy = dy.contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_b = need_b and ctx.has_bias
        dx = torch.empty_like(x) if need_x else None
        dw = torch.empty_like(weight) if need_w else None
        db = torch.empty(weight.shape[0], dtype=torch.float32, device=x.device) if need_b else None
        work = None
        if need_w or need_b:
            wf = _WORK_FLOATS.get(ctx.args)
            if wf is None:
                wf = _WORK_FLOATS[ctx.args] = max(N.query_i64("bcnf_conv_block_work_bytes", *ctx.args) // 4, 1)
            work = torch.empty(wf, dtype=torch.float32, device=x.device)
        N.call("bcnf_conv_block_backward", x, weight, dy, code, *ctx.args, dx, dw, db, work,
               N.stream_handle(x.device))
        return dx, dw, db, None, None, None, None, None


def _pair(v) -> tuple:
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class CNN(FeatureRngMixin, FeatureNetwork):
    fused = True        # False: the torch modules (fallback tests, tools/cnn_feature_ab.py)

    def __init__(self, hidden_channels: list[int], kernel_sizes: list[int], strides: list[int], output_size_lin: int,
                 output_size: int, image_input_size: tuple[int, int] = (90, 160), dropout_prob: float = 0.5,
                 num_CNN: int = 1, verbose: bool = False) -> None:
        super().__init__()
        self.input_size = image_input_size
        self.output_size = output_size
        self.cnn_layers = nn.ModuleList()
        self.pool = nn.MaxPool2d(2, 2)
        self.example_camera_input = torch.randn(1, 1, image_input_size[0], image_input_size[1])
        if verbose:
            print(f'Example camera input size: {self.example_camera_input.shape}')
        self.output_size_lin = output_size_lin
        self.num_CNN = num_CNN

        def padding_of(i: int, height: int, width: int) -> tuple[int, int]:
            return (((strides[i] - 1) * height - strides[i] + kernel_sizes[i]) // 2,
                    ((strides[i] - 1) * width - strides[i] + kernel_sizes[i]) // 2)

        shape = None
        for _ in range(num_CNN):
            layers: list[nn.Module] = []
            channels = [1] + list(hidden_channels)
            for i in range(len(hidden_channels)):
                # layer 0 is padded for the image; layer i >= 1 for the previous layer's output, from kernel_sizes[i - 1]
                # and strides[i - 1] (the reference's index quirk: not the layer's own kernel)
                padding = padding_of(0, *image_input_size) if i == 0 else padding_of(i - 1, shape[2], shape[3])
                layers += [nn.Conv2d(channels[i], channels[i + 1], kernel_sizes[i], strides[i], padding), nn.ReLU(),
                           nn.Dropout(dropout_prob), self.pool]
                shape = self._calc_output_shape(self.example_camera_input, layers)
                if verbose:
                    print(f'Output size after layer {i}: {shape}')
            layers.append(nn.Flatten())
            self.cnn_layers.append(nn.Sequential(*layers))

        self.final_output_size = shape[1] * shape[2] * shape[3]
        if verbose:
            print(f'Final output size: {self.final_output_size * 2}')
        self.final_layer = HIPLinear(self.final_output_size * 2, self.output_size_lin)
        if verbose:
            print(self.cnn_layers)

    def _calc_output_shape(self, input: torch.Tensor, layers: list[nn.Module]) -> torch.Size:
        """The shape probe: the layers built so far on the example image, Dropout modules in training mode (each
        probe draws their masks from the CPU generator, as the reference's does)."""
        for layer in layers:
            input = layer(input)
        return input.shape

    def _block_on_kernels(self, x: torch.Tensor, conv: nn.Module, pool: nn.Module) -> bool:
        if not (self.fused and isinstance(conv, nn.Conv2d) and isinstance(pool, nn.MaxPool2d)):
            return False
        if not (x.dim() == 4 and x.numel() > 0 and _on_kernels(x, conv.weight, conv.bias) and conv.weight.is_cuda):
            return False
        k = conv.kernel_size
        pad = conv.padding
        if isinstance(pad, str) or conv.padding_mode != "zeros" or conv.groups != 1:
            return False
        if _pair(conv.stride) != (1, 1) or _pair(conv.dilation) != (1, 1) or k[0] != k[1] or not 1 <= k[0] <= CONV_MAX_K:
            return False
        if not (1 <= conv.in_channels <= CONV_MAX_C and 1 <= conv.out_channels <= CONV_MAX_C
                and x.shape[1] == conv.in_channels):
            return False
        if not (0 <= pad[0] <= k[0] - 1 and 0 <= pad[1] <= k[0] - 1):
            return False
        if x.shape[2] + 2 * pad[0] - k[0] + 1 < 2 or x.shape[3] + 2 * pad[1] - k[0] + 1 < 2:
            return False
        return (_pair(pool.kernel_size) == (2, 2) and _pair(pool.stride) == (2, 2) and _pair(pool.padding) == (0, 0)
                and _pair(pool.dilation) == (1, 1) and not pool.ceil_mode and not pool.return_indices)

    def run(self, index: int, x: torch.Tensor) -> torch.Tensor:
        """cnn_layers[index] on the images x (n, 1, H, W): each Conv2d -> ReLU -> Dropout -> pool group inside the
        kernels' limits as one _ConvBlockFn launch (salt = 256 index + the Conv2d's module index), the rest as the
        modules themselves."""
        mods = list(self.cnn_layers[index])
        i = 0
        rng = bump = None
        while i < len(mods):
            if i + 3 < len(mods) and isinstance(mods[i + 1], nn.ReLU) and isinstance(mods[i + 2], nn.Dropout) \
                    and self._block_on_kernels(x, mods[i], mods[i + 3]):
                conv, drop = mods[i], mods[i + 2]
                p = drop.p if drop.training else 0.0
                if p >= 1.0:                          # nn.Dropout(1): everything dropped; outside the kernels' limits
                    x = mods[i + 3](drop(mods[i + 1](conv(x))))
                    i += 4
                    continue
                if p > 0.0 and rng is None:
                    rng, owner_bumps = self._rng(x.device)
                    bump = None if owner_bumps else rng
                x = _ConvBlockFn.apply(x.contiguous(), conv.weight, conv.bias, conv.padding[0], conv.padding[1], p,
                                       rng if p > 0.0 else None, 256 * index + i)
                i += 4
                continue
            x = mods[i](x)
            i += 1
        if bump is not None:
            bump[1:2].add_(1)
        return x

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        batch_size, num_cameras, sequence_length, img_x, img_y = x.size()
        if self.num_CNN == 1 and self.fused and _on_kernels(x):
            # images are independent: the CNN on them in the input's own (batch, camera, frame) order gives the
            # (batch, camera, frame, features) tensor the reference reaches through two permutes
            y = self.run(0, x.reshape(batch_size * num_cameras * sequence_length, 1, img_x, img_y))
            y = y.view(batch_size, num_cameras, sequence_length, -1)
        else:
            x = x.permute(1, 0, 2, 3, 4)
            if self.num_CNN > 1:
                x = x.reshape(num_cameras, batch_size * sequence_length, 1, img_x, img_y)
                y = torch.stack([self.run(i, x[i]) for i in range(self.num_CNN)], dim=0)
            else:
                y = self.run(0, x.reshape(batch_size * num_cameras * sequence_length, 1, img_x, img_y))
            y = y.view(num_cameras, batch_size, sequence_length, -1).permute(1, 0, 2, 3)
        # the reference's reshape of (batch, camera, frame, features) to (batch, frame, camera * features): a plain
        # reshape, not a transpose of camera and frame
        shape = y.shape
        y = y.reshape(shape[0], shape[2], shape[1] * shape[3])
        return _rows_linear(self.final_layer, y)


FEATURE_NETWORKS["CNN"] = CNN
