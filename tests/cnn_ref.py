"""Test-side restatement of the CNN layer kernels' dropout draw (include/bcnf_amd.h "CNN layer", bcnf_conv.hip) in
numpy, and the float64 torch chain conv2d -> relu -> keep / (1 - p) -> max_pool2d the GPU tests hold the kernels to.

The draw: element e -- the flat index of a unit in the layer's (n_images, c_out, Hc, Wc) convolution output -- keeps
iff u32(e) >= thresh32(p), u32(e) = word e & 3 of Philox4x32-10 with counter (e >> 2 low, e >> 2 high, offset low,
offset high) and key (seed low ^ salt 0x9E3779B9, seed high ^ 0x40000000). feature_keep's key (dropout_ref.py) has
0x80000000 in its second word.
"""
import numpy as np
import torch

from dropout_ref import philox4x32_10, thresh32

CONV_KEY = 0x40000000


def conv_keep(p, seed, offset, salt, shape):
    """bool array of `shape` = (n_images, c_out, Hc, Wc): the keep mask of one bcnf_conv_block_forward launch."""
    n = int(np.prod(shape))
    if not p > 0.0:
        return np.ones(shape, dtype=bool)
    seed, offset = int(seed) & (2**64 - 1), int(offset) & (2**64 - 1)
    k0 = (seed & 0xFFFFFFFF) ^ (((int(salt) & 0xFFFFFFFF) * 0x9E3779B9) & 0xFFFFFFFF)
    k1 = ((seed >> 32) ^ CONV_KEY) & 0xFFFFFFFF
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10(q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), offset & 0xFFFFFFFF, offset >> 32, k0, k1)
    u = np.stack(words, axis=1).reshape(-1)[:n]
    return (u >= np.uint64(thresh32(p))).reshape(shape)


def windows(a):
    """(N, C, Hc, Wc) -> (N, C, Hc // 2, Wc // 2, 4): the 2 x 2 windows in row-major order, floor mode."""
    n, c, hc, wc = a.shape
    hp, wp = hc // 2, wc // 2
    return a[:, :, :2 * hp, :2 * wp].reshape(n, c, hp, 2, wp, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, hp, wp, 4)


def block_f64(x, w, b, pad, p, keep):
    """float64 pre-activation scaled by the mask, and a = relu(pre) keep / (1 - p); x, w, b: float64 tensors (x and
    the parameters may require grad), keep: bool tensor of pre's shape."""
    pre = torch.nn.functional.conv2d(x, w, b, stride=1, padding=pad)
    scaled = pre * (keep.to(pre.dtype) / (1.0 - p))
    return scaled, torch.relu(scaled)


def near_tie_census(a, tol):
    """(windows with a positive maximum, those of them whose two largest values are closer than tol) of a float64
    activation a (N, C, Hc, Wc)."""
    top = windows(a.detach()).sort(dim=-1, descending=True).values
    positive = top[..., 0] > 0
    near = positive & ((top[..., 0] - top[..., 1]) < tol)
    return int(positive.sum()), int(near.sum())


def validate_code(code, a, tol):
    """The kernel's code bytes against the float64 activation a: the winner's value within tol of the window maximum,
    the float64 argmax wherever the two largest values are at least tol apart, and the positive bit right wherever the
    winner is further than tol from zero. Returns (winner index, alive) as int64 / float64 tensors."""
    win = (code & 3).to(torch.int64)
    alive = ((code >> 2) & 1).to(torch.float64)
    assert int((code >> 3).max()) == 0 if code.numel() else True
    wv = windows(a.detach())
    top = wv.sort(dim=-1, descending=True).values
    chosen = wv.gather(-1, win.unsqueeze(-1)).squeeze(-1)
    assert bool((top[..., 0] - chosen <= tol).all()), "a winner further than tol below its window's maximum"
    clear = (top[..., 0] - top[..., 1]) >= tol
    assert bool((win[clear] == wv.argmax(dim=-1)[clear]).all()), "a clear winner missed"
    far = chosen.abs() > tol
    assert bool((alive[far] == (chosen[far] > 0).to(torch.float64)).all()), "positive bit wrong"
    return win, alive
