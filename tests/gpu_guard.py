"""NaN-guarded device buffers for the GPU tests that drive the C-ABI directly (tests/test_gpu_transformer.py,
tests/test_gpu_linear.py): a kernel that writes outside its output kills a canary, one that leaves part of its output
unwritten leaves a NaN inside."""
import torch

DEV = "cuda"
GUARD = 64
NAN = float("nan")


def guarded(rows, width, ld=None, data=None):
    """(buffer, view): a (rows, width) view with row stride ld inside a NaN-filled buffer with GUARD floats either
    side; `data` is copied into the view, everything else stays NaN."""
    ld = width if ld is None else ld
    buf = torch.full((2 * GUARD + rows * ld,), NAN, dtype=torch.float32, device=DEV)
    view = buf[GUARD:GUARD + rows * ld].view(rows, ld)[:, :width]
    if data is not None:
        view.copy_(data)
    return buf, view


def canaries_alive(buf, rows, width, ld=None):
    ld = width if ld is None else ld
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[GUARD:GUARD + rows * ld].view(rows, ld)[:, :width] = False
    inside = buf[~outside]
    return bool(torch.isnan(buf[outside]).all()) and bool(torch.isfinite(inside).all())
